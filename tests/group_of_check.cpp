// Stand-alone check of csrc/group_of.h on the host: both group id forms against exact integer division, at the keys
// q d - 1, q d, q d + 1 across their whole ranges ([0, 2^53) for the double form, [0, 2^63) for the integer form), with a
// bound on the integer form's correction steps.  Built and run by tests/test_group_of_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// 3 roundings of 2^-53 relative on a quotient below 2^63, plus the clamp's 1023 (see group_of.h)
static const long STEP_LIMIT = 3072 + 1023;
static long g_steps = 0, g_max_steps = 0;
static int64_t g_key = 0, g_div = 0;
static void step() {
  if (++g_steps > STEP_LIMIT) {
    std::printf("FAIL: more than %ld correction steps at key %lld, divisor %lld\n", STEP_LIMIT, (long long)g_key, (long long)g_div);
    std::exit(1);
  }
}
#define SPAMD_GROUP_OF_STEP() step()
#include "group_of.h"

static long g_checked = 0, g_bad = 0;

static void check_int(const spamd::GroupOf& g, int64_t k) {
  g_steps = 0;
  g_key = k;
  const int64_t got = g(k), want = k / g.d;
  if (g_steps > g_max_steps) g_max_steps = g_steps;
  ++g_checked;
  if (got != want && ++g_bad <= 20)
    std::printf("FAIL: GroupOf  k=%lld d=%lld got %lld want %lld\n", (long long)k, (long long)g.d, (long long)got, (long long)want);
}

static void check_dbl(const spamd::GroupOfD& g, int64_t d, int64_t k) {
  const double got = g(k), want = (double)(k / d);
  ++g_checked;
  if (got != want && ++g_bad <= 20)
    std::printf("FAIL: GroupOfD k=%lld d=%lld got %.17g want %.17g\n", (long long)k, (long long)d, got, want);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t next_random() {  // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

// keys q d - 1, q d, q d + 1 below `limit` (limit <= 2^63, passed as unsigned so that 2^63 itself fits)
template <typename F>
static void around(uint64_t q, uint64_t d, uint64_t limit, F&& f) {
  const unsigned __int128 k = (unsigned __int128)q * d;
  for (int o = -1; o <= 1; ++o) {
    if (k == 0 && o < 0) continue;
    const unsigned __int128 x = k + o;
    if (x < limit) f((int64_t)(uint64_t)x);
  }
}

template <typename F>
static void sweep(uint64_t d, uint64_t limit, F&& f) {
  const uint64_t qtop = (limit - 1) / d;
  for (uint64_t q = 0; q <= 4096 && q <= qtop; ++q) around(q, d, limit, f);               // the bottom
  for (uint64_t i = 0; i <= 4096 && i <= qtop; ++i) around(qtop - i, d, limit, f);         // the top
  for (int b = 1; b < 64; ++b)                                                            // around every power of two
    for (int64_t o = -2; o <= 2; ++o) {
      const uint64_t q = ((uint64_t)1 << b) + (uint64_t)o;
      if (q <= qtop) around(q, d, limit, f);
    }
  for (int b = 1; b < 64; ++b)                                                            // keys (not quotients) at 2^b
    for (int64_t o = -2; o <= 2; ++o) {
      const uint64_t k = ((uint64_t)1 << b) + (uint64_t)o;
      if (k < limit) f((int64_t)k);
    }
  for (int i = 0; i < 300000; ++i) {                                                      // everywhere, every magnitude
    const uint64_t q = (next_random() >> (next_random() % 64)) % (qtop + 1);
    around(q, d, limit, f);
  }
  for (uint64_t i = 1; i <= 4096 && i <= limit; ++i) f((int64_t)(limit - i));              // the last keys of the range
}

int main() {
  const int64_t divisors[] = {1, 3, 141, 2147483647ll, 2147483648ll, 1000000000039ll, 7, 4097, (1ll << 53) - 1, (1ll << 62) + 3};
  for (int64_t d : divisors) {
    g_div = d;
    const spamd::GroupOf gi{d, 1.0 / (double)d};
    sweep((uint64_t)d, (uint64_t)1 << 63, [&](int64_t k) { check_int(gi, k); });
    if (d < (1ll << 53)) {
      const spamd::GroupOfD gd{(double)d, 1.0 / (double)d};
      sweep((uint64_t)d, (uint64_t)1 << 53, [&](int64_t k) { check_dbl(gd, d, k); });
    }
  }
  std::printf("%s: %ld keys checked, %ld wrong, at most %ld correction steps (limit %ld)\n", g_bad ? "FAIL" : "OK", g_checked, g_bad,
              g_max_steps, STEP_LIMIT);
  return g_bad ? 1 : 0;
}

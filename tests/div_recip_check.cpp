// Stand-alone check of csrc/div_recip.h on the host: div_recip<uint32_t> (dividends below 2^32) and div_recip<uint64_t>
// (dividends below 2^52) against exact integer division at the dividends q d - 1, q d, q d + 1, for divisors that are small,
// prime, powers of two +- 1, near 2^16, 2^26, 2^31 and near the end of the range, with quotients that take the dividend up
// to the end of the range, plus a few million random pairs.  It counts how often each of the two repairs fires, and checks
// that the product estimate * divisor (at most r + d when the estimate is one too large) fits the 32-bit form's word for
// every pair.  Built and run by tests/test_div_recip_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static long g_down = 0, g_up = 0;
#define SPAMD_DIV_RECIP_DOWN() (++g_down)
#define SPAMD_DIV_RECIP_UP() (++g_up)
#include "div_recip.h"

static long g_checked = 0, g_bad = 0, g_wrap = 0;
static uint64_t g_max_back32 = 0;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t next_random() {  // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

template <typename U>
static void check(uint64_t r, uint64_t d) {
  const double inv = 1.0 / (double)d;
  const U got = spamd::div_recip<U>((U)r, (U)d, inv);
  const uint64_t want = r / d;
  ++g_checked;
  if ((uint64_t)got != want && ++g_bad <= 20)
    std::printf("FAIL: div_recip<uint%d_t> r=%llu d=%llu got %llu want %llu\n", (int)(8 * sizeof(U)), (unsigned long long)r,
                (unsigned long long)d, (unsigned long long)got, (unsigned long long)want);
  if (sizeof(U) == 4) {   // the estimate's product in full width: it must be the 32-bit product the function forms
    const uint64_t est = (uint64_t)(U)((double)(U)r * inv);
    const uint64_t back = est * d;
    if (back > g_max_back32) g_max_back32 = back;
    if (back > 0xffffffffull && ++g_wrap <= 20)
      std::printf("FAIL: 32-bit product wraps: r=%llu d=%llu estimate %llu\n", (unsigned long long)r, (unsigned long long)d,
                  (unsigned long long)est);
  }
}

// dividends q d - 1, q d, q d + 1 below `limit`
template <typename U>
static void around(uint64_t q, uint64_t d, uint64_t limit) {
  const unsigned __int128 k = (unsigned __int128)q * d;
  for (int o = -1; o <= 1; ++o) {
    if (k == 0 && o < 0) continue;
    const unsigned __int128 x = k + o;
    if (x < limit) check<U>((uint64_t)x, d);
  }
}

template <typename U>
static void sweep(uint64_t d, uint64_t limit) {
  const uint64_t qtop = (limit - 1) / d;
  for (uint64_t q = 0; q <= 2048 && q <= qtop; ++q) around<U>(q, d, limit);              // the bottom
  for (uint64_t i = 0; i <= 2048 && i <= qtop; ++i) around<U>(qtop - i, d, limit);        // the dividend approaches the limit
  for (int b = 1; b < 53; ++b)                                                           // quotients around every power of two
    for (int64_t o = -2; o <= 2; ++o) {
      const uint64_t q = ((uint64_t)1 << b) + (uint64_t)o;
      if (q <= qtop) around<U>(q, d, limit);
    }
  for (int b = 1; b < 53; ++b)                                                           // dividends (not quotients) at 2^b
    for (int64_t o = -2; o <= 2; ++o) {
      const uint64_t r = ((uint64_t)1 << b) + (uint64_t)o;
      if (r < limit) check<U>(r, d);
    }
  for (int i = 0; i < 20000; ++i) {                                                      // every magnitude of quotient
    const uint64_t q = (next_random() >> (next_random() % 64)) % (qtop + 1);
    around<U>(q, d, limit);
  }
  for (uint64_t i = 1; i <= 2048 && i <= limit; ++i) check<U>(limit - i, d);              // the last dividends of the range
}

template <typename U>
static void run(int bits) {
  const uint64_t limit = (uint64_t)1 << bits;
  const long down0 = g_down, up0 = g_up, checked0 = g_checked;
  // small, prime, 2^k +- 1, near 2^16 / 2^26 / 2^31, near the range's end
  uint64_t divisors[512];
  int nd = 0;
  for (uint64_t d = 1; d <= 20; ++d) divisors[nd++] = d;
  const uint64_t primes[] = {23, 97, 141, 251, 257, 4093, 65521, 65537, 1000003, 67108859, 67108879, 2147483647ull, 2147483659ull,
                             4294967291ull, 1000000000039ull, 4503599627370449ull};
  for (uint64_t p : primes) divisors[nd++] = p;
  for (int b = 2; b < bits; ++b)
    for (int64_t o = -1; o <= 1; ++o) divisors[nd++] = ((uint64_t)1 << b) + (uint64_t)o;
  const int near[] = {16, 26, 31};
  for (int b : near)
    for (int64_t o = -3; o <= 3; ++o) divisors[nd++] = ((uint64_t)1 << b) + (uint64_t)o;
  for (uint64_t i = 1; i <= 8; ++i) divisors[nd++] = limit - i;
  divisors[nd++] = limit / 2 + 1;
  divisors[nd++] = limit / 3;
  for (int i = 0; i < nd; ++i)
    if (divisors[i] >= 1 && divisors[i] < limit) sweep<U>(divisors[i], limit);
  for (int i = 0; i < 4000000; ++i) {                                                    // random pairs, every magnitude of both
    const uint64_t d = (next_random() >> (next_random() % 64)) % (limit - 1) + 1;
    const uint64_t r = (next_random() >> (next_random() % 64)) % limit;
    check<U>(r, d);
    around<U>(r / d, d, limit);
  }
  std::printf("div_recip<uint%d_t>, dividends below 2^%d: %ld pairs, --q repairs %ld, ++q repairs %ld\n", (int)(8 * sizeof(U)), bits,
              g_checked - checked0, g_down - down0, g_up - up0);
}

int main() {
  run<uint32_t>(32);
  std::printf("largest estimate * divisor of the 32-bit form: %llu (limit %llu)\n", (unsigned long long)g_max_back32, 0xffffffffull);
  run<uint64_t>(52);
  const bool bad = g_bad || g_wrap;
  std::printf("%s: %ld pairs checked, %ld wrong, %ld wrapped 32-bit products, repairs --q %ld ++q %ld\n", bad ? "FAIL" : "OK", g_checked, g_bad,
              g_wrap, g_down, g_up);
  return bad ? 1 : 0;
}

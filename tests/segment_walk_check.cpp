// Stand-alone check of csrc/segment_walk.h on the host: seg_of, seg_slot and seg_window_pieces, the arithmetic by which the
// long forms of softmax, attention, the semiring products and mttkrp find the pieces of their long segments.  For chunk in
// {64, 128, 192} and pointer arrays of 1 to 12 segments whose lengths are drawn from {0, 1, 3, chunk - 1, chunk, chunk + 1,
// 2 chunk - 1, 2 chunk, 2 chunk + 1, 3 chunk + 5, random}, with 32-bit and 64-bit pointers, it asserts that
//   - the pieces that seg_window_pieces hands out over all windows are exactly the pieces of the segments longer than `chunk`,
//     each once, at most two per window;
//   - seg_slot is injective over them, every slot is below 2 nwin, and slot / 2 is the window that found the piece;
//   - seg_of is the last r with ptr[r] <= pos.
// The fixed array of lengths [3, 130, 70, 1, 200] at chunk 64 is among them: both slots of its window 2 are used.
// Built and run by tests/test_segment_walk_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "segment_walk.h"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t next_random() {  // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

static long g_arrays = 0, g_pieces = 0, g_two = 0, g_bad = 0;

struct Piece {
  int64_t seg, b, s, e;
};

#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (++g_bad <= 20) {                      \
        std::printf("FAIL: " __VA_ARGS__);      \
        std::printf("  [%s]\n", #cond);         \
      }                                         \
    }                                           \
  } while (0)

template <typename I>
static void check_array(const std::vector<int64_t>& len, int64_t chunk) {
  const int64_t nseg = (int64_t)len.size();
  std::vector<I> ptr(nseg + 1, 0);
  for (int64_t r = 0; r < nseg; ++r) ptr[r + 1] = (I)(ptr[r] + len[r]);
  const int64_t nnz = (int64_t)ptr[nseg];
  const int64_t nwin = (nnz + chunk - 1) / chunk;
  ++g_arrays;

  for (int64_t pos = 0; pos < nnz; ++pos) {   // seg_of: the non-empty segment that holds pos
    int64_t want = 0;
    for (int64_t r = 0; r <= nseg; ++r)
      if ((int64_t)ptr[r] <= pos) want = r;
    const int64_t got = spamd::seg_of(ptr.data(), nseg, pos);
    CHECK(got == want, "seg_of pos %lld: got %lld want %lld\n", (long long)pos, (long long)got, (long long)want);
    CHECK(got < nseg && (int64_t)ptr[got] <= pos && pos < (int64_t)ptr[got + 1], "seg_of pos %lld: segment %lld does not hold it\n",
          (long long)pos, (long long)got);
  }

  std::vector<Piece> want;
  for (int64_t r = 0; r < nseg; ++r)
    if (len[r] > chunk)
      for (int64_t s = ptr[r]; s < (int64_t)ptr[r + 1]; s += chunk)
        want.push_back({r, (int64_t)ptr[r], s, s + chunk < (int64_t)ptr[r + 1] ? s + chunk : (int64_t)ptr[r + 1]});

  std::vector<int> slot_used(2 * nwin, 0), seen(want.size(), 0);
  for (int64_t g = 0; g < nwin; ++g) {
    int in_window = 0;
    int64_t last_slot = -1;
    spamd::seg_window_pieces(ptr.data(), nseg, nnz, chunk, g, [&](int64_t seg, int64_t b, int64_t s, int64_t e) {
      ++in_window;
      ++g_pieces;
      size_t w = 0;
      while (w < want.size() && !(want[w].seg == seg && want[w].s == s)) ++w;
      CHECK(w < want.size(), "window %lld: (seg %lld, start %lld) is no piece of a long segment\n", (long long)g, (long long)seg,
            (long long)s);
      if (w < want.size()) {
        CHECK(want[w].b == b && want[w].e == e, "piece (seg %lld, start %lld): b %lld e %lld, want b %lld e %lld\n", (long long)seg,
              (long long)s, (long long)b, (long long)e, (long long)want[w].b, (long long)want[w].e);
        CHECK(++seen[w] == 1, "piece (seg %lld, start %lld) found twice\n", (long long)seg, (long long)s);
      }
      const int64_t slot = spamd::seg_slot(b, s, chunk);
      CHECK(slot >= 0 && slot < 2 * nwin, "slot %lld outside [0, %lld)\n", (long long)slot, (long long)(2 * nwin));
      CHECK(slot / 2 == g, "slot %lld of a piece found by window %lld\n", (long long)slot, (long long)g);
      CHECK(slot > last_slot, "window %lld: slot %lld after slot %lld\n", (long long)g, (long long)slot, (long long)last_slot);
      last_slot = slot;
      if (slot >= 0 && slot < 2 * nwin) CHECK(++slot_used[slot] == 1, "slot %lld used twice\n", (long long)slot);
    });
    CHECK(in_window <= 2, "window %lld holds %d piece starts\n", (long long)g, in_window);
    if (in_window == 2) ++g_two;
  }
  for (size_t w = 0; w < want.size(); ++w)
    CHECK(seen[w] == 1, "piece (seg %lld, start %lld) of chunk %lld found %d times\n", (long long)want[w].seg, (long long)want[w].s,
          (long long)chunk, seen[w]);
}

static void check_both(const std::vector<int64_t>& len, int64_t chunk) {
  check_array<int32_t>(len, chunk);
  check_array<int64_t>(len, chunk);
}

int main() {
  const long two_before = g_two;
  check_both({3, 130, 70, 1, 200}, 64);
  if (g_two == two_before) {
    std::printf("FAIL: no window of the fixed array holds two piece starts\n");
    ++g_bad;
  }
  const int64_t chunks[3] = {64, 128, 192};
  for (int64_t chunk : chunks) {
    const int64_t menu[10] = {0, 1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 5};
    for (int nseg = 1; nseg <= 12; ++nseg) {
      for (int m = 0; m < 10; ++m) check_both(std::vector<int64_t>(nseg, menu[m]), chunk);   // every length by itself
      for (int trial = 0; trial < 300; ++trial) {
        std::vector<int64_t> len(nseg);
        for (int r = 0; r < nseg; ++r) {
          const uint64_t pick = next_random() % 11;
          len[r] = pick < 10 ? menu[pick] : (int64_t)(next_random() % (uint64_t)(5 * chunk));
        }
        check_both(len, chunk);
      }
    }
  }
  if (g_bad) {
    std::printf("FAILED: %ld checks\n", g_bad);
    return 1;
  }
  std::printf("OK: %ld pointer arrays, %ld pieces, %ld windows with two piece starts\n", g_arrays, g_pieces, g_two);
  return 0;
}

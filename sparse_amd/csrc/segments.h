// What the segment walkers - softmax (A14), sparse attention (A15, A16), the semiring products (A17, A18) and mttkrp (A12) -
// share beside the arithmetic of csrc/segment_walk.h: the wave's ballot over 64 segment lengths, the two joins in piece order,
// and the host side of a launch (grid size, sub-group dispatch, parameter check).  DESIGN.md "The shared segment walk".
#pragma once
#include "common.h"
#include "segment_walk.h"

#include <algorithm>

namespace spamd {

// the 64 segments from `base`, one per lane: f(src, b, n) - wave-uniform, all 64 lanes stay together - for every segment
// base + src (first position b, n elements) whose length satisfies pred(n)
// (ag_wide_kernel of csrc/attention_grad.hip keeps a loop of its own: its scalar file is full, see there)
template <typename I, typename P, typename F>
__device__ __forceinline__ void seg_wave_each(const I* __restrict__ ptr, int64_t nseg, int64_t base, int lane, P pred, F f) {
  const int64_t mine = base + lane;
  int64_t mb = 0, mn = 0;
  if (mine < nseg) {
    mb = (int64_t)ptr[mine];
    mn = (int64_t)ptr[mine + 1] - mb;
  }
  unsigned long long todo = __ballot(pred(mn));
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    f(src, wave_bcast(mb, src), wave_bcast(mn, src));
  }
}

// v(0) + v(1) + .. + v(np - 1) added one after the other in piece order, the first value being the start: 64 values at a
// time, one per lane, then broadcast.  Every lane returns the sum
template <typename T, typename V>
__device__ __forceinline__ T seg_join_sum(int64_t np, int lane, V v) {
#pragma clang fp contract(off)
  T s = T(0);
  for (int64_t k0 = 0; k0 < np; k0 += 64) {
    const int cnt = (int)(np - k0 < 64 ? np - k0 : 64);
    const T x = lane < cnt ? v(k0 + lane) : T(0);
    for (int u = 0; u < cnt; ++u) {
      const T pv = wave_bcast(x, u);
      s = (k0 + u == 0) ? pv : s + pv;
    }
  }
  return s;
}

// the piece rows (`pitch` values each, at the slots of csrc/segment_walk.h) of the segment of np pieces that starts at b,
// added one after the other in piece order, the first piece's row being the start: out(j, sum) for the columns j < width,
// lane u taking u, u + 64, ..
template <typename T, typename O>
__device__ __forceinline__ void seg_join_rows(const T* __restrict__ part, int64_t pitch, int64_t width, int64_t b, int64_t np,
                                              int64_t chunk, int lane, O out) {
#pragma clang fp contract(off)
  const int64_t slot0 = seg_slot(b, b, chunk);
  for (int64_t j = lane; j < width; j += 64) {
    T s = part[slot0 * pitch + j];
    for (int64_t k = 1; k < np; ++k) s = s + part[seg_slot(b, b + k * chunk, chunk) * pitch + j];
    out(j, s);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
inline unsigned seg_grid(int64_t items, int64_t per_block, int64_t cap = (int64_t)1 << 20) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), cap));
}

inline bool seg_group_ok(int group) { return group == 8 || group == 16 || group == 32 || group == 64; }

inline bool seg_chunk_ok(int64_t chunk, int64_t max_chunk) { return chunk >= 64 && chunk <= max_chunk && chunk % 64 == 0; }

inline bool seg_params_ok(int group, int64_t chunk, int64_t max_chunk, int64_t short_max) {
  return seg_group_ok(group) && seg_chunk_ok(chunk, max_chunk) && short_max >= 0 && short_max <= 64;
}

// the statement with G = the sub-group width `group` as a constant (8 | 16 | 32, 64 otherwise)
#define SEG_GROUP(group, G, ...)                                  \
  do {                                                            \
    if ((group) == 8) { constexpr int G = 8; __VA_ARGS__; }       \
    else if ((group) == 16) { constexpr int G = 16; __VA_ARGS__; } \
    else if ((group) == 32) { constexpr int G = 32; __VA_ARGS__; } \
    else { constexpr int G = 64; __VA_ARGS__; }                   \
  } while (0)

}  // namespace spamd

// The keep decision of attention dropout (A15 / A16), shared by csrc/attention.hip, csrc/attention_grad.hip and
// spamd_attention_keep: a counter-based generator, so that the decision is a pure function of (seed, head, stored position) -
// no state, no atomics, the same in every kernel form, launch geometry and mask format, recomputed by the backward pass.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library):
//   key      (seed low 32 bits, seed high 32 bits)
//   counter  (pos low, pos high, h low, h high): pos = the stored position in CSR order, s_ptr[r] + i; h = the head's number
//            in the flattened leading axes of the whole call (head0 + the head's index), both as 64-bit values
//   round    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by
//            (W0, W1) between rounds; ten rounds
// Only output word 0, x, is used: the element is kept iff x >= thr, thr = (uint32) floor(rate * 2^32) computed in double by
// the host (exact for 0 <= rate < 1).  The drop probability is thr / 2^32; rate = 0 keeps everything.
// tests/attention_dropout_cases.py restates this file; a change here is a change there.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attention_common.h"

namespace spamd {

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// word 0 of Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1)
__host__ __device__ __forceinline__ uint32_t philox4x32_10_x(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                             uint32_t c3) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return c0;
}

__host__ __device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t h, uint64_t pos, uint32_t thr) {
  return philox4x32_10_x((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pos, (uint32_t)(pos >> 32), (uint32_t)h,
                         (uint32_t)(h >> 32)) >= thr;
}

// thr of a rate in [0, 1): floor(rate * 2^32), the multiply exact in double
inline uint32_t dropout_threshold(double rate) { return (uint32_t)(rate * 4294967296.0); }

inline bool dropout_rate_ok(double rate) { return rate >= 0.0 && rate < 1.0; }   // (NaN fails both)

// the dropout argument of the A15 / A16 kernels: pd = keep ? p * c : +0.0 with c = (T)(1 / (1 - rate)), one multiply.
// `head0` is the number of the launch's first head in the whole call.  P = false is an empty argument: the kernels of the
// entries without dropout compile as before it existed
template <typename T, bool P>
struct AtDrop {
  uint64_t seed;
  uint64_t head0;
  uint32_t thr;
  T c;
  __device__ __forceinline__ bool keep(int64_t head, int64_t pos) const {
    return dropout_keep(seed, head0 + (uint64_t)head, (uint64_t)pos, thr);
  }
  __device__ __forceinline__ T mul(bool kept, T x) const {
#pragma clang fp contract(off)
    return kept ? x * c : T(0);
  }
};

template <typename T>
struct AtDrop<T, false> {
  __device__ __forceinline__ bool keep(int64_t, int64_t) const { return true; }
  __device__ __forceinline__ T mul(bool, T x) const { return x; }
};

// the bias and the dropout of one launch as ONE kernel argument: an empty base takes no room, so the argument block of a
// kernel without dropout is the one it had before dropout existed
template <typename T, bool B, bool P>
struct AtMods : AtBias<T, B>, AtDrop<T, P> {
  __host__ __device__ AtMods(const AtBias<T, B>& bz, const AtDrop<T, P>& dz) : AtBias<T, B>(bz), AtDrop<T, P>(dz) {}
};

}  // namespace spamd

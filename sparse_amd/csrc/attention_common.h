// Device helpers shared by csrc/attention.hip (A15) and csrc/attention_grad.hip (A16): the NaN-propagating maximum, the
// halving folds, the 64-accumulator dot product of four gathered rows and the four-rows-in-flight fma loops, so that both files
// compute the same bits from the same code.  csrc/softmax.hip (A14) and the semiring products (A17, A18) use the maximum and the
// folds too.  The segment walk of the piece forms is csrc/segments.h.
#pragma once
#include "segments.h"

#include <algorithm>
#include <limits>

#define ATTENTION_MAX_CHUNK 1024

namespace spamd {

template <typename T>
__device__ __forceinline__ T at_nmax(T a, T b) {   // NaN wins from either side
  return (a > b || a != a) ? a : b;
}

template <typename T, int W>
__device__ __forceinline__ T at_xmax(T m) {
#pragma unroll
  for (int h = W / 2; h >= 1; h /= 2) m = at_nmax(m, __shfl_xor(m, h, W));
  return m;
}

// a[l] = a[l] + a[l ^ h], h = W / 2 .. 1: every lane ends with the bits of the halving fold (the sum of two is commutative)
template <typename T, int W>
__device__ __forceinline__ T at_xsum(T s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int h = W / 2; h >= 1; h /= 2) s = s + __shfl_xor(s, h, W);
  return s;
}

template <typename T>
__device__ __forceinline__ T at_fma(T a, T b, T c) {
  if constexpr (sizeof(T) == 4) return __builtin_fmaf(a, b, c);
  else return __builtin_fma(a, b, c);
}

template <typename T>
__device__ __forceinline__ T at_neg_inf() {
  return -std::numeric_limits<T>::infinity();
}

// the additive per-element bias of A15 / A16: b[head * bh + pos] is added to the score of the stored (CSR) position pos, one add
// after the scale; bh = 0 shares one bias between the heads.  `db` (the backward pass only; may be null) takes z at
// db[head * nnz + pos].  B = false is an empty argument: the kernels of the entries without a bias compile as before it existed
template <typename T, bool B>
struct AtBias {
  const T* b;
  int64_t bh;
  T* db;
  __device__ __forceinline__ T add(T t, int64_t head, int64_t pos) const {
#pragma clang fp contract(off)
    return t + b[head * bh + pos];
  }
};

template <typename T>
struct AtBias<T, false> {
  __device__ __forceinline__ T add(T t, int64_t, int64_t) const { return t; }
};

// one block of 64 elements (from e0) of four dot products: a[e][m] = fma(q[l], k_e[l], a[e][m]) at l = e0 + sub + G m.  TAIL: the
// block may reach past D - such an element is read at D - 1 and not used (no branch around a load)
template <typename T, int G, bool TAIL>
__device__ __forceinline__ void at_dot4_block(const T* __restrict__ q, const T* __restrict__ k0, const T* __restrict__ k1,
                                              const T* __restrict__ k2, const T* __restrict__ k3, int D, int e0, int sub,
                                              T (&a)[4][64 / G]) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  constexpr int MB = sizeof(T) * V > 32 ? V / 2 : V;   // loads in flight per k row: at most 32 bytes a lane
#pragma unroll
  for (int m0 = 0; m0 < V; m0 += MB) {
    T qv[MB], kv[4][MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const int l = e0 + sub + G * (m0 + m);
      const int e = TAIL ? std::min(l, D - 1) : l;
      qv[m] = q[e];
      kv[0][m] = k0[e];
      kv[1][m] = k1[e];
      kv[2][m] = k2[e];
      kv[3][m] = k3[e];
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const bool in = !TAIL || e0 + sub + G * (m0 + m) < D;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const T f = at_fma(qv[m], kv[e][m], a[e][m0 + m]);
        a[e][m0 + m] = in ? f : a[e][m0 + m];
      }
    }
  }
}

// four dot products of the row `q` with the rows k0 .. k3 by a sub-group of G lanes (lane `sub`): every lane returns all four
template <typename T, int G>
__device__ __forceinline__ void at_dot4(const T* __restrict__ q, const T* __restrict__ k0, const T* __restrict__ k1,
                                        const T* __restrict__ k2, const T* __restrict__ k3, int D, int sub, T (&w)[4]) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  T a[4][V];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int m = 0; m < V; ++m) a[e][m] = T(0);
  int e0 = 0;
  for (; e0 + 64 <= D; e0 += 64) at_dot4_block<T, G, false>(q, k0, k1, k2, k3, D, e0, sub, a);
  if (e0 < D) at_dot4_block<T, G, true>(q, k0, k1, k2, k3, D, e0, sub, a);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int hv = V / 2; hv >= 1; hv /= 2)   // h = 32 .. G: both accumulators live in this lane
#pragma unroll
      for (int m = 0; m < hv; ++m) a[e][m] = a[e][m] + a[e][m + hv];
    w[e] = at_xsum<T, G>(a[e][0]);
  }
}

// acc[c] = fma(p_e, v_e[j], acc[c]) for e = 0 .. 3 in order, at the columns j = jb + sub + G c of this lane.  EDGE: fewer than
// four elements are live (`left`), or the block reaches past Dv - such a column is read at Dv - 1 and never stored
template <typename T, int G, bool EDGE>
__device__ __forceinline__ void at_out4(const T (&pp)[4], const T* const (&vr)[4], int jb, int sub, int Dv, int left,
                                        T (&acc)[64 / G]) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  constexpr int MB = sizeof(T) * V > 32 ? V / 2 : V;   // loads in flight per v row: at most 32 bytes a lane
#pragma unroll
  for (int c0 = 0; c0 < V; c0 += MB) {
    T vv[4][MB];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < MB; ++c) {
        const int j = jb + sub + G * (c0 + c);
        vv[e][c] = vr[e][EDGE ? std::min(j, Dv - 1) : j];
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool live = !EDGE || e < left;
#pragma unroll
      for (int c = 0; c < MB; ++c) {
        const T f = at_fma(pp[e], vv[e][c], acc[c0 + c]);
        acc[c0 + c] = live ? f : acc[c0 + c];
      }
    }
  }
}

// ---- the wave's output loop: acc = fma(p_i, v[c_i, j], acc), i ascending, from +0.0, for the column j of this lane -----------
// `p(i)` and `c(i)` give element i's probability and column to every lane (wave-uniform values)
template <typename T, typename P, typename C>
__device__ __forceinline__ T at_wave_out(const T* __restrict__ vh, int64_t vp, int j, bool live, int cnt, P p, C c) {
#pragma clang fp contract(off)
  T acc = T(0);
  for (int i = 0; i < cnt; i += 4) {
    T pp[4], vv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int src = i + e < cnt ? i + e : i;
      pp[e] = p(src);
      vv[e] = live ? vh[c(src) * vp + j] : T(0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < cnt) acc = at_fma(pp[e], vv[e], acc);
  }
  return acc;
}

}  // namespace spamd

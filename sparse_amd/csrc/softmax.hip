// A14  softmax over the stored elements of a sparse array: unstored positions count as minus infinity, the result keeps the
// stored structure.  The stored elements come grouped into segments: segptr[g] .. segptr[g + 1] are the positions of group g
// in plan order, perm[] maps a plan position to a stored position (NULL: the stored order is the plan order).
//
// Order (the contract tests/softmax_cases.py restates, bit for bit), for one group t_0 .. t_{n-1} in plan order
// (t_i = scale * x_i, one multiply, when a scale is given):
//   m    the maximum (exact; a NaN anywhere makes it NaN; the sign of a zero maximum changes no result)
//   d_i  = t_i - m
//   e_i  = exp_det(d_i)                                                         (csrc/exp_det.h)
//   s    the group is cut into pieces of `chunk` elements (a multiple of 64).  A piece is summed by 64 accumulators:
//        accumulator l adds the piece's elements l, l + 64, l + 128, .. in order; they are folded by halving,
//        a[l] = a[l] + a[l + h] for h = 32, 16, 8, 4, 2, 1.  The piece sums are added in piece order.  (An accumulator
//        without an element is +0.0, and x + +0.0 is exact for the x >= +0 and the NaN that occur.)
//   p_i  = e_i / s                                                              (one correctly rounded division)
// No atomics; every output is written once; neither `group`, `short_max`, `max_len` nor the launch geometry changes a bit.
// `chunk` is part of the order for the groups it cuts, and only for those: a group of at most `chunk` elements is one piece.
//
// Three forms, chosen per segment from its length n:
//   short  1 <= n <= short_max (<= 64): a sub-group of G = 8 | 16 | 32 | 64 lanes owns the group, lane u holds the elements
//          u, u + G, .. (64 / G registers): they ARE the 64 accumulators, so the first folds (h >= G) happen inside a lane
//          and the rest across lanes.  One read, one write.
//   wide   short_max < n <= chunk: a wave owns the group, 16 registers per lane hold it (chunk <= 1024).  Waves find their
//          groups by a ballot over 64 segment lengths.  One read, one write.
//   long   n > chunk: pieces of `chunk` elements, one wave each.  Wave g looks at the plan positions [g * chunk, (g + 1) *
//          chunk): at most two pieces of long groups START there (csrc/segment_walk.h has the argument) - workspace slots 2g and
//          2g + 1.  Five launches that each END before the next reads what it wrote - no workgroup waits for another:
//          piece maxima, group maxima, piece sums, group sums (sequential, piece order), outputs.  Three reads, one write.
#include "attention_common.h"
#include "exp_det.h"

#define SOFTMAX_MAX_CHUNK 1024

namespace spamd {

template <typename T>
struct SmIn {
  const T* x;
  const int64_t* perm;
  T scale;
  bool has_scale;
  __device__ __forceinline__ int64_t pos(int64_t q) const { return perm ? perm[q] : q; }
  __device__ __forceinline__ T at(int64_t p) const {
#pragma clang fp contract(off)
    const T v = x[p];
    return has_scale ? scale * v : v;
  }
};

// ---- short: a sub-group of G lanes per group ------------------------------------------------------------------------------
template <typename T, typename I, int G>
__global__ void __launch_bounds__(256)
sm_short_kernel(SmIn<T> in, int64_t nseg, const I* __restrict__ segptr, int64_t short_max, T* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  constexpr int GPB = 256 / G;
  const int sub = threadIdx.x % G;
  for (int64_t seg = (int64_t)blockIdx.x * GPB + threadIdx.x / G; seg < nseg; seg += (int64_t)gridDim.x * GPB) {
    const int64_t b = (int64_t)segptr[seg];
    const int64_t n = (int64_t)segptr[seg + 1] - b;
    if (n < 1 || n > short_max) continue;   // (the same in every lane of the sub-group)
    T t[V];
    int64_t p[V];
    T m = at_neg_inf<T>();
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = sub + j * G;
      p[j] = 0;
      t[j] = at_neg_inf<T>();
      if (q < n) {
        p[j] = in.pos(b + q);
        t[j] = in.at(p[j]);
        m = at_nmax(m, t[j]);
      }
    }
    m = at_xmax<T, G>(m);
    T a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      t[j] = sub + j * G < n ? exp_det(t[j] - m) : T(0);
      a[j] = t[j];
    }
#pragma unroll
    for (int hv = V / 2; hv >= 1; hv /= 2)   // h = 32 .. G: both accumulators live in this lane
#pragma unroll
      for (int j = 0; j < hv; ++j) a[j] = a[j] + a[j + hv];
    const T s = at_xsum<T, G>(a[0]);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (sub + j * G < n) out[p[j]] = t[j] / s;
  }
}

// ---- wide: a wave per group of at most SOFTMAX_MAX_CHUNK elements ----------------------------------------------------------
template <typename T>
__device__ __forceinline__ void sm_wave_group(const SmIn<T>& in, int64_t b, int64_t n, int lane, T* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int V = SOFTMAX_MAX_CHUNK / 64;
  T t[V];
  int64_t p[V];
  T m = at_neg_inf<T>();
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int q = lane + j * 64;
    p[j] = 0;
    t[j] = at_neg_inf<T>();
    if (q < n) {
      p[j] = in.pos(b + q);
      t[j] = in.at(p[j]);
      m = at_nmax(m, t[j]);
    }
  }
  m = at_xmax<T, 64>(m);
  T acc = T(0);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (lane + j * 64 < n) {
      t[j] = exp_det(t[j] - m);
      acc = acc + t[j];
    }
  }
  const T s = at_xsum<T, 64>(acc);
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (lane + j * 64 < n) out[p[j]] = t[j] / s;
}

template <typename T, typename I>
__global__ void __launch_bounds__(256)
sm_wide_kernel(SmIn<T> in, int64_t nseg, const I* __restrict__ segptr, int64_t above, int64_t upto, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < nseg; base += nwaves * 64)
    seg_wave_each(segptr, nseg, base, lane, [&](int64_t n) { return n > above && n <= upto; },
                  [&](int, int64_t b, int64_t n) { sm_wave_group<T>(in, b, n, lane, out); });
}

// ---- long: pieces ------------------------------------------------------------------------------------------------------------
// workspace: four arrays of 2 * nwin values - piece maxima, piece sums, group maxima and group sums (the last two at the
// slot of the group's first piece)
template <typename T, int PHASE>
__device__ __forceinline__ void sm_piece(const SmIn<T>& in, int64_t b, int64_t s, int64_t e, int64_t chunk, int64_t nwin,
                                         int lane, T* __restrict__ ws, T* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t slot = seg_slot(b, s, chunk), slot0 = seg_slot(b, b, chunk);
  if (PHASE == 0) {
    T m = at_neg_inf<T>();
    for (int64_t q = s + lane; q < e; q += 64) m = at_nmax(m, in.at(in.pos(q)));
    m = at_xmax<T, 64>(m);
    if (lane == 0) ws[slot] = m;
  } else if (PHASE == 1) {
    const T m = ws[4 * nwin + slot0];
    T acc = T(0);
    for (int64_t q = s + lane; q < e; q += 64) acc = acc + exp_det(in.at(in.pos(q)) - m);
    acc = at_xsum<T, 64>(acc);
    if (lane == 0) ws[2 * nwin + slot] = acc;
  } else {
    const T m = ws[4 * nwin + slot0], sum = ws[6 * nwin + slot0];
    for (int64_t q = s + lane; q < e; q += 64) {
      const int64_t p = in.pos(q);
      out[p] = exp_det(in.at(p) - m) / sum;
    }
  }
}

template <typename T, typename I, int PHASE>
__global__ void __launch_bounds__(256)
sm_piece_kernel(SmIn<T> in, int64_t nnz, int64_t nseg, const I* __restrict__ segptr, int64_t chunk, int64_t nwin,
                T* __restrict__ ws, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < nwin; g += (int64_t)gridDim.x * 4)
    seg_window_pieces(segptr, nseg, nnz, chunk, g, [&](int64_t, int64_t b, int64_t s, int64_t e) {
      sm_piece<T, PHASE>(in, b, s, e, chunk, nwin, lane, ws, out);
    });
}

// PHASE 0: group maxima from the piece maxima; PHASE 1: group sums, the piece sums added one after the other in piece order
template <typename T, typename I, int PHASE>
__global__ void __launch_bounds__(256)
sm_join_kernel(int64_t nseg, const I* __restrict__ segptr, int64_t chunk, int64_t nwin, T* __restrict__ ws) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < nseg; base += nwaves * 64)
    seg_wave_each(segptr, nseg, base, lane, [&](int64_t n) { return n > chunk; }, [&](int, int64_t b, int64_t n) {
      const int64_t np = (n + chunk - 1) / chunk;
      const int64_t slot0 = seg_slot(b, b, chunk);
      if (PHASE == 0) {
        T m = at_neg_inf<T>();
        for (int64_t k = lane; k < np; k += 64) m = at_nmax(m, ws[seg_slot(b, b + k * chunk, chunk)]);
        m = at_xmax<T, 64>(m);
        if (lane == 0) ws[4 * nwin + slot0] = m;
      } else {
        const T s = seg_join_sum<T>(np, lane, [&](int64_t k) { return ws[2 * nwin + seg_slot(b, b + k * chunk, chunk)]; });
        if (lane == 0) ws[6 * nwin + slot0] = s;
      }
    });
}

template <typename T, typename I>
static int softmax_typed(int64_t nseg, int64_t nnz, const void* segptr_, const int64_t* perm, const void* x, int has_scale,
                         double scale, int group, int64_t short_max, int64_t chunk, int64_t max_len, void* ws_, void* out_,
                         hipStream_t st) {
  const I* segptr = (const I*)segptr_;
  T* ws = (T*)ws_;
  T* out = (T*)out_;
  SmIn<T> in{(const T*)x, perm, (T)scale, has_scale != 0};
  const dim3 wg(256);
  if (short_max > 0)
    SEG_GROUP(group, G, SPAMD_LAUNCH((sm_short_kernel<T, I, G>), dim3(seg_grid(nseg, 256 / G)), wg, 0, st, in, nseg, segptr, short_max, out));
  if (std::min(max_len, chunk) > short_max)
    SPAMD_LAUNCH((sm_wide_kernel<T, I>), dim3(seg_grid(nseg, 256)), wg, 0, st, in, nseg, segptr, short_max, chunk, out);
  if (max_len > chunk) {
    const int64_t nwin = ceil_div(nnz, chunk);
    const dim3 pg(seg_grid(nwin, 4)), jg(seg_grid(nseg, 256));
    SPAMD_LAUNCH((sm_piece_kernel<T, I, 0>), pg, wg, 0, st, in, nnz, nseg, segptr, chunk, nwin, ws, out);
    SPAMD_LAUNCH((sm_join_kernel<T, I, 0>), jg, wg, 0, st, nseg, segptr, chunk, nwin, ws);
    SPAMD_LAUNCH((sm_piece_kernel<T, I, 1>), pg, wg, 0, st, in, nnz, nseg, segptr, chunk, nwin, ws, out);
    SPAMD_LAUNCH((sm_join_kernel<T, I, 1>), jg, wg, 0, st, nseg, segptr, chunk, nwin, ws);
    SPAMD_LAUNCH((sm_piece_kernel<T, I, 2>), pg, wg, 0, st, in, nnz, nseg, segptr, chunk, nwin, ws, out);
  }
  return 0;
}

}  // namespace spamd

using namespace spamd;

extern "C" int64_t spamd_softmax_ws_bytes(int val_dtype, int64_t nnz, int64_t chunk) {
  const int64_t esz = val_dtype == SPAMD_F32 ? 4 : (val_dtype == SPAMD_F64 ? 8 : 0);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || !seg_chunk_ok(chunk, SOFTMAX_MAX_CHUNK)) return SPAMD_EINVAL;
  if (nnz <= chunk) return 0;
  return 8 * ceil_div(nnz, chunk) * esz;
}

extern "C" int spamd_softmax(int val_dtype, int idx_dtype, int64_t nseg, int64_t nnz, const void* segptr, const int64_t* perm,
                             const void* x, int has_scale, double scale, int group, int64_t short_max, int64_t chunk,
                             int64_t max_len, void* ws, int64_t ws_bytes, void* out, void* stream) {
  if (val_dtype != SPAMD_F32 && val_dtype != SPAMD_F64) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (nseg < 0 || nnz < 0 || max_len < 0 || max_len > nnz) return SPAMD_EINVAL;
  if (!seg_params_ok(group, chunk, SOFTMAX_MAX_CHUNK, short_max)) return SPAMD_EINVAL;
  if (nseg == 0 || nnz == 0 || max_len == 0) return 0;
  if (!segptr || !x || !out || out == x) return SPAMD_EINVAL;
  if (max_len > chunk && (!ws || ws_bytes < spamd_softmax_ws_bytes(val_dtype, nnz, chunk))) return SPAMD_EWS;
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (val_dtype == SPAMD_F32)
      return softmax_typed<float, I>(nseg, nnz, segptr, perm, x, has_scale, scale, group, short_max, chunk, max_len, ws, out, st);
    return softmax_typed<double, I>(nseg, nnz, segptr, perm, x, has_scale, scale, group, short_max, chunk, max_len, ws, out, st);
  })
  return SPAMD_ETYPE;
}

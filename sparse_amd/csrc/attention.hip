// A15  sparse attention: for every head, out = softmax_over_stored(scale * (s (.) (q k^T))) @ v over the stored positions of a
// 2-D mask s (M x N, CSR: ptr, idx, sv), fused - the SDDMM scores, the softmax of A14 and the SpMM by v in one pass over the
// mask, the scores never written (rows of at most `chunk` elements).  q (H, M, D), k (H, N, D), v (H, N, Dv) are dense with
// a row pitch and a head stride each (last axis contiguous); out is (H, M, Dv), contiguous.  Every head reads the same mask.
//
// Order (the contract tests/attention_cases.py restates, bit for bit; include/sparse_amd.h A15), for row r of one head with
// stored elements i = 0 .. n-1 in stored order and columns c_i:
//   w_i  = dot(q[r], k[c_i]) by 64 accumulators: accumulator l starts at +0.0 and takes a_l = fma(q[l + 64 j], k[c_i][l + 64 j],
//          a_l) for j ascending (an element past D contributes nothing); folded by halving, a[l] = a[l] + a[l + h], h = 32 .. 1
//   t_i  = s_i * w_i (one multiply);  t_i = scale * t_i (one more) when a scale is given;  t_i = t_i + b_i (one add, after the
//          scale) when a bias is given (spamd_attention_bias; B of AtBias<T, B>: the kernels without one compile as before it existed)
//   p_i  = A14's softmax of t_0 .. t_{n-1} (maximum first, exp_det, 64 accumulators per piece of `chunk`, one division)
//   pd_i = keep_i ? p_i * c : +0.0 with dropout (spamd_attention_dropout; P of AtDrop<T, P>, csrc/attention_dropout.h): c =
//          (T)(1 / (1 - rate)), keep_i from (seed, head, stored position); it takes the place of p_i below, a dropped element as +0.0
//   out[r, j]: the elements are cut into pieces of `chunk`; a piece starts at +0.0 and takes acc = fma(p_i, v[c_i, j], acc) for
//          i ascending; the piece sums are added in piece order (the first piece's sum is the start).  An empty row is +0.0.
// No atomics; every output is written once; neither `group`, `short_max`, `max_len` nor the launch geometry changes a bit.
//
// Three forms, chosen per row from its length n:
//   short  0 <= n <= short_max (<= 64): a sub-group of G = 8 | 16 | 32 | 64 lanes owns (row, head).  The lanes run along D for
//          the dot products - lane u holds the accumulators u, u + G, .. (64 / G registers), four elements at a time so that
//          their k rows are in flight together -, the score of element i lands in lane i mod G, register i / G, where A14's
//          short form finds it; then the lanes run along Dv, p_i and c_i broadcast by shuffle, four v rows in flight.
//   wide   short_max < n <= chunk: a wave (a workgroup of its own) per (row, head); the scores are parked in LDS (chunk values),
//          A14's wide form runs over them in place, then the same output loop.
//   long   n > chunk: unfused through the workspace, in pieces of `chunk` elements found by windows (csrc/segment_walk.h).
//          Six launches that each END before the next reads what it wrote: piece scores and maxima, row maxima, piece sums,
//          row sums (piece order), piece outputs, row outputs (piece order).
#include "attention_common.h"
#include "attention_dropout.h"
#include "exp_det.h"

namespace spamd {

template <typename T, typename I>
struct AtIn {
  const I* ptr;
  const I* idx;
  const T* sv;
  const T* q;
  const T* k;
  const T* v;
  int64_t qp, qh, kp, kh, vp, vh;   // row pitch and head stride, in elements
  int64_t M, H;   // H: heads of this launch (at most 65535: grid.y), the host offsets the pointers for more
  int D, Dv;
  T scale;
  bool has_scale;
  T* out;
  __device__ __forceinline__ T score(T s, T w) const {
#pragma clang fp contract(off)
    const T t = s * w;
    return has_scale ? scale * t : t;
  }
};

// ---- short: a sub-group of G lanes per (row, head) ----------------------------------------------------------------------------
// (P: with dropout - spamd_attention_dropout; P = false compiles as before it existed, AtDrop<T, false> being an empty argument)
template <typename T, typename I, int G, bool B, bool P>
__global__ void __launch_bounds__(256)
at_short_kernel(AtIn<T, I> in, int64_t short_max, AtMods<T, B, P> mz) {
#pragma clang fp contract(off)
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  constexpr int V = 64 / G;
  constexpr int GPB = 256 / G;
  const int sub = threadIdx.x % G;
  {
    const int64_t head = blockIdx.y;
    const T* __restrict__ kh = in.k + head * in.kh;
    const T* __restrict__ vh = in.v + head * in.vh;
    for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < in.M; row += (int64_t)gridDim.x * GPB) {
      const int64_t b = (int64_t)in.ptr[row];
      const int n = (int)std::min<int64_t>((int64_t)in.ptr[row + 1] - b, 65);
      if (n > short_max) continue;   // (the same in every lane of the sub-group)
      const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
      T t[V], sv[V];
      int64_t col[V];
#pragma unroll
      for (int r = 0; r < V; ++r) {
        const int i = sub + r * G;
        col[r] = 0;
        sv[r] = T(0);
        t[r] = at_neg_inf<T>();
        if (i < n) {
          col[r] = (int64_t)in.idx[b + i];
          sv[r] = in.sv[b + i];
          if constexpr (B) t[r] = bz.b[head * bz.bh + b + i];   // the bias waits where its score will land
        }
      }
      // phase 1: the scores, four elements at a time; r is unrolled so that no register array is indexed
#pragma unroll
      for (int r = 0; r < V; ++r) {
        const int cnt = n - r * G;   // elements of register r: the lanes 0 .. min(cnt, G) - 1
        for (int ii = 0; ii < G && ii < cnt; ii += 4) {
          const T* kr[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) kr[e] = kh + __shfl(col[r], ii + e < cnt ? ii + e : ii, G) * in.kp;
          T w[4];
          at_dot4<T, G>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, sub, w);
          T mine = w[0];
#pragma unroll
          for (int e = 1; e < 4; ++e) mine = sub == ii + e ? w[e] : mine;
          mine = in.score(sv[r], mine);
          if constexpr (B) mine = mine + t[r];   // (every live lane passes here once: t[r] is still its bias)
          t[r] = sub >= ii && sub < ii + 4 && sub < cnt ? mine : t[r];   // the lanes that hold these four elements
        }
      }
      // phase 2: A14's short form on the registers
      T m = at_neg_inf<T>();
#pragma unroll
      for (int r = 0; r < V; ++r)
        if (sub + r * G < n) m = at_nmax(m, t[r]);
      m = at_xmax<T, G>(m);
      T a[V];
#pragma unroll
      for (int r = 0; r < V; ++r) {
        t[r] = sub + r * G < n ? exp_det(t[r] - m) : T(0);
        a[r] = t[r];
      }
#pragma unroll
      for (int hv = V / 2; hv >= 1; hv /= 2)
#pragma unroll
        for (int r = 0; r < hv; ++r) a[r] = a[r] + a[r + hv];
      const T s = at_xsum<T, G>(a[0]);
#pragma unroll
      for (int r = 0; r < V; ++r) t[r] = t[r] / s;
      if constexpr (P) {   // pd_i = keep_i ? p_i * c : +0.0: t holds pd from here on
#pragma unroll
        for (int r = 0; r < V; ++r)
          if (sub + r * G < n) t[r] = dz.mul(dz.keep(head, b + sub + r * G), t[r]);
      }
      // phase 3: the output row, 64 columns at a time (lane u: the columns u, u + G, ..), four v rows in flight
      T* __restrict__ orow = in.out + (head * in.M + row) * in.Dv;
      for (int jb = 0; jb < in.Dv; jb += 64) {
        T acc[V];
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = T(0);
#pragma unroll
        for (int r = 0; r < V; ++r) {
          const int cnt = n - r * G;
          for (int ii = 0; ii < G && ii < cnt; ii += 4) {
            T pp[4];
            const T* vr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int src = ii + e < cnt ? ii + e : ii;
              pp[e] = __shfl(t[r], src, G);
              vr[e] = vh + __shfl(col[r], src, G) * in.vp;
            }
            if (ii + 4 <= cnt && jb + 64 <= in.Dv) at_out4<T, G, false>(pp, vr, jb, sub, in.Dv, cnt - ii, acc);
            else at_out4<T, G, true>(pp, vr, jb, sub, in.Dv, cnt - ii, acc);
          }
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const int j = jb + sub + G * c;
          if (j < in.Dv) orow[j] = acc[c];
        }
      }
    }
  }
}

// ---- wide: a wave (one workgroup) per (row, head), the scores in LDS ------------------------------------------------------------
template <typename T, typename I, bool B, bool P>
__global__ void __launch_bounds__(64)
at_wide_kernel(AtIn<T, I> in, int64_t above, int64_t upto, AtMods<T, B, P> mz) {
#pragma clang fp contract(off)
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  extern __shared__ __attribute__((aligned(16))) unsigned char at_smem[];
  T* __restrict__ lds = reinterpret_cast<T*>(at_smem);   // `upto` values
  const int lane = threadIdx.x;
  {
    const int64_t head = blockIdx.y;
    const T* __restrict__ kh = in.k + head * in.kh;
    const T* __restrict__ vh = in.v + head * in.vh;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < in.M; base += (int64_t)gridDim.x * 64)
      seg_wave_each(in.ptr, in.M, base, lane, [&](int64_t len) { return len > above && len <= upto; }, [&](int src, int64_t b, int64_t len) {
        const int64_t row = base + src;
        const int n = (int)len;
        const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
        const I* __restrict__ idx = in.idx + b;
        for (int i = 0; i < n; i += 4) {
          const T* kr[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) kr[e] = kh + (int64_t)idx[i + e < n ? i + e : i] * in.kp;
          T w[4];
          at_dot4<T, 64>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, lane, w);
          if (lane == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (i + e < n) lds[i + e] = bz.add(in.score(in.sv[b + i + e], w[e]), head, b + i + e);
          }
        }
        __syncthreads();
        // A14's wide form: lane u owns the elements u, u + 64, ..
        T m = at_neg_inf<T>();
        for (int x = lane; x < n; x += 64) m = at_nmax(m, lds[x]);
        m = at_xmax<T, 64>(m);
        T acc = T(0);
        for (int x = lane; x < n; x += 64) {
          const T e = exp_det(lds[x] - m);
          lds[x] = e;
          acc = acc + e;
        }
        const T s = at_xsum<T, 64>(acc);
        for (int x = lane; x < n; x += 64) lds[x] = dz.mul(dz.keep(head, b + x), lds[x] / s);
        __syncthreads();
        T* __restrict__ orow = in.out + (head * in.M + row) * in.Dv;
        for (int jb = 0; jb < in.Dv; jb += 64) {
          const int j = jb + lane;
          const T o = at_wave_out<T>(vh, in.vp, j, j < in.Dv, n, [&](int x) { return lds[x]; },
                                     [&](int x) { return (int64_t)idx[x]; });
          if (j < in.Dv) orow[j] = o;
        }
        __syncthreads();   // the next row writes the scores again
      });
  }
}

// ---- long: pieces ------------------------------------------------------------------------------------------------------------------
// workspace of one head, in values: the scores (nnz, at stored positions), four arrays of 2 * nwin - piece maxima, piece sums,
// row maxima and row sums (the last two at the slot of the row's first piece) -, the piece outputs (2 * nwin rows of Dv)
__host__ __device__ __forceinline__ int64_t at_ws_values(int64_t nnz, int64_t nwin, int64_t Dv) {
  return nnz + 8 * nwin + 2 * nwin * Dv;
}

template <typename T, typename I, int PHASE, bool B, bool P>
__device__ __forceinline__ void at_piece(const AtIn<T, I>& in, const AtBias<T, B>& bz, const AtDrop<T, P>& dz, int64_t head, int64_t row, int64_t b, int64_t s, int64_t e,
                                         int64_t chunk, int64_t nnz, int64_t nwin, int lane, T* __restrict__ ws) {
#pragma clang fp contract(off)
  T* __restrict__ sc = ws;
  T* __restrict__ st = ws + nnz;
  T* __restrict__ part = ws + nnz + 8 * nwin;
  const int64_t slot = seg_slot(b, s, chunk), slot0 = seg_slot(b, b, chunk);
  if (PHASE == 0) {
    const T* __restrict__ kh = in.k + head * in.kh;
    const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
    T m = at_neg_inf<T>();
    for (int64_t x = s; x < e; x += 4) {
      const T* kr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kr[u] = kh + (int64_t)in.idx[x + u < e ? x + u : x] * in.kp;
      T w[4];
      at_dot4<T, 64>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, lane, w);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (x + u < e) {
          const T t = bz.add(in.score(in.sv[x + u], w[u]), head, x + u);
          m = at_nmax(m, t);
          if (lane == 0) sc[x + u] = t;
        }
      }
    }
    if (lane == 0) st[slot] = m;
  } else if (PHASE == 1) {
    const T m = st[4 * nwin + slot0];
    T acc = T(0);
    for (int64_t x = s + lane; x < e; x += 64) acc = acc + exp_det(sc[x] - m);
    acc = at_xsum<T, 64>(acc);
    if (lane == 0) st[2 * nwin + slot] = acc;
  } else {
    const T* __restrict__ vh = in.v + head * in.vh;
    const T m = st[4 * nwin + slot0], sum = st[6 * nwin + slot0];
    for (int jb = 0; jb < in.Dv; jb += 64) {
      const int j = jb + lane;
      const bool live = j < in.Dv;
      T acc = T(0);
      for (int64_t x0 = s; x0 < e; x0 += 64) {   // 64 probabilities, one per lane, then broadcast one after the other
        const int cnt = (int)std::min<int64_t>(e - x0, 64);
        T p = T(0);
        int64_t c = 0;
        if (lane < cnt) {
          p = dz.mul(dz.keep(head, x0 + lane), exp_det(sc[x0 + lane] - m) / sum);   // (the decision is made here, where the piece outputs are formed)
          c = (int64_t)in.idx[x0 + lane];
        }
        for (int i = 0; i < cnt; i += 4) {
          T pp[4], vv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int src = i + u < cnt ? i + u : i;
            pp[u] = wave_bcast(p, src);
            vv[u] = live ? vh[wave_bcast(c, src) * in.vp + j] : T(0);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (i + u < cnt) acc = at_fma(pp[u], vv[u], acc);
        }
      }
      if (live) part[slot * (int64_t)in.Dv + j] = acc;
    }
  }
}

// (P: the piece outputs, PHASE 2, with dropout; the scores, maxima and sums before them do not see it)
template <typename T, typename I, int PHASE, bool B, bool P>
__global__ void __launch_bounds__(256)
at_piece_kernel(AtIn<T, I> in, int64_t nnz, int64_t chunk, int64_t nwin, T* __restrict__ ws_all, AtMods<T, B, P> mz) {
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  const int lane = threadIdx.x & 63;
  const int64_t M = in.M;
  {
    const int64_t head = blockIdx.y;
    T* __restrict__ ws = ws_all + head * at_ws_values(nnz, nwin, in.Dv);
    for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < nwin; g += (int64_t)gridDim.x * 4)
      seg_window_pieces(in.ptr, M, nnz, chunk, g, [&](int64_t row, int64_t b, int64_t s, int64_t e) {
        at_piece<T, I, PHASE, B, P>(in, bz, dz, head, row, b, s, e, chunk, nnz, nwin, lane, ws);
      });
  }
}

// PHASE 0: row maxima from the piece maxima; PHASE 1: row sums, the piece sums added one after the other in piece order;
// PHASE 2: output rows, the piece outputs added one after the other in piece order
template <typename T, typename I, int PHASE>
__global__ void __launch_bounds__(256)
at_join_kernel(AtIn<T, I> in, int64_t nnz, int64_t chunk, int64_t nwin, T* __restrict__ ws_all) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  {
    const int64_t head = blockIdx.y;
    T* __restrict__ st = ws_all + head * at_ws_values(nnz, nwin, in.Dv) + nnz;
    const T* __restrict__ part = st + 8 * nwin;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < in.M; base += nwaves * 64)
      seg_wave_each(in.ptr, in.M, base, lane, [&](int64_t len) { return len > chunk; }, [&](int src, int64_t b, int64_t n) {
        const int64_t np = (n + chunk - 1) / chunk;
        const int64_t slot0 = seg_slot(b, b, chunk);
        if (PHASE == 0) {
          T m = at_neg_inf<T>();
          for (int64_t k = lane; k < np; k += 64) m = at_nmax(m, st[seg_slot(b, b + k * chunk, chunk)]);
          m = at_xmax<T, 64>(m);
          if (lane == 0) st[4 * nwin + slot0] = m;
        } else if (PHASE == 1) {
          const T s = seg_join_sum<T>(np, lane, [&](int64_t k) { return st[2 * nwin + seg_slot(b, b + k * chunk, chunk)]; });
          if (lane == 0) st[6 * nwin + slot0] = s;
        } else {
          T* __restrict__ orow = in.out + (head * in.M + base + src) * in.Dv;
          seg_join_rows(part, in.Dv, in.Dv, b, np, chunk, lane, [&](int64_t j, T s) { orow[j] = s; });
        }
      });
  }
}

template <typename T, typename I, bool B, bool P>
static int attention_typed(AtIn<T, I> in, AtBias<T, B> bz, AtDrop<T, P> dz, int64_t nnz, int group, int64_t short_max, int64_t chunk,
                           int64_t max_len, void* ws_, hipStream_t st) {
  const unsigned gy = (unsigned)in.H;
  const dim3 wg(256);
  // (always: the rows without a stored element are written here)
  SEG_GROUP(group, G, SPAMD_LAUNCH((at_short_kernel<T, I, G, B, P>), dim3(seg_grid(in.M, 256 / G), gy), wg, 0, st, in, short_max, AtMods<T, B, P>(bz, dz)));
  if (std::min(max_len, chunk) > short_max)
    SPAMD_LAUNCH((at_wide_kernel<T, I, B, P>), dim3(seg_grid(in.M, 64), gy), dim3(64), (size_t)chunk * sizeof(T), st, in, short_max, chunk,
                 AtMods<T, B, P>(bz, dz));
  if (max_len > chunk) {
    T* ws = (T*)ws_;
    const int64_t nwin = ceil_div(nnz, chunk);
    const dim3 pg(seg_grid(nwin, 4), gy), jg(seg_grid(in.M, 256), gy);
    const AtBias<T, false> nob{};   // the biased scores are in the workspace from here on
    const AtDrop<T, false> nod{};   // only the piece outputs see dropout
    SPAMD_LAUNCH((at_piece_kernel<T, I, 0, B, false>), pg, wg, 0, st, in, nnz, chunk, nwin, ws, AtMods<T, B, false>(bz, nod));
    SPAMD_LAUNCH((at_join_kernel<T, I, 0>), jg, wg, 0, st, in, nnz, chunk, nwin, ws);
    SPAMD_LAUNCH((at_piece_kernel<T, I, 1, false, false>), pg, wg, 0, st, in, nnz, chunk, nwin, ws, AtMods<T, false, false>(nob, nod));
    SPAMD_LAUNCH((at_join_kernel<T, I, 1>), jg, wg, 0, st, in, nnz, chunk, nwin, ws);
    SPAMD_LAUNCH((at_piece_kernel<T, I, 2, false, P>), pg, wg, 0, st, in, nnz, chunk, nwin, ws, AtMods<T, false, P>(nob, dz));
    SPAMD_LAUNCH((at_join_kernel<T, I, 2>), jg, wg, 0, st, in, nnz, chunk, nwin, ws);
  }
  return 0;
}

struct AtArgs {
  int64_t M, nnz, H, D, Dv;
  const void *ptr, *idx, *sv, *q, *k, *v;
  int64_t qp, qh, kp, kh, vp, vh;
  int has_scale;
  double scale;
  int group;
  int64_t short_max, chunk, max_len;
  const void* bias;
  int64_t bias_head;
  double rate;   // 0: no dropout - the kernels of spamd_attention / spamd_attention_bias
  uint64_t seed;
  int64_t head0;
  void *ws, *out;
};

template <typename T, typename I>
static int attention_in(const AtArgs& a, hipStream_t st) {
  const int64_t ws_head = a.max_len > a.chunk ? at_ws_values(a.nnz, ceil_div(a.nnz, a.chunk), a.Dv) : 0;
  for (int64_t h0 = 0; h0 < a.H; h0 += 65535) {   // a head per grid.y: at most 65535 of them in one launch
    AtIn<T, I> in{(const I*)a.ptr, (const I*)a.idx, (const T*)a.sv, (const T*)a.q + h0 * a.qh, (const T*)a.k + h0 * a.kh,
                  (const T*)a.v + h0 * a.vh, a.qp, a.qh, a.kp, a.kh, a.vp, a.vh, a.M, std::min<int64_t>(a.H - h0, 65535), (int)a.D,
                  (int)a.Dv, (T)a.scale, a.has_scale != 0, (T*)a.out + h0 * a.M * a.Dv};
    T* wsh = a.ws ? (T*)a.ws + h0 * ws_head : nullptr;
    const AtBias<T, true> bz{(const T*)a.bias + h0 * a.bias_head, a.bias_head, nullptr};
    // (the head's number goes on across the launches: head 65535 does not repeat head 0's decisions)
    const AtDrop<T, true> dz{a.seed, (uint64_t)a.head0 + (uint64_t)h0, dropout_threshold(a.rate), (T)(1.0 / (1.0 - a.rate))};
    int rc;
    if (a.rate > 0.0) {
      if (a.bias) rc = attention_typed<T, I, true, true>(in, bz, dz, a.nnz, a.group, a.short_max, a.chunk, a.max_len, wsh, st);
      else rc = attention_typed<T, I, false, true>(in, AtBias<T, false>{}, dz, a.nnz, a.group, a.short_max, a.chunk, a.max_len, wsh, st);
    } else {
      const AtDrop<T, false> nod{};
      if (a.bias) rc = attention_typed<T, I, true, false>(in, bz, nod, a.nnz, a.group, a.short_max, a.chunk, a.max_len, wsh, st);
      else rc = attention_typed<T, I, false, false>(in, AtBias<T, false>{}, nod, a.nnz, a.group, a.short_max, a.chunk, a.max_len, wsh, st);
    }
    if (rc) return rc;
  }
  return 0;
}

// out[h * nnz + p] = keep(seed, head0 + h, pos0 + p): the decisions by themselves (spamd_attention_keep)
__global__ void __launch_bounds__(256)
at_keep_kernel(int64_t nnz, int64_t total, uint64_t pos0, uint64_t head0, uint64_t seed, uint32_t thr, uint8_t* __restrict__ out) {
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (int64_t)gridDim.x * 256) {
    const int64_t h = x / nnz, p = x - h * nnz;
    out[x] = dropout_keep(seed, head0 + (uint64_t)h, pos0 + (uint64_t)p, thr) ? 1 : 0;
  }
}

}  // namespace spamd

using namespace spamd;

extern "C" int64_t spamd_attention_ws_bytes(int val_dtype, int64_t nnz, int64_t H, int64_t Dv, int64_t chunk) {
  const int64_t esz = val_dtype == SPAMD_F32 ? 4 : (val_dtype == SPAMD_F64 ? 8 : 0);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || H < 0 || Dv < 0 || !seg_chunk_ok(chunk, ATTENTION_MAX_CHUNK)) return SPAMD_EINVAL;
  if (nnz <= chunk) return 0;
  return H * at_ws_values(nnz, ceil_div(nnz, chunk), Dv) * esz;
}

// the entry with dropout on the probabilities: pd_i = keep_i ? p_i * c : +0.0 takes the place of p_i in the output loop, c =
// (T)(1 / (1 - rate)), keep_i decided by csrc/attention_dropout.h from (seed, head0 + head, stored position).  rate = 0 is
// spamd_attention_bias (the same kernels); bias = NULL is no bias.  The workspace is that of spamd_attention_ws_bytes
extern "C" int spamd_attention_dropout(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                                       const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch,
                                       int64_t q_head, const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                                       int64_t v_head, int has_scale, double scale, int group, int64_t short_max, int64_t chunk,
                                       int64_t max_len, const void* bias, int64_t bias_head, double rate, int64_t seed, int64_t head0,
                                       void* ws, int64_t ws_bytes, void* out, void* stream) {
  if (val_dtype != SPAMD_F32 && val_dtype != SPAMD_F64) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (M < 0 || N < 0 || nnz < 0 || H < 0 || D < 0 || Dv < 0 || max_len < 0 || max_len > nnz) return SPAMD_EINVAL;
  if (D > INT32_MAX - 128 || Dv > INT32_MAX - 128) return SPAMD_EINVAL;   // (row widths are 32-bit in the kernels)
  if (q_pitch < 0 || q_head < 0 || k_pitch < 0 || k_head < 0 || v_pitch < 0 || v_head < 0) return SPAMD_EINVAL;
  if (bias_head < 0) return SPAMD_EINVAL;
  if (!dropout_rate_ok(rate) || head0 < 0) return SPAMD_EINVAL;
  if (!seg_params_ok(group, chunk, ATTENTION_MAX_CHUNK, short_max)) return SPAMD_EINVAL;
  if (M == 0 || H == 0 || Dv == 0) return 0;
  if (!out || !s_ptr) return SPAMD_EINVAL;
  if (nnz > 0 && (!s_idx || !s_val || !k || !v || (D > 0 && !q))) return SPAMD_EINVAL;
  if (max_len > chunk && (!ws || ws_bytes < spamd_attention_ws_bytes(val_dtype, nnz, H, Dv, chunk))) return SPAMD_EWS;
  const AtArgs a{M, nnz, H, D, Dv, s_ptr, s_idx, s_val, q, k, v, q_pitch, q_head, k_pitch, k_head, v_pitch, v_head, has_scale, scale,
                 group, short_max, chunk, max_len, bias, bias_head, rate, (uint64_t)seed, head0, ws, out};
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (val_dtype == SPAMD_F32) return attention_in<float, I>(a, st);
    return attention_in<double, I>(a, st);
  })
  return SPAMD_ETYPE;
}

// the entry with an additive bias: b[head * bias_head + pos] (in elements; bias_head = 0: one bias for every head) is added to
// the score of the stored position pos after the scale.  bias = NULL is spamd_attention
extern "C" int spamd_attention_bias(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                                    const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch,
                                    int64_t q_head, const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                                    int64_t v_head, int has_scale, double scale, int group, int64_t short_max, int64_t chunk,
                                    int64_t max_len, const void* bias, int64_t bias_head, void* ws, int64_t ws_bytes, void* out,
                                    void* stream) {
  return spamd_attention_dropout(val_dtype, idx_dtype, M, N, nnz, H, D, Dv, s_ptr, s_idx, s_val, q, q_pitch, q_head, k, k_pitch, k_head,
                                 v, v_pitch, v_head, has_scale, scale, group, short_max, chunk, max_len, bias, bias_head, 0.0, 0, 0, ws,
                                 ws_bytes, out, stream);
}

extern "C" int spamd_attention(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                               const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch,
                               int64_t q_head, const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                               int64_t v_head, int has_scale, double scale, int group, int64_t short_max, int64_t chunk,
                               int64_t max_len, void* ws, int64_t ws_bytes, void* out, void* stream) {
  return spamd_attention_bias(val_dtype, idx_dtype, M, N, nnz, H, D, Dv, s_ptr, s_idx, s_val, q, q_pitch, q_head, k, k_pitch, k_head,
                              v, v_pitch, v_head, has_scale, scale, group, short_max, chunk, max_len, nullptr, 0, ws, ws_bytes, out,
                              stream);
}

// the keep decisions by themselves, from the device helper the attention kernels call: out[h * nnz + p] = 1 when the stored
// position pos0 + p of head head0 + h is kept at `rate` under `seed`, else 0 (h < H, p < nnz)
extern "C" int spamd_attention_keep(int64_t nnz, int64_t H, int64_t pos0, int64_t head0, double rate, int64_t seed, uint8_t* out,
                                    void* stream) {
  if (nnz < 0 || H < 0 || pos0 < 0 || head0 < 0 || !dropout_rate_ok(rate)) return SPAMD_EINVAL;
  if (nnz == 0 || H == 0) return 0;
  if (H > INT64_MAX / nnz || !out) return SPAMD_EINVAL;
  const int64_t total = nnz * H;
  SPAMD_LAUNCH(at_keep_kernel, dim3(seg_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, nnz, total, (uint64_t)pos0, (uint64_t)head0,
               (uint64_t)seed, dropout_threshold(rate), out);
  return 0;
}

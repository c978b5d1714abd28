// A16  the backward pass of sparse attention (A15): from g = d loss / d out, for every head, dq (H, M, D), dk (H, N, D) and
// dv (H, N, Dv) over the stored positions of the 2-D mask s (M x N, CSR: ptr, idx, sv).  Two passes over the mask: a ROW pass
// that recomputes the forward's scores and probabilities, forms the softmax derivative and dq, and writes p_i and y_i - two
// values per stored element and head, written once - to the workspace; a COLUMN pass that reads them once through the column
// grouping (cptr, cperm, crow: pattern-only state built by the host) and sums dk and dv without an atomic.
//
// Order (the contract tests/attention_grad_cases.py restates, bit for bit; include/sparse_amd.h A16).  Row r of one head,
// stored elements i = 0 .. n-1 in stored order, columns c_i:
//   t_i, p_i  A15's steps 1 to 3 (the code of csrc/attention_common.h and the softmax of csrc/attention.hip)
//   e_i  = dot(g[r], v[c_i]) by A15's 64 accumulators over Dv
//   u_i  = p_i * e_i
//   delta = sum u_i in A14's order: 64 accumulators per piece of `chunk` (accumulator l holds u[l], then adds u[l + 64], ..),
//          folded by halving, the piece sums added in piece order
//   z_i  = p_i * (e_i - delta);  y_i = s_i * z_i;  y_i = scale * y_i when a scale is given
//   dbias[pos_i] = z_i with a bias (spamd_attention_grad_bias): t_i then carries A15's bias step, and the row pass stores z_i once
//   with dropout (spamd_attention_grad_dropout): keep_i is recomputed; ed_i = keep_i ? e_i * c : +0.0 takes the place of e_i in
//          u_i, delta and z_i, and pd_i = keep_i ? p_i * c : +0.0 is what the row pass parks for dv - the column pass is unchanged
//   dq[r, j]: pieces of `chunk`; a piece starts at +0.0 and takes acc = fma(y_i, k[c_i, j], acc), i ascending; piece sums in
//          piece order
// Column c of one head, the stored elements of column c in stored order (positions pos_i = cperm[..], rows r_i = crow[..]), cut
// into pieces of `chunk`:  dv[c, j]: acc = fma(p[pos_i], g[r_i, j], acc);  dk[c, j]: acc = fma(y[pos_i], q[r_i, j], acc).
// No atomics; every output is written once; no width, threshold, hint or launch geometry changes a bit.
//
// Row forms, by the row's length n:
//   short  n <= short_max (<= 64): a sub-group of G lanes per (row, head); t, e, then p and y stay in registers (element i in
//          lane i mod G, register i / G), four gathered rows in flight, the register index unrolled.
//   wide   short_max < n <= chunk: a wave per (row, head); t / p and e / y in LDS (2 x chunk values).
//   long   n > chunk: pieces through the workspace, nine launches that each END before the next reads what it wrote.
// Column forms, by the column's length m: a sub-group of CG lanes per (column, head) up to short_max, a wave up to chunk, both
// with lanes along Dv and then D; longer columns in pieces of `chunk` (a wave per piece) and a join in piece order.
#include "attention_common.h"
#include "attention_dropout.h"
#include "exp_det.h"

namespace spamd {

template <typename T, typename I>
struct AgIn {
  const I* ptr;
  const I* idx;
  const T* sv;
  const I* cptr;          // N + 1 column pointers into the column order
  const int64_t* cperm;   // column order -> stored position (stable: ascending within a column)
  const I* crow;          // row id per element, in column order
  const T* q;
  const T* k;
  const T* v;
  const T* g;
  int64_t qp, qh, kp, kh, vp, vh, gp, gh;   // row pitch and head stride, in elements
  int64_t M, N, H, nnz;   // H: heads of this launch (at most 65535: grid.y)
  int D, Dv;
  T scale;
  bool has_scale;
  T* ws;             // per head: p (nnz), y (nnz), then the piece forms' 12 nwin statistics and 2 nwin rows of D + Dv
  int64_t ws_head;   // values per head
  T* dq;
  T* dk;
  T* dv;
  __device__ __forceinline__ T score(T s, T w) const {
#pragma clang fp contract(off)
    const T t = s * w;
    return has_scale ? scale * t : t;
  }
  __device__ __forceinline__ T zval(T p, T e, T delta) const {   // the derivative with respect to the score: dbias
#pragma clang fp contract(off)
    const T d = e - delta;
    return p * d;
  }
  __device__ __forceinline__ T yof(T s, T z) const {
#pragma clang fp contract(off)
    const T y = s * z;
    return has_scale ? scale * y : y;
  }
};

// acc[c] = fma(val_i, base[row_i][j], acc[c]) for the elements x = s .. e-1 in order, at the columns j = jb + sub + G c of this
// lane: val_i = vals[perm ? perm[x] : x], row_i = rows[x].  G elements are loaded at a time, one per lane, and handed round by
// shuffle, four gathered rows in flight (at_out4)
template <typename T, typename I, int G>
__device__ __forceinline__ void ag_gather_acc(const T* __restrict__ vals, const int64_t* __restrict__ perm,
                                              const I* __restrict__ rows, int64_t s, int64_t e, const T* __restrict__ base,
                                              int64_t pitch, int width, int jb, int sub, T (&acc)[64 / G]) {
#pragma clang fp contract(off)
  for (int64_t x0 = s; x0 < e; x0 += G) {
    const int cnt = (int)std::min<int64_t>(e - x0, G);
    T val = T(0);
    int64_t row = 0;
    if (sub < cnt) {
      const int64_t pos = perm ? perm[x0 + sub] : x0 + sub;
      val = vals[pos];
      row = (int64_t)rows[x0 + sub];
    }
    for (int ii = 0; ii < cnt; ii += 4) {
      T pp[4];
      const T* vr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int src = ii + u < cnt ? ii + u : ii;
        pp[u] = __shfl(val, src, G);
        vr[u] = base + __shfl(row, src, G) * pitch;
      }
      if (ii + 4 <= cnt && jb + 64 <= width) at_out4<T, G, false>(pp, vr, jb, sub, width, cnt - ii, acc);
      else at_out4<T, G, true>(pp, vr, jb, sub, width, cnt - ii, acc);
    }
  }
}

// ---- row pass, short: a sub-group of G lanes per (row, head) ---------------------------------------------------------------------
// (P: with dropout - spamd_attention_grad_dropout; P = false compiles as before it existed, AtDrop<T, false> being an empty argument)
template <typename T, typename I, int G, bool B, bool P>
__global__ void __launch_bounds__(256)
ag_short_kernel(AgIn<T, I> in, int64_t short_max, AtMods<T, B, P> mz) {
#pragma clang fp contract(off)
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  constexpr int V = 64 / G;
  constexpr int GPB = 256 / G;
  const int sub = threadIdx.x % G;
  const int64_t head = blockIdx.y;
  const T* __restrict__ kh = in.k + head * in.kh;
  const T* __restrict__ vh = in.v + head * in.vh;
  T* __restrict__ wp = in.ws + head * in.ws_head;
  T* __restrict__ wy = wp + in.nnz;
  for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < in.M; row += (int64_t)gridDim.x * GPB) {
    const int64_t b = (int64_t)in.ptr[row];
    const int n = (int)std::min<int64_t>((int64_t)in.ptr[row + 1] - b, 65);
    if (n > short_max) continue;   // (the same in every lane of the sub-group)
    const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
    const T* __restrict__ grow = in.g + head * in.gh + row * in.gp;
    T t[V], ev[V], sv[V];
    int64_t col[V];
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const int i = sub + r * G;
      col[r] = 0;
      sv[r] = T(0);
      ev[r] = T(0);
      t[r] = at_neg_inf<T>();
      if (i < n) {
        col[r] = (int64_t)in.idx[b + i];
        sv[r] = in.sv[b + i];
        if constexpr (B) t[r] = bz.b[head * bz.bh + b + i];   // the bias waits where its score will land
      }
    }
    // phase 1: the scores and e = g[r] . v[c], four elements at a time; r is unrolled so that no register array is indexed
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const int cnt = n - r * G;
      for (int ii = 0; ii < G && ii < cnt; ii += 4) {
        const T* kr[4];
        const T* vr[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t c = __shfl(col[r], ii + e < cnt ? ii + e : ii, G);
          kr[e] = kh + c * in.kp;
          vr[e] = vh + c * in.vp;
        }
        T w[4], x[4];
        at_dot4<T, G>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, sub, w);
        at_dot4<T, G>(grow, vr[0], vr[1], vr[2], vr[3], in.Dv, sub, x);
        T mine = w[0], minx = x[0];
#pragma unroll
        for (int e = 1; e < 4; ++e) {
          mine = sub == ii + e ? w[e] : mine;
          minx = sub == ii + e ? x[e] : minx;
        }
        mine = in.score(sv[r], mine);
        if constexpr (B) mine = mine + t[r];   // (every live lane passes here once: t[r] is still its bias)
        const bool here = sub >= ii && sub < ii + 4 && sub < cnt;   // the lanes that hold these four elements
        t[r] = here ? mine : t[r];
        ev[r] = here ? minx : ev[r];
      }
    }
    // phase 2: A14's short form on the registers (as csrc/attention.hip)
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
    // phase 3: delta = sum p e (accumulator l holds u[l]: one piece of at most 64), then y; p and y go to the workspace
    [[maybe_unused]] T pd[P ? V : 1];   // with dropout: pd_i = keep_i ? p_i * c : +0.0 is parked, and e becomes ed_i likewise
    if constexpr (P) {
#pragma unroll
      for (int r = 0; r < V; ++r) {
        const bool kept = sub + r * G < n && dz.keep(head, b + sub + r * G);
        pd[r] = dz.mul(kept, t[r]);
        ev[r] = dz.mul(kept, ev[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < V; ++r) a[r] = sub + r * G < n ? t[r] * ev[r] : T(0);
#pragma unroll
    for (int hv = V / 2; hv >= 1; hv /= 2)
#pragma unroll
      for (int r = 0; r < hv; ++r) a[r] = a[r] + a[r + hv];
    const T delta = at_xsum<T, G>(a[0]);
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const int i = sub + r * G;
      const T z = in.zval(t[r], ev[r], delta);
      ev[r] = in.yof(sv[r], z);   // ev holds y from here on
      if (i < n) {
        if constexpr (P) wp[b + i] = pd[r];
        else wp[b + i] = t[r];
        wy[b + i] = ev[r];
        if constexpr (B)
          if (bz.db) bz.db[head * in.nnz + b + i] = z;
      }
    }
    // phase 4: the dq row, 64 columns at a time (lane u: the columns u, u + G, ..), four k rows in flight
    T* __restrict__ orow = in.dq + (head * in.M + row) * in.D;
    for (int jb = 0; jb < in.D; jb += 64) {
      T acc[V];
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] = T(0);
#pragma unroll
      for (int r = 0; r < V; ++r) {
        const int cnt = n - r * G;
        for (int ii = 0; ii < G && ii < cnt; ii += 4) {
          T pp[4];
          const T* kr[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int src = ii + e < cnt ? ii + e : ii;
            pp[e] = __shfl(ev[r], src, G);
            kr[e] = kh + __shfl(col[r], src, G) * in.kp;
          }
          if (ii + 4 <= cnt && jb + 64 <= in.D) at_out4<T, G, false>(pp, kr, jb, sub, in.D, cnt - ii, acc);
          else at_out4<T, G, true>(pp, kr, jb, sub, in.D, cnt - ii, acc);
        }
      }
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const int j = jb + sub + G * c;
        if (j < in.D) orow[j] = acc[c];
      }
    }
  }
}

// ---- row pass, wide: a wave (one workgroup) per (row, head), t / p and e / y in LDS -------------------------------------------------
template <typename T, typename I, bool B, bool P>
__global__ void __launch_bounds__(64)
ag_wide_kernel(AgIn<T, I> in, int64_t above, int64_t upto, AtMods<T, B, P> mz) {
#pragma clang fp contract(off)
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_smem[];
  T* __restrict__ lt = reinterpret_cast<T*>(ag_smem);   // `upto` values: t, then p
  T* __restrict__ le = lt + upto;                       // `upto` values: e, then y
  const int lane = threadIdx.x;
  const int64_t head = blockIdx.y;
  const T* __restrict__ kh = in.k + head * in.kh;
  const T* __restrict__ vh = in.v + head * in.vh;
  T* __restrict__ wp = in.ws + head * in.ws_head;
  T* __restrict__ wy = wp + in.nnz;
  // (the ballot loop of seg_wave_each, written out: through the helper the bias-and-dropout instances spill one scalar more)
  for (int64_t base = (int64_t)blockIdx.x * 64; base < in.M; base += (int64_t)gridDim.x * 64) {
    const int64_t mine = base + lane;
    int64_t mb = 0, mn = 0;
    if (mine < in.M) {
      mb = (int64_t)in.ptr[mine];
      mn = (int64_t)in.ptr[mine + 1] - mb;
    }
    unsigned long long todo = __ballot(mn > above && mn <= upto);
    while (todo) {   // wave-uniform: all 64 lanes stay together
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      // the row and its first position travel in vector registers (a shuffle, not a broadcast to scalars): the pointers that
      // follow from them would otherwise crowd the scalar file, which the kernel arguments nearly fill
      const int64_t row = base + __shfl(lane, src, 64), b = __shfl(mb, src, 64);
      const int n = (int)wave_bcast(mn, src);
      const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
      const T* __restrict__ grow = in.g + head * in.gh + row * in.gp;
      const I* __restrict__ idx = in.idx + b;
      for (int i = 0; i < n; i += 4) {   // the scores
        const T* kr[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) kr[e] = kh + (int64_t)idx[i + e < n ? i + e : i] * in.kp;
        T w[4];
        at_dot4<T, 64>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, lane, w);
        if (lane == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e < n) lt[i + e] = bz.add(in.score(in.sv[b + i + e], w[e]), head, b + i + e);
        }
      }
      for (int i = 0; i < n; i += 4) {   // e = g[r] . v[c] (a loop of its own: half as many wave-uniform pointers live)
        const T* vr[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) vr[e] = vh + (int64_t)idx[i + e < n ? i + e : i] * in.vp;
        T x[4];
        at_dot4<T, 64>(grow, vr[0], vr[1], vr[2], vr[3], in.Dv, lane, x);
        if (lane == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e < n) le[i + e] = x[e];
        }
      }
      __syncthreads();
      // A14's wide form: lane u owns the elements u, u + 64, ..
      T m = at_neg_inf<T>();
      for (int x = lane; x < n; x += 64) m = at_nmax(m, lt[x]);
      m = at_xmax<T, 64>(m);
      T acc = T(0);
      for (int x = lane; x < n; x += 64) {
        const T e = exp_det(lt[x] - m);
        lt[x] = e;
        acc = acc + e;
      }
      const T s = at_xsum<T, 64>(acc);
      acc = T(0);   // accumulator `lane` of delta: u[lane], then + u[lane + 64], ..
      for (int x = lane; x < n; x += 64) {
        const T p = lt[x] / s;
        lt[x] = p;
        if constexpr (P) {   // ed_i takes the place of e_i; pd_i is parked here, where the decision is at hand
          const bool kept = dz.keep(head, b + x);
          le[x] = dz.mul(kept, le[x]);
          wp[b + x] = dz.mul(kept, p);
        }
        const T u = p * le[x];
        acc = x == lane ? u : acc + u;
      }
      const T delta = at_xsum<T, 64>(acc);
      for (int x = lane; x < n; x += 64) {
        const T z = in.zval(lt[x], le[x], delta);
        const T y = in.yof(in.sv[b + x], z);
        le[x] = y;
        if constexpr (!P) wp[b + x] = lt[x];
        wy[b + x] = y;
        if constexpr (B)
          if (bz.db) bz.db[head * in.nnz + b + x] = z;
      }
      __syncthreads();
      T* __restrict__ orow = in.dq + (head * in.M + row) * in.D;
      for (int jb = 0; jb < in.D; jb += 64) {
        const int j = jb + lane;
        const T o = at_wave_out<T>(kh, in.kp, j, j < in.D, n, [&](int x) { return le[x]; },
                                   [&](int x) { return (int64_t)idx[x]; });
        if (j < in.D) orow[j] = o;
      }
      __syncthreads();   // the next row writes the LDS again
    }
  }
}

// ---- pieces ----------------------------------------------------------------------------------------------------------------------
// workspace of one head, in values: p and y (nnz each, at stored positions; the long rows park t and e there first), six arrays
// of 2 * nwin - piece maxima, piece sums, row maxima, row sums, piece deltas, row deltas (row values at the slot of the row's
// first piece) -, the piece outputs (2 * nwin rows of D + Dv: dq pieces in the row pass, then dv | dk pieces in the column pass)
__host__ __device__ __forceinline__ int64_t ag_ws_values(int64_t nnz, int64_t nwin, int64_t D, int64_t Dv) {
  return 2 * nnz + (nwin ? 12 * nwin + 2 * nwin * (D + Dv) : 0);
}

// row phases: 0 t, e and piece maxima; 1 piece sums of exp; 2 p and piece deltas; 3 y; 4 dq pieces.  Column phase: 5 dv | dk pieces
template <typename T, typename I, int PHASE, bool B, bool P>
__device__ __forceinline__ void ag_piece(const AgIn<T, I>& in, const AtBias<T, B>& bz, const AtDrop<T, P>& dz, int64_t head, int64_t row, int64_t b, int64_t s, int64_t e,
                                         int64_t chunk, int64_t nwin, int lane, T* __restrict__ ws) {
#pragma clang fp contract(off)
  T* __restrict__ wp = ws;
  T* __restrict__ wy = ws + in.nnz;
  T* __restrict__ st = ws + 2 * in.nnz;
  const int64_t W = (int64_t)in.D + in.Dv;
  T* __restrict__ part = st + 12 * nwin;
  const int64_t slot = seg_slot(b, s, chunk), slot0 = seg_slot(b, b, chunk);
  if (PHASE == 0) {
    const T* __restrict__ kh = in.k + head * in.kh;
    const T* __restrict__ vh = in.v + head * in.vh;
    const T* __restrict__ qrow = in.q + head * in.qh + row * in.qp;
    const T* __restrict__ grow = in.g + head * in.gh + row * in.gp;
    T m = at_neg_inf<T>();
    for (int64_t x = s; x < e; x += 4) {
      const T* kr[4];
      const T* vr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t c = (int64_t)in.idx[x + u < e ? x + u : x];
        kr[u] = kh + c * in.kp;
        vr[u] = vh + c * in.vp;
      }
      T w[4], xe[4];
      at_dot4<T, 64>(qrow, kr[0], kr[1], kr[2], kr[3], in.D, lane, w);
      at_dot4<T, 64>(grow, vr[0], vr[1], vr[2], vr[3], in.Dv, lane, xe);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (x + u < e) {
          const T t = bz.add(in.score(in.sv[x + u], w[u]), head, x + u);
          m = at_nmax(m, t);
          if (lane == 0) {
            wp[x + u] = t;
            wy[x + u] = xe[u];
          }
        }
      }
    }
    if (lane == 0) st[slot] = m;
  } else if (PHASE == 1) {
    const T m = st[4 * nwin + slot0];
    T acc = T(0);
    for (int64_t x = s + lane; x < e; x += 64) acc = acc + exp_det(wp[x] - m);
    acc = at_xsum<T, 64>(acc);
    if (lane == 0) st[2 * nwin + slot] = acc;
  } else if (PHASE == 2) {
    const T m = st[4 * nwin + slot0], sum = st[6 * nwin + slot0];
    T acc = T(0);
    for (int64_t x = s + lane; x < e; x += 64) {
      const T p = exp_det(wp[x] - m) / sum;
      wp[x] = p;
      if constexpr (P) wy[x] = dz.mul(dz.keep(head, x), wy[x]);   // ed_i takes the place of e_i
      const T u = p * wy[x];
      acc = x == s + lane ? u : acc + u;
    }
    acc = at_xsum<T, 64>(acc);
    if (lane == 0) st[8 * nwin + slot] = acc;
  } else if (PHASE == 3) {
    const T delta = st[10 * nwin + slot0];
    for (int64_t x = s + lane; x < e; x += 64) {
      const T s_x = in.sv[x];
      const T z = in.zval(wp[x], wy[x], delta);
      wy[x] = in.yof(s_x, z);
      if constexpr (P) wp[x] = dz.mul(dz.keep(head, x), wp[x]);   // pd_i is parked for the column pass (the decision again)
      if constexpr (B)
        if (bz.db) bz.db[head * in.nnz + x] = z;
    }
  } else if (PHASE == 4) {
    const T* __restrict__ kh = in.k + head * in.kh;
    for (int jb = 0; jb < in.D; jb += 64) {
      T acc[1] = {T(0)};
      ag_gather_acc<T, I, 64>(wy, nullptr, in.idx, s, e, kh, in.kp, in.D, jb, lane, acc);
      if (jb + lane < in.D) part[slot * W + jb + lane] = acc[0];
    }
  } else {   // (row = the column, b .. its first position in the column order)
    const T* __restrict__ gh = in.g + head * in.gh;
    const T* __restrict__ qh = in.q + head * in.qh;
    for (int jb = 0; jb < in.Dv; jb += 64) {
      T acc[1] = {T(0)};
      ag_gather_acc<T, I, 64>(wp, in.cperm, in.crow, s, e, gh, in.gp, in.Dv, jb, lane, acc);
      if (jb + lane < in.Dv) part[slot * W + jb + lane] = acc[0];
    }
    for (int jb = 0; jb < in.D; jb += 64) {
      T acc[1] = {T(0)};
      ag_gather_acc<T, I, 64>(wy, in.cperm, in.crow, s, e, qh, in.qp, in.D, jb, lane, acc);
      if (jb + lane < in.D) part[slot * W + in.Dv + jb + lane] = acc[0];
    }
  }
}

// a wave per window of `chunk` positions: the window holds at most two piece starts of long rows (csrc/segment_walk.h)
// (P: the phases that see dropout are 2 - ed_i - and 3 - pd_i)
template <typename T, typename I, int PHASE, bool B, bool P>
__global__ void __launch_bounds__(256)
ag_piece_kernel(AgIn<T, I> in, int64_t chunk, int64_t nwin, AtMods<T, B, P> mz) {
  const AtBias<T, B>& bz = mz;
  const AtDrop<T, P>& dz = mz;
  const int lane = threadIdx.x & 63;
  const I* __restrict__ ptr = PHASE == 5 ? in.cptr : in.ptr;
  const int64_t R = PHASE == 5 ? in.N : in.M, nnz = in.nnz;
  const int64_t head = blockIdx.y;
  T* __restrict__ ws = in.ws + head * in.ws_head;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < nwin; g += (int64_t)gridDim.x * 4)
    seg_window_pieces(ptr, R, nnz, chunk, g, [&](int64_t row, int64_t b, int64_t s, int64_t e) {
      ag_piece<T, I, PHASE, B, P>(in, bz, dz, head, row, b, s, e, chunk, nwin, lane, ws);
    });
}

// row phases: 0 row maxima; 1 row sums, 2 row deltas (piece values added one after the other in piece order); 3 dq rows.
// Column phase: 4 dv and dk rows.  Piece outputs are added one after the other in piece order
template <typename T, typename I, int PHASE>
__global__ void __launch_bounds__(256)
ag_join_kernel(AgIn<T, I> in, int64_t chunk, int64_t nwin) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const I* __restrict__ ptr = PHASE == 4 ? in.cptr : in.ptr;
  const int64_t R = PHASE == 4 ? in.N : in.M;
  const int64_t W = (int64_t)in.D + in.Dv;
  const int64_t head = blockIdx.y;
  T* __restrict__ st = in.ws + head * in.ws_head + 2 * in.nnz;
  const T* __restrict__ part = st + 12 * nwin;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < R; base += nwaves * 64)
    seg_wave_each(ptr, R, base, lane, [&](int64_t len) { return len > chunk; }, [&](int src, int64_t b, int64_t n) {
      const int64_t np = (n + chunk - 1) / chunk;
      const int64_t slot0 = seg_slot(b, b, chunk);
      if (PHASE == 0) {
        T m = at_neg_inf<T>();
        for (int64_t k = lane; k < np; k += 64) m = at_nmax(m, st[seg_slot(b, b + k * chunk, chunk)]);
        m = at_xmax<T, 64>(m);
        if (lane == 0) st[4 * nwin + slot0] = m;
      } else if (PHASE == 1 || PHASE == 2) {
        const int64_t from = PHASE == 1 ? 2 * nwin : 8 * nwin, to = PHASE == 1 ? 6 * nwin : 10 * nwin;
        const T s = seg_join_sum<T>(np, lane, [&](int64_t k) { return st[from + seg_slot(b, b + k * chunk, chunk)]; });
        if (lane == 0) st[to + slot0] = s;
      } else if (PHASE == 3) {
        T* __restrict__ orow = in.dq + (head * in.M + base + src) * in.D;
        seg_join_rows(part, W, in.D, b, np, chunk, lane, [&](int64_t j, T s) { orow[j] = s; });
      } else {
        T* __restrict__ vrow = in.dv + (head * in.N + base + src) * in.Dv;
        T* __restrict__ krow = in.dk + (head * in.N + base + src) * in.D;
        seg_join_rows(part, W, W, b, np, chunk, lane, [&](int64_t j, T s) {
          if (j < in.Dv) vrow[j] = s;
          else krow[j - in.Dv] = s;
        });
      }
    });
}

// ---- column pass: a sub-group of G lanes per (column, head); G = 64 is the wave form ------------------------------------------------
// columns of above < m <= upto elements (above = -1: the columns without a stored element too - they get +0.0)
template <typename T, typename I, int G>
__global__ void __launch_bounds__(256)
ag_col_kernel(AgIn<T, I> in, int64_t above, int64_t upto) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  constexpr int GPB = 256 / G;
  const int sub = threadIdx.x % G;
  const int64_t head = blockIdx.y;
  const T* __restrict__ wp = in.ws + head * in.ws_head;
  const T* __restrict__ wy = wp + in.nnz;
  const T* __restrict__ gh = in.g + head * in.gh;
  const T* __restrict__ qh = in.q + head * in.qh;
  for (int64_t col = (int64_t)blockIdx.x * GPB + threadIdx.x / G; col < in.N; col += (int64_t)gridDim.x * GPB) {
    const int64_t b = (int64_t)in.cptr[col];
    const int64_t m = (int64_t)in.cptr[col + 1] - b;
    if (m <= above || m > upto) continue;   // (the same in every lane of the sub-group)
    T* __restrict__ vrow = in.dv + (head * in.N + col) * in.Dv;
    T* __restrict__ krow = in.dk + (head * in.N + col) * in.D;
    for (int jb = 0; jb < in.Dv; jb += 64) {
      T acc[V];
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] = T(0);
      ag_gather_acc<T, I, G>(wp, in.cperm, in.crow, b, b + m, gh, in.gp, in.Dv, jb, sub, acc);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const int j = jb + sub + G * c;
        if (j < in.Dv) vrow[j] = acc[c];
      }
    }
    for (int jb = 0; jb < in.D; jb += 64) {
      T acc[V];
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] = T(0);
      ag_gather_acc<T, I, G>(wy, in.cperm, in.crow, b, b + m, qh, in.qp, in.D, jb, sub, acc);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const int j = jb + sub + G * c;
        if (j < in.D) krow[j] = acc[c];
      }
    }
  }
}

template <typename T, typename I, bool B, bool P>
static int attention_grad_typed(AgIn<T, I> in, AtBias<T, B> bz, AtDrop<T, P> dz, int group, int col_group, int64_t short_max, int64_t chunk, int64_t max_row,
                                int64_t max_col, hipStream_t st) {
  const unsigned gy = (unsigned)in.H;
  const int64_t nwin = ceil_div(in.nnz, chunk);
  const dim3 pg(seg_grid(nwin, 4), gy), wg(256);
  const AtBias<T, false> nob{};   // the launches that neither form a score nor hold z
  const AtDrop<T, false> nod{};   // the launches that neither form ed nor park pd
  if (in.M > 0) {   // the row pass; the short form always runs: it writes the dq rows of the rows without a stored element
    SEG_GROUP(group, G, SPAMD_LAUNCH((ag_short_kernel<T, I, G, B, P>), dim3(seg_grid(in.M, 256 / G), gy), wg, 0, st, in, short_max, AtMods<T, B, P>(bz, dz)));
    if (std::min(max_row, chunk) > short_max)
      SPAMD_LAUNCH((ag_wide_kernel<T, I, B, P>), dim3(seg_grid(in.M, 64), gy), dim3(64), (size_t)(2 * chunk) * sizeof(T), st, in, short_max, chunk,
                   AtMods<T, B, P>(bz, dz));
    if (max_row > chunk) {
      const dim3 jg(seg_grid(in.M, 256), gy);
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 0, B, false>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, B, false>(bz, nod));
      SPAMD_LAUNCH((ag_join_kernel<T, I, 0>), jg, wg, 0, st, in, chunk, nwin);
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 1, false, false>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, false, false>(nob, nod));
      SPAMD_LAUNCH((ag_join_kernel<T, I, 1>), jg, wg, 0, st, in, chunk, nwin);
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 2, false, P>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, false, P>(nob, dz));
      SPAMD_LAUNCH((ag_join_kernel<T, I, 2>), jg, wg, 0, st, in, chunk, nwin);
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 3, B, P>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, B, P>(bz, dz));
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 4, false, false>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, false, false>(nob, nod));
      SPAMD_LAUNCH((ag_join_kernel<T, I, 3>), jg, wg, 0, st, in, chunk, nwin);
    }
  }
  if (in.N > 0 && (in.D > 0 || in.Dv > 0)) {   // the column pass; its first launch writes the empty columns
    SEG_GROUP(col_group, G, SPAMD_LAUNCH((ag_col_kernel<T, I, G>), dim3(seg_grid(in.N, 256 / G), gy), wg, 0, st, in, (int64_t)-1, short_max));
    if (std::min(max_col, chunk) > short_max)
      SPAMD_LAUNCH((ag_col_kernel<T, I, 64>), dim3(seg_grid(in.N, 4), gy), wg, 0, st, in, short_max, chunk);
    if (max_col > chunk) {
      SPAMD_LAUNCH((ag_piece_kernel<T, I, 5, false, false>), pg, wg, 0, st, in, chunk, nwin, AtMods<T, false, false>(nob, nod));
      SPAMD_LAUNCH((ag_join_kernel<T, I, 4>), dim3(seg_grid(in.N, 256), gy), wg, 0, st, in, chunk, nwin);
    }
  }
  return 0;
}

struct AgArgs {
  int64_t M, N, nnz, H, D, Dv;
  const void *s_ptr, *s_idx, *s_val, *c_ptr, *c_perm, *c_row, *q, *k, *v, *g;
  int64_t qp, qh, kp, kh, vp, vh, gp, gh;
  int has_scale;
  double scale;
  int group, col_group;
  int64_t short_max, chunk, max_row, max_col;
  void *ws, *dq, *dk, *dv;
  const void* bias;
  int64_t bias_head;
  void* dbias;
  double rate;   // 0: no dropout - the kernels of spamd_attention_grad / spamd_attention_grad_bias
  uint64_t seed;
  int64_t head0;
};

template <typename T, typename I>
static int attention_grad_in(const AgArgs& a, hipStream_t st) {
  const int64_t ws_head = ag_ws_values(a.nnz, a.nnz > a.chunk ? ceil_div(a.nnz, a.chunk) : 0, a.D, a.Dv);
  for (int64_t h0 = 0; h0 < a.H; h0 += 65535) {   // a head per grid.y: at most 65535 of them in one launch
    AgIn<T, I> in{(const I*)a.s_ptr, (const I*)a.s_idx, (const T*)a.s_val, (const I*)a.c_ptr, (const int64_t*)a.c_perm,
                  (const I*)a.c_row, (const T*)a.q + h0 * a.qh, (const T*)a.k + h0 * a.kh, (const T*)a.v + h0 * a.vh,
                  (const T*)a.g + h0 * a.gh, a.qp, a.qh, a.kp, a.kh, a.vp, a.vh, a.gp, a.gh, a.M, a.N,
                  std::min<int64_t>(a.H - h0, 65535), a.nnz, (int)a.D, (int)a.Dv, (T)a.scale, a.has_scale != 0,
                  a.ws ? (T*)a.ws + h0 * ws_head : nullptr, ws_head, (T*)a.dq + h0 * a.M * a.D, (T*)a.dk + h0 * a.N * a.D,
                  (T*)a.dv + h0 * a.N * a.Dv};
    const AtBias<T, true> bz{(const T*)a.bias + h0 * a.bias_head, a.bias_head, a.dbias ? (T*)a.dbias + h0 * a.nnz : nullptr};
    const AtBias<T, false> nob{};
    // (the head's number goes on across the launches: head 65535 does not repeat head 0's decisions)
    const AtDrop<T, true> dz{a.seed, (uint64_t)a.head0 + (uint64_t)h0, dropout_threshold(a.rate), (T)(1.0 / (1.0 - a.rate))};
    const AtDrop<T, false> nod{};
    int rc;
    if (a.rate > 0.0) {
      if (a.bias) rc = attention_grad_typed<T, I, true, true>(in, bz, dz, a.group, a.col_group, a.short_max, a.chunk, a.max_row, a.max_col, st);
      else rc = attention_grad_typed<T, I, false, true>(in, nob, dz, a.group, a.col_group, a.short_max, a.chunk, a.max_row, a.max_col, st);
    } else {
      if (a.bias) rc = attention_grad_typed<T, I, true, false>(in, bz, nod, a.group, a.col_group, a.short_max, a.chunk, a.max_row, a.max_col, st);
      else rc = attention_grad_typed<T, I, false, false>(in, nob, nod, a.group, a.col_group, a.short_max, a.chunk, a.max_row, a.max_col, st);
    }
    if (rc) return rc;
  }
  return 0;
}

}  // namespace spamd

using namespace spamd;

extern "C" int64_t spamd_attention_grad_ws_bytes(int val_dtype, int64_t nnz, int64_t H, int64_t D, int64_t Dv, int64_t chunk) {
  const int64_t esz = val_dtype == SPAMD_F32 ? 4 : (val_dtype == SPAMD_F64 ? 8 : 0);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || H < 0 || D < 0 || Dv < 0 || !seg_chunk_ok(chunk, ATTENTION_MAX_CHUNK)) return SPAMD_EINVAL;
  return H * ag_ws_values(nnz, nnz > chunk ? ceil_div(nnz, chunk) : 0, D, Dv) * esz;
}

// the entry with dropout (spamd_attention_dropout): keep_i is recomputed from (seed, head0 + head, stored position); ed_i =
// keep_i ? e_i * c : +0.0 takes the place of e_i in u_i, delta and z_i, and the row pass parks pd_i = keep_i ? p_i * c : +0.0
// in the place of p_i, so the column pass is the one without dropout.  rate = 0 is spamd_attention_grad_bias (the same
// kernels); bias = NULL is no bias (dbias is not written)
extern "C" int spamd_attention_grad_dropout(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D,
                                    int64_t Dv, const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr,
                                    const int64_t* c_perm, const void* c_row, const void* q, int64_t q_pitch, int64_t q_head,
                                    const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                                    int64_t v_head, const void* g, int64_t g_pitch, int64_t g_head, int has_scale, double scale,
                                    int group, int col_group, int64_t short_max, int64_t chunk, int64_t max_row, int64_t max_col,
                                    const void* bias, int64_t bias_head, void* dbias, double rate, int64_t seed, int64_t head0,
                                    void* ws, int64_t ws_bytes, void* dq, void* dk, void* dv, void* stream) {
  if (val_dtype != SPAMD_F32 && val_dtype != SPAMD_F64) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (M < 0 || N < 0 || nnz < 0 || H < 0 || D < 0 || Dv < 0) return SPAMD_EINVAL;
  if (max_row < 0 || max_row > nnz || max_col < 0 || max_col > nnz) return SPAMD_EINVAL;
  if (D > INT32_MAX - 128 || Dv > INT32_MAX - 128 - D) return SPAMD_EINVAL;   // (row widths, and D + Dv, are 32-bit in the kernels)
  if (q_pitch < 0 || q_head < 0 || k_pitch < 0 || k_head < 0 || v_pitch < 0 || v_head < 0 || g_pitch < 0 || g_head < 0)
    return SPAMD_EINVAL;
  if (bias_head < 0) return SPAMD_EINVAL;
  if (!dropout_rate_ok(rate) || head0 < 0) return SPAMD_EINVAL;
  if (!seg_params_ok(group, chunk, ATTENTION_MAX_CHUNK, short_max) || !seg_group_ok(col_group)) return SPAMD_EINVAL;
  const bool has_dq = M > 0 && D > 0, has_dk = N > 0 && D > 0, has_dv = N > 0 && Dv > 0;
  if (H == 0 || !(has_dq || has_dk || has_dv)) return 0;   // nothing to write
  if ((has_dq && !dq) || (has_dk && !dk) || (has_dv && !dv)) return SPAMD_EINVAL;
  if ((M > 0 && !s_ptr) || (N > 0 && !c_ptr)) return SPAMD_EINVAL;
  if (nnz > 0) {
    if (!s_idx || !s_val || !c_perm || !c_row) return SPAMD_EINVAL;
    if ((D > 0 && (!q || !k)) || (Dv > 0 && (!v || !g))) return SPAMD_EINVAL;
    if (!ws || ws_bytes < spamd_attention_grad_ws_bytes(val_dtype, nnz, H, D, Dv, chunk)) return SPAMD_EWS;
  }
  const AgArgs a{M, N, nnz, H, D, Dv, s_ptr, s_idx, s_val, c_ptr, c_perm, c_row, q, k, v, g, q_pitch, q_head, k_pitch, k_head,
                 v_pitch, v_head, g_pitch, g_head, has_scale, scale, group, col_group, short_max, chunk, max_row, max_col, ws, dq,
                 dk, dv, bias, bias_head, dbias, rate, (uint64_t)seed, head0};
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (val_dtype == SPAMD_F32) return attention_grad_in<float, I>(a, st);
    return attention_grad_in<double, I>(a, st);
  })
  return SPAMD_ETYPE;
}

// the entry with an additive bias (spamd_attention_bias): t_i and p_i are recomputed with it, and dbias (H, nnz) contiguous, when
// not NULL, takes z_i at [head][stored position].  bias = NULL is spamd_attention_grad (dbias is not written)
extern "C" int spamd_attention_grad_bias(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D,
                                    int64_t Dv, const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr,
                                    const int64_t* c_perm, const void* c_row, const void* q, int64_t q_pitch, int64_t q_head,
                                    const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                                    int64_t v_head, const void* g, int64_t g_pitch, int64_t g_head, int has_scale, double scale,
                                    int group, int col_group, int64_t short_max, int64_t chunk, int64_t max_row, int64_t max_col,
                                    const void* bias, int64_t bias_head, void* dbias, void* ws, int64_t ws_bytes, void* dq, void* dk,
                                    void* dv, void* stream) {
  return spamd_attention_grad_dropout(val_dtype, idx_dtype, M, N, nnz, H, D, Dv, s_ptr, s_idx, s_val, c_ptr, c_perm, c_row, q, q_pitch,
                                      q_head, k, k_pitch, k_head, v, v_pitch, v_head, g, g_pitch, g_head, has_scale, scale, group,
                                      col_group, short_max, chunk, max_row, max_col, bias, bias_head, dbias, 0.0, 0, 0, ws, ws_bytes, dq,
                                      dk, dv, stream);
}

extern "C" int spamd_attention_grad(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D,
                                    int64_t Dv, const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr,
                                    const int64_t* c_perm, const void* c_row, const void* q, int64_t q_pitch, int64_t q_head,
                                    const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                                    int64_t v_head, const void* g, int64_t g_pitch, int64_t g_head, int has_scale, double scale,
                                    int group, int col_group, int64_t short_max, int64_t chunk, int64_t max_row, int64_t max_col,
                                    void* ws, int64_t ws_bytes, void* dq, void* dk, void* dv, void* stream) {
  return spamd_attention_grad_bias(val_dtype, idx_dtype, M, N, nnz, H, D, Dv, s_ptr, s_idx, s_val, c_ptr, c_perm, c_row, q, q_pitch,
                                   q_head, k, k_pitch, k_head, v, v_pitch, v_head, g, g_pitch, g_head, has_scale, scale, group,
                                   col_group, short_max, chunk, max_row, max_col, nullptr, 0, nullptr, ws, ws_bytes, dq, dk, dv, stream);
}

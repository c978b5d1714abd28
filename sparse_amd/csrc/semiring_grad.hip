// A18  the backward pass of the semiring products of A17 (csrc/semiring_spmm.hip): from g = d loss / d out (M x N) and the forward's
// arg, the gradients da (nnz, with respect to the stored values, CSR order), db (K x N) and dinit (M x N).  Only arg is needed, not
// the add: output (i, j) credits the stored elements e of row i with k_e == arg[i][j]; arg -1 (the init or the identity) credits
// the init alone.  arg is only ever COMPARED with stored indices, never used as an address.
//   hit(e, j) = (arg[i_e][j] == k_e)
//   da[e]     = sum over the hit j of g[i][j] (plus) | g[i][j] * b[k][j] (times), by A15's 64 accumulators over the N columns:
//               accumulator l starts at +0.0 and takes j = l, l + 64, .. ascending - a = a + g, or a = fma(g, b, a), on a hit, unchanged
//               otherwise -, then the fold by halving, h = 32 .. 1
//   db[k][j]  = the column's stored elements in stored order (c_ptr / c_perm / c_row of A16), cut into pieces of `chunk`; a piece
//               starts at +0.0 and takes acc = acc + g[r][j] (plus) | acc = fma(a[pos], g[r][j], acc) (times) on a hit; the piece sums
//               are added in piece order, the first piece's sum being the start.  A16's dv with a predicate
//   dinit[i][j] = arg[i][j] == -1 ? g[i][j] : +0.0
// Every operation is rounded once, every output element is written exactly once, no atomic touches a value; the result depends on
// neither group, col_group, short_max nor the launch geometry.
//
// Element pass: sub-groups of G = 8 .. 64 lanes run along the N columns of one stored element, 64 / G accumulators a lane.  A
//   sub-group owns a window of SG_WINDOW consecutive stored positions - not a row: a hub row costs what its elements cost -, walks
//   the row pointers along it and keeps the row's arg and g values in registers across the elements of a row segment (results of
//   at most 64 columns; wider ones re-read the row's blocks, which the consecutive elements of a row find in cache).  b is read
//   only where an element is hit; for plus neither the values nor b are read.
// Column pass, A16's three forms: sub-groups of col_group lanes own a column of at most short_max elements, each lane 16 bytes of
//   contiguous output columns (col_group 1: results of at most 4 columns, a lane owns a whole column's outputs); a wave owns a
//   column of at most `chunk` elements; longer columns go in pieces of `chunk`, a wave each, through the workspace, and a join
//   launch - it starts after the piece launch has ENDED - adds them in piece order.
#include "attention_common.h"
#include "group_of.h"

namespace spamd {

constexpr int64_t SG_MAX_CHUNK = (int64_t)1 << 30;
constexpr int64_t SG_WINDOW = 16;      // stored positions a sub-group of the element pass walks
constexpr int SG_LANE_MAX_N = 4;       // col_group 1: a lane holds that many outputs

template <typename T, typename I>
struct SgIn {
  int64_t M, K, N, nnz;
  const I* ptr;            // CSR of a
  const I* idx;
  const T* val;            // times, column pass only
  const I* cptr;           // column grouping (A16)
  const int64_t* cperm;
  const I* crow;
  const T* b;              // times, element pass only
  int64_t ldb;
  const int64_t* arg;
  int64_t lda;
  const T* g;
  int64_t ldg;
  T* da;
  T* db;
  int64_t lddb;
  T* dinit;
  int64_t lddi;
  int aligned;             // N, lda, ldg and the addresses of arg and g allow loads of 16 bytes
};

template <typename T>
struct SgVec {
  static constexpr int N = 16 / (int)sizeof(T);
};

// ---- element pass -------------------------------------------------------------------------------------------------------------------
template <typename T, typename I, bool TIMES, int G>
__global__ void __launch_bounds__(256)
sg_elem_kernel(SgIn<T, I> p) {
#pragma clang fp contract(off)
  constexpr int V = 64 / G;
  constexpr int SPB = 256 / G;
  const int sub = threadIdx.x % G;
  const int64_t nwin = (p.nnz + SG_WINDOW - 1) / SG_WINDOW;
  const bool cached = p.N <= 64;
  for (int64_t w = (int64_t)blockIdx.x * SPB + threadIdx.x / G; w < nwin; w += (int64_t)gridDim.x * SPB) {
    const int64_t lo = w * SG_WINDOW;
    const int64_t hi = lo + SG_WINDOW < p.nnz ? lo + SG_WINDOW : p.nnz;
    int64_t row = seg_of(p.ptr, p.M, lo);   // lo < nnz: row < M and the row is not empty
    int64_t row_end = (int64_t)p.ptr[row + 1];
    bool fresh = true;
    int64_t ar[V];
    T gr[V];
    for (int64_t e = lo; e < hi; ++e) {
      while (e >= row_end) {   // e < nnz = ptr[M]: ends with row < M
        ++row;
        row_end = (int64_t)p.ptr[row + 1];
        fresh = true;
      }
      const int64_t k = (int64_t)p.idx[e];
      T acc[V];
#pragma unroll
      for (int m = 0; m < V; ++m) acc[m] = T(0);
      for (int64_t jb = 0; jb < p.N; jb += 64) {
        if (fresh || !cached) {
#pragma unroll
          for (int m = 0; m < V; ++m) {
            const int64_t j = jb + sub + G * m;
            const bool in = j < p.N;
            ar[m] = in ? p.arg[row * p.lda + j] : (int64_t)-1;   // (no stored index is -1: never a hit)
            gr[m] = in ? p.g[row * p.ldg + j] : T(0);
          }
        }
#pragma unroll
        for (int m = 0; m < V; ++m) {
          const bool hit = ar[m] == k;
          if constexpr (TIMES) {
            const T bv = hit ? p.b[k * p.ldb + jb + sub + G * m] : T(0);   // (a hit lies inside the row: j < N)
            const T f = at_fma(gr[m], bv, acc[m]);
            acc[m] = hit ? f : acc[m];
          } else {
            const T f = acc[m] + gr[m];
            acc[m] = hit ? f : acc[m];
          }
        }
      }
      fresh = false;
#pragma unroll
      for (int hv = V / 2; hv >= 1; hv /= 2)   // h = 32 .. G: both accumulators live in this lane
#pragma unroll
        for (int m = 0; m < hv; ++m) acc[m] = acc[m] + acc[m + hv];
      const T s = at_xsum<T, G>(acc[0]);
      if (sub == 0) p.da[e] = s;
    }
  }
}

// ---- dinit --------------------------------------------------------------------------------------------------------------------------
template <typename T, typename I>
__global__ void __launch_bounds__(256)
sg_init_kernel(SgIn<T, I> p) {
  const int64_t items = p.M * p.N;
  const GroupOf row_of{p.N, 1.0 / (double)p.N};
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t i = row_of(it), j = it - i * p.N;
    p.dinit[i * p.lddi + j] = p.arg[i * p.lda + j] == (int64_t)-1 ? p.g[i * p.ldg + j] : T(0);
  }
}

// ---- column pass: the lane's VEC output columns from `col` of column k over the elements [s, e) of the column order -----------------
// every lane of the sub-group calls it with the same range (the lanes without an output column hand on their elements all the same)
template <typename T, typename I, bool TIMES, int VEC>
__device__ __forceinline__ void sg_fold_col(const SgIn<T, I>& p, int64_t k, int64_t col, int64_t s, int64_t e, int G, int gl, int gbase,
                                            T (&acc)[VEC]) {
#pragma clang fp contract(off)
  const bool col_ok = col < p.N;
  const bool vec = p.aligned != 0;
  auto load = [&](I r, int64_t(&av)[VEC], T(&gv)[VEC]) {
    const int64_t* arow = p.arg + (int64_t)r * p.lda;
    const T* grow = p.g + (int64_t)r * p.ldg;
    if (vec) {
#pragma unroll
      for (int h = 0; h < VEC; h += 2) {
        const Vec<int64_t, 2> x = *reinterpret_cast<const Vec<int64_t, 2>*>(arow + col + h);
        av[h] = x.v[0];
        av[h + 1] = x.v[1];
      }
      const Vec<T, VEC> y = *reinterpret_cast<const Vec<T, VEC>*>(grow + col);
#pragma unroll
      for (int v = 0; v < VEC; ++v) gv[v] = y.v[v];
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int64_t j = col + v < p.N ? col + v : p.N - 1;   // (read inside the row, never stored)
        av[v] = arow[j];
        gv[v] = grow[j];
      }
    }
  };
  auto step = [&](T a, const int64_t(&av)[VEC], const T(&gv)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const bool hit = av[v] == k;
      const T f = TIMES ? at_fma(a, gv[v], acc[v]) : acc[v] + gv[v];
      acc[v] = hit ? f : acc[v];
    }
  };
  for (int64_t q = s; q < e; q += G) {
    const int64_t mine = q + gl;
    I ri = 0;
    T ai = T(0);
    if (mine < e) {
      ri = p.crow[mine];
      if constexpr (TIMES) ai = p.val[p.cperm[mine]];
    }
    const int cnt = (int)(e - q < (int64_t)G ? e - q : (int64_t)G);
    int i = 0;
    for (; i + 4 <= cnt; i += 4) {   // four rows of arg and g in flight
      I rj[4];
      T aj[4], gv[4][VEC];
      int64_t av[4][VEC];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rj[u] = lane_shfl(ri, gbase + i + u);
        aj[u] = T(0);
        if constexpr (TIMES) aj[u] = lane_shfl(ai, gbase + i + u);
      }
      if (col_ok) {
#pragma unroll
        for (int u = 0; u < 4; ++u) load(rj[u], av[u], gv[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) step(aj[u], av[u], gv[u]);
      }
    }
    for (; i < cnt; ++i) {
      const I rj = lane_shfl(ri, gbase + i);
      T aj = T(0);
      if constexpr (TIMES) aj = lane_shfl(ai, gbase + i);
      if (col_ok) {
        int64_t av[VEC];
        T gv[VEC];
        load(rj, av, gv);
        step(aj, av, gv);
      }
    }
  }
}

// columns of above < m <= upto elements (above = -1: the columns without a stored element too - they get +0.0)
template <typename T, typename I, bool TIMES>
__global__ void __launch_bounds__(256)
sg_col_kernel(SgIn<T, I> p, int G, int64_t above, int64_t upto) {
  constexpr int VEC = SgVec<T>::N;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1), gbase = lane - gl, gpb = 256 / G;
  for (int64_t k = (int64_t)blockIdx.x * gpb + threadIdx.x / G; k < p.K; k += (int64_t)gridDim.x * gpb) {
    const int64_t b = (int64_t)p.cptr[k];
    const int64_t m = (int64_t)p.cptr[k + 1] - b;
    if (m <= above || m > upto) continue;   // (the same in every lane of the sub-group)
    for (int64_t c0 = 0; c0 < p.N; c0 += (int64_t)G * VEC) {
      const int64_t col = c0 + (int64_t)gl * VEC;
      T acc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = T(0);
      sg_fold_col<T, I, TIMES, VEC>(p, k, col, b, b + m, G, gl, gbase, acc);
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (col + v < p.N) p.db[k * p.lddb + col + v] = acc[v];
    }
  }
}

// results of at most SG_LANE_MAX_N columns: a lane owns the outputs of a whole column of at most `upto` elements (the empty ones too)
template <typename T, typename I, bool TIMES>
__global__ void __launch_bounds__(256)
sg_col_lane_kernel(SgIn<T, I> p, int64_t upto) {
#pragma clang fp contract(off)
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < p.K; k += (int64_t)gridDim.x * 256) {
    const int64_t b = (int64_t)p.cptr[k];
    const int64_t m = (int64_t)p.cptr[k + 1] - b;
    if (m > upto) continue;
    T acc[SG_LANE_MAX_N];
#pragma unroll
    for (int v = 0; v < SG_LANE_MAX_N; ++v) acc[v] = T(0);
    for (int64_t i = b; i < b + m; ++i) {
      const int64_t r = (int64_t)p.crow[i];
      T a = T(0);
      if constexpr (TIMES) a = p.val[p.cperm[i]];
#pragma unroll
      for (int v = 0; v < SG_LANE_MAX_N; ++v) {
        if (v < p.N) {
          const bool hit = p.arg[r * p.lda + v] == k;
          const T gv = p.g[r * p.ldg + v];
          const T f = TIMES ? at_fma(a, gv, acc[v]) : acc[v] + gv;
          acc[v] = hit ? f : acc[v];
        }
      }
    }
#pragma unroll
    for (int v = 0; v < SG_LANE_MAX_N; ++v)
      if (v < p.N) p.db[k * p.lddb + v] = acc[v];
  }
}

// a wave per window of `chunk` positions of the column order: the window holds at most two piece starts of long columns
// (csrc/segment_walk.h) - workspace rows 2g and 2g + 1 of N values
template <typename T, typename I, bool TIMES>
__device__ __forceinline__ void sg_piece(const SgIn<T, I>& p, int64_t k, int64_t b, int64_t s, int64_t e, int64_t chunk, int lane,
                                         T* __restrict__ part) {
  constexpr int VEC = SgVec<T>::N;
  const int64_t slot = seg_slot(b, s, chunk);
  for (int64_t c0 = 0; c0 < p.N; c0 += (int64_t)64 * VEC) {
    const int64_t col = c0 + (int64_t)lane * VEC;
    T acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = T(0);
    sg_fold_col<T, I, TIMES, VEC>(p, k, col, s, e, 64, lane, 0, acc);
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (col + v < p.N) part[slot * p.N + col + v] = acc[v];
  }
}

template <typename T, typename I, bool TIMES>
__global__ void __launch_bounds__(256)
sg_piece_kernel(SgIn<T, I> p, int64_t chunk, int64_t nwin, T* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < nwin; g += (int64_t)gridDim.x * 4)
    seg_window_pieces(p.cptr, p.K, p.nnz, chunk, g, [&](int64_t k, int64_t b, int64_t s, int64_t e) {
      sg_piece<T, I, TIMES>(p, k, b, s, e, chunk, lane, part);
    });
}

// the piece sums of every long column added one after the other in piece order, the first piece's sum being the start
template <typename T, typename I>
__global__ void __launch_bounds__(256)
sg_join_kernel(SgIn<T, I> p, int64_t chunk, const T* __restrict__ part) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < p.K; base += nwaves * 64)
    seg_wave_each(p.cptr, p.K, base, lane, [&](int64_t len) { return len > chunk; }, [&](int src, int64_t b, int64_t n) {
      T* __restrict__ orow = p.db + (base + src) * p.lddb;
      seg_join_rows(part, p.N, p.N, b, (n + chunk - 1) / chunk, chunk, lane, [&](int64_t j, T s) { orow[j] = s; });
    });
}

static int64_t sg_ws_bytes(int64_t esz, int64_t nnz, int64_t N, int64_t chunk) {
  return 2 * ceil_div(nnz, chunk) * N * esz;
}

template <typename T, typename I, bool TIMES>
static int semiring_grad_typed(SgIn<T, I> p, int group, int col_group, int64_t short_max, int64_t chunk, int64_t max_col, void* ws,
                               hipStream_t st) {
  const dim3 wg(256);
  if (p.da && p.nnz > 0)
    SEG_GROUP(group, G, SPAMD_LAUNCH((sg_elem_kernel<T, I, TIMES, G>), dim3(seg_grid(ceil_div(p.nnz, SG_WINDOW), 256 / G)), wg, 0, st, p));
  if (p.dinit && p.M > 0 && p.N > 0) SPAMD_LAUNCH((sg_init_kernel<T, I>), dim3(seg_grid(p.M * p.N, 256)), wg, 0, st, p);
  if (p.db && p.K > 0 && p.N > 0) {   // the first launch writes the columns without a stored element
    if (col_group == 1) SPAMD_LAUNCH((sg_col_lane_kernel<T, I, TIMES>), dim3(seg_grid(p.K, 256)), wg, 0, st, p, short_max);
    else SPAMD_LAUNCH((sg_col_kernel<T, I, TIMES>), dim3(seg_grid(p.K, 256 / col_group)), wg, 0, st, p, col_group, (int64_t)-1, short_max);
    if (std::min(max_col, chunk) > short_max)
      SPAMD_LAUNCH((sg_col_kernel<T, I, TIMES>), dim3(seg_grid(p.K, 4)), wg, 0, st, p, 64, short_max, chunk);
    if (max_col > chunk) {
      const int64_t nwin = ceil_div(p.nnz, chunk);
      SPAMD_LAUNCH((sg_piece_kernel<T, I, TIMES>), dim3(seg_grid(nwin, 4)), wg, 0, st, p, chunk, nwin, (T*)ws);
      SPAMD_LAUNCH((sg_join_kernel<T, I>), dim3(seg_grid(p.K, 256)), wg, 0, st, p, chunk, (const T*)ws);
    }
  }
  return 0;
}

struct SgArgs {
  int mul;
  int64_t M, K, N, nnz;
  const void *a_ptr, *a_idx, *a_val, *c_ptr, *c_perm, *c_row, *b;
  int64_t ldb;
  const int64_t* arg;
  int64_t lda;
  const void* g;
  int64_t ldg;
  int group, col_group;
  int64_t short_max, chunk, max_col;
  void *ws, *da, *db;
  int64_t lddb;
  void* dinit;
  int64_t lddi;
};

template <typename T, typename I>
static int semiring_grad_in(const SgArgs& a, hipStream_t st) {
  constexpr int VEC = SgVec<T>::N;
  SgIn<T, I> p{a.M, a.K, a.N, a.nnz, (const I*)a.a_ptr, (const I*)a.a_idx, (const T*)a.a_val, (const I*)a.c_ptr,
               (const int64_t*)a.c_perm, (const I*)a.c_row, (const T*)a.b, a.ldb, a.arg, a.lda, (const T*)a.g, a.ldg, (T*)a.da, (T*)a.db,
               a.lddb, (T*)a.dinit, a.lddi, 0};
  p.aligned = a.N % VEC == 0 && a.lda % 2 == 0 && a.ldg % VEC == 0 && (uintptr_t)a.arg % 16 == 0 && (uintptr_t)a.g % 16 == 0;
  if (a.mul == SPAMD_SEMIRING_TIMES) return semiring_grad_typed<T, I, true>(p, a.group, a.col_group, a.short_max, a.chunk, a.max_col, a.ws, st);
  return semiring_grad_typed<T, I, false>(p, a.group, a.col_group, a.short_max, a.chunk, a.max_col, a.ws, st);
}

}  // namespace spamd

using namespace spamd;

static int64_t sg_esz(int val_dtype) {
  return val_dtype == SPAMD_F32 ? 4 : (val_dtype == SPAMD_F64 ? 8 : 0);
}

extern "C" int64_t spamd_semiring_grad_ws_bytes(int val_dtype, int64_t nnz, int64_t N, int64_t chunk) {
  const int64_t esz = sg_esz(val_dtype);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || N < 0 || !seg_chunk_ok(chunk, SG_MAX_CHUNK)) return SPAMD_EINVAL;
  if (nnz <= chunk) return 0;
  return sg_ws_bytes(esz, nnz, N, chunk);
}

extern "C" int spamd_semiring_grad(int val_dtype, int idx_dtype, int mul, int64_t M, int64_t K, int64_t N, int64_t nnz, const void* a_ptr,
                                   const void* a_idx, const void* a_val, const void* c_ptr, const int64_t* c_perm, const void* c_row,
                                   const void* b, int64_t ldb, const int64_t* arg, int64_t lda, const void* g, int64_t ldg, int group,
                                   int col_group, int64_t short_max, int64_t chunk, int64_t max_col, void* ws, int64_t ws_bytes,
                                   void* da, void* db, int64_t lddb, void* dinit, int64_t lddi, void* stream) {
  const int64_t esz = sg_esz(val_dtype);
  if (!esz) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (mul != SPAMD_SEMIRING_PLUS && mul != SPAMD_SEMIRING_TIMES) return SPAMD_EINVAL;
  const bool times = mul == SPAMD_SEMIRING_TIMES;
  if (M < 0 || K < 0 || N < 0 || nnz < 0 || max_col < 0 || max_col > nnz) return SPAMD_EINVAL;
  if (!seg_params_ok(group, chunk, SG_MAX_CHUNK, short_max) || (col_group != 1 && !seg_group_ok(col_group))) return SPAMD_EINVAL;
  if (col_group == 1 && N > SG_LANE_MAX_N) return SPAMD_EINVAL;
  if (lda < N || ldg < N || (times && ldb < N) || (db && lddb < N) || (dinit && lddi < N)) return SPAMD_EINVAL;
  const bool elem = da && nnz > 0, cols = db && K > 0 && N > 0, init = dinit && M > 0 && N > 0;
  if (!elem && !cols && !init) return 0;
  if (N > 0 && (!arg || !g)) return SPAMD_EINVAL;
  if (elem && (!a_ptr || !a_idx || M == 0 || K == 0 || (times && N > 0 && !b))) return SPAMD_EINVAL;
  if (cols && (!c_ptr || (nnz > 0 && (!c_row || M == 0 || (times && (!c_perm || !a_val)))))) return SPAMD_EINVAL;
  if (cols && max_col > chunk && (!ws || ws_bytes < sg_ws_bytes(esz, nnz, N, chunk))) return SPAMD_EWS;
  hipStream_t st = (hipStream_t)stream;
  const SgArgs a{mul, M, K, N, nnz, a_ptr, a_idx, a_val, c_ptr, c_perm, c_row, b, ldb, arg, lda, g, ldg, group, col_group,
                 short_max, chunk, max_col, ws, da, db, lddb, dinit, lddi};
  if (val_dtype == SPAMD_F32) {
    if (idx_dtype == SPAMD_I32) return semiring_grad_in<float, int32_t>(a, st);
    return semiring_grad_in<float, int64_t>(a, st);
  }
  if (idx_dtype == SPAMD_I32) return semiring_grad_in<double, int32_t>(a, st);
  return semiring_grad_in<double, int64_t>(a, st);
}

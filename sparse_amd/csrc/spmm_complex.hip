// CSR x dense -> dense SpMM for complex64 / complex128 values on gfx950 (the complex case of `_dot_csr_ndarray`,
// reference sparse/numba_backend/_common.py:720-755, whose loop `val[j] += v * b[ind, j]` is dtype-generic).
//
// Values are interleaved (re, im) pairs of R = float / double, as NumPy and torch store them; ldb / ldo count complex
// elements.  Two kernels, the complex counterparts of spmm_csr.hip's:
//
//  * row-group: G lanes of a wave own one compressed row, each lane owns CH groups of VEC contiguous output columns and sums
//    the row's stored elements in storage (k-ascending) order.  Every output element is written once, by one lane: no
//    atomics, deterministic, and in the exact mode bit-identical to the reference.  A lane fetches 16 bytes of a B row per
//    load wherever alignment allows - one complex128 column or two adjacent complex64 columns (8-byte accesses run at
//    0.54-0.70 of the 16-byte rate on this chip); an odd N or a B / result that is not 16-byte aligned takes 8 bytes.
//  * row-vector (results of at most 4 complex64 / 2 complex128 columns; N = 1 is the matrix-vector product): L lanes run
//    ALONG a row's stored elements and a butterfly over them forms the row's sums - a fixed tree order, deterministic but
//    not the reference's, so SPAMD_EXACT_MULADD and SPAMD_SPMM_ROWGROUP keep the row-group kernel.
//
// One term is  acc_re += ar*br - ai*bi;  acc_im += ar*bi + ai*br.  Default mode: four FMAs.  Exact mode: four rounded
// products, one rounded subtraction, one rounded addition, then the rounded accumulate - NumPy's scalar complex multiply
// followed by its complex add.
#include "common.h"

namespace spamd {

template <bool EXACT, typename R>
__device__ __forceinline__ void cmul_add(R ar, R ai, R br, R bi, R& acc_re, R& acc_im) {
#pragma clang fp contract(off)
  if constexpr (EXACT) {
    const R p1 = ar * br, p2 = ai * bi, p3 = ar * bi, p4 = ai * br;
    const R re = p1 - p2, im = p3 + p4;
    acc_re = acc_re + re;
    acc_im = acc_im + im;
  } else if constexpr (std::is_same<R, float>::value) {
    acc_re = __builtin_fmaf(ar, br, acc_re);
    acc_re = __builtin_fmaf(-ai, bi, acc_re);
    acc_im = __builtin_fmaf(ar, bi, acc_im);
    acc_im = __builtin_fmaf(ai, br, acc_im);
  } else {
    acc_re = __builtin_fma(ar, br, acc_re);
    acc_re = __builtin_fma(-ai, bi, acc_re);
    acc_im = __builtin_fma(ar, bi, acc_im);
    acc_im = __builtin_fma(ai, br, acc_im);
  }
}

// NR reals (NR / 2 complex elements) from p: one aligned vector access of NR * sizeof(R) bytes when WIDE, else
// accesses of 8 bytes (one complex64, or one half of a complex128)
template <typename R, int NR, bool WIDE>
__device__ __forceinline__ void cload(const R* p, R (&o)[NR]) {
  if constexpr (WIDE) {
    const Vec<R, NR> v = *reinterpret_cast<const Vec<R, NR>*>(p);
#pragma unroll
    for (int e = 0; e < NR; ++e) o[e] = v.v[e];
  } else {
    constexpr int PER = 8 / (int)sizeof(R);
#pragma unroll
    for (int q = 0; q < NR / PER; ++q) {
      const Vec<R, PER> v = *reinterpret_cast<const Vec<R, PER>*>(p + q * PER);
#pragma unroll
      for (int e = 0; e < PER; ++e) o[q * PER + e] = v.v[e];
    }
  }
}

template <typename R, int NR, bool WIDE>
__device__ __forceinline__ void cstore_nt(R* p, const R (&v)[NR]) {
  if constexpr (WIDE) {
    nt_store<R, NR>(p, v);
  } else {
    constexpr int PER = 8 / (int)sizeof(R);
#pragma unroll
    for (int q = 0; q < NR / PER; ++q) {
      R t[PER];
#pragma unroll
      for (int e = 0; e < PER; ++e) t[e] = v[q * PER + e];
      nt_store<R, PER>(p + q * PER, t);
    }
  }
}

// ---- row-group kernel ----------------------------------------------------------------------------------------------
// VEC complex columns per lane and column group (2 only for float with WIDE); WIDE: 16-byte accesses of A's values, B and
// the result (the dispatcher has checked every alignment), else 8-byte ones.
template <typename R, typename I, int VEC, int G, bool EXACT, int CH, bool WIDE>
__global__ void __launch_bounds__(256)
spmm_csr_complex_rowgroup_kernel(int64_t M, int64_t N, const R* __restrict__ a_data, const I* __restrict__ a_idx,
                                 const I* __restrict__ a_ptr, const R* __restrict__ b, int64_t ldb, R* __restrict__ out,
                                 int64_t ldo) {
  constexpr int RPW = SPAMD_WAVE / G;   // rows per wave
  constexpr int NR = 2 * VEC;           // reals per lane and column group
  constexpr int U = (8 / (CH * (int)(sizeof(R) / 4))) < 1 ? 1 : (8 / (CH * (int)(sizeof(R) / 4)));   // B rows in flight: 8 / CH
  // accesses per lane for float as in the real row-group kernel, half as many for double (measured on config 2's matrix with
  // 8 / CH for double as well: N = 128 21.9 against 22.5 ms, but N = 8 2.03 against 1.54 ms - 140 VGPRs against 96)
  const int lane = threadIdx.x & (SPAMD_WAVE - 1);
  const int gl = lane % G;
  const int gbase = lane - gl;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / SPAMD_WAVE) + (threadIdx.x / SPAMD_WAVE);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / SPAMD_WAVE);

  for (int64_t row0 = wave * RPW; row0 < M; row0 += nwaves * RPW) {
    const int64_t row = row0 + lane / G;
    const bool row_ok = row < M;
    const int64_t start = row_ok ? (int64_t)a_ptr[row] : 0;
    const int64_t end = row_ok ? (int64_t)a_ptr[row + 1] : 0;

    for (int64_t c0 = 0; c0 < N; c0 += (int64_t)G * VEC * CH) {
      int64_t col[CH];
      bool col_ok[CH];   // N % VEC == 0 (dispatcher): a lane's VEC columns are inside the row or all outside
      R acc[CH][NR];
#pragma unroll
      for (int h = 0; h < CH; ++h) {
        col[h] = c0 + (int64_t)h * G * VEC + (int64_t)gl * VEC;
        col_ok[h] = col[h] < N;
#pragma unroll
        for (int e = 0; e < NR; ++e) acc[h][e] = R(0);
      }

      for (int64_t p = start; p < end; p += G) {
        const int64_t mine = p + gl;
        I ci = 0;
        R vr = R(0), vi = R(0);
        if (mine < end) {
          ci = a_idx[mine];
          R t[2];
          cload<R, 2, WIDE>(a_data + 2 * mine, t);
          vr = t[0];
          vi = t[1];
        }
        const int cnt = (int)((end - p) < (int64_t)G ? (end - p) : (int64_t)G);
        int j = 0;
        for (; j + U <= cnt; j += U) {
          I cj[U];
          R ar[U], ai[U];
          R bj[U][CH][NR];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (G == SPAMD_WAVE) {
              cj[u] = wave_bcast(ci, j + u);
              ar[u] = wave_bcast(vr, j + u);
              ai[u] = wave_bcast(vi, j + u);
            } else {
              cj[u] = lane_shfl(ci, gbase + j + u);
              ar[u] = lane_shfl(vr, gbase + j + u);
              ai[u] = lane_shfl(vi, gbase + j + u);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int h = 0; h < CH; ++h)
              if (col_ok[h]) cload<R, NR, WIDE>(b + 2 * ((int64_t)cj[u] * ldb + col[h]), bj[u][h]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int h = 0; h < CH; ++h) {
              if (col_ok[h]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                  cmul_add<EXACT>(ar[u], ai[u], bj[u][h][2 * e], bj[u][h][2 * e + 1], acc[h][2 * e], acc[h][2 * e + 1]);
              }
            }
          }
        }
        for (; j < cnt; ++j) {
          I cj;
          R ar, ai;
          if constexpr (G == SPAMD_WAVE) {
            cj = wave_bcast(ci, j);
            ar = wave_bcast(vr, j);
            ai = wave_bcast(vi, j);
          } else {
            cj = lane_shfl(ci, gbase + j);
            ar = lane_shfl(vr, gbase + j);
            ai = lane_shfl(vi, gbase + j);
          }
#pragma unroll
          for (int h = 0; h < CH; ++h) {
            if (col_ok[h]) {
              R bj[NR];
              cload<R, NR, WIDE>(b + 2 * ((int64_t)cj * ldb + col[h]), bj);
#pragma unroll
              for (int e = 0; e < VEC; ++e) cmul_add<EXACT>(ar, ai, bj[2 * e], bj[2 * e + 1], acc[h][2 * e], acc[h][2 * e + 1]);
            }
          }
        }
      }
#pragma unroll
      for (int h = 0; h < CH; ++h)
        if (row_ok && col_ok[h]) cstore_nt<R, NR, WIDE>(out + 2 * (row * ldo + col[h]), acc[h]);
    }
  }
}

// ---- row-vector kernel ---------------------------------------------------------------------------------------------
// L lanes (a power of two chosen inside the kernel from nnz / M = indptr[M] / M) share one row; a lane takes the stored
// elements p, p + L, p + 2L, ... of it with coalesced loads of (index, value), gathers the NV entries of B's row - with
// 16-byte accesses when `wide` - and accumulates privately; a butterfly over the L lanes then forms the row's sums.
template <typename R, int NV>
__device__ __forceinline__ void crv_load(const R* p, bool wide, R (&o)[2 * NV]) {
  constexpr int PER = 16 / (int)sizeof(R);   // reals per 16 bytes
  if constexpr ((2 * NV) % PER == 0) {
    if (wide) {
#pragma unroll
      for (int q = 0; q < 2 * NV / PER; ++q) {
        const Vec<R, PER> v = *reinterpret_cast<const Vec<R, PER>*>(p + q * PER);
#pragma unroll
        for (int e = 0; e < PER; ++e) o[q * PER + e] = v.v[e];
      }
      return;
    }
  }
  cload<R, 2 * NV, false>(p, o);
}

template <typename R, typename I, int NV, int L>
__device__ __forceinline__ void crowvec_body(int64_t M, const R* __restrict__ a_data, const I* __restrict__ a_idx,
                                             const I* __restrict__ a_ptr, const R* __restrict__ b, int64_t ldb,
                                             R* __restrict__ out, int64_t ldo, bool wide, bool a_wide) {
  constexpr int RPW = SPAMD_WAVE / L;
  const int lane = threadIdx.x & (SPAMD_WAVE - 1);
  const int gl = lane & (L - 1);
  const int sub = lane / L;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / SPAMD_WAVE) + (threadIdx.x / SPAMD_WAVE);
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x / SPAMD_WAVE) * RPW;
  auto value = [&](int64_t p, R& vr, R& vi) {
    R t[2];
    if (a_wide) cload<R, 2, true>(a_data + 2 * p, t);
    else cload<R, 2, false>(a_data + 2 * p, t);
    vr = t[0];
    vi = t[1];
  };
  for (int64_t base = wave * RPW; base < M; base += stride) {
    const int64_t r = base + sub;
    int64_t s = 0, e = 0;
    if (r < M) {
      s = (int64_t)a_ptr[r];
      e = (int64_t)a_ptr[r + 1];
    }
    R acc[2 * NV];
#pragma unroll
    for (int q = 0; q < 2 * NV; ++q) acc[q] = R(0);
    // two stored elements per lane and trip: their gathers are in flight together
    for (int64_t p = s + gl; p < e; p += 2 * L) {
      const bool two = p + L < e;
      const I j0 = a_idx[p];
      R w0r, w0i, w1r = R(0), w1i = R(0);
      value(p, w0r, w0i);
      I j1 = 0;
      if (two) {
        j1 = a_idx[p + L];
        value(p + L, w1r, w1i);
      }
      R g0[2 * NV], g1[2 * NV];
      crv_load<R, NV>(b + 2 * (int64_t)j0 * ldb, wide, g0);
      if (two) crv_load<R, NV>(b + 2 * (int64_t)j1 * ldb, wide, g1);
#pragma unroll
      for (int q = 0; q < NV; ++q) cmul_add<false>(w0r, w0i, g0[2 * q], g0[2 * q + 1], acc[2 * q], acc[2 * q + 1]);
      if (two) {
#pragma unroll
        for (int q = 0; q < NV; ++q) cmul_add<false>(w1r, w1i, g1[2 * q], g1[2 * q + 1], acc[2 * q], acc[2 * q + 1]);
      }
    }
    // every lane of the wave is back here: butterfly over the row's L lanes
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
#pragma unroll
      for (int q = 0; q < 2 * NV; ++q) acc[q] = acc[q] + lane_shfl(acc[q], lane ^ off);
    }
    if (r < M && gl == 0) {
#pragma unroll
      for (int q = 0; q < 2 * NV; ++q) out[2 * r * ldo + q] = acc[q];
    }
  }
}

template <typename R, typename I, int NV>
__global__ void __launch_bounds__(256)
spmm_csr_complex_rowvec_kernel(int64_t M, const R* __restrict__ a_data, const I* __restrict__ a_idx,
                               const I* __restrict__ a_ptr, const R* __restrict__ b, int64_t ldb, R* __restrict__ out,
                               int64_t ldo, int wide, int a_wide) {
  // lanes per row: the power of two with 2 L >= nnz / M (one trip covers an average row), 4..64
  const int64_t avg = uniform((int64_t)a_ptr[M]) / M;
  if (avg > 64) crowvec_body<R, I, NV, 64>(M, a_data, a_idx, a_ptr, b, ldb, out, ldo, wide != 0, a_wide != 0);
  else if (avg > 32) crowvec_body<R, I, NV, 32>(M, a_data, a_idx, a_ptr, b, ldb, out, ldo, wide != 0, a_wide != 0);
  else if (avg > 16) crowvec_body<R, I, NV, 16>(M, a_data, a_idx, a_ptr, b, ldb, out, ldo, wide != 0, a_wide != 0);
  else if (avg > 8) crowvec_body<R, I, NV, 8>(M, a_data, a_idx, a_ptr, b, ldb, out, ldo, wide != 0, a_wide != 0);
  else crowvec_body<R, I, NV, 4>(M, a_data, a_idx, a_ptr, b, ldb, out, ldo, wide != 0, a_wide != 0);
}

template <typename R>
constexpr int crowvec_max_n() { return sizeof(R) == 4 ? 4 : 2; }

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename R, typename I>
static int launch_complex_rowvec(int64_t M, int64_t N, const R* a_data, const I* a_idx, const I* a_ptr, const R* b,
                                 int64_t ldb, R* out, int64_t ldo, hipStream_t s) {
  int64_t blocks = ceil_div(M, 4);   // the grid is sized for the widest choice of L (one row per wave) and strides over the rows
  if (blocks > 256 * 8) blocks = 256 * 8;
  const size_t csize = 2 * sizeof(R);
  const int wide = (N * csize) % 16 == 0 && aligned16(b) && (ldb * csize) % 16 == 0;
  const int a_wide = sizeof(R) == 8 && aligned16(a_data);
#define SPAMD_CRV(NV)                                                                                                    \
  case NV:                                                                                                               \
    hipLaunchKernelGGL((spmm_csr_complex_rowvec_kernel<R, I, NV>), dim3((unsigned)blocks), dim3(256), 0, s, M, a_data,   \
                       a_idx, a_ptr, b, ldb, out, ldo, wide, a_wide);                                                    \
    break;
  if constexpr (sizeof(R) == 4) {
    switch (N) {
      SPAMD_CRV(1)
      SPAMD_CRV(2)
      SPAMD_CRV(3)
      SPAMD_CRV(4)
      default: return SPAMD_EINVAL;
    }
  } else {
    switch (N) {
      SPAMD_CRV(1)
      SPAMD_CRV(2)
      default: return SPAMD_EINVAL;
    }
  }
#undef SPAMD_CRV
  return launch_status();
}

template <typename R, typename I, int VEC, int G, bool EXACT, int CH, bool WIDE>
static int launch_complex_rowgroup(int64_t M, int64_t N, const R* a_data, const I* a_idx, const I* a_ptr, const R* b,
                                   int64_t ldb, R* out, int64_t ldo, hipStream_t s) {
  constexpr int RPW = SPAMD_WAVE / G;
  constexpr int WPB = 4;   // waves per 256-thread block
  int64_t blocks = ceil_div(M, (int64_t)RPW * WPB);
  const int64_t cap = 256 * 8 * 4;   // grid-stride above this many blocks
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((spmm_csr_complex_rowgroup_kernel<R, I, VEC, G, EXACT, CH, WIDE>), dim3((unsigned)blocks), dim3(256), 0,
                     s, M, N, a_data, a_idx, a_ptr, b, ldb, out, ldo);
  return launch_status();
}

template <typename R, typename I, bool EXACT>
static int dispatch_complex_shape(int64_t M, int64_t N, const R* a_data, const I* a_idx, const I* a_ptr, const R* b,
                                  int64_t ldb, R* out, int64_t ldo, hipStream_t s) {
  // 16 bytes per lane and access wherever the shapes and alignments allow: two complex64 columns (N, ldb, ldo even) or one
  // complex128 column; the value of A rides in one access of its own size then, too
  const bool base16 = aligned16(b) && aligned16(out);
  bool wide;
  int vec = 1;
  if constexpr (sizeof(R) == 4) {
    wide = base16 && N % 2 == 0 && ldb % 2 == 0 && ldo % 2 == 0;
    if (wide) vec = 2;
  } else {
    wide = base16 && aligned16(a_data);
  }
  // the row's lanes: the power of two (16 / 32 / 64) that covers N in one pass if possible; wider results take up to four
  // column groups per lane, so that A is read once per G * 16 * CH bytes of a result row
  const int64_t lanes = ceil_div(N, vec);
  const int g = lanes <= 16 ? 16 : (lanes <= 32 ? 32 : 64);
  const int64_t groups = ceil_div(N, (int64_t)g * vec);
  const int ch = groups >= 4 ? 4 : (groups >= 2 ? 2 : 1);
#define SPAMD_CCASE(V, GG, W)                                                                                            \
  if (vec == V && g == GG && wide == W) {                                                                                \
    if (ch == 4) return launch_complex_rowgroup<R, I, V, GG, EXACT, 4, W>(M, N, a_data, a_idx, a_ptr, b, ldb, out, ldo, s); \
    if (ch == 2) return launch_complex_rowgroup<R, I, V, GG, EXACT, 2, W>(M, N, a_data, a_idx, a_ptr, b, ldb, out, ldo, s); \
    return launch_complex_rowgroup<R, I, V, GG, EXACT, 1, W>(M, N, a_data, a_idx, a_ptr, b, ldb, out, ldo, s);           \
  }
  SPAMD_CCASE(1, 16, false)
  SPAMD_CCASE(1, 32, false)
  SPAMD_CCASE(1, 64, false)
  if constexpr (sizeof(R) == 4) {
    SPAMD_CCASE(2, 16, true)
    SPAMD_CCASE(2, 32, true)
    SPAMD_CCASE(2, 64, true)
  } else {
    SPAMD_CCASE(1, 16, true)
    SPAMD_CCASE(1, 32, true)
    SPAMD_CCASE(1, 64, true)
  }
#undef SPAMD_CCASE
  return SPAMD_EINVAL;
}

template <typename R, typename I>
static int spmm_csr_complex_typed(int64_t M, int64_t N, const void* a_data, const void* a_indices, const void* a_indptr,
                                  const void* b, int64_t ldb, void* out, int64_t ldo, unsigned flags, hipStream_t s) {
  const R* ad = (const R*)a_data;
  const I* ai = (const I*)a_indices;
  const I* ap = (const I*)a_indptr;
  const R* bb = (const R*)b;
  R* oo = (R*)out;
  // interleaved pairs are read 8 bytes at a time at least
  if (((uintptr_t)a_data | (uintptr_t)b | (uintptr_t)out) & 7) return SPAMD_EINVAL;
  if (flags & SPAMD_EXACT_MULADD) return dispatch_complex_shape<R, I, true>(M, N, ad, ai, ap, bb, ldb, oo, ldo, s);
  if (N <= crowvec_max_n<R>() && !(flags & SPAMD_SPMM_ROWGROUP)) return launch_complex_rowvec<R, I>(M, N, ad, ai, ap, bb, ldb, oo, ldo, s);
  return dispatch_complex_shape<R, I, false>(M, N, ad, ai, ap, bb, ldb, oo, ldo, s);
}

}  // namespace spamd

extern "C" int spamd_spmm_csr_complex(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t N, const void* a_data,
                                      const void* a_indices, const void* a_indptr, const void* b, int64_t ldb, void* out,
                                      int64_t ldo, unsigned flags, void* stream) {
  using namespace spamd;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (M < 0 || K < 0 || N < 0) return SPAMD_EINVAL;
  if (M == 0 || N == 0) return 0;
  if (!a_indptr || !out || ldo < N || (K > 0 && (!b || ldb < N))) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (val_dtype == SPAMD_C64) {
    SPAMD_DISPATCH_IDX(idx_dtype, I, return (spmm_csr_complex_typed<float, I>(M, N, a_data, a_indices, a_indptr, b, ldb, out, ldo, flags, s)))
  } else {
    SPAMD_DISPATCH_IDX(idx_dtype, I, return (spmm_csr_complex_typed<double, I>(M, N, a_data, a_indices, a_indptr, b, ldb, out, ldo, flags, s)))
  }
  return SPAMD_ETYPE;
}

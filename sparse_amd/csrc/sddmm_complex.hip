// A9 for complex64 / complex128 operands:  out[n] = s[n] * sum_k A[i_n, k] * Bt[j_n, k]  (no conjugation: the reference's
// `s * (a @ b)`, examples/sddmm_example.py:51-52, at the mask's coordinates).
//
// The kernels are the complex twins of sddmm.hip's gather and row-cached kernels, in a file of their own so that the real
// kernels' code objects stay as they are.  A row of K complex values is K interleaved (re, im) pairs: a 16-byte load holds
// two complex64 or one complex128.  One term is four fused multiply-adds on separate accumulators,
//   re = fma(ar, br, re); re = fma(-ai, bi, re); im = fma(ar, bi, im); im = fma(ai, br, im)
// (fp32 for complex64, fp64 for complex128), the lane reduction runs on both parts, and the mask value is applied with one
// complex multiply (`Cplx`'s operator*: four rounded products).  Gather-bound like the real kernels: 2 * K * sizeof(complex)
// bytes per stored element.  No matrix-core tiles (there is no complex MFMA), no LDS-staged panel kernel, no conjugating form.
#include "sddmm_common.h"
#include "complex_ops.h"
#include <algorithm>

namespace spamd {

template <typename R>
using CxVec = Vec<R, 16 / (int)sizeof(R)>;   // 16 bytes: (re, im, re, im) of complex64, (re, im) of complex128

// (re, im) += the complex products of the pairs of two 16-byte vectors
template <typename R>
__device__ __forceinline__ void cx_fma(const CxVec<R>& a, const CxVec<R>& b, R& re, R& im) {
  constexpr int EPL = 16 / (int)sizeof(R);
#pragma unroll
  for (int e = 0; e < EPL; e += 2) {
    re = fma_r<R>(a.v[e], b.v[e], re);
    re = fma_r<R>(-a.v[e + 1], b.v[e + 1], re);
    im = fma_r<R>(a.v[e], b.v[e + 1], im);
    im = fma_r<R>(a.v[e + 1], b.v[e], im);
  }
}

// s * acc as it is stored: a zero part is written as +0 whatever the signs of the mask value ((-0) + (+0) = +0), so that a
// result of a zero mask value, a zero row or an all-(-0.0) operand has the bits of the fill value and is pruned
template <typename R>
__device__ __forceinline__ Cplx<R> cx_scaled(Cplx<R> s, Cplx<R> acc) {
  return s * acc + Cplx<R>{R(0), R(0)};
}

// Gather form, any K: LPN lanes of a wave own one stored element and stream its two rows with 16-byte loads; UNR stored
// elements per lane group are in flight (all their row loads are issued before any FMA).  Elements past nnz are clamped
// to the last one and not stored.
template <typename R, typename I, int LPN, int UNR>
__global__ void __launch_bounds__(256)
sddmm_complex_kernel(int64_t nnz, const I* __restrict__ rows, const I* __restrict__ cols, const Cplx<R>* __restrict__ s_data,
                     const Cplx<R>* __restrict__ A, int64_t lda, const Cplx<R>* __restrict__ Bt, int64_t ldb, int64_t K,
                     Cplx<R>* __restrict__ out) {
  using VT = CxVec<R>;
  constexpr int CPL = 16 / (int)sizeof(Cplx<R>);  // complex elements per 16-byte load
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPN;
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPN;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / LPN;
  const int64_t kvec = (K / CPL) * CPL;
  for (int64_t n0 = group * UNR; n0 < nnz; n0 += ngroups * UNR) {
    const Cplx<R>* ar[UNR];
    const Cplx<R>* br[UNR];
    R re[UNR], im[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t n = (n0 + u < nnz) ? (n0 + u) : (nnz - 1);  // clamp: duplicates are not stored
      ar[u] = A + (int64_t)rows[n] * lda;
      br[u] = Bt + (int64_t)cols[n] * ldb;
      re[u] = 0;
      im[u] = 0;
    }
    for (int64_t k = (int64_t)sub * CPL; k + CPL <= K; k += (int64_t)LPN * CPL) {
      VT av[UNR], bv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        av[u] = *reinterpret_cast<const VT*>(ar[u] + k);
        bv[u] = *reinterpret_cast<const VT*>(br[u] + k);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) cx_fma<R>(av[u], bv[u], re[u], im[u]);
    }
    // tail (complex64 with odd K: one element past the whole vectors), on the lane whose turn it is
    if constexpr (CPL > 1) {
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        for (int64_t kk = kvec + sub; kk < K; kk += LPN) {
          const Cplx<R> x = ar[u][kk], y = br[u][kk];
          re[u] = fma_r<R>(x.re, y.re, re[u]);
          re[u] = fma_r<R>(-x.im, y.im, re[u]);
          im[u] = fma_r<R>(x.re, y.im, im[u]);
          im[u] = fma_r<R>(x.im, y.re, im[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int off = LPN / 2; off > 0; off >>= 1) {
        re[u] += __shfl_xor(re[u], off, 64);
        im[u] += __shfl_xor(im[u], off, 64);
      }
      if (sub == 0 && n0 + u < nnz) out[n0 + u] = cx_scaled<R>(s_data[n0 + u], Cplx<R>{re[u], im[u]});
    }
  }
}

// <a, b> of a lane group over KS vectors per lane, both parts summed over the group and left in every lane.  One sum over
// the lanes' whole shares for every row length (the real kernels' two-half sum of 1 KB rows belongs to the two-pass panel
// kernel, which has no complex form).
template <typename R, int LPN, int KS>
__device__ __forceinline__ Cplx<R> cx_dot_group(const CxVec<R> (&av)[KS], const CxVec<R> (&bv)[KS]) {
  R re = 0, im = 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) cx_fma<R>(av[s], bv[s], re, im);
  return Cplx<R>{sd_group_sum<LPN>(re), sd_group_sum<LPN>(im)};
}

// Elements base .. base+3 of a step (see sddmm_complex_rowcache_kernel): the four Bt rows are requested first, then each
// element is finished in turn; the A row is (re)loaded only when the element's row differs from the one in registers.
// U0 >= 0: base = U0, row / column come from lane U0 + k of the group by DPP or shuffle.  U0 < 0 (64 lanes: the group is
// the wave): base = u0 at run time, wave-uniform, and row / column are read with v_readlane into scalar registers - one
// batch at a time, so that a step does not hold 64 rows and columns in scalar registers at once.
template <typename R, typename I, int LPN, int KS, int U0>
__device__ __forceinline__ void cx_batch4(int cnt, int u0, int sub, I myrow, I mycol, const char* Ab, const char* Bb,
                                          int64_t lda_b, int64_t ldb_b, int64_t koff_b, I& cur, CxVec<R> (&av)[KS],
                                          Cplx<R>& res) {
  using VT = CxVec<R>;
  constexpr int64_t step_b = (int64_t)LPN * 16;
  const int base = U0 < 0 ? u0 : U0;
  VT bv[4][KS];
  I r[4];
#define CX_LOAD(k)                                                                                            \
  {                                                                                                           \
    I c;                                                                                                      \
    if constexpr (U0 < 0) {                                                                                   \
      c = wave_bcast(mycol, base + k);                                                                        \
      r[k] = wave_bcast(myrow, base + k);                                                                     \
    } else {                                                                                                  \
      c = sd_bcast<LPN, U0 + k>(mycol);                                                                       \
      r[k] = sd_bcast<LPN, U0 + k>(myrow);                                                                    \
    }                                                                                                         \
    const char* bp = Bb + ((int64_t)c * ldb_b + koff_b);                                                      \
    _Pragma("unroll") for (int s = 0; s < KS; ++s) bv[k][s] = *reinterpret_cast<const VT*>(bp + s * step_b); \
  }
  CX_LOAD(0) CX_LOAD(1) CX_LOAD(2) CX_LOAD(3)
#undef CX_LOAD
#define CX_DOT(k)                                                                                             \
  if (base + k < cnt) {                                                                                       \
    if (r[k] != cur) {                                                                                        \
      cur = r[k];                                                                                             \
      const char* ap = Ab + ((int64_t)cur * lda_b + koff_b);                                                  \
      _Pragma("unroll") for (int s = 0; s < KS; ++s) av[s] = *reinterpret_cast<const VT*>(ap + s * step_b);  \
    }                                                                                                         \
    const Cplx<R> t = cx_dot_group<R, LPN, KS>(av, bv[k]);                                                    \
    res.re = sub == base + k ? t.re : res.re;                                                                 \
    res.im = sub == base + k ? t.im : res.im;                                                                 \
  }
  CX_DOT(0) CX_DOT(1) CX_DOT(2) CX_DOT(3)
#undef CX_DOT
}

template <typename R, typename I, int LPN, int KS, int U0>
struct CxStep {
  template <typename... Args>
  static __device__ __forceinline__ void run(int cnt, Args&... args) {
    if constexpr (LPN == 64) {
      const int n = uniform(cnt);
#pragma unroll 1
      for (int u0 = 0; u0 < n; u0 += 4) cx_batch4<R, I, LPN, KS, -1>(n, u0, args...);
    } else if constexpr (U0 < LPN) {
      if (U0 < cnt) cx_batch4<R, I, LPN, KS, U0>(cnt, U0, args...);
      CxStep<R, I, LPN, KS, U0 + 4>::run(cnt, args...);
    }
  }
};

// a (re, im) pair as one 8- or 16-byte access with the non-temporal hint
template <typename R>
__device__ __forceinline__ Cplx<R> cx_load_nt(const Cplx<R>* p) {
  const typename ExtVec<R, 2>::type x = __builtin_nontemporal_load(reinterpret_cast<const typename ExtVec<R, 2>::type*>(p));
  return Cplx<R>{x[0], x[1]};
}
template <typename R>
__device__ __forceinline__ void cx_store_nt(Cplx<R>* p, Cplx<R> v) {
  typename ExtVec<R, 2>::type x;
  x[0] = v.re;
  x[1] = v.im;
  __builtin_nontemporal_store(x, reinterpret_cast<typename ExtVec<R, 2>::type*>(p));
}

// Row-cached form, rows of exactly LPN * KS vectors: a lane group walks a CONTIGUOUS chunk of stored elements LPN at a
// time.  Lane u of the group loads element u's row, column, mask value (and output position) - one coalesced load per
// array and step; row / column are broadcast across the group, the A row of consecutive elements is usually the same one
// and stays in registers (KS vectors per lane), four Bt rows are in flight, the group's sums land in lane u, and ONE store
// per step writes the LPN results.
//
// PERM (column-panel order): rows / cols / s_data come in panel order, `perm[n]` is the element's position in out, and
// every lane group takes one short chunk; with `xstate` (first[9]) workgroup b takes piece b / 8 of the range of XCD b % 8
// (see sddmm_rowcache_kernel in sddmm.hip).  Every stored element is computed by the same lanes in the same order as
// without PERM, so the two orders give the same bits.
template <typename R, typename I, int LPN, int KS, bool PERM>
__global__ void __launch_bounds__(256)
sddmm_complex_rowcache_kernel(int64_t nnz, int64_t chunk, const I* __restrict__ rows, const I* __restrict__ cols,
                              const Cplx<R>* __restrict__ s_data, const Cplx<R>* __restrict__ A, int64_t lda,
                              const Cplx<R>* __restrict__ Bt, int64_t ldb, Cplx<R>* __restrict__ out,
                              const int64_t* __restrict__ perm, const int64_t* __restrict__ xstate) {
  using VT = CxVec<R>;
  static_assert(LPN % 4 == 0, "whole batches of four per step");
  const int sub = (threadIdx.x & 63) % LPN;
  // elements [cbeg0, cbeg0 + chunk), then every `cstride`-th chunk after it, below nnz_end
  int64_t cbeg0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPN) * chunk;
  int64_t cstride = ((int64_t)gridDim.x * blockDim.x / LPN) * chunk;
  int64_t nnz_end = nnz;
  if constexpr (PERM) {
    if (xstate) {
      __shared__ int64_t piece_s[2];
      const int64_t piece = (int64_t)(blockDim.x / LPN) * chunk;
      const int x = (int)(blockIdx.x & 7u);
      const int64_t lo = (int64_t)xstate[x], hi = (int64_t)xstate[x + 1];
      const int64_t b = lo + (int64_t)(blockIdx.x >> 3) * piece;
      if (threadIdx.x == 0) {
        piece_s[0] = b < hi ? b : 0;
        piece_s[1] = b < hi ? (b + piece < hi ? b + piece : hi) : 0;
      }
      __syncthreads();
      cbeg0 = piece_s[0] + (int64_t)(threadIdx.x / LPN) * chunk;
      cstride = (int64_t)1 << 40;   // one chunk per lane group
      nnz_end = piece_s[1];
    }
  }
  const char* const Ab = reinterpret_cast<const char*>(A);
  const char* const Bb = reinterpret_cast<const char*>(Bt);
  const int64_t lda_b = lda * (int64_t)sizeof(Cplx<R>), ldb_b = ldb * (int64_t)sizeof(Cplx<R>);
  const int64_t koff_b = (int64_t)sub * 16;
  I cur = (I)-1;
  VT av[KS];
  for (int64_t cbeg = cbeg0; cbeg < nnz_end; cbeg += cstride) {
    const int64_t cend = cbeg + chunk < nnz_end ? cbeg + chunk : nnz_end;
    for (int64_t nbeg = cbeg; nbeg < cend; nbeg += LPN) {
      const int cnt = (int)(cend - nbeg < LPN ? cend - nbeg : LPN);  // uniform inside the group
      const bool mine = sub < cnt;
      const int64_t nl = nbeg + (mine ? sub : 0);
      // (panel order: the mask's arrays are a once-through stream)
      const I myrow = PERM ? __builtin_nontemporal_load(rows + nl) : rows[nl];
      const I mycol = PERM ? __builtin_nontemporal_load(cols + nl) : cols[nl];
      const Cplx<R> mys = PERM ? cx_load_nt<R>(s_data + nl) : s_data[nl];
      int64_t mypos = nl;
      if constexpr (PERM) mypos = __builtin_nontemporal_load(perm + nl);
      Cplx<R> res{0, 0};
      int lane_in_group = sub;
      CxStep<R, I, LPN, KS, 0>::run(cnt, lane_in_group, myrow, mycol, Ab, Bb, lda_b, ldb_b, koff_b, cur, av, res);
      if (mine) {
        const Cplx<R> v = cx_scaled<R>(mys, res);
        if constexpr (PERM) cx_store_nt<R>(out + mypos, v);  // scattered: keep these lines from displacing the Bt panel in L2
        else out[mypos] = v;
      }
    }
  }
}

// (L, KS) of the row-cached kernel for rows of `vecs` 16-byte vectors - the first L of 16, 32, 64 with vecs = L * KS,
// KS in 1..4 - or false
static bool cx_rowcache_shape(int64_t vecs, int& L, int& ks) {
  for (L = 16; L <= 64; L <<= 1) {
    if (vecs % L) continue;
    const int64_t q = vecs / L;
    if (q >= 1 && q <= 4) {
      ks = (int)q;
      return true;
    }
  }
  return false;
}

template <typename R, typename I>
static int launch_sddmm_complex(int64_t nnz, const I* rows, const I* cols, const Cplx<R>* s, const Cplx<R>* A, int64_t lda,
                                const Cplx<R>* Bt, int64_t ldb, int64_t K, Cplx<R>* out, hipStream_t st, const int64_t* perm,
                                int64_t perm_chunk, const int64_t* xstate, int64_t xmax) {
  constexpr int CPL = 16 / (int)sizeof(Cplx<R>);
  const int64_t vecs = K / CPL;
  int L = 0, ks = 0;
  if (K > 0 && K % CPL == 0 && cx_rowcache_shape(vecs, L, ks)) {
    // the launch geometry of launch_sddmm (sddmm.hip)
    const int64_t groups_wanted = 256 * 16 * (256 / L);  // 16 workgroups per CU
    int64_t chunk = ceil_div(nnz, groups_wanted);
    chunk = ceil_div(chunk, (int64_t)L) * L;  // whole steps of L elements
    if (perm) {
      const int64_t want = perm_chunk > 0 ? ceil_div(perm_chunk, (int64_t)L) * L : (int64_t)L;
      if (chunk > want) chunk = want;
    }
    const int64_t groups = perm ? ceil_div(nnz, chunk) : std::min(ceil_div(nnz, chunk), groups_wanted);
    int64_t blocks = ceil_div(groups * L, (int64_t)256);
    if (perm && xstate)   // a piece per workgroup, eight workgroups (one per XCD) per piece index
      blocks = 8 * std::max<int64_t>(ceil_div(xmax, (int64_t)(256 / L) * chunk), 1);
#define CXL(LL, KK, PP)                                                                                         \
  hipLaunchKernelGGL((sddmm_complex_rowcache_kernel<R, I, LL, KK, PP>), dim3((unsigned)blocks), dim3(256), 0, st, nnz, \
                     chunk, rows, cols, s, A, lda, Bt, ldb, out, perm, xstate)
#define CXR(LL, KK)                                                                                             \
  if (L == LL && ks == KK) {                                                                                    \
    if (perm) CXL(LL, KK, true);                                                                                \
    else CXL(LL, KK, false);                                                                                    \
    return launch_status();                                                                                     \
  }
    // (the pairs cx_rowcache_shape can return: 32 or 64 lanes with one or two vectors are rows that 16 lanes take)
    CXR(16, 1) CXR(16, 2) CXR(16, 3) CXR(16, 4) CXR(32, 3) CXR(32, 4) CXR(64, 3) CXR(64, 4)
#undef CXR
#undef CXL
    return SPAMD_EINVAL;
  }
  if (perm) return SPAMD_EINVAL;  // the panel order exists for the row-cached kernel only
  int lpn = 4;
  while (lpn < 64 && vecs > lpn * 2) lpn <<= 1;  // ~2 vector loads per lane per operand
  constexpr int UNR = 4;
  int64_t blocks = ceil_div(ceil_div(nnz, UNR) * lpn, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (blocks < 1) blocks = 1;
#define CXG(LL)                                                                                                 \
  if (lpn == LL) {                                                                                              \
    hipLaunchKernelGGL((sddmm_complex_kernel<R, I, LL, UNR>), dim3((unsigned)blocks), dim3(256), 0, st, nnz, rows, cols, s, \
                       A, lda, Bt, ldb, K, out);                                                                \
    return launch_status();                                                                                     \
  }
  CXG(4) CXG(8) CXG(16) CXG(32) CXG(64)
#undef CXG
  return SPAMD_EINVAL;
}

}  // namespace spamd

using namespace spamd;

// 1 when rows of K elements of val_dtype (SPAMD_C64 | SPAMD_C128) have a row-cached kernel - what the column-panel
// order (perm != NULL) of spamd_sddmm_complex needs -, else 0.
extern "C" int spamd_sddmm_complex_has_rowcache(int val_dtype, int64_t K) {
  const int esz = val_dtype == SPAMD_C64 ? 8 : (val_dtype == SPAMD_C128 ? 16 : 0);
  if (!esz || K <= 0 || (K * esz) % 16) return 0;
  int L = 0, ks = 0;
  return cx_rowcache_shape(K * esz / 16, L, ks) ? 1 : 0;
}

extern "C" int spamd_sddmm_complex(int val_dtype, int idx_dtype, int64_t nnz, const void* rows, const void* cols,
                                   const void* s_data, const void* A, int64_t lda, const void* Bt, int64_t ldb, int64_t K,
                                   void* out, const int64_t* perm, int64_t perm_chunk, const int64_t* xstate, int64_t xmax,
                                   void* stream) {
  if (nnz < 0 || K < 0 || lda < 0 || ldb < 0 || perm_chunk < 0 || (xstate && xmax < 0)) return SPAMD_EINVAL;
  if (nnz == 0) return 0;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  const int esz = val_dtype == SPAMD_C64 ? 8 : 16;
  if (((uintptr_t)A % 16) || ((uintptr_t)Bt % 16) || ((uintptr_t)s_data % esz) || ((uintptr_t)out % esz)) return SPAMD_EINVAL;
  if ((lda * esz) % 16 || (ldb * esz) % 16 || lda < K || ldb < K) return SPAMD_EINVAL;
  if (perm && !spamd_sddmm_complex_has_rowcache(val_dtype, K)) return SPAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    const I* r = (const I*)rows;
    const I* c = (const I*)cols;
    if (val_dtype == SPAMD_C64)
      return launch_sddmm_complex<float, I>(nnz, r, c, (const Cplx<float>*)s_data, (const Cplx<float>*)A, lda,
                                            (const Cplx<float>*)Bt, ldb, K, (Cplx<float>*)out, st, perm, perm_chunk, xstate, xmax);
    return launch_sddmm_complex<double, I>(nnz, r, c, (const Cplx<double>*)s_data, (const Cplx<double>*)A, lda,
                                           (const Cplx<double>*)Bt, ldb, K, (Cplx<double>*)out, st, perm, perm_chunk, xstate, xmax);
  })
  return SPAMD_ETYPE;
}

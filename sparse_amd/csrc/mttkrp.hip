// A12  MTTKRP: the matricised tensor times Khatri-Rao product of an N-D COO tensor with N - 1 dense factor matrices,
//   out[i, r] = sum over the stored elements n with coords[mode][n] == i of data[n] * prod_{d != mode} U_d[coords[d][n], r]
// (the reference writes it as two broadcast multiplies and a sum, examples/mttkrp_example.py; fused it reads the tensor
// once plus N - 1 gathered factor rows per stored element and forms no intermediate).
//
// The stored elements come grouped by coords[mode]: rowptr[i] .. rowptr[i + 1] are the positions of row i in plan order,
// perm[] maps a plan position to a stored position (NULL: the stored order is the plan order - mode 0 of a canonical COO).
//
// Order (the contract the tests restate, bit for bit under SPAMD_EXACT_MULADD):
//   a term   t = data[n]; for d ascending, d != mode: t = t * U_d[coords[d][n], r]
//   a row    its elements, in plan order, are cut into pieces of `chunk`; a piece is summed sequentially from +0.0, the
//            piece sums are added in piece order.  A row of at most `chunk` elements is one sequential sum.
// Without SPAMD_EXACT_MULADD the last multiply of a term and the accumulate are one fma.
//
// Lanes run along r: a sub-group of G lanes (16 | 32 | 64, the smallest that holds R, 64 beyond) owns one row piece, so a
// factor-row gather is one contiguous segment per stored element and the sub-groups of a wave walk DIFFERENT rows - the sum
// order never depends on the lane mapping.  Every out element is written once, by one lane; there is no atomic anywhere.
//
// Launches:
//   1. mttkrp_kernel, two block ranges.  Row blocks: one sub-group per row; rows of at most `chunk` elements are finished
//      (empty rows store +0.0), longer rows are left alone.  Window blocks (only when nnz > chunk): sub-group g walks the
//      window g of `chunk` plan positions (csrc/segment_walk.h): at most two pieces of longer rows START inside it, found
//      with two binary searches over rowptr; their sums go to the workspace slots 2g and 2g + 1 - no piece list, no count
//      brought back to the host.
//   2. mttkrp_join_kernel (only when nnz > chunk): one sub-group per row; a row of more than `chunk` elements adds its
//      piece sums in piece order and stores the result.
#include "segments.h"

#define MTTKRP_MAX_NDIM 8

namespace spamd {

template <typename T, typename I>
struct MtArgs {
  const I* c[MTTKRP_MAX_NDIM - 1];   // coordinate rows of the dimensions d != mode, d ascending
  const T* U[MTTKRP_MAX_NDIM - 1];   // their factors
  int64_t ld[MTTKRP_MAX_NDIM - 1];   // row pitches, in elements
  int nf;                            // ndim - 1
};

template <bool EXACT, typename T>
__device__ __forceinline__ T mt_mul(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}

// acc[j] (+)= the terms of the plan positions [b, e) at the columns col0 + sub + j * G, in plan order.
// The sub-group takes G positions per step: lane u loads position u's value and factor-row offsets (one coalesced load per
// array when perm == NULL, one gather through perm otherwise), so the loads that depend on an index are issued once per G
// elements and not once per element; the elements are then finished in order, UNR at a time: their value and offsets come
// from lane u by a shuffle, the UNR x nf factor-row loads are in flight together, the accumulation stays sequential.
template <typename T, typename I, bool EXACT, int NF, int G, int CPL>
__device__ __forceinline__ void mt_piece(const MtArgs<T, I>& a, const T* __restrict__ data, const int64_t* __restrict__ perm,
                                         int64_t b, int64_t e, int64_t col0, int sub, int64_t R, T (&acc)[CPL]) {
  constexpr int UNR = NF > 0 ? 4 : 2;   // (the generic form holds UNR x 7 factor values per column in registers)
  constexpr int FMAX = NF > 0 ? NF : MTTKRP_MAX_NDIM - 1;
  const int nf = NF > 0 ? NF : a.nf;
  const int lane0 = (int)(threadIdx.x & 63) - sub;   // the sub-group's first lane in the wave
  bool on[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) on[j] = col0 + sub + (int64_t)j * G < R;
  for (int64_t n0 = b; n0 < e; n0 += G) {
    const int cnt = (int)(e - n0 < G ? e - n0 : G);   // the same in every lane of the sub-group
    const int64_t nl = n0 + (sub < cnt ? sub : cnt - 1);
    const int64_t p = perm ? perm[nl] : nl;
    const T myv = data[p];
    int64_t myoff[FMAX];
#pragma unroll
    for (int f = 0; f < FMAX; ++f) myoff[f] = f < nf ? (int64_t)a.c[f][p] * a.ld[f] : 0;
    for (int u0 = 0; u0 < cnt; u0 += UNR) {
      T t[UNR];
      T x[UNR][FMAX][CPL];
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        const int u = u0 + k < cnt ? u0 + k : cnt - 1;   // past the end: the last element again, loaded and not added
        t[k] = __shfl(myv, lane0 + u, 64);
#pragma unroll
        for (int f = 0; f < FMAX; ++f) {
          if (f < nf) {
            const T* rowp = a.U[f] + __shfl(myoff[f], lane0 + u, 64) + (col0 + sub);
#pragma unroll
            for (int j = 0; j < CPL; ++j) x[k][f][j] = on[j] ? rowp[(int64_t)j * G] : T(0);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        if (u0 + k < cnt) {
#pragma unroll
          for (int j = 0; j < CPL; ++j) {
            T tt = t[k];
#pragma unroll
            for (int f = 0; f < FMAX; ++f)
              if (f + 1 < nf) tt = mt_mul<EXACT, T>(tt, x[k][f][j]);   // all but the last factor: rounded products
            T last = x[k][0][j];
#pragma unroll
            for (int f = 1; f < FMAX; ++f)
              if (f == nf - 1) last = x[k][f][j];
            acc[j] = mul_add<EXACT, T>(tt, last, acc[j]);
          }
        }
      }
    }
  }
}

// the sum of [b, e) at every column, stored to dst[r * 1] (dst: a row of out or a workspace slot)
template <typename T, typename I, bool EXACT, int NF, int G, int CPL>
__device__ __forceinline__ void mt_piece_to(const MtArgs<T, I>& a, const T* __restrict__ data, const int64_t* __restrict__ perm,
                                            int64_t b, int64_t e, int sub, int64_t R, T* __restrict__ dst) {
  for (int64_t col0 = 0; col0 < R; col0 += (int64_t)G * CPL) {
    T acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = T(0);
    mt_piece<T, I, EXACT, NF, G, CPL>(a, data, perm, b, e, col0, sub, R, acc);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int64_t r = col0 + sub + (int64_t)j * G;
      if (r < R) dst[r] = acc[j];
    }
  }
}

template <typename T, typename I, bool EXACT, int NF, int G, int CPL>
__global__ void __launch_bounds__(256)
mttkrp_kernel(MtArgs<T, I> a, int64_t nnz, int64_t nrows, int64_t R, const T* __restrict__ data,
              const int64_t* __restrict__ perm, const int64_t* __restrict__ rowptr, int64_t chunk, int64_t row_blocks,
              T* __restrict__ ws, T* __restrict__ out, int64_t ldo) {
  constexpr int GPB = 256 / G;   // sub-groups per workgroup
  const int sub = threadIdx.x % G;
  const int gib = threadIdx.x / G;
  if ((int64_t)blockIdx.x < row_blocks) {
    for (int64_t row = (int64_t)blockIdx.x * GPB + gib; row < nrows; row += row_blocks * GPB) {
      const int64_t b = rowptr[row], e = rowptr[row + 1];
      if (e - b > chunk) continue;   // pieces: the window blocks and the join
      mt_piece_to<T, I, EXACT, NF, G, CPL>(a, data, perm, b, e, sub, R, out + row * ldo);
    }
    return;
  }
  const int64_t nwin = (nnz + chunk - 1) / chunk;
  const int64_t win_blocks = (int64_t)gridDim.x - row_blocks;
  for (int64_t g = ((int64_t)blockIdx.x - row_blocks) * GPB + gib; g < nwin; g += win_blocks * GPB)
    seg_window_pieces(rowptr, nrows, nnz, chunk, g, [&](int64_t, int64_t b, int64_t s, int64_t e) {
      mt_piece_to<T, I, EXACT, NF, G, CPL>(a, data, perm, s, e, sub, R, ws + seg_slot(b, s, chunk) * R);
    });
}

template <typename T, int G>
__global__ void __launch_bounds__(256)
mttkrp_join_kernel(int64_t nrows, int64_t R, const int64_t* __restrict__ rowptr, int64_t chunk, const T* __restrict__ ws,
                   T* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  constexpr int GPB = 256 / G;
  const int sub = threadIdx.x % G;
  for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < nrows; row += (int64_t)gridDim.x * GPB) {
    const int64_t b = rowptr[row], e = rowptr[row + 1];
    if (e - b <= chunk) continue;
    for (int64_t r = sub; r < R; r += G) {
      T s = ws[seg_slot(b, b, chunk) * R + r];
      for (int64_t p = b + chunk; p < e; p += chunk) s = s + ws[seg_slot(b, p, chunk) * R + r];
      out[row * ldo + r] = s;
    }
  }
}

template <typename T, typename I, bool EXACT, int NF, int G, int CPL>
static int launch_mttkrp_as(const MtArgs<T, I>& a, int64_t nnz, int64_t nrows, int64_t R, const T* data, const int64_t* perm,
                            const int64_t* rowptr, int64_t chunk, T* ws, T* out, int64_t ldo, hipStream_t st) {
  constexpr int GPB = 256 / G;
  const int64_t row_blocks = seg_grid(nrows, GPB);   // (nrows > 0: the entry returns before)
  const bool pieces = nnz > chunk;
  const int64_t win_blocks = pieces ? seg_grid(ceil_div(nnz, chunk), GPB) : 0;
  SPAMD_LAUNCH((mttkrp_kernel<T, I, EXACT, NF, G, CPL>), dim3((unsigned)(row_blocks + win_blocks)), dim3(256), 0, st, a, nnz, nrows, R, data,
               perm, rowptr, chunk, row_blocks, ws, out, ldo);
  if (pieces)
    SPAMD_LAUNCH((mttkrp_join_kernel<T, G>), dim3((unsigned)row_blocks), dim3(256), 0, st, nrows, R, rowptr, chunk, (const T*)ws, out, ldo);
  return 0;
}

template <typename T, typename I, bool EXACT>
static int launch_mttkrp(const MtArgs<T, I>& a, int64_t nnz, int64_t nrows, int64_t R, const T* data, const int64_t* perm,
                         const int64_t* rowptr, int64_t chunk, T* ws, T* out, int64_t ldo, hipStream_t st) {
#define MT_GO(NF, G, CPL) \
  return launch_mttkrp_as<T, I, EXACT, NF, G, CPL>(a, nnz, nrows, R, data, perm, rowptr, chunk, ws, out, ldo, st)
  // (NF = 2: the three-mode tensor of CP / PARAFAC gets its factor loop unrolled; 0: the loop runs over a.nf)
  if (a.nf == 2) {
    if (R <= 16) MT_GO(2, 16, 1);
    if (R <= 32) MT_GO(2, 32, 1);
    if (R <= 64) MT_GO(2, 64, 1);
    MT_GO(2, 64, 2);
  }
  if (R <= 16) MT_GO(0, 16, 1);
  if (R <= 32) MT_GO(0, 32, 1);
  if (R <= 64) MT_GO(0, 64, 1);
  MT_GO(0, 64, 2);
#undef MT_GO
}

template <typename T>
__global__ void mttkrp_zero_kernel(int64_t nrows, int64_t R, T* __restrict__ out, int64_t ldo) {
  const int64_t n = nrows * R;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[(i / R) * ldo + i % R] = T(0);
}

template <typename T, typename I>
static int mttkrp_typed(int ndim, int mode, int64_t nnz, int64_t R, const void* coords, int64_t ldc, const void* data,
                        const void* const* factors, const int64_t* pitches, const int64_t* perm, const int64_t* rowptr,
                        int64_t nrows, int64_t chunk, void* ws, void* out, int64_t ldo, unsigned flags, hipStream_t st) {
  if (nnz == 0) {
    const int64_t n = nrows * R;
    SPAMD_LAUNCH((mttkrp_zero_kernel<T>), dim3(seg_grid(n, 256, 65536)), dim3(256), 0, st, nrows, R, (T*)out, ldo);
    return 0;
  }
  MtArgs<T, I> a;
  a.nf = 0;
  for (int d = 0; d < ndim; ++d) {
    if (d == mode) continue;
    if (!factors[d] || pitches[d] < R) return SPAMD_EINVAL;
    a.c[a.nf] = (const I*)coords + (int64_t)d * ldc;
    a.U[a.nf] = (const T*)factors[d];
    a.ld[a.nf] = pitches[d];
    ++a.nf;
  }
  for (int f = a.nf; f < MTTKRP_MAX_NDIM - 1; ++f) {
    a.c[f] = nullptr;
    a.U[f] = nullptr;
    a.ld[f] = 0;
  }
  if (flags & SPAMD_EXACT_MULADD)
    return launch_mttkrp<T, I, true>(a, nnz, nrows, R, (const T*)data, perm, rowptr, chunk, (T*)ws, (T*)out, ldo, st);
  return launch_mttkrp<T, I, false>(a, nnz, nrows, R, (const T*)data, perm, rowptr, chunk, (T*)ws, (T*)out, ldo, st);
}

}  // namespace spamd

using namespace spamd;

extern "C" int64_t spamd_mttkrp_ws_bytes(int val_dtype, int64_t nnz, int64_t R, int64_t chunk) {
  const int64_t esz = val_dtype == SPAMD_F32 ? 4 : (val_dtype == SPAMD_F64 ? 8 : 0);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || R < 0 || chunk < 1) return SPAMD_EINVAL;
  if (nnz <= chunk) return 0;
  return 2 * ceil_div(nnz, chunk) * R * esz;
}

extern "C" int spamd_mttkrp(int val_dtype, int idx_dtype, int ndim, int mode, int64_t nnz, int64_t R, const void* coords,
                            int64_t ldc, const void* data, const void* const* factors, const int64_t* pitches,
                            const int64_t* perm, const int64_t* rowptr, int64_t nrows, int64_t chunk, void* ws,
                            int64_t ws_bytes, void* out, int64_t ldo, unsigned flags, void* stream) {
  if (val_dtype != SPAMD_F32 && val_dtype != SPAMD_F64) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (nnz < 0 || R < 0 || nrows < 0 || ldc < nnz || ldo < R || chunk < 1) return SPAMD_EINVAL;
  if (ndim < 2 || ndim > MTTKRP_MAX_NDIM || mode < 0 || mode >= ndim) return SPAMD_EINVAL;
  if (R == 0 || nrows == 0) return 0;
  if (!out || (nnz > 0 && (!coords || !data || !factors || !pitches || !rowptr))) return SPAMD_EINVAL;
  if (ws_bytes < spamd_mttkrp_ws_bytes(val_dtype, nnz, R, chunk) || (nnz > chunk && !ws)) return SPAMD_EWS;
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (val_dtype == SPAMD_F32)
      return mttkrp_typed<float, I>(ndim, mode, nnz, R, coords, ldc, data, factors, pitches, perm, rowptr, nrows, chunk, ws, out,
                                    ldo, flags, st);
    return mttkrp_typed<double, I>(ndim, mode, nnz, R, coords, ldc, data, factors, pitches, perm, rowptr, nrows, chunk, ws, out,
                                   ldo, flags, st);
  })
  return SPAMD_ETYPE;
}

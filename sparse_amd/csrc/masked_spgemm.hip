// A13  Masked SpGEMM: the sparse x sparse product sampled at a sparse mask,
//   out[e] = m[e] * sum over k stored in BOTH row i of A and column j of B of A[i, k] * B[k, j]       (i, j) = mask position e
// (the reference writes it as s * (a @ b), examples/triangles_example.py: `sparse.sum(a @ a * a) / 6`; that forms the whole
// product - about (mean degree) times the mask's stored elements - and intersects it with the mask afterwards.  Here the
// product is never formed: per mask element the sorted column list of A's row i is intersected with the sorted row list of
// B's column j).
//
// Forms: the mask as CSR (s_ptr, s_idx, s_val), A as CSR (a_ptr, a_idx, a_val), B as CSC (b_ptr over columns, b_idx = row
// ids, b_val) - the CSR arrays of B^T.  Index lists ascend inside a row / column and hold no duplicates.
//
// Order (the contract the tests restate, bit for bit under SPAMD_EXACT_MULADD):
//   acc = +0; for every common k, ascending: acc = acc + A[i, k] * B[k, j]; out = m * acc
// Without SPAMD_EXACT_MULADD the multiply and add of a term are one fma; the mask multiply is always its own operation;
// integers wrap.  A position without a common k gets +0 whatever m is (a NaN / inf mask value stays contained).
//
// Mapping.  The mask's stored elements, in CSR order, are cut into windows of `window` elements, whatever row they fall in:
// a wave owns a window (a row of any length is spread over as many waves as it has windows; a window of short rows walks
// them one after the other).  For each row segment of its window the wave stages the column list of A's row i in its
// share of the LDS when it has at most `cap` entries.  A sub-group of G lanes (8 | 16 | 32 | 64) owns one mask element
// (i, j) and walks column j of B G entries at a time: lane u loads its k, binary-searches it in the staged list (in global
// memory for a longer row), `__ballot` (64 bits) tells the sub-group which of its lanes matched, and the matching lanes'
// values are folded into acc in ascending lane order, i.e. ascending k - matches are rare, the chain is short.  Only
// matching lanes load values.  Every out element is written once, by the sub-group's first lane; no atomic touches a value.
// Neither G, cap nor window changes the order of any sum: every variant gives the same bits.
// The count of results whose bits are all zero (what the container's prune would otherwise count in a pass of its own) is
// added up per wave and leaves through one integer add per wave, as in the SpGEMM pack kernel.
#include "common.h"

#include <algorithm>

#define MSG_BLOCK 256
#define MSG_MAX_CAP 2048   // entries of A's row a wave stages: 4 waves x 2048 x 8 B = 64 KiB of LDS at most

namespace spamd {

template <typename T>
__device__ __forceinline__ T ms_mul(T a, T b) {
#pragma clang fp contract(off)
  if constexpr (std::is_integral<T>::value) {
    using U = typename std::make_unsigned<T>::type;   // wrap-around, as NumPy's integers
    return (T)((U)a * (U)b);
  } else {
    return a * b;
  }
}

template <bool EXACT, typename T>
__device__ __forceinline__ T ms_mul_add(T a, T b, T c) {
  if constexpr (std::is_integral<T>::value) {
    using U = typename std::make_unsigned<T>::type;
    return (T)((U)a * (U)b + (U)c);
  } else {
    return mul_add<EXACT, T>(a, b, c);
  }
}

template <typename T>
__device__ __forceinline__ bool ms_zero_bits(T v) {
  if constexpr (sizeof(T) == 8) return __builtin_bit_cast(uint64_t, v) == 0;
  else return __builtin_bit_cast(uint32_t, v) == 0;
}

// first position in [0, n) of the ascending list p[] with p[pos] >= k (n if none)
template <typename P, typename I>
__device__ __forceinline__ int64_t ms_lower_bound(P p, int64_t n, I k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (p[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// last r in [0, nrows) with ptr[r] <= pos, for 0 <= pos < ptr[nrows]: the (non-empty) row that holds position pos
template <typename I>
__device__ __forceinline__ int64_t ms_row_of(const I* __restrict__ ptr, int64_t nrows, int64_t pos) {
  int64_t lo = 0, hi = nrows - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)ptr[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <typename T, typename I, bool EXACT, int G>
__global__ void __launch_bounds__(MSG_BLOCK)
masked_spgemm_kernel(int64_t M, int64_t nnz, const I* __restrict__ s_ptr, const I* __restrict__ s_idx, const T* __restrict__ s_val,
                     const I* __restrict__ a_ptr, const I* __restrict__ a_idx, const T* __restrict__ a_val,
                     const I* __restrict__ b_ptr, const I* __restrict__ b_idx, const T* __restrict__ b_val, int64_t window,
                     int cap, T* __restrict__ out, unsigned long long* __restrict__ zeros) {
  extern __shared__ __attribute__((aligned(16))) char raw[];
  constexpr int NSG = 64 / G;                              // sub-groups per wave
  const int lane = threadIdx.x & 63;
  const int sub = lane % G, sg = lane / G;
  const int lane0 = lane - sub;                            // the sub-group's first lane in the wave
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1);
  I* __restrict__ staged = reinterpret_cast<I*>(raw) + (size_t)(threadIdx.x >> 6) * cap;   // this wave's share
  const int64_t nwin = (nnz + window - 1) / window;
  const int64_t wave = ((int64_t)blockIdx.x * MSG_BLOCK + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * MSG_BLOCK) >> 6;
  int nz = 0;
  for (int64_t w = wave; w < nwin; w += nwaves) {
    const int64_t lo = w * window;
    const int64_t hi = lo + window < nnz ? lo + window : nnz;
    int64_t row = ms_row_of(s_ptr, M, lo);
    int64_t pos = lo;
    while (pos < hi) {                                     // (wave-uniform: row, pos and every bound below)
      while ((int64_t)s_ptr[row + 1] <= pos) ++row;        // empty mask rows; ends at the latest at the row that holds hi - 1
      const int64_t rend = (int64_t)s_ptr[row + 1] < hi ? (int64_t)s_ptr[row + 1] : hi;
      const int64_t ab = a_ptr[row];
      const int64_t alen = (int64_t)a_ptr[row + 1] - ab;
      const bool in_lds = alen <= cap;
      if (in_lds) {
        for (int64_t t = lane; t < alen; t += 64) staged[t] = a_idx[ab + t];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const I* __restrict__ arow = a_idx + ab;
      for (int64_t e = pos + sg; e < rend; e += NSG) {     // one mask element per sub-group
        const int64_t j = s_idx[e];
        const int64_t bb = b_ptr[j], be = b_ptr[j + 1];
        T acc = T(0);
        bool any = false;
        if (alen > 0) {
          for (int64_t t0 = bb; t0 < be; t0 += G) {
            const int64_t t = t0 + sub;
            bool found = false;
            int64_t p = 0;
            if (t < be) {
              const I k = b_idx[t];
              p = in_lds ? ms_lower_bound(staged, alen, k) : ms_lower_bound(arow, alen, k);
              found = p < alen && (in_lds ? staged[p] : arow[p]) == k;
            }
            unsigned long long hit = (__ballot(found) >> lane0) & gmask;   // the sub-group's matching lanes
            if (hit) {
              T av = T(0), bv = T(0);
              if (found) {
                av = a_val[ab + p];
                bv = b_val[t];
              }
              any = true;
              while (hit) {                                // ascending lane = ascending k
                const int u = __builtin_ctzll(hit);
                hit &= hit - 1;
                acc = ms_mul_add<EXACT, T>(__shfl(av, lane0 + u, 64), __shfl(bv, lane0 + u, 64), acc);
              }
            }
          }
        }
        if (sub == 0) {
          const T r = any ? ms_mul<T>(s_val[e], acc) : T(0);
          out[e] = r;
          nz += ms_zero_bits(r) ? 1 : 0;
        }
      }
      __builtin_amdgcn_wave_barrier();                     // the next segment overwrites the staged list
      pos = rend;
      ++row;
    }
  }
  if (zeros) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) nz += __shfl_xor(nz, d, 64);
    if (lane == 0 && nz) atomicAdd(zeros, (unsigned long long)nz);
  }
}

template <typename T, typename I, bool EXACT, int G>
static int launch_masked_as(int64_t M, int64_t nnz, const I* s_ptr, const I* s_idx, const T* s_val, const I* a_ptr, const I* a_idx,
                            const T* a_val, const I* b_ptr, const I* b_idx, const T* b_val, int64_t window, int cap, T* out,
                            unsigned long long* zeros, hipStream_t st) {
  const int lds = (MSG_BLOCK / 64) * cap * (int)sizeof(I);
  auto kern = masked_spgemm_kernel<T, I, EXACT, G>;
  // (opted in once per device and kernel, so with the largest size any `cap` can ask for: 64 KiB with 64-bit indices)
  constexpr int lds_max = (MSG_BLOCK / 64) * MSG_MAX_CAP * (int)sizeof(I);
  if (lds > 32768)
    if (int rc = set_max_dynamic_lds((const void*)kern, lds_max)) return rc;
  const int64_t nwin = ceil_div(nnz, window);
  const int64_t blocks = std::min<int64_t>(ceil_div(nwin, MSG_BLOCK / 64), (int64_t)1 << 20);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(MSG_BLOCK), lds, st, M, nnz, s_ptr, s_idx, s_val, a_ptr, a_idx, a_val, b_ptr,
                     b_idx, b_val, window, cap, out, zeros);
  return launch_status();
}

template <typename T, typename I, bool EXACT>
static int launch_masked(int group, int64_t M, int64_t nnz, const void* s_ptr, const void* s_idx, const void* s_val, const void* a_ptr,
                         const void* a_idx, const void* a_val, const void* b_ptr, const void* b_idx, const void* b_val, int64_t window,
                         int cap, void* out, void* zeros, hipStream_t st) {
#define MSG_GO(G)                                                                                                                  \
  return launch_masked_as<T, I, EXACT, G>(M, nnz, (const I*)s_ptr, (const I*)s_idx, (const T*)s_val, (const I*)a_ptr, (const I*)a_idx, \
                                          (const T*)a_val, (const I*)b_ptr, (const I*)b_idx, (const T*)b_val, window, cap, (T*)out,    \
                                          (unsigned long long*)zeros, st)
  switch (group) {
    case 8: MSG_GO(8);
    case 16: MSG_GO(16);
    case 32: MSG_GO(32);
    case 64: MSG_GO(64);
  }
#undef MSG_GO
  return SPAMD_EINVAL;
}

}  // namespace spamd

using namespace spamd;

extern "C" int spamd_masked_spgemm(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t K, int64_t nnz, const void* s_ptr,
                                   const void* s_idx, const void* s_val, const void* a_ptr, const void* a_idx, const void* a_val,
                                   const void* b_ptr, const void* b_idx, const void* b_val, int group, int cap, int64_t window,
                                   void* out, void* zeros, unsigned flags, void* stream) {
  if (val_dtype != SPAMD_F32 && val_dtype != SPAMD_F64 && val_dtype != SPAMD_I32 && val_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (M < 0 || N < 0 || K < 0 || nnz < 0) return SPAMD_EINVAL;
  if (group != 8 && group != 16 && group != 32 && group != 64) return SPAMD_EINVAL;
  if (cap < 1 || cap > MSG_MAX_CAP || window < 1) return SPAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (zeros)
    if (hipError_t e = hipMemsetAsync(zeros, 0, sizeof(unsigned long long), st); e != hipSuccess) return (int)e;
  if (nnz == 0 || M == 0 || N == 0) return 0;
  if (!s_ptr || !s_idx || !s_val || !a_ptr || !b_ptr || !out) return SPAMD_EINVAL;
  if (window > nnz) window = nnz;   // one window holds everything; keeps `lo + window` and the window count far from overflow
  const bool exact = (flags & SPAMD_EXACT_MULADD) != 0;
#define MSG_ARGS group, M, nnz, s_ptr, s_idx, s_val, a_ptr, a_idx, a_val, b_ptr, b_idx, b_val, window, cap, out, zeros, st
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (val_dtype == SPAMD_F32) return exact ? launch_masked<float, I, true>(MSG_ARGS) : launch_masked<float, I, false>(MSG_ARGS);
    if (val_dtype == SPAMD_F64) return exact ? launch_masked<double, I, true>(MSG_ARGS) : launch_masked<double, I, false>(MSG_ARGS);
    if (val_dtype == SPAMD_I32) return launch_masked<int32_t, I, true>(MSG_ARGS);
    return launch_masked<int64_t, I, true>(MSG_ARGS);
  })
#undef MSG_ARGS
  return SPAMD_ETYPE;
}

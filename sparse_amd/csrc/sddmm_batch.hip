// A9 with an N-D mask: the fold of a stored element (l_1 .. l_p, i, j) to the pair the 2-D kernels take,
//
//     row' = ba * M + i,   ba = sum_d l_d * a_stride[d]      (ordinal of the element's batch in the leading shape A HAS)
//     col' = bb * N + j,   bb = sum_d l_d * b_stride[d]      (the same for Bt),
//
// so that sddmm.hip / sddmm_panel.hip / sddmm_mfma.hip run unchanged on A viewed as [Ba * M, K] and Bt as [Bb * N, K].  A leading
// axis over which an operand is broadcast (size 1 there, or the operand has fewer axes) has stride 0.  One pass: the p + 2
// coordinate rows are read once (coalesced along the element index), both outputs are written once.
#include "common.h"

namespace spamd {

struct SdFoldStrides {
  int64_t a[SPAMD_MAX_NDIM];
  int64_t b[SPAMD_MAX_NDIM];
};

template <typename I, typename O>
__global__ void __launch_bounds__(256) sddmm_batch_fold_kernel(int nlead, int64_t nnz, const I* __restrict__ coords, int64_t ldc,
                                                               SdFoldStrides st, int64_t M, int64_t N, O* __restrict__ rows,
                                                               O* __restrict__ cols) {
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nnz; n += (int64_t)gridDim.x * blockDim.x) {
    int64_t ba = 0, bb = 0;
    for (int d = 0; d < nlead; ++d) {
      const int64_t l = (int64_t)coords[(int64_t)d * ldc + n];
      ba += l * st.a[d];
      bb += l * st.b[d];
    }
    rows[n] = (O)(ba * M + (int64_t)coords[(int64_t)nlead * ldc + n]);
    cols[n] = (O)(bb * N + (int64_t)coords[(int64_t)(nlead + 1) * ldc + n]);
  }
}

}  // namespace spamd

using namespace spamd;

// coords: [nlead + 2, nnz] of idx_dtype, row pitch ldc (elements).  a_strides / b_strides: nlead HOST words each.  rows / cols:
// nnz words of out_dtype (I32 when the caller knows that Ba * M and Bb * N fit, else I64).
extern "C" int spamd_sddmm_batch_fold(int idx_dtype, int out_dtype, int nlead, int64_t nnz, const void* coords, int64_t ldc,
                                      const int64_t* a_strides, const int64_t* b_strides, int64_t M, int64_t N, void* rows,
                                      void* cols, void* stream) {
  if (nlead < 0 || nlead + 2 > SPAMD_MAX_NDIM || nnz < 0 || ldc < nnz || M < 0 || N < 0) return SPAMD_EINVAL;
  if (nlead > 0 && (!a_strides || !b_strides)) return SPAMD_EINVAL;
  if (out_dtype != SPAMD_I32 && out_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if (nnz == 0) return 0;
  if (!coords || !rows || !cols) return SPAMD_EINVAL;
  SdFoldStrides st = {};
  for (int d = 0; d < nlead; ++d) {
    if (a_strides[d] < 0 || b_strides[d] < 0) return SPAMD_EINVAL;
    st.a[d] = a_strides[d];
    st.b[d] = b_strides[d];
  }
  int64_t blocks = ceil_div(nnz, (int64_t)256);
  if (blocks > 256 * 32) blocks = 256 * 32;
  SPAMD_DISPATCH_IDX(idx_dtype, I, {
    if (out_dtype == SPAMD_I32)
      hipLaunchKernelGGL((sddmm_batch_fold_kernel<I, int32_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, nlead,
                         nnz, (const I*)coords, ldc, st, M, N, (int32_t*)rows, (int32_t*)cols);
    else
      hipLaunchKernelGGL((sddmm_batch_fold_kernel<I, int64_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, nlead,
                         nnz, (const I*)coords, ldc, st, M, N, (int64_t*)rows, (int64_t*)cols);
    return launch_status();
  })
  return SPAMD_ETYPE;
}

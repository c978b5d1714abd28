// A7 for complex64 / complex128 values: the merge-path union of two canonical key arrays fused with the elementwise
// function and the fill-value prune - merge.hip's single-pass form (tiles of spamd_merge_num_blocks' size, cut by
// spamd_merge_partition, output offsets chained by look-back) with 8- / 16-byte values, the functions of complex_ops.h and
// fill values that are passed by address (a complex128 fill value does not fit merge.hip's one 64-bit word per fill).
// A key present in both operands is emitted once, by the thread that takes it from A; out = func(a or fill_a, b or fill_b);
// results whose (re, im) pair is bit-identical to the result's fill value are dropped.  Output keys ascend strictly.
#include "complex_ops.h"

namespace spamd {
namespace {

constexpr int CM_THREADS = 1024, CM_VT = 4, CM_TILE = CM_THREADS * CM_VT;   // = merge.hip's MP_TILE (checked on the host)

template <typename R, bool TO_BOOL>
__global__ void __launch_bounds__(CM_THREADS)
cm_union_kernel(int op, const int64_t* __restrict__ ka, const Cplx<R>* __restrict__ va, int64_t na,
                const int64_t* __restrict__ kb, const Cplx<R>* __restrict__ vb, int64_t nb, Cplx<R> fill_a, Cplx<R> fill_b,
                Cplx<R> fill_out, uint8_t fill_out_bool, const int64_t* __restrict__ part, int64_t* __restrict__ counts,
                int64_t* __restrict__ out_keys, void* __restrict__ out_vals_) {
  using T = Cplx<R>;
  using O = typename std::conditional<TO_BOOL, uint8_t, T>::type;
  __shared__ int64_t sk[CM_TILE + 4];
  __shared__ T sv[CM_TILE + 4];
  __shared__ int wave_tot[CM_THREADS / 64];
  __shared__ int64_t ticket, excl_s;
  O* const out_vals = static_cast<O*>(out_vals_);
  const int tid = threadIdx.x;
  const int64_t nblocks = gridDim.x;
  unsigned long long* const states = reinterpret_cast<unsigned long long*>(counts);
  // ticket order = start order: a tile only ever waits for tiles that are already running
  if (tid == 0) ticket = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(counts + nblocks), 1ull);
  __syncthreads();
  const int64_t blk = ticket;
  int64_t d0 = blk * CM_TILE, d1 = (blk + 1) * CM_TILE;
  if (d1 > na + nb) d1 = na + nb;
  const int64_t a0 = part[blk], a1 = part[blk + 1];
  const int64_t b0 = d0 - a0, b1 = d1 - a1;
  const int la = (int)(a1 - a0), lb = (int)(b1 - b0);
  // LDS layout: [0] = a[a0-1] | A segment [1 .. la] | B segment [la+1 .. la+lb] | [la+lb+1] = b[b1]
  for (int t = tid; t < la + lb + 2; t += CM_THREADS) {
    int64_t k;
    T v{R(0), R(0)};
    if (t == 0) k = a0 > 0 ? ka[a0 - 1] : (int64_t)-1;
    else if (t <= la) { k = ka[a0 + t - 1]; v = va[a0 + t - 1]; }
    else if (t <= la + lb) { k = kb[b0 + (t - la - 1)]; v = vb[b0 + (t - la - 1)]; }
    else k = b1 < nb ? kb[b1] : INT64_MAX;
    sk[t] = k;
    sv[t] = v;
  }
  __syncthreads();
  const int64_t* A = sk + 1;        // A[i], i in [-1, la)
  const int64_t* B = sk + 1 + la;   // B[j], j in [0, lb]
  const T* AV = sv + 1;
  const T* BV = sv + 1 + la;
  int diag = tid * CM_VT;
  const int total = la + lb;
  if (diag > total) diag = total;
  int lo = diag > lb ? diag - lb : 0, hi = diag < la ? diag : la;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] <= B[diag - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  int i = lo, j = diag - lo;
  int64_t okey[CM_VT];
  O oval[CM_VT];
  int cnt = 0;
  auto emit = [&](int64_t k, T x, T y) {
    if constexpr (TO_BOOL) {
      const uint8_t r = cbin_bool<R>(op, x, y);
      if (r != fill_out_bool) { okey[cnt] = k; oval[cnt] = r; ++cnt; }
    } else {
      const T r = cbin<R>(op, x, y);
      if (!csame_bits<R>(r, fill_out)) { okey[cnt] = k; oval[cnt] = r; ++cnt; }
    }
  };
#pragma unroll
  for (int s = 0; s < CM_VT; ++s) {
    if (diag + s < total) {
      const bool takeA = (i < la) && (j >= lb || A[i] <= B[j]);
      if (takeA) {
        const int64_t k = A[i];
        const bool matched = (B[j] == k);  // B[lb] is the look-ahead key (or INT64_MAX)
        T bvv = fill_b;
        if (matched) bvv = (j < lb) ? BV[j] : vb[b1];
        emit(k, AV[i], bvv);
        ++i;
      } else {
        const int64_t k = B[j];
        if (A[i - 1] != k) emit(k, fill_a, BV[j]);  // A[-1] is the look-behind key (or -1): a matched B key went out with its A
        ++j;
      }
    }
  }
  // block-wide exclusive scan of cnt
  const int lane = tid & 63, wv = tid >> 6;
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int n = __shfl_up(incl, off, 64);
    if (lane >= off) incl += n;
  }
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < CM_THREADS / 64; ++w) {
    if (w < wv) base += wave_tot[w];
    tot += wave_tot[w];
  }
  const int lbase = base + (incl - cnt);
  if (tid < 64) {  // wave 0 looks back 64 predecessors at a time
    const unsigned long long excl = lookback_exclusive(states, blk, (unsigned long long)tot, tid);
    if (tid == 0) {
      if (blk == nblocks - 1) counts[nblocks + 1] = (int64_t)(excl + (unsigned long long)tot);
      excl_s = (int64_t)excl;
    }
  }
  __syncthreads();   // (also: everyone is done reading sk / sv)
  const int64_t o = excl_s;
  // stage the tile's outputs in LDS and copy them out with consecutive lanes on consecutive elements
  O* const so = reinterpret_cast<O*>(sv);
#pragma unroll
  for (int s = 0; s < CM_VT; ++s) {
    if (s < cnt) {
      sk[lbase + s] = okey[s];
      so[lbase + s] = oval[s];
    }
  }
  __syncthreads();
  for (int t = tid; t < tot; t += CM_THREADS) {
    out_keys[o + t] = sk[t];
    out_vals[o + t] = so[t];
  }
}

}  // namespace
}  // namespace spamd

using namespace spamd;

extern "C" int spamd_merge_union_complex(int op, int val_dtype, int64_t na, const int64_t* ka, const void* va, int64_t nb,
                                         const int64_t* kb, const void* vb, const void* fill_a, const void* fill_b,
                                         const void* fill_out, const int64_t* part, int64_t* counts, int64_t* out_keys,
                                         void* out_vals, void* stream) {
  if (na < 0 || nb < 0 || !fill_a || !fill_b || !fill_out) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  const bool to_bool = op == CB_EQ || op == CB_NE;
  if (!to_bool && (op < CB_ADD || op > CB_DIV)) return SPAMD_EINVAL;
  const int64_t nblocks = spamd_merge_num_blocks(na, nb);
  if (nblocks == 0) return 0;
  if (nblocks != ceil_div(na + nb, CM_TILE)) return SPAMD_EINVAL;   // (the partition's tiles are this kernel's tiles)
  if (!part || !counts || !out_keys || !out_vals) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)(nblocks + 2) * sizeof(int64_t), s); e != hipSuccess) return (int)e;
#define CM_LAUNCH(R, TB)                                                                                               \
  do {                                                                                                                 \
    const Cplx<R> fa = *static_cast<const Cplx<R>*>(fill_a), fb = *static_cast<const Cplx<R>*>(fill_b);                \
    const Cplx<R> fo = TB ? Cplx<R>{R(0), R(0)} : *static_cast<const Cplx<R>*>(fill_out);                              \
    const uint8_t fob = TB ? *static_cast<const uint8_t*>(fill_out) : (uint8_t)0;                                      \
    hipLaunchKernelGGL((cm_union_kernel<R, TB>), dim3((unsigned)nblocks), dim3(CM_THREADS), 0, s, op, ka,              \
                       (const Cplx<R>*)va, na, kb, (const Cplx<R>*)vb, nb, fa, fb, fo, fob, part, counts, out_keys,    \
                       out_vals);                                                                                      \
  } while (0)
  if (val_dtype == SPAMD_C64) {
    if (to_bool) CM_LAUNCH(float, true); else CM_LAUNCH(float, false);
  } else {
    if (to_bool) CM_LAUNCH(double, true); else CM_LAUNCH(double, false);
  }
#undef CM_LAUNCH
  return launch_status();
}

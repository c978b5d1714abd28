// A11 (second half): complex64 / complex128 elementwise value kernels, conversions and reductions (the functions
// themselves: complex_ops.h).
//   sum  : `np.add.reduceat`'s order: x0 + P(x1 .. x(m-1)) per component, P = NumPy's pairwise sum over complex values
//          (four accumulators per leaf of at most 64 values, leaves joined in a tree that depends on the length alone).
//   prod : `np.multiply.reduceat`: left to right with the plain (unfused) product.
//
// Memory: one 16-byte packet per lane and access where every array is 16-byte aligned (complex128: one element, complex64:
// two); buffers that are only 8-byte aligned take the same kernels with 8-byte accesses.
#include "complex_ops.h"

namespace spamd {
namespace {

// ---- 16-byte packets -------------------------------------------------------------------------------------------------
template <typename R>
struct Packet {
  static constexpr int EPL = 16 / (int)sizeof(Cplx<R>);   // elements per lane: 1 (complex128) or 2 (complex64)
  typedef R vec __attribute__((ext_vector_type(2 * EPL)));
};

// elements [i0, i0 + EPL) of p (those below n); A16: p is 16-byte aligned and the packet is whole -> one 16-byte access
template <typename R, bool A16>
__device__ __forceinline__ void load_packet(const Cplx<R>* __restrict__ p, int64_t i0, int64_t n, Cplx<R> (&v)[Packet<R>::EPL]) {
  constexpr int EPL = Packet<R>::EPL;
  if (A16 && i0 + EPL <= n) {
    const typename Packet<R>::vec x = *reinterpret_cast<const typename Packet<R>::vec*>(p + i0);
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] = Cplx<R>{x[2 * e], x[2 * e + 1]};
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] = i0 + e < n ? p[i0 + e] : Cplx<R>{R(0), R(0)};
  }
}
template <typename R, bool A16>
__device__ __forceinline__ void store_packet(Cplx<R>* __restrict__ p, int64_t i0, int64_t n, const Cplx<R> (&v)[Packet<R>::EPL]) {
  constexpr int EPL = Packet<R>::EPL;
  if (A16 && i0 + EPL <= n) {
    typename Packet<R>::vec x;
#pragma unroll
    for (int e = 0; e < EPL; ++e) { x[2 * e] = v[e].re; x[2 * e + 1] = v[e].im; }
    *reinterpret_cast<typename Packet<R>::vec*>(p + i0) = x;
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e)
      if (i0 + e < n) p[i0 + e] = v[e];
  }
}

#define CPLX_PACKETS(pk, n, EPL)                                                                          \
  for (int64_t pk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, np_ = ((n) + (EPL) - 1) / (EPL);       \
       pk < np_; pk += (int64_t)gridDim.x * blockDim.x)

static inline unsigned cgrid(int64_t packets) {
  int64_t b = ceil_div(packets, 256);
  if (b < 1) b = 1;
  if (b > 256 * 64) b = 256 * 64;
  return (unsigned)b;
}
static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// out = a (op) b; a scalar operand is one element, read once
template <typename R, bool A16, bool TO_BOOL>
__global__ void __launch_bounds__(256) cplx_binary_kernel(int op, const Cplx<R>* __restrict__ a, int a_scalar,
                                                          const Cplx<R>* __restrict__ b, int b_scalar, int64_t n,
                                                          void* __restrict__ out) {
  constexpr int EPL = Packet<R>::EPL;
  Cplx<R> sa{R(0), R(0)}, sb{R(0), R(0)};
  if (a_scalar) sa = a[0];
  if (b_scalar) sb = b[0];
  CPLX_PACKETS(pk, n, EPL) {
    const int64_t i0 = pk * EPL;
    Cplx<R> x[EPL], y[EPL];
    if (a_scalar) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) x[e] = sa;
    } else {
      load_packet<R, A16>(a, i0, n, x);
    }
    if (b_scalar) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) y[e] = sb;
    } else {
      load_packet<R, A16>(b, i0, n, y);
    }
    if constexpr (TO_BOOL) {
      uint8_t* o = static_cast<uint8_t*>(out);
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        if (i0 + e < n) o[i0 + e] = cbin_bool<R>(op, x[e], y[e]);
    } else {
      Cplx<R> r[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = cbin<R>(op, x[e], y[e]);
      store_packet<R, A16>(static_cast<Cplx<R>*>(out), i0, n, r);
    }
  }
}

// KIND 0: complex out, 1: real out, 2: bool (0/1 bytes) out
template <typename R, bool A16, int KIND>
__global__ void __launch_bounds__(256) cplx_unary_kernel(int op, const Cplx<R>* __restrict__ a, int64_t n, void* __restrict__ out) {
  constexpr int EPL = Packet<R>::EPL;
  CPLX_PACKETS(pk, n, EPL) {
    const int64_t i0 = pk * EPL;
    Cplx<R> x[EPL];
    load_packet<R, A16>(a, i0, n, x);
    if constexpr (KIND == 0) {
      Cplx<R> r[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = cun<R>(op, x[e]);
      store_packet<R, A16>(static_cast<Cplx<R>*>(out), i0, n, r);
    } else if constexpr (KIND == 1) {
      R* o = static_cast<R*>(out);
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        if (i0 + e < n) o[i0 + e] = cun_real<R>(op, x[e]);
    } else {
      uint8_t* o = static_cast<uint8_t*>(out);
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        if (i0 + e < n) o[i0 + e] = cun_bool<R>(op, x[e]);
    }
  }
}

// real / integer / bool / complex -> complex (imaginary part 0 for real sources; complex128 -> complex64 rounds each part)
template <typename S, typename R>
__global__ void __launch_bounds__(256) cplx_convert_kernel(const S* __restrict__ src, int64_t n, Cplx<R>* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (std::is_same<S, Cplx<float>>::value || std::is_same<S, Cplx<double>>::value) {
      const S v = src[i];
      dst[i] = Cplx<R>{(R)v.re, (R)v.im};
    } else {
      dst[i] = Cplx<R>{(R)src[i], R(0)};
    }
  }
}

template <typename R>
__global__ void __launch_bounds__(256) cplx_fill_kernel(Cplx<R>* __restrict__ out, int64_t n, Cplx<R> v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = v;
}

// ---- reductions --------------------------------------------------------------------------------------------------------
constexpr int PW_LEAF = 64;

// NumPy's pairwise sum P over c <= 64 complex values (c >= 1)
template <typename R>
__device__ __forceinline__ Cplx<R> pw_leaf(const Cplx<R>* __restrict__ x, int64_t c) {
#pragma clang fp contract(off)
  if (c < 4) {
    R re = R(-0.0), im = R(-0.0);
    for (int64_t i = 0; i < c; ++i) { const Cplx<R> v = x[i]; re = re + v.re; im = im + v.im; }
    return Cplx<R>{re, im};
  }
  Cplx<R> a0 = x[0], a1 = x[1], a2 = x[2], a3 = x[3];
  const int64_t whole = c & ~(int64_t)3;
  for (int64_t i = 4; i < whole; i += 4) {
    a0 = a0 + x[i]; a1 = a1 + x[i + 1]; a2 = a2 + x[i + 2]; a3 = a3 + x[i + 3];
  }
  Cplx<R> s = (a0 + a1) + (a2 + a3);
  for (int64_t i = whole; i < c; ++i) s = s + x[i];
  return s;
}

__host__ __device__ __forceinline__ int64_t pw_left(int64_t c) { return (c - (c & 7)) >> 1; }

// One thread per run.  op 0: x0 + P(x1 ..) (`np.add.reduceat`); the tree of P is walked leaf by leaf, each leaf found from
// the root by its path (the tree depends on the length alone), pending left siblings on a stack in LDS.
// op 1: product left to right, plain (unfused) multiply (`np.multiply.reduceat`).  Runs longer than max_len are skipped
// (max_len > 0: the caller sums them with spamd_cplx_sum_long).
constexpr int PW_THREADS = 64, PW_STACK = 40;
template <typename R>
__global__ void __launch_bounds__(PW_THREADS) cplx_segment_kernel(int op, const Cplx<R>* __restrict__ data,
                                                                   const int64_t* __restrict__ starts, int64_t nseg,
                                                                   int64_t max_len, Cplx<R>* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ Cplx<R> stack[PW_STACK][PW_THREADS];
  const int tid = threadIdx.x;
  for (int64_t seg = (int64_t)blockIdx.x * PW_THREADS + tid; seg < nseg; seg += (int64_t)gridDim.x * PW_THREADS) {
    const int64_t s0 = starts[seg], m = starts[seg + 1] - s0;
    if (m <= 0 || (max_len > 0 && m > max_len)) continue;
    const Cplx<R>* x = data + s0;
    Cplx<R> acc = x[0];
    if (op == 1) {
      for (int64_t i = 1; i < m; ++i) acc = acc * x[i];
      out[seg] = acc;
      continue;
    }
    if (m > 1) {
      const Cplx<R>* y = x + 1;
      const int64_t C = m - 1;
      uint64_t path = 0;
      int d = 0, sp = 0;
      Cplx<R> v;
      for (;;) {
        int64_t off = 0, c = C;
        int k = 0;
        while (c > PW_LEAF) {
          const int64_t c1 = pw_left(c);
          if (k < d && ((path >> k) & 1)) { off += c1; c -= c1; }
          else c = c1;
          ++k;
        }
        if (k > d) d = k;               // (the bits above the old depth are zero: the leftmost leaf below that node)
        v = pw_leaf<R>(y + off, c);
        while (d > 0 && ((path >> (d - 1)) & 1)) {
          v = stack[--sp][tid] + v;
          --d;
          path &= ~(1ull << d);
        }
        if (d == 0) break;
        stack[sp++][tid] = v;
        path |= 1ull << (d - 1);
      }
      acc = acc + v;
    }
    out[seg] = acc;
  }
}

// One LONG run: P over c values by 2^D virtual leaves (D = the depth at which every node of the tree holds at most 64
// values; index bits from the top = the path; a node that is a leaf above depth D lives at the index whose remaining bits
// are zero).  A pass joins up to 8 levels inside a workgroup of 256 in the tree's own order and writes one value per
// workgroup; the host repeats it until one value is left, to which the last pass adds the run's first element.
__device__ __forceinline__ bool pw_node(int64_t C, int D, int64_t t, int depth, int64_t& c) {
  // the size of the node at `depth` on index t's path; false when an ancestor is already a leaf
  c = C;
  for (int k = 0; k < depth; ++k) {
    if (c <= PW_LEAF) return false;
    const int64_t c1 = pw_left(c);
    c = ((t >> (D - 1 - k)) & 1) ? c - c1 : c1;
  }
  return true;
}

template <typename R, bool LEAVES>
__global__ void __launch_bounds__(256) cplx_sum_long_kernel(const Cplx<R>* __restrict__ x, int64_t C, int D,
                                                            const Cplx<R>* __restrict__ in, Cplx<R>* __restrict__ out,
                                                            const Cplx<R>* __restrict__ first) {
#pragma clang fp contract(off)
  __shared__ Cplx<R> V[256];
  const int tid = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * 256 + tid, total = (int64_t)1 << D;
  Cplx<R> v{R(0), R(0)};
  if (t < total) {
    if constexpr (LEAVES) {
      // the leaf on t's path; it is this index's own only when the bits below the leaf's depth are zero
      int64_t off = 0, c = C;
      int k = 0;
      while (c > PW_LEAF) {
        const int64_t c1 = pw_left(c);
        if ((t >> (D - 1 - k)) & 1) { off += c1; c -= c1; }
        else c = c1;
        ++k;
      }
      if ((t & (((int64_t)1 << (D - k)) - 1)) == 0) v = pw_leaf<R>(x + off, c);
    } else {
      v = in[t];
    }
  }
  V[tid] = v;
  __syncthreads();
  const int levels = D < 8 ? D : 8;
  for (int s = 0; s < levels; ++s) {
    const bool mine = t < total && (tid & ((2 << s) - 1)) == 0;
    Cplx<R> r = V[tid];
    if (mine) {
      int64_t c;
      if (pw_node(C, D, t, D - s - 1, c) && c > PW_LEAF) r = V[tid] + V[tid + (1 << s)];
    }
    __syncthreads();
    if (mine) V[tid] = r;
    __syncthreads();
  }
  if (tid == 0) {
    Cplx<R> r = V[0];
    if (D <= 8 && first) r = *first + r;
    out[blockIdx.x] = r;
  }
}

static int pw_depth(int64_t C) {   // levels until the largest node (the right-most chain) holds at most 64 values
  int d = 0;
  while (C > PW_LEAF) { C -= pw_left(C); ++d; }
  return d;
}

template <typename R>
static int sum_long(const Cplx<R>* run, int64_t m, Cplx<R>* out, Cplx<R>* ws, hipStream_t s) {
  const int64_t C = m - 1;
  int D = pw_depth(C);
  const int64_t h0 = (int64_t)1 << (D > 8 ? D - 8 : 0);
  Cplx<R>* bufs[2] = {ws, ws + h0};
  const Cplx<R>* in = nullptr;
  int which = 0;
  bool leaves = true;
  for (;;) {
    const int64_t blocks = ceil_div((int64_t)1 << D, 256);
    Cplx<R>* dst = D <= 8 ? out : bufs[which];
    if (leaves)
      hipLaunchKernelGGL((cplx_sum_long_kernel<R, true>), dim3((unsigned)blocks), dim3(256), 0, s, run + 1, C, D, in, dst, run);
    else
      hipLaunchKernelGGL((cplx_sum_long_kernel<R, false>), dim3((unsigned)blocks), dim3(256), 0, s, run + 1, C, D, in, dst, run);
    if (D <= 8) break;
    // the next pass sees the tree cut at depth D - 8: the same C, the same paths, 8 fewer index bits
    in = dst;
    which ^= 1;
    D -= 8;
    leaves = false;
  }
  return launch_status();
}

}  // namespace
}  // namespace spamd

using namespace spamd;

extern "C" int spamd_cplx_binary(int op, int val_dtype, int64_t n, const void* a, int a_is_scalar, const void* b,
                                 int b_is_scalar, void* out, void* stream) {
  if (n < 0) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  const bool to_bool = op == CB_EQ || op == CB_NE;
  if (!to_bool && (op < CB_ADD || op > CB_DIV)) return SPAMD_EINVAL;
  if (n == 0) return 0;
  if (!a || !b || !out) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool a16 = (a_is_scalar || al16(a)) && (b_is_scalar || al16(b)) && (to_bool || al16(out));
#define CB_LAUNCH(R, A16, TB)                                                                                      \
  hipLaunchKernelGGL((cplx_binary_kernel<R, A16, TB>), dim3(cgrid(ceil_div(n, Packet<R>::EPL))), dim3(256), 0, s, op, \
                     (const Cplx<R>*)a, a_is_scalar, (const Cplx<R>*)b, b_is_scalar, n, out)
#define CB_PICK(R)                                                  \
  do {                                                              \
    if (a16 && to_bool) CB_LAUNCH(R, true, true);                   \
    else if (a16) CB_LAUNCH(R, true, false);                        \
    else if (to_bool) CB_LAUNCH(R, false, true);                    \
    else CB_LAUNCH(R, false, false);                                \
  } while (0)
  if (val_dtype == SPAMD_C64) CB_PICK(float); else CB_PICK(double);
#undef CB_PICK
#undef CB_LAUNCH
  return launch_status();
}

extern "C" int spamd_cplx_unary(int op, int val_dtype, int64_t n, const void* a, void* out, void* stream) {
  if (n < 0) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  int kind;
  switch (op) {
    case CU_NEG: case CU_SQUARE: case CU_POS: case CU_CONJ: kind = 0; break;
    case CU_ABS: case CU_REAL: case CU_IMAG: kind = 1; break;
    case CU_ISNAN: case CU_ISINF: case CU_ISFINITE: kind = 2; break;
    default: return SPAMD_EINVAL;
  }
  if (n == 0) return 0;
  if (!a || !out) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool a16 = al16(a) && (kind != 0 || al16(out));
#define CU_LAUNCH(R, A16, KIND)                                                                                       \
  hipLaunchKernelGGL((cplx_unary_kernel<R, A16, KIND>), dim3(cgrid(ceil_div(n, Packet<R>::EPL))), dim3(256), 0, s, op, \
                     (const Cplx<R>*)a, n, out)
#define CU_PICK(R)                                                          \
  do {                                                                      \
    if (a16) {                                                              \
      if (kind == 0) CU_LAUNCH(R, true, 0);                                 \
      else if (kind == 1) CU_LAUNCH(R, true, 1);                            \
      else CU_LAUNCH(R, true, 2);                                           \
    } else {                                                                \
      if (kind == 0) CU_LAUNCH(R, false, 0);                                \
      else if (kind == 1) CU_LAUNCH(R, false, 1);                           \
      else CU_LAUNCH(R, false, 2);                                          \
    }                                                                       \
  } while (0)
  if (val_dtype == SPAMD_C64) CU_PICK(float); else CU_PICK(double);
#undef CU_PICK
#undef CU_LAUNCH
  return launch_status();
}

extern "C" int spamd_cplx_convert(int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst, void* stream) {
  if (n < 0) return SPAMD_EINVAL;
  if (dst_dtype != SPAMD_C64 && dst_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (src_dtype == SPAMD_BF16 || src_dtype < SPAMD_F32 || src_dtype > SPAMD_C128) return SPAMD_ETYPE;
  if (n == 0) return 0;
  if (!src || !dst) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
#define CC_LAUNCH(S, R) \
  hipLaunchKernelGGL((cplx_convert_kernel<S, R>), dim3(cgrid(n)), dim3(256), 0, s, (const S*)src, n, (Cplx<R>*)dst)
#define CC_PICK(R)                                                    \
  switch (src_dtype) {                                                \
    case SPAMD_F32: CC_LAUNCH(float, R); break;                       \
    case SPAMD_F64: CC_LAUNCH(double, R); break;                      \
    case SPAMD_I32: CC_LAUNCH(int32_t, R); break;                     \
    case SPAMD_I64: CC_LAUNCH(int64_t, R); break;                     \
    case SPAMD_U8: CC_LAUNCH(uint8_t, R); break;                      \
    case SPAMD_C64: CC_LAUNCH(Cplx<float>, R); break;                 \
    default: CC_LAUNCH(Cplx<double>, R); break;                       \
  }
  if (dst_dtype == SPAMD_C64) { CC_PICK(float) } else { CC_PICK(double) }
#undef CC_PICK
#undef CC_LAUNCH
  return launch_status();
}

extern "C" int spamd_cplx_fill(int val_dtype, int64_t n, void* out, double re, double im, void* stream) {
  if (n < 0) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (n == 0) return 0;
  if (!out) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (val_dtype == SPAMD_C64)
    hipLaunchKernelGGL(cplx_fill_kernel<float>, dim3(cgrid(n)), dim3(256), 0, s, (Cplx<float>*)out, n, Cplx<float>{(float)re, (float)im});
  else
    hipLaunchKernelGGL(cplx_fill_kernel<double>, dim3(cgrid(n)), dim3(256), 0, s, (Cplx<double>*)out, n, Cplx<double>{re, im});
  return launch_status();
}

extern "C" int spamd_cplx_segment_reduce(int op, int val_dtype, int64_t n, const void* data, const int64_t* starts,
                                         int64_t nseg, int64_t max_len, void* out, void* stream) {
  if (n < 0 || nseg < 0 || (op != 0 && op != 1)) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (n == 0 || nseg == 0) return 0;
  if (!data || !starts || !out) return SPAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = ceil_div(nseg, PW_THREADS);
  if (blocks > 256 * 64) blocks = 256 * 64;
  if (val_dtype == SPAMD_C64)
    hipLaunchKernelGGL(cplx_segment_kernel<float>, dim3((unsigned)blocks), dim3(PW_THREADS), 0, s, op, (const Cplx<float>*)data,
                       starts, nseg, max_len, (Cplx<float>*)out);
  else
    hipLaunchKernelGGL(cplx_segment_kernel<double>, dim3((unsigned)blocks), dim3(PW_THREADS), 0, s, op, (const Cplx<double>*)data,
                       starts, nseg, max_len, (Cplx<double>*)out);
  return launch_status();
}

extern "C" int64_t spamd_cplx_sum_long_ws_bytes(int64_t m) {
  if (m < 2) return 16;
  const int D = pw_depth(m - 1);
  const int64_t h0 = (int64_t)1 << (D > 8 ? D - 8 : 0), h1 = (int64_t)1 << (D > 16 ? D - 16 : 0);
  return (h0 + h1) * 16;
}

extern "C" int spamd_cplx_sum_long(int val_dtype, int64_t m, const void* run, void* out, void* ws, int64_t ws_bytes,
                                   void* stream) {
  if (m < 2 || !run || !out || !ws) return SPAMD_EINVAL;
  if (val_dtype != SPAMD_C64 && val_dtype != SPAMD_C128) return SPAMD_ETYPE;
  if (ws_bytes < spamd_cplx_sum_long_ws_bytes(m)) return SPAMD_EWS;
  hipStream_t s = (hipStream_t)stream;
  if (val_dtype == SPAMD_C64) return sum_long<float>((const Cplx<float>*)run, m, (Cplx<float>*)out, (Cplx<float>*)ws, s);
  return sum_long<double>((const Cplx<double>*)run, m, (Cplx<double>*)out, (Cplx<double>*)ws, s);
}

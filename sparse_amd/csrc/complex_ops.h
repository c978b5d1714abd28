// The complex64 / complex128 elementwise functions as NumPy's ufunc loops evaluate them, statement for statement (shared by
// the value kernels of ewise_complex.hip and the complex merge of merge_complex.hip):
//   multiply : NumPy's ARRAY loop fuses - re = fma(ar, br, -(ai * bi)), im = fma(ar, bi, ai * br) with the inner products
//              rounded.  (`Cplx`'s operator* in common.h is the SCALAR product - four rounded products - which the
//              interpreted loops of the matrix products and `multiply.reduceat` perform: a different function.)
//   divide   : Smith's form as NumPy writes it, unfused.
//   abs      : hypot(re, im), the device function of the real `hypot` op (the one ulp-bounded op here).
// Nothing is contracted by the compiler (-ffp-contract=off and the pragmas); fused steps are written as fma calls.
#pragma once
#include "common.h"

namespace spamd {

// binary op codes (those of spamd_ewise_binary) and unary op codes (those of spamd_ewise_unary plus 96-98)
constexpr int CB_ADD = 0, CB_SUB = 1, CB_MUL = 2, CB_DIV = 3, CB_EQ = 36, CB_NE = 37;
constexpr int CU_NEG = 0, CU_ABS = 1, CU_SQUARE = 20, CU_POS = 22, CU_ISNAN = 64, CU_ISINF = 65, CU_ISFINITE = 66,
              CU_CONJ = 96, CU_REAL = 97, CU_IMAG = 98;

template <typename R>
__device__ __forceinline__ R fma_r(R a, R b, R c) {
  if constexpr (std::is_same<R, float>::value) return __builtin_fmaf(a, b, c);
  else return __builtin_fma(a, b, c);
}
template <typename R>
__device__ __forceinline__ R abs_r(R a) {
  if constexpr (std::is_same<R, float>::value) return __builtin_fabsf(a);
  else return __builtin_fabs(a);
}

template <typename R>
__device__ __forceinline__ Cplx<R> cmul_fused(Cplx<R> a, Cplx<R> b) {
#pragma clang fp contract(off)
  const R p = a.im * b.im, q = a.im * b.re;
  return Cplx<R>{fma_r<R>(a.re, b.re, -p), fma_r<R>(a.re, b.im, q)};
}

template <typename R>
__device__ __forceinline__ Cplx<R> cdiv_smith(Cplx<R> a, Cplx<R> b) {
#pragma clang fp contract(off)
  const R abr = abs_r<R>(b.re), abi = abs_r<R>(b.im);
  if (abr >= abi) {
    if (abr == R(0) && abi == R(0)) return Cplx<R>{a.re / abr, a.im / abi};
    const R rat = b.im / b.re;
    const R t = b.im * rat;
    const R scl = R(1) / (b.re + t);
    const R u = a.im * rat, v = a.re * rat;
    return Cplx<R>{(a.re + u) * scl, (a.im - v) * scl};
  }
  const R rat = b.re / b.im;
  const R t = b.re * rat;
  const R scl = R(1) / (b.im + t);
  const R u = a.re * rat, v = a.im * rat;
  return Cplx<R>{(u + a.im) * scl, (v - a.re) * scl};
}

template <typename R>
__device__ __forceinline__ Cplx<R> cbin(int op, Cplx<R> a, Cplx<R> b) {
#pragma clang fp contract(off)
  switch (op) {
    case CB_ADD: return Cplx<R>{a.re + b.re, a.im + b.im};
    case CB_SUB: return Cplx<R>{a.re - b.re, a.im - b.im};
    case CB_MUL: return cmul_fused<R>(a, b);
    default: return cdiv_smith<R>(a, b);
  }
}
template <typename R>
__device__ __forceinline__ uint8_t cbin_bool(int op, Cplx<R> a, Cplx<R> b) {
  const bool eq = a.re == b.re && a.im == b.im;
  return op == CB_EQ ? eq : !eq;
}

template <typename R>
__device__ __forceinline__ Cplx<R> cun(int op, Cplx<R> a) {
  switch (op) {
    case CU_NEG: return Cplx<R>{-a.re, -a.im};
    case CU_CONJ: return Cplx<R>{a.re, -a.im};
    case CU_SQUARE: return cmul_fused<R>(a, a);
    default: return a;
  }
}
template <typename R>
__device__ __forceinline__ R cun_real(int op, Cplx<R> a) {
  switch (op) {
    case CU_ABS: return hypot(a.re, a.im);
    case CU_REAL: return a.re;
    default: return a.im;
  }
}
template <typename R>
__device__ __forceinline__ uint8_t cun_bool(int op, Cplx<R> a) {
  const bool nan = a.re != a.re || a.im != a.im;
  const bool inf = __builtin_isinf(a.re) || __builtin_isinf(a.im);
  switch (op) {
    case CU_ISNAN: return nan;
    case CU_ISINF: return inf;
    default: return !nan && !inf;
  }
}

// bit-wise equality of the pair (the prune against the result's fill value)
template <typename R>
__device__ __forceinline__ bool csame_bits(Cplx<R> x, Cplx<R> y) {
  if constexpr (sizeof(R) == 8)
    return __builtin_bit_cast(uint64_t, x.re) == __builtin_bit_cast(uint64_t, y.re) &&
           __builtin_bit_cast(uint64_t, x.im) == __builtin_bit_cast(uint64_t, y.im);
  else
    return __builtin_bit_cast(uint32_t, x.re) == __builtin_bit_cast(uint32_t, y.re) &&
           __builtin_bit_cast(uint32_t, x.im) == __builtin_bit_cast(uint32_t, y.im);
}

}  // namespace spamd

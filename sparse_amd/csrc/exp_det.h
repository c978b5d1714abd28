// exp_det: the library's own exponential for arguments <= 0 (A14, csrc/softmax.hip).  It exists so that NumPy can restate
// it: every step below is ONE exactly rounded IEEE operation, written out - no device math library call, no a * b + c left
// for the compiler to contract either way (the build passes -ffp-contract=off, the pragma holds whatever the flags).
//
//   d < LO (or NaN)   +0 when d < LO (the exact exp is below half the smallest subnormal; -inf included), d itself when NaN
//   k  = rint(d * LOG2E)                              one multiply, round-half-even to an integer
//   r  = fma(-k, LN2_HI, d);  r = fma(-k, LN2_LO, r)  Cody-Waite: |r| <= ln2 / 2 (+ rounding)
//   p  = C[N];  p = fma(p, r, C[i]) for i = N-1 .. 0  Horner, C[i] = the double quotient 1.0 / i!, for float32 narrowed
//                                                     to float after that (two roundings; the restatement does the same)
//   e  = ldexp(p, (int)k)                             one rounding, and only when the result is subnormal
// EXP(+0) = EXP(-0) = 1 exactly: k = +-0, r = 0, p = fma(.., 0, 1) = 1.  N = 7 for float32, 13 for float64 (the first
// dropped Taylor term is 0.09 / 0.04 ulp at |r| = ln2 / 2).  Measured error: DESIGN A14.
// tests/softmax_cases.py restates this file; a change here is a change there.
#pragma once
#include <hip/hip_runtime.h>

namespace spamd {

__device__ __forceinline__ float exp_det(float d) {
#pragma clang fp contract(off)
  constexpr float LO = -104.0f;               // exp(-104) = 2^-150.04 < 2^-150: rounds to +0
  constexpr float LOG2E = 0x1.715476p+0f;
  constexpr float LN2_HI = 0x1.62e400p-1f;    // 15 significant bits: k * LN2_HI is exact for |k| < 2^9
  constexpr float LN2_LO = 0x1.7f7d1cp-20f;
  if (!(d >= LO)) return d != d ? d : 0.0f;
  const float k = __builtin_rintf(d * LOG2E);
  float r = __builtin_fmaf(-k, LN2_HI, d);
  r = __builtin_fmaf(-k, LN2_LO, r);
  float p = (float)(1.0 / 5040.0);
  p = __builtin_fmaf(p, r, (float)(1.0 / 720.0));
  p = __builtin_fmaf(p, r, (float)(1.0 / 120.0));
  p = __builtin_fmaf(p, r, (float)(1.0 / 24.0));
  p = __builtin_fmaf(p, r, (float)(1.0 / 6.0));
  p = __builtin_fmaf(p, r, 0.5f);
  p = __builtin_fmaf(p, r, 1.0f);
  p = __builtin_fmaf(p, r, 1.0f);
  return __builtin_ldexpf(p, (int)k);
}

__device__ __forceinline__ double exp_det(double d) {
#pragma clang fp contract(off)
  constexpr double LO = -746.0;               // exp(-746) = 2^-1076.3 < 2^-1075: rounds to +0
  constexpr double LOG2E = 0x1.71547652b82fep+0;
  constexpr double LN2_HI = 0x1.62e42fee00000p-1;   // 32 significant bits: k * LN2_HI is exact for |k| < 2^21
  constexpr double LN2_LO = 0x1.a39ef35793c76p-33;
  if (!(d >= LO)) return d != d ? d : 0.0;
  const double k = __builtin_rint(d * LOG2E);
  double r = __builtin_fma(-k, LN2_HI, d);
  r = __builtin_fma(-k, LN2_LO, r);
  double p = 1.0 / 6227020800.0;
  p = __builtin_fma(p, r, 1.0 / 479001600.0);
  p = __builtin_fma(p, r, 1.0 / 39916800.0);
  p = __builtin_fma(p, r, 1.0 / 3628800.0);
  p = __builtin_fma(p, r, 1.0 / 362880.0);
  p = __builtin_fma(p, r, 1.0 / 40320.0);
  p = __builtin_fma(p, r, 1.0 / 5040.0);
  p = __builtin_fma(p, r, 1.0 / 720.0);
  p = __builtin_fma(p, r, 1.0 / 120.0);
  p = __builtin_fma(p, r, 1.0 / 24.0);
  p = __builtin_fma(p, r, 1.0 / 6.0);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)k);
}

}  // namespace spamd

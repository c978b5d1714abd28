// Group id of a key: k / d for 0 <= k, the two forms the grouped reduce (group_reduce.hip) instantiates its kernels
// for.  Host and device: tests/test_group_of_host.py compiles a stand-alone program against this header and checks both
// forms against exact integer division over their whole key ranges.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPAMD_HD __host__ __device__ __forceinline__
#else
#define SPAMD_HD inline
#endif

// (a host test program counts the correction steps through this hook; it is empty everywhere else)
#ifndef SPAMD_GROUP_OF_STEP
#define SPAMD_GROUP_OF_STEP()
#endif

namespace spamd {

// k / d for 0 <= k: reciprocal multiply in double, then an exact integer correction (a hardware 64-bit divide
// is ~100 instructions).
// Any non-negative int64 key is safe.  The estimate is off by the three roundings of (double)k, rd and their product,
// at most 3 * 2^-53 * 2^63 = 3072 quotients, so the correction loops are that short (one or two steps below 2^53).  It
// is clamped to the largest double below 2^63 before the conversion: for d == 1 and k >= 2^63 - 512 the product is 2^63,
// which no int64 holds (the conversion's result is then undefined, and the corrections would start anywhere); the clamp
// adds at most 1023 steps.  The remainder is formed in unsigned arithmetic: q * d may pass 2^63 by the estimate's error.
struct GroupOf {
  int64_t d;
  double rd;
  SPAMD_HD int64_t operator()(int64_t k) const {
    double e = (double)k * rd;
    if (e > 9223372036854774784.0) e = 9223372036854774784.0;  // 2^63 - 1024
    int64_t q = (int64_t)e;
    int64_t r = (int64_t)((uint64_t)k - (uint64_t)q * (uint64_t)d);
    while (r < 0) { --q; r += d; SPAMD_GROUP_OF_STEP(); }
    while (r >= d) { ++q; r -= d; SPAMD_GROUP_OF_STEP(); }
    return q;
  }
};

// The same for keys below 2^53 (every array with fewer than 2^53 elements), entirely in double precision: k, the
// quotient and the remainder k - q*d are all exactly representable, so one fma decides the +-1 correction and no
// 64-bit integer multiply or conversion back is needed.  Group ids are compared (and stored) as doubles.
struct GroupOfD {
  double d, rd;
  SPAMD_HD double operator()(int64_t k) const {
    const double kd = (double)k;
    double q = __builtin_floor(kd * rd);
    const double r = __builtin_fma(-q, d, kd);
    if (r < 0.0) q -= 1.0;
    if (r >= d) q += 1.0;
    return q;
  }
};

}  // namespace spamd

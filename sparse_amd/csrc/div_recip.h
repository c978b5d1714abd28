// floor(r / d) through the FP64 pipe, the division of every key <-> coordinate conversion (prims.hip).  Host and device:
// tests/test_div_recip_host.py compiles a stand-alone program against this header and checks both instantiations against
// exact integer division.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPAMD_DIV_HD __device__ __forceinline__
#else
#define SPAMD_DIV_HD inline
#endif

// (a host test program counts how often each repair fires through these hooks; they are empty everywhere else)
#ifndef SPAMD_DIV_RECIP_DOWN
#define SPAMD_DIV_RECIP_DOWN()
#endif
#ifndef SPAMD_DIV_RECIP_UP
#define SPAMD_DIV_RECIP_UP()
#endif

namespace spamd {

// floor(r / d) for r < 2^52 (U = uint64_t) / r < 2^32 (U = uint32_t), inv = 1.0 / (double)d: the truncated product with 1/d
// is off by at most one (r and the quotient are exact doubles, 1/d and the product carry 2^-53 relative error each), two
// compares repair it.  A 64-bit integer division is ~100 emulated instructions on CDNA; this is ~10, and every
// key <-> coordinate conversion does one per dimension per stored element.
// Only the ++q repair is ever needed in range: the estimate can exceed the quotient only when its error, below
// 2^-52 r / d, reaches the 1 / d by which (q d - 1) / d falls short of q, i.e. from r = 2^52 on.  The host check
// (tests/div_recip_check.cpp: 2.5 x 10^7 pairs below 2^32, 3 x 10^7 below 2^52, dividends q d - 1, q d, q d + 1 up to the
// range's end) counts 0 `--q` and 1.4 x 10^5 / 1.3 x 10^5 `++q` repairs (r = q d with 1/d rounded down), and the largest
// estimate * d of the 32-bit form is 2^32 - 1: `back` never wraps.  The `--q` compare stays as the guard of that argument
// (tests/test_div_recip_host.py fails if it ever fires).
template <typename U>
SPAMD_DIV_HD U div_recip(U r, U d, double inv) {
  U q = (U)((double)r * inv);
  const U back = q * d;
  if (back > r) { --q; SPAMD_DIV_RECIP_DOWN(); }
  else if (r - back >= d) { ++q; SPAMD_DIV_RECIP_UP(); }
  return q;
}

}  // namespace spamd

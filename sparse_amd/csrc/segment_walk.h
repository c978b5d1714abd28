// The arithmetic of the long form that softmax (A14), sparse attention (A15, A16), the semiring products (A17, A18) and
// mttkrp (A12) share: segments (rows, columns or groups: ptr[r] .. ptr[r + 1] of nnz positions) of more than `chunk`
// elements are cut into pieces of `chunk`, and the pieces are found by windows.  Host and device: the qualifiers are empty
// without the HIP language, and tests/test_segment_walk_host.py compiles a stand-alone program, tests/segment_walk_check.cpp,
// against this header that checks the claims below over pointer arrays with every boundary case.
//
// Window g is the positions [g * chunk, (g + 1) * chunk) (cut at nnz).  A segment of more than `chunk` elements spans more
// than a window, so at most two pieces of such segments START inside one window:
//   - one piece k >= 0 of the segment that holds the window's first position: its pieces start `chunk` apart, so exactly one
//     start falls in a range of `chunk` positions (if the segment goes on that far);
//   - piece 0 of the segment that holds the window's last position, if that is another segment.  Every segment between the
//     two starts and ends inside the window, so it has at most `chunk` elements and is no business of the long form.
// The first of them takes the workspace slot 2g and the second 2g + 1: a piece start s that is its segment's first position b
// and not a window's first position (b % chunk != 0) is the second kind, every other start is the first kind.  So a slot is
// computed from (b, s) alone, by the kernel that writes a piece and by the one that joins the pieces, with no piece list and
// no count brought back to the host; slots are below 2 * nwin, nwin = ceil(nnz / chunk).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPAMD_SEG_HD __device__ __forceinline__
#else
#define SPAMD_SEG_HD inline __attribute__((always_inline))
#endif

namespace spamd {

// last r in [0, nseg] with ptr[r] <= pos (ptr[0] = 0 <= pos): the non-empty segment that holds pos when pos < nnz
template <typename I>
SPAMD_SEG_HD int64_t seg_of(const I* __restrict__ ptr, int64_t nseg, int64_t pos) {
  int64_t lo = 0, hi = nseg;   // invariant: ptr[lo] <= pos; the answer is in [lo, hi]
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)ptr[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the workspace slot of the piece of a long segment (first position b) that starts at position s
SPAMD_SEG_HD int64_t seg_slot(int64_t b, int64_t s, int64_t chunk) {
  return 2 * (s / chunk) + (s == b && b % chunk != 0 ? 1 : 0);
}

// the walk of window g < ceil(nnz / chunk): f(seg, b, s, e) for the at most two pieces [s, e) of segments of more than
// `chunk` elements (seg, first position b) that start in the window, the one of slot 2g first
template <typename I, typename F>
SPAMD_SEG_HD void seg_window_pieces(const I* __restrict__ ptr, int64_t nseg, int64_t nnz, int64_t chunk, int64_t g, F f) {
  const int64_t lo = g * chunk;
  const int64_t hi = lo + chunk < nnz ? lo + chunk : nnz;
  const int64_t r0 = seg_of(ptr, nseg, lo);   // lo < nnz: r0 < nseg and the segment is not empty
  {
    const int64_t b0 = (int64_t)ptr[r0], e0 = (int64_t)ptr[r0 + 1];
    if (e0 - b0 > chunk) {
      const int64_t s = b0 + (lo - b0 + chunk - 1) / chunk * chunk;   // the one piece start of this segment in [lo, lo + chunk)
      if (s < hi && s < e0) f(r0, b0, s, s + chunk < e0 ? s + chunk : e0);
    }
  }
  const int64_t r1 = seg_of(ptr, nseg, hi - 1);
  if (r1 > r0) {   // starts inside the window; only the last such segment can be longer than the window
    const int64_t b1 = (int64_t)ptr[r1], e1 = (int64_t)ptr[r1 + 1];
    if (e1 - b1 > chunk) f(r1, b1, b1, b1 + chunk);
  }
}

}  // namespace spamd

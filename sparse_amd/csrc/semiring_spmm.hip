// A17  semiring products sparse @ dense -> dense whose "add" is min or max and whose "mul" is plus or times, with the arg:
//   out[i, j] = min | max over the stored (i, k) of  a[i, k] + b[k, j]  |  a[i, k] * b[k, j]      arg[i, j] = the k that was picked
// Unstored positions are absent (not 0); stored zeros take part as the value 0.
//
// Order (the contract tests/semiring_cases.py restates, bit for bit; "min", "max" mirrored), for output (i, j): the stored elements
// of row i in CSR stored order, e = 0 .. n - 1 with inner indices k_e, give t_e = a[i, k_e] (+ | *) b[k_e, j] - one operation,
// integers wrap (computed unsigned).  The sequence is [init[i, j]] (when an init is given) followed by t_0 .. t_{n-1}; the result
// is the element np.argmin picks: the first NaN if there is one, else the FIRST element that attains the minimum (-0.0 and +0.0
// compare equal: the first of them wins and keeps its sign).  out is its value (the payload of a NaN is no result), arg its k_e,
// -1 for the init.  An empty sequence gives the identity of the add (+-inf, the integer type's max / min) and arg -1.
// "First NaN, else leftmost minimum" is associative over any in-order split, so neither the form, `group`, `chunk`, `max_len` nor
// the launch geometry changes a bit.  No atomics; every output is written once.
//
// A piece of a sequence is folded to a state in one of two shapes:
//   ordered   (value, k): elements enter in order, a later one replaces the state only when it is a NaN and the state is not, or
//             strictly better than it (`sr_takes`); an empty state is k = SR_EMPTY (kernels without the arg output start from the
//             identity instead, which gives the same VALUE, and carry no k)
//   placed    (value, position): lanes hold elements out of order, the choice between two states is the total order "NaN first,
//             then the better value, then the smaller position" (`sr_wins`); an empty state is (identity, SR_NOPOS)
//
// Three forms:
//   rows   G = 8 | 16 | 32 | 64 lanes own a row of at most `chunk` elements; lane u owns VEC contiguous output columns (16 bytes) per
//          column pass, so a wave-load of a b row is coalesced.  The row's (index, value) pairs are fetched G at a time and
//          broadcast; every lane folds its columns over them in stored order (ordered states in registers), four b rows in flight.
//   lanes  narrow results: G lanes own one output (i, j) and run ALONG the row, lane u folds the elements u, u + G, .. (four
//          gathers of b in flight), then a butterfly over placed states.  Bound by the gather of b[k].
//   long   rows longer than `chunk`: pieces of `chunk` elements, one wave each, found by windows of `chunk` positions (csrc/segment_walk.h:
//          at most two piece starts per window, workspace slots 2g and 2g + 1).  A piece is folded in the lanes shape
//          (narrow) or by 64 / G sub-groups in the rows shape over consecutive parts of it, joined in order.  Piece states go to
//          the workspace; a join launch - it starts after the piece launch has ENDED - folds them in piece order after the init.
#include "attention_common.h"

#include <limits>
#include <type_traits>

namespace spamd {

constexpr int SR_EMPTY = -2;                                     // the k of an ordered state that holds nothing (-1: the init)
constexpr int SR_NOPOS = std::numeric_limits<int>::max();        // the position of a placed state that holds nothing
constexpr int64_t SR_MAX_CHUNK = (int64_t)1 << 30;
constexpr int64_t SR_GRID_CAP = (int64_t)1 << 16;                // workgroups per launch (the other segment walkers: 2^20)

template <typename T, bool MAX>
__device__ __forceinline__ T sr_identity() {
  if constexpr (std::is_integral<T>::value) return MAX ? std::numeric_limits<T>::min() : std::numeric_limits<T>::max();
  else return MAX ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::infinity();
}

template <typename T, bool TIMES>
__device__ __forceinline__ T sr_mul(T a, T b) {
#pragma clang fp contract(off)
  if constexpr (std::is_integral<T>::value) {
    using U = typename std::make_unsigned<T>::type;
    return (T)(TIMES ? (U)a * (U)b : (U)a + (U)b);
  } else {
    return TIMES ? a * b : a + b;
  }
}

template <typename T, bool MAX>
__device__ __forceinline__ bool sr_better(T a, T b) {
  return MAX ? a > b : a < b;
}

// does the LATER value c replace the earlier value cur?
template <typename T, bool MAX>
__device__ __forceinline__ bool sr_takes(T c, T cur) {
  if constexpr (std::is_integral<T>::value) return sr_better<T, MAX>(c, cur);
  else return !(cur != cur) && (sr_better<T, MAX>(c, cur) || c != c);
}

// ordered states: does the later state (rv, ra) replace the earlier (lv, la)?
template <typename T, typename I, bool MAX, bool ARG>
__device__ __forceinline__ bool sr_later_wins(T lv, I la, T rv, I ra) {
  if constexpr (ARG) return ra != (I)SR_EMPTY && (la == (I)SR_EMPTY || sr_takes<T, MAX>(rv, lv));
  else return sr_takes<T, MAX>(rv, lv);
}

// placed states: is (a, apos) the choice before (b, bpos)?
template <typename T, bool MAX>
__device__ __forceinline__ bool sr_wins(T a, int apos, T b, int bpos) {
  if constexpr (!std::is_integral<T>::value) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || apos < bpos);
  }
  return sr_better<T, MAX>(a, b) || (!sr_better<T, MAX>(b, a) && apos < bpos);
}

template <typename T, typename I>
struct SrIn {
  int64_t M, N;
  const I* ptr;
  const I* idx;
  const T* val;
  const T* b;
  int64_t ldb;
  const T* init;   // may be null
  int64_t ldi;
  T* out;
  int64_t ldo;
  int64_t* arg;    // null in the kernels without the arg output
  int64_t lda;
  int aligned;     // N, ldb and the address of b allow loads of 16 bytes
};

template <typename T>
struct SrVec {
  static constexpr int N = 16 / (int)sizeof(T);
};

// ---- rows shape: the lane's VEC columns from `col` folded over the elements [start, end) in order ----------------------------------
// every lane of the sub-group calls it with the same range (the lanes without a column hand on their elements all the same)
template <typename T, typename I, bool MAX, bool TIMES, bool ARG, int VEC>
__device__ __forceinline__ void sr_fold_cols(const SrIn<T, I>& p, int64_t col, int64_t start, int64_t end, int G, int gl, int gbase,
                                             T (&val)[VEC], I (&ar)[VEC]) {
  const bool col_ok = col < p.N;
  const bool vec = p.aligned != 0;
  auto load = [&](I k, T(&o)[VEC]) {
    const T* r = p.b + (int64_t)k * p.ldb;
    if (vec) {
      const Vec<T, VEC> v = *reinterpret_cast<const Vec<T, VEC>*>(r + col);
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = v.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = r[col + e < p.N ? col + e : p.N - 1];   // (read inside the row, never stored)
    }
  };
  auto step = [&](I k, T a, const T(&bj)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const T t = sr_mul<T, TIMES>(a, bj[e]);
      bool take = sr_takes<T, MAX>(t, val[e]);
      if constexpr (ARG) {
        take = take || ar[e] == (I)SR_EMPTY;
        ar[e] = take ? k : ar[e];
      }
      val[e] = take ? t : val[e];
    }
  };
  for (int64_t q = start; q < end; q += G) {
    const int64_t mine = q + gl;
    I ci = 0;
    T vi = T(0);
    if (mine < end) {
      ci = p.idx[mine];
      vi = p.val[mine];
    }
    const int cnt = (int)(end - q < (int64_t)G ? end - q : (int64_t)G);
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {   // four b rows in flight: at most 64 bytes a lane
      I cj[4];
      T vj[4], bj[4][VEC];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        cj[u] = lane_shfl(ci, gbase + j + u);
        vj[u] = lane_shfl(vi, gbase + j + u);
      }
      if (col_ok) {
#pragma unroll
        for (int u = 0; u < 4; ++u) load(cj[u], bj[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) step(cj[u], vj[u], bj[u]);
      }
    }
    for (; j < cnt; ++j) {
      const I cj = lane_shfl(ci, gbase + j);
      const T vj = lane_shfl(vi, gbase + j);
      if (col_ok) {
        T bj[VEC];
        load(cj, bj);
        step(cj, vj, bj);
      }
    }
  }
}

template <typename T, typename I, bool MAX, bool TIMES, bool ARG>
__global__ void __launch_bounds__(256)
sr_rows_kernel(SrIn<T, I> p, int G, int64_t upto) {
  constexpr int VEC = SrVec<T>::N;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1), gbase = lane - gl, rpw = 64 / G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row0 = wave * rpw; row0 < p.M; row0 += nwaves * rpw) {
    const int64_t row = row0 + lane / G;
    bool ok = row < p.M;
    int64_t start = 0, end = 0;
    if (ok) {
      start = (int64_t)p.ptr[row];
      end = (int64_t)p.ptr[row + 1];
    }
    if (end - start > upto) {   // the long form has it (the same in every lane of the sub-group)
      ok = false;
      start = end = 0;
    }
    for (int64_t c0 = 0; c0 < p.N; c0 += (int64_t)G * VEC) {
      const int64_t col = c0 + (int64_t)gl * VEC;
      T val[VEC];
      I ar[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        val[e] = sr_identity<T, MAX>();
        ar[e] = (I)SR_EMPTY;
        if (p.init && ok && col + e < p.N) {
          val[e] = p.init[row * p.ldi + col + e];
          ar[e] = (I)-1;
        }
      }
      sr_fold_cols<T, I, MAX, TIMES, ARG, VEC>(p, col, start, end, G, gl, gbase, val, ar);
      if (ok) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (col + e < p.N) {
            p.out[row * p.ldo + col + e] = val[e];
            if constexpr (ARG) p.arg[row * p.lda + col + e] = ar[e] == (I)SR_EMPTY ? (int64_t)-1 : (int64_t)ar[e];
          }
        }
      }
    }
  }
}

// ---- lanes shape: G lanes along the n elements from s, for the column bcol = b + j; every lane returns the placed state --------------
template <typename T, typename I, bool MAX, bool TIMES>
__device__ __forceinline__ void sr_lanes_fold(const I* __restrict__ idx, const T* __restrict__ av, const T* __restrict__ bcol,
                                              int64_t ldb, int64_t s, int64_t n, int G, int gl, T& val, int& pos) {
  val = sr_identity<T, MAX>();
  pos = SR_NOPOS;
  for (int64_t q0 = gl; q0 < n; q0 += 4 * (int64_t)G) {
    I k[4];
    T a[4], bb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = q0 + (int64_t)u * G;
      const int64_t qq = q < n ? q : q0;   // (an element past the end is read at q0 and not used: no branch around a load)
      k[u] = idx[s + qq];
      a[u] = av[s + qq];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) bb[u] = bcol[(int64_t)k[u] * ldb];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = q0 + (int64_t)u * G;
      const T t = sr_mul<T, TIMES>(a[u], bb[u]);
      const bool take = q < n && (pos == SR_NOPOS || sr_takes<T, MAX>(t, val));
      val = take ? t : val;
      pos = take ? (int)q : pos;
    }
  }
  for (int h = G >> 1; h >= 1; h >>= 1) {
    const T ov = __shfl_xor(val, h, 64);
    const int op = __shfl_xor(pos, h, 64);
    const bool take = sr_wins<T, MAX>(ov, op, val, pos);
    val = take ? ov : val;
    pos = take ? op : pos;
  }
}

// the init (the sequence's first element, when given) against the placed state of the rest: pos -1 = the init was picked
template <typename T, bool MAX>
__device__ __forceinline__ void sr_finish(const T* init, T& val, int& pos) {
  if (!init) return;
  const T iv = *init;
  if (pos == SR_NOPOS || !sr_takes<T, MAX>(val, iv)) {
    val = iv;
    pos = -1;
  }
}

template <typename T, typename I, bool MAX, bool TIMES, bool ARG>
__global__ void __launch_bounds__(256)
sr_lanes_kernel(SrIn<T, I> p, int G, int64_t upto) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1), rpw = 64 / G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  const int64_t items = p.M * p.N;
  for (int64_t item = wave * rpw + lane / G; item < items; item += nwaves * rpw) {
    const int64_t row = item / p.N, j = item - row * p.N;
    const int64_t s = (int64_t)p.ptr[row], n = (int64_t)p.ptr[row + 1] - s;
    if (n > upto) continue;   // (the same in every lane of the sub-group)
    T val;
    int pos;
    sr_lanes_fold<T, I, MAX, TIMES>(p.idx, p.val, p.b + j, p.ldb, s, n, G, gl, val, pos);
    if (gl == 0) {
      sr_finish<T, MAX>(p.init ? p.init + row * p.ldi + j : nullptr, val, pos);
      p.out[row * p.ldo + j] = val;
      if constexpr (ARG) p.arg[row * p.lda + j] = (pos == SR_NOPOS || pos < 0) ? (int64_t)-1 : (int64_t)p.idx[s + pos];
    }
  }
}

// ---- long: pieces ----------------------------------------------------------------------------------------------------------------
// workspace: wsa int64[N * nslots] (the kernels with the arg output only), then wsv T[N * nslots]; column j's slots are contiguous
template <typename T, typename I, bool MAX, bool TIMES, bool ARG, bool NARROW>
__device__ __forceinline__ void sr_piece(const SrIn<T, I>& p, int64_t b, int64_t s, int64_t e, int64_t chunk, int64_t nslots,
                                         int G, int lane, T* __restrict__ wsv, int64_t* __restrict__ wsa) {
  const int64_t slot = seg_slot(b, s, chunk);
  if constexpr (NARROW) {
    for (int64_t j = 0; j < p.N; ++j) {
      T val;
      int pos;
      sr_lanes_fold<T, I, MAX, TIMES>(p.idx, p.val, p.b + j, p.ldb, s, e - s, 64, lane, val, pos);
      if (lane == 0) {   // (a piece is never empty)
        wsv[j * nslots + slot] = val;
        if constexpr (ARG) wsa[j * nslots + slot] = (int64_t)p.idx[s + pos];
      }
    }
  } else {
    constexpr int VEC = SrVec<T>::N;
    const int gl = lane & (G - 1), gbase = lane - gl, sub = lane / G;
    const int64_t part = (e - s + 64 / G - 1) / (64 / G);
    const int64_t ps = s + sub * part < e ? s + sub * part : e;
    const int64_t pe = ps + part < e ? ps + part : e;
    for (int64_t c0 = 0; c0 < p.N; c0 += (int64_t)G * VEC) {
      const int64_t col = c0 + (int64_t)gl * VEC;
      T val[VEC];
      I ar[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        val[v] = sr_identity<T, MAX>();
        ar[v] = (I)SR_EMPTY;
      }
      sr_fold_cols<T, I, MAX, TIMES, ARG, VEC>(p, col, ps, pe, G, gl, gbase, val, ar);
      for (int h = G; h < 64; h <<= 1) {   // the sub-groups' states joined in order: the lower sub-group is the earlier one
        const bool lower = (lane & h) == 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const T ov = __shfl_xor(val[v], h, 64);
          I oa = (I)SR_EMPTY;
          if constexpr (ARG) oa = __shfl_xor(ar[v], h, 64);
          const bool other = lower ? sr_later_wins<T, I, MAX, ARG>(val[v], ar[v], ov, oa)
                                   : !sr_later_wins<T, I, MAX, ARG>(ov, oa, val[v], ar[v]);
          val[v] = other ? ov : val[v];
          ar[v] = other ? oa : ar[v];
        }
      }
      if (sub == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (col + v < p.N) {
            wsv[(col + v) * nslots + slot] = val[v];
            if constexpr (ARG) wsa[(col + v) * nslots + slot] = (int64_t)ar[v];
          }
        }
      }
    }
  }
}

template <typename T, typename I, bool MAX, bool TIMES, bool ARG, bool NARROW>
__global__ void __launch_bounds__(256)
sr_piece_kernel(SrIn<T, I> p, int64_t nnz, int64_t chunk, int64_t nwin, int64_t nslots, int G, T* __restrict__ wsv,
                int64_t* __restrict__ wsa) {
  const int lane = threadIdx.x & 63;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < nwin; g += (int64_t)gridDim.x * 4)
    seg_window_pieces(p.ptr, p.M, nnz, chunk, g, [&](int64_t, int64_t b, int64_t s, int64_t e) {
      sr_piece<T, I, MAX, TIMES, ARG, NARROW>(p, b, s, e, chunk, nslots, G, lane, wsv, wsa);
    });
}

// the piece states of every long row folded in piece order after the init: lanes along the pieces, placed by piece number
template <typename T, typename I, bool MAX, bool ARG>
__global__ void __launch_bounds__(256)
sr_join_kernel(SrIn<T, I> p, int64_t chunk, int64_t nslots, const T* __restrict__ wsv, const int64_t* __restrict__ wsa) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < p.M; base += nwaves * 64)
    seg_wave_each(p.ptr, p.M, base, lane, [&](int64_t len) { return len > chunk; }, [&](int src, int64_t b, int64_t n) {
      const int64_t row = base + src;
      const int64_t np = (n + chunk - 1) / chunk;
      for (int64_t j = 0; j < p.N; ++j) {
        T val = sr_identity<T, MAX>();
        int pos = SR_NOPOS;
        for (int64_t k = lane; k < np; k += 64) {
          const T t = wsv[j * nslots + seg_slot(b, b + k * chunk, chunk)];
          const bool take = pos == SR_NOPOS || sr_takes<T, MAX>(t, val);
          val = take ? t : val;
          pos = take ? (int)k : pos;
        }
        for (int h = 32; h >= 1; h >>= 1) {
          const T ov = __shfl_xor(val, h, 64);
          const int op = __shfl_xor(pos, h, 64);
          const bool take = sr_wins<T, MAX>(ov, op, val, pos);
          val = take ? ov : val;
          pos = take ? op : pos;
        }
        if (lane == 0) {
          sr_finish<T, MAX>(p.init ? p.init + row * p.ldi + j : nullptr, val, pos);
          p.out[row * p.ldo + j] = val;
          if constexpr (ARG) p.arg[row * p.lda + j] = pos < 0 ? (int64_t)-1 : wsa[j * nslots + seg_slot(b, b + (int64_t)pos * chunk, chunk)];
        }
      }
    });
}

static int64_t sr_ws_bytes(int64_t esz, int64_t nnz, int64_t N, int64_t chunk, int with_arg) {
  return 2 * ceil_div(nnz, chunk) * N * (esz + (with_arg ? 8 : 0));
}

template <typename T, typename I, bool MAX, bool TIMES, bool ARG>
static int semiring_typed(SrIn<T, I> p, int64_t nnz, int narrow, int group, int64_t chunk, int64_t max_len, void* ws, hipStream_t st) {
  const int rpw = 64 / group;
  const dim3 wg(256);
  if (narrow) SPAMD_LAUNCH((sr_lanes_kernel<T, I, MAX, TIMES, ARG>), dim3(seg_grid(p.M * p.N, 4 * rpw, SR_GRID_CAP)), wg, 0, st, p, group, chunk);
  else SPAMD_LAUNCH((sr_rows_kernel<T, I, MAX, TIMES, ARG>), dim3(seg_grid(p.M, 4 * rpw, SR_GRID_CAP)), wg, 0, st, p, group, chunk);
  if (max_len > chunk) {
    const int64_t nwin = ceil_div(nnz, chunk), nslots = 2 * nwin;
    int64_t* wsa = ARG ? (int64_t*)ws : nullptr;
    T* wsv = (T*)((char*)ws + (ARG ? 8 * p.N * nslots : 0));
    const dim3 pg(seg_grid(nwin, 4, SR_GRID_CAP));
    if (narrow) SPAMD_LAUNCH((sr_piece_kernel<T, I, MAX, TIMES, ARG, true>), pg, wg, 0, st, p, nnz, chunk, nwin, nslots, group, wsv, wsa);
    else SPAMD_LAUNCH((sr_piece_kernel<T, I, MAX, TIMES, ARG, false>), pg, wg, 0, st, p, nnz, chunk, nwin, nslots, group, wsv, wsa);
    SPAMD_LAUNCH((sr_join_kernel<T, I, MAX, ARG>), dim3(seg_grid(p.M, 256, SR_GRID_CAP)), wg, 0, st, p, chunk, nslots, wsv, wsa);
  }
  return 0;
}

template <typename T, typename I>
static int semiring_ops(SrIn<T, I> p, int add, int mul, int64_t nnz, int narrow, int group, int64_t chunk, int64_t max_len, void* ws,
                        hipStream_t st) {
#define SR_CASE(MX, TM)                                                                                          \
  if ((add != 0) == MX && (mul != 0) == TM) {                                                                    \
    if (p.arg) return semiring_typed<T, I, MX, TM, true>(p, nnz, narrow, group, chunk, max_len, ws, st);         \
    return semiring_typed<T, I, MX, TM, false>(p, nnz, narrow, group, chunk, max_len, ws, st);                   \
  }
  SR_CASE(false, false)
  SR_CASE(false, true)
  SR_CASE(true, false)
  SR_CASE(true, true)
#undef SR_CASE
  return SPAMD_EINVAL;
}

}  // namespace spamd

using namespace spamd;

static int64_t sr_esz(int val_dtype) {
  return (val_dtype == SPAMD_F32 || val_dtype == SPAMD_I32) ? 4 : ((val_dtype == SPAMD_F64 || val_dtype == SPAMD_I64) ? 8 : 0);
}

extern "C" int64_t spamd_semiring_spmm_ws_bytes(int val_dtype, int64_t nnz, int64_t N, int64_t chunk, int with_arg) {
  const int64_t esz = sr_esz(val_dtype);
  if (!esz) return SPAMD_ETYPE;
  if (nnz < 0 || N < 0 || !seg_chunk_ok(chunk, SR_MAX_CHUNK)) return SPAMD_EINVAL;
  if (nnz <= chunk) return 0;
  return sr_ws_bytes(esz, nnz, N, chunk, with_arg);
}

extern "C" int spamd_semiring_spmm(int val_dtype, int idx_dtype, int add, int mul, int64_t M, int64_t K, int64_t N, int64_t nnz,
                                   const void* a_ptr, const void* a_idx, const void* a_val, const void* b, int64_t ldb,
                                   const void* init, int64_t ldi, int narrow, int group, int64_t chunk, int64_t max_len, void* ws,
                                   int64_t ws_bytes, void* out, int64_t ldo, int64_t* arg, int64_t lda, void* stream) {
  const int64_t esz = sr_esz(val_dtype);
  if (!esz) return SPAMD_ETYPE;
  if (idx_dtype != SPAMD_I32 && idx_dtype != SPAMD_I64) return SPAMD_ETYPE;
  if ((add != SPAMD_SEMIRING_MIN && add != SPAMD_SEMIRING_MAX) || (mul != SPAMD_SEMIRING_PLUS && mul != SPAMD_SEMIRING_TIMES))
    return SPAMD_EINVAL;
  if (M < 0 || K < 0 || N < 0 || nnz < 0 || max_len < 0 || max_len > nnz) return SPAMD_EINVAL;
  if (!seg_params_ok(group, chunk, SR_MAX_CHUNK, 0)) return SPAMD_EINVAL;
  if (ldb < N || ldo < N || (init && ldi < N) || (arg && lda < N)) return SPAMD_EINVAL;
  if (M == 0 || N == 0) return 0;
  if (!a_ptr || !out || (nnz > 0 && (!a_idx || !a_val || !b || K == 0))) return SPAMD_EINVAL;
  if (max_len > chunk && (!ws || ws_bytes < sr_ws_bytes(esz, nnz, N, chunk, arg != nullptr))) return SPAMD_EWS;
  hipStream_t st = (hipStream_t)stream;
  SPAMD_DISPATCH_VAL(val_dtype, T, {
    SPAMD_DISPATCH_IDX(idx_dtype, I, {
      constexpr int VEC = SrVec<T>::N;
      SrIn<T, I> p{M, N, (const I*)a_ptr, (const I*)a_idx, (const T*)a_val, (const T*)b, ldb, (const T*)init, ldi, (T*)out, ldo, arg, lda, 0};
      p.aligned = N % VEC == 0 && ldb % VEC == 0 && (uintptr_t)b % 16 == 0;
      return semiring_ops<T, I>(p, add, mul, nnz, narrow != 0, group, chunk, max_len, ws, st);
    })
  })
  return SPAMD_ETYPE;
}

"""Raw-array kernel layer: the analogue of the reference's jitted `_dot_*` kernels.

Each function takes device tensors (raw arrays, no containers), allocates and returns fresh
outputs — the reference's ownership rule — and launches exactly one C-ABI
entry point of libsparse_amd.so (a few for the composite kernels) on the current HIP stream.  The arithmetic of the
path (products, sums, sorts, scans, merges) happens in that library; torch is used for allocation, views, dtype
casts of operands and host<->device copies.
"""
import functools
import os

import numpy as np
import torch

from . import _ffi
from ._device import code_of, np_dtype, ptr, require_hip, stream_ptr, torch_dtype


def dot_dtype(dt1, dt2):
    """Result dtype rule of every `_dot` kernel: `(zeros(dt1) * zeros(dt2)).dtype`
    (reference sparse/numba_backend/_common.py:635-636)."""
    return (np.zeros((), dtype=np_dtype(dt1)) * np.zeros((), dtype=np_dtype(dt2))).dtype


_COMPLEX_CODE = {torch.complex64: _ffi.C64, torch.complex128: _ffi.C128}


def product_code(dt):
    """C-ABI value code of a PRODUCT's result type: what `code_of` knows plus complex64 / complex128, which only the
    product kernels take (`spamd_spmm_csr_complex`, `spamd_spgemm_expand`, `spamd_segment_reduce` with add).  Kept apart
    from `code_of`, whose TypeError is the "no device kernel for this dtype" probe of the elementwise and reduction layers."""
    dt = torch_dtype(dt)
    code = _COMPLEX_CODE.get(dt)
    return code_of(dt) if code is None else code


def _as_reals(t):
    """A complex tensor as its interleaved (re, im) reals, flat (a view); anything else unchanged."""
    return torch.view_as_real(t).reshape(-1) if t.is_complex() else t


def _unify_index(*idx):
    """Index arrays handed to one kernel share a width: int32 only if all are int32."""
    want = torch.int32 if all(i.dtype == torch.int32 for i in idx) else torch.int64
    return [i if i.dtype == want else i.to(want) for i in idx], want


def stream_passes(M, K, N, dtr, a_data, a_indices, flags=0):
    """Passes over A the stream form of CSR x dense (csrc/spmm_stream.hip) takes for this product, 0 = another kernel has
    it: the rule of `spamd_spmm_csr`'s own dispatch (`spamd_spmm_csr_stream_passes`), under its `flags`.  A pass holds 4
    columns (3 of 8-byte values; fewer when K x width values of B do not fit the LDS) and costs A's stream whatever its width -
    0.16-0.18 ms at config 2's matrix, 0.25 with 8-byte values -, so (round 6, tools/r06/width_sweep.py) up to 12 columns are
    worth 3 passes (the tiled executor's padded panel: 0.77 / 1.0 ms), at most 4 columns of 8-byte values 2 (the row-vector
    kernel: 0.85-0.96 ms) and at most 4 columns of 4-byte values 1 (two tie with the row-vector kernel).  `a_data` /
    `a_indices`: the tensors or their addresses."""
    addr = lambda t: t if isinstance(t, int) else ptr(t)    # noqa: E731
    return int(_ffi.lib().spamd_spmm_csr_stream_passes(code_of(dtr), M, K, N, addr(a_data), addr(a_indices), flags))


def dot_csr_ndarray(out_shape, a_data, a_indices, a_indptr, b, *, exact=False, out=None, keep_order=False, rowvec=False):
    """C = A @ B, A in CSR, B dense row-major, C dense — `_dot_csr_ndarray`
    (reference _common.py:720-755).  `exact=True` reproduces the reference's separate
    multiply/add bit-for-bit; the default uses one FMA per term (same k-ascending order; results of at most 4 columns
    are summed in a per-row tree order by the stream / row-vector kernels unless `keep_order`; `rowvec` keeps the
    row-vector kernel where the stream form would run)."""
    M, N = int(out_shape[0]), int(out_shape[1])
    dev = require_hip(a_data, a_indices, a_indptr, b)
    dtr = torch_dtype(dot_dtype(a_data.dtype, b.dtype))
    vcode = product_code(dtr)
    if a_data.dtype != dtr:
        a_data = a_data.to(dtr)
    if b.dtype != dtr:
        b = b.to(dtr)
    b = b.contiguous()  # the reference's np.ascontiguousarray(b), _common.py:744
    if b.dim() != 2 or b.shape[1] != N:
        raise ValueError(f"dense operand has shape {tuple(b.shape)}, expected (K, {N})")
    K = int(b.shape[0])
    (a_indices, a_indptr), it = _unify_index(a_indices.contiguous(), a_indptr.contiguous())
    if a_indptr.numel() != M + 1:
        raise ValueError(f"indptr has {a_indptr.numel()} entries, expected {M + 1}")
    a_data = a_data.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=dtr, device=dev)
    elif out.shape != (M, N) or out.dtype != dtr or not out.is_contiguous():
        raise ValueError("out buffer has wrong shape/dtype/layout")
    flags = (_ffi.EXACT_MULADD if exact else 0) | (_ffi.SPMM_ROWGROUP if keep_order else 0) | (_ffi.SPMM_ROWVEC if rowvec else 0)
    if dtr.is_complex:
        # csrc/spmm_complex.hip: the row-group and row-vector kernels for (re, im) pairs; the LDS-resident-B, stream and
        # executor forms are real-only (mixed real x complex operands were promoted above, like the reference's `v * b[k, j]`)
        _ffi.call("spamd_spmm_csr_complex", vcode, code_of(it), M, K, N, ptr(a_data), ptr(a_indices), ptr(a_indptr),
                  ptr(b), max(N, 1), ptr(out), max(N, 1), flags & ~_ffi.SPMM_ROWVEC, stream_ptr(dev))
        return out
    if stream_passes(M, K, N, dtr, a_data, a_indices, flags):
        # what spamd_spmm_csr's own dispatch would pick, with the number of stored elements handed over (the kernel need
        # not read it from indptr at the head of every wave's start-up chain)
        _ffi.call("spamd_spmm_csr_stream", vcode, code_of(it), M, K, N, ptr(a_data), ptr(a_indices), ptr(a_indptr),
                  ptr(b), N, ptr(out), N, int(a_data.numel()), 0, stream_ptr(dev))
        return out
    _ffi.call("spamd_spmm_csr", vcode, code_of(it), M, K, N, ptr(a_data), ptr(a_indices),
              ptr(a_indptr), ptr(b), max(N, 1), ptr(out), max(N, 1), flags, stream_ptr(dev))
    return out


def transposed_copy(x):
    """`x.t().contiguous()` of a dense 2-D tensor through csrc/transpose.hip (64 x 64 LDS tiles: torch's strided copy runs
    at 1.3 TB/s on a 128 x 10^6 operand - a third of the `dense @ sparse` product it prepares, round 6); other layouts and
    element sizes keep torch's copy."""
    if (not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_cuda or not x.is_contiguous() or x.numel() == 0
            or x.element_size() not in (1, 2, 4, 8) or x.is_complex()):
        return x.t().contiguous()
    out = torch.empty((x.shape[1], x.shape[0]), dtype=x.dtype, device=x.device)
    _ffi.call("spamd_transpose_2d", x.element_size(), int(x.shape[0]), int(x.shape[1]), ptr(x), int(x.shape[1]), ptr(out),
              int(x.shape[0]), stream_ptr(x.device))
    return out


def has_nan(data):
    """Any NaN in a float tensor?  (reference `nan_check`, _common.py:51-69).  One streaming
    pass on the device; the 4-byte flag is the only thing copied back."""
    dev = require_hip(data)
    if data.numel() == 0 or not (data.is_floating_point() or data.is_complex()):
        return False
    data = _as_reals(data.contiguous())     # a complex buffer is scanned as twice as many reals
    if data.data_ptr() % 16:
        data = data.clone()
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _ffi.call("spamd_has_nan", code_of(data.dtype), data.numel(), ptr(data), ptr(flag), stream_ptr(dev))
    return bool(flag.item())


class _WordMailbox:
    """Per device: pinned host slots the device delivers a few int64 words into (C ABI `spamd_deliver_words`), so that a
    data-dependent size reaches the host without `tolist()`'s blocking copy (a stream synchronisation plus a copy command,
    ~20 us).  Slots are used round-robin with a per-call sequence number as the marker: the late store of an abandoned
    call cannot be mistaken for the current one's."""

    _pool = {}
    SLOTS, WIDTH = 64, 17

    def __init__(self):
        import threading

        self.pinned = torch.zeros(self.SLOTS * self.WIDTH, dtype=torch.int64).pin_memory()
        self.view = self.pinned.numpy()
        self.seq = 0
        self.lock = threading.Lock()     # slots are handed out under it (two host threads must not share one)

    def take(self):
        with self.lock:
            self.seq += 1
            return self.seq % self.SLOTS, self.seq

    @classmethod
    def get(cls, dev):
        m = cls._pool.get(dev.index)
        if m is None:
            m = cls._pool[dev.index] = cls()
        return m


def read_words(t):
    """The int64 words of a small device tensor (<= 16) as Python ints, behind everything queued on the current stream."""
    n = int(t.numel())
    dev = t.device
    if n > 16 or t.dtype != torch.int64 or not t.is_contiguous():
        return [int(v) for v in t.tolist()]
    m = _WordMailbox.get(dev)
    k, marker = m.take()
    base = k * m.WIDTH
    _ffi.call("spamd_deliver_words", ptr(t), n, m.pinned.data_ptr() + 8 * base, marker, stream_ptr(dev))
    view = m.view
    for _ in range(4_000_000):        # (~0.1 s; then a synchronisation decides)
        if int(view[base + n]) == marker:
            break
    else:
        torch.cuda.current_stream(dev).synchronize()
        if int(view[base + n]) != marker:
            raise _ffi.HipBackendError("spamd_deliver_words did not deliver")
    return [int(v) for v in view[base: base + n]]


class NanProbe:
    """A NaN scan in flight: the kernel writes its verdict into a pinned host int; `result()` waits for the event
    recorded right behind the scan — NOT for whatever was queued after it — and reads the int."""

    # verdict slots: ONE pinned int32 slab, handed out by index (a pinned allocation per probe costs ~0.1 ms of host time,
    # which a loop that runs many products ahead of the device would pay once per product in flight)
    _SLOTS = 1024
    _slab = None      # pinned int32[_SLOTS]
    _view = None      # its NumPy view: host-side reads / writes of a verdict without a tensor op
    _free = []        # free slot indices
    _events = []      # reusable events

    @classmethod
    def _take(cls):
        if cls._slab is None:
            cls._slab = torch.zeros(cls._SLOTS, dtype=torch.int32).pin_memory()
            cls._view = cls._slab.numpy()
            cls._free = list(range(cls._SLOTS))
        if not cls._free:
            return None
        return cls._free.pop()

    def __init__(self, data):
        dev = require_hip(data)
        self.slot = NanProbe._take()
        if self.slot is None:            # more than _SLOTS scans in flight: a private pinned word
            self.own = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.view, self.at, addr = self.own.numpy(), 0, self.own.data_ptr()
        else:
            self.own = None
            self.view, self.at, addr = NanProbe._view, self.slot, NanProbe._slab.data_ptr() + 4 * self.slot
        self.event = NanProbe._events.pop() if NanProbe._events else torch.cuda.Event()
        self.view[self.at] = 0
        self.done = None
        self.launched = False
        self._keep = data  # the scanned buffer must outlive the kernel
        try:
            _ffi.call("spamd_has_nan_async", code_of(data.dtype), data.numel(), ptr(data), addr, stream_ptr(dev))
            self.launched = True
            # behind the scan on ITS stream: the array may live on another device than the current one (`to_device`)
            self.event.record(torch.cuda.current_stream(dev))
            self.recorded = True
        except BaseException:
            self.discard()
            raise

    def discard(self):
        """Give the verdict slot and the event back without reading the verdict (the launch failed, or the product
        this scan belonged to raised before asking)."""
        if self.done is None:
            self.done = False
            if self.launched:
                # the scan may still be running and will write its verdict word: the slot (and the scanned buffer) go back
                # only once it has finished - behind the event when that was recorded, else behind the whole device
                if getattr(self, "recorded", False):
                    self.event.synchronize()
                else:
                    torch.cuda.synchronize()
            if self.slot is not None:
                NanProbe._free.append(self.slot)
            if self.event is not None:
                NanProbe._events.append(self.event)
            self._keep = self.view = self.event = self.own = None

    def ready(self):
        """True once the scan has finished (never blocks)"""
        return self.done is not None or self.event.query()

    def result(self):
        if self.done is None:
            self.event.synchronize()
            self.done = bool(int(self.view[self.at]))
            if self.slot is not None:
                NanProbe._free.append(self.slot)
            NanProbe._events.append(self.event)
            self._keep = self.view = self.event = self.own = None
        return self.done


def has_nan_async(data):
    """`has_nan` without draining the stream: returns a NanProbe (or False when `data` cannot hold a NaN)."""
    if data.numel() == 0 or not (data.is_floating_point() or data.is_complex()):
        return False
    data = _as_reals(data.contiguous())     # a complex buffer is scanned as twice as many reals
    if data.data_ptr() % 16:
        data = data.clone()
    return NanProbe(data)


# ---------------------------------------------------------------------------------------------
# key primitives (prims.hip): thin wrappers, one C-ABI call each
# ---------------------------------------------------------------------------------------------
import ctypes as _ct


def _harr64(vals):
    return (_ct.c_int64 * max(len(vals), 1))(*[int(v) for v in vals])


def _harr32(vals):
    return (_ct.c_int32 * max(len(vals), 1))(*[int(v) for v in vals])


def c_strides(shape):
    """C-order element strides of `shape` (host ints)."""
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= int(d)
    return list(reversed(st))


def _check_ndim(n):
    if n > _ffi.MAX_NDIM:
        raise NotImplementedError(f"arrays with more than {_ffi.MAX_NDIM} dimensions are not supported by the hip backend")


def _key_bits(max_key):
    return max(1, int(max_key).bit_length())


def index_dtype_ok(t):
    return t.dtype in (torch.int32, torch.int64)


def linearize(coords, shape, axis_order=None):
    """C-order keys of `coords[axis_order]` w.r.t. `shape[axis_order]` — `linear_loc`
    (reference _coo/common.py:56-64)."""
    dev = require_hip(coords)
    ndim, nnz = int(coords.shape[0]), int(coords.shape[1])
    _check_ndim(ndim)
    order = list(range(ndim)) if axis_order is None else [int(a) for a in axis_order]
    rshape = [int(shape[a]) for a in order]
    keys = torch.empty(nnz, dtype=torch.int64, device=dev)
    if ndim == 0 or nnz == 0:
        return keys.zero_()
    coords = coords.contiguous()
    _ffi.call("spamd_coo_linearize", code_of(coords.dtype), ndim, nnz, ptr(coords), nnz,
              _harr64(c_strides(rshape)), _harr32(order), ptr(keys), stream_ptr(dev))
    return keys


def delinearize(keys, shape, idx_dtype=torch.int64):
    """keys -> coords[ndim, nnz] for `shape` (the div/mod chain of reference core.py:1090-1098)."""
    dev = require_hip(keys)
    ndim, nnz = len(shape), int(keys.numel())
    _check_ndim(ndim)
    coords = torch.empty((ndim, nnz), dtype=idx_dtype, device=dev)
    if ndim and nnz:
        _ffi.call("spamd_coo_delinearize", code_of(idx_dtype), ndim, nnz, ptr(keys), _harr64(c_strides(shape)),
                  _harr64(shape), ptr(coords), nnz, stream_ptr(dev))
    return coords


def permute_keys(keys, src_shape, perm):
    """Keys of the array transposed with `axes=perm` (destination axis d <- source axis perm[d])."""
    dev = require_hip(keys)
    ndim = len(src_shape)
    _check_ndim(ndim)
    if list(perm) == list(range(ndim)) or keys.numel() == 0:
        return keys
    out = torch.empty_like(keys)
    _ffi.call("spamd_permute_keys", ndim, keys.numel(), ptr(keys), _harr64(c_strides(src_shape)),
              _harr64(src_shape), _harr32(perm), ptr(out), stream_ptr(dev))
    return out


LEAD_LAST = True               # reductions over the leading axes: the kept-axes-first order by merging the slabs (csrc/lead_rotate.hip)
LEAD_LAST_RANGE = 2048         # elements a cell range should hold (the kernel's arrays take 4096)
LEAD_LAST_MAX_NNZ = 1 << 22     # beyond this the radix sort wins (it streams; the merge is a latency chain per range): measured at
#                                S = 1000, P = 10^6, whole reduction by merge / by sort: 10^6 elements 0.15 / 0.22 ms, 2 x 10^6: 0.22 / 0.25,
#                                10^7: merge kernel alone 0.43 ms against 0.64 ms for everything with the sort
LEAD_LAST_MIN_SLABS = 64
LEAD_LAST_MAX_BOUNDS = 1 << 20  # boundary words (runs x (ranges + 1)) of the slab merge: 4 MB
LEAD_LAST_STATS = {}


def lead_last_plan(n, n_slabs, n_cells, max_slabs=2048, max_cells=2048):
    """(cells per range, ranges) of the slab merge for n elements in n_slabs sorted runs over n_cells kept cells, or None when
    the problem is the sort's: too many runs, or a key space so much larger than the element count that most workgroups (one
    per range) and most boundary words (one per run and range) would be empty.  A range aims at LEAD_LAST_RANGE elements."""
    if n <= 0 or n > LEAD_LAST_MAX_NNZ or n_slabs > max_slabs or n_cells >= 2 ** 42 or n_cells < 1:
        return None
    # (a run's piece of a range is walked by ONE thread: a range holds at most ~32 elements per run, and below 64 runs a
    # workgroup's 512 threads have nothing to share - the sort)
    if n_slabs < LEAD_LAST_MIN_SLABS:
        return None
    target = min(LEAD_LAST_RANGE, 32 * n_slabs)
    cells = 1
    while cells * 2 <= max_cells and cells * 2 * n <= target * n_cells:
        cells *= 2
    ranges = -(-n_cells // cells)
    # (every range is a workgroup, every (run, range) a boundary word found by a binary search of the keys)
    if ranges > max(4096, n // 64) or n_slabs * (ranges + 1) > LEAD_LAST_MAX_BOUNDS:
        return None
    return cells, ranges


def keys_lead_last(keys, vals, n_slabs, n_cells, failed):
    """(keys', vals') of a canonical COO whose leading axes (n_slabs index values) are moved behind the kept ones (n_cells):
    keys' = cell * n_slabs + slab, ascending - what `permute_keys` + `sort_key_value` return, without the sort.  None when
    the shape of the problem is not the kernel's (`lead_last_plan`); `failed`: a device int64 word the kernels set when a range
    was too full (the caller reads it with its own read-back and takes the sort then)."""
    dev = require_hip(keys, vals)
    n = int(keys.numel())
    lim = _ffi.lib().spamd_keys_lead_last_limits
    plan = lead_last_plan(n, n_slabs, n_cells, int(lim(0)), int(lim(1))) if LEAD_LAST and vals.element_size() in (4, 8) else None
    if plan is None:
        return None
    cells, ranges = plan
    bounds = torch.empty(n_slabs * (ranges + 1), dtype=torch.int32, device=dev)
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    _ffi.call("spamd_keys_lead_last", vals.element_size(), n, ptr(keys.contiguous()), ptr(vals.contiguous()), int(n_slabs), int(n_cells),
              cells, ptr(bounds), ptr(ko), ptr(vo), ptr(failed), stream_ptr(dev))
    LEAD_LAST_STATS.update(cells=cells, ranges=ranges, calls=LEAD_LAST_STATS.get("calls", 0) + 1)
    return ko, vo


def keys_check(keys):
    """(not_sorted, has_duplicates) of a key array — the `np.diff(linear)` checks of reference
    core.py:1310-1313,1331-1338.  Synchronises (8 bytes copied back)."""
    dev = require_hip(keys)
    if keys.numel() < 2:
        return False, False
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    _ffi.call("spamd_keys_check", keys.numel(), ptr(keys), ptr(flags), stream_ptr(dev))
    f = flags.tolist()
    return bool(f[0]), bool(f[1])


def coords_in_range(coords, shape):
    """True if every coordinate lies in [0, shape[d]) — one read-only pass, 4 bytes copied back."""
    dev = require_hip(coords)
    ndim, nnz = int(coords.shape[0]), int(coords.shape[1])
    if ndim == 0 or nnz == 0:
        return True
    _check_ndim(ndim)
    coords = coords.contiguous()
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _ffi.call("spamd_coords_check", code_of(coords.dtype), ndim, nnz, ptr(coords), nnz, _harr64(shape), ptr(flag),
              stream_ptr(dev))
    return int(flag.item()) == 0


def sort_keys(keys, max_key):
    """Stable sort of int64 keys in [0, max_key]; returns (sorted_keys, perm) with
    sorted_keys == keys[perm] — `np.argsort(kind="mergesort")` (reference core.py:1315)."""
    dev = require_hip(keys)
    n = int(keys.numel())
    if n == 0:
        return keys, torch.empty(0, dtype=torch.int64, device=dev)
    iota = torch.empty(n, dtype=torch.int64, device=dev)
    _ffi.call("spamd_iota", n, ptr(iota), stream_ptr(dev))
    ws_bytes = int(_ffi.lib().spamd_sort_pairs_ws_bytes(n))
    if ws_bytes < 0:
        raise _ffi.HipBackendError(f"spamd_sort_pairs_ws_bytes failed: {ws_bytes}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    ko, po = torch.empty_like(keys), torch.empty_like(iota)
    _ffi.call("spamd_sort_pairs", n, ptr(keys.contiguous()), ptr(ko), ptr(iota), ptr(po), _key_bits(max_key),
              ptr(ws), ws_bytes, stream_ptr(dev))
    return ko, po


def sort_key_value(keys, vals, max_key):
    """Stable sort of (int64 key, value) pairs by key; values are moved bit-wise."""
    dev = require_hip(keys, vals)
    n = int(keys.numel())
    if n == 0:
        return keys, vals
    ws_bytes = int(_ffi.lib().spamd_sort_kv_ws_bytes(vals.element_size(), n))
    if ws_bytes < 0:
        raise _ffi.HipBackendError(f"spamd_sort_kv_ws_bytes failed: {ws_bytes}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    _ffi.call("spamd_sort_kv", vals.element_size(), n, ptr(keys.contiguous()), ptr(ko), ptr(vals.contiguous()), ptr(vo),
              _key_bits(max_key), ptr(ws), ws_bytes, stream_ptr(dev))
    return ko, vo


def exclusive_scan(flags):
    """`flags` holds n+1 int64 entries (the last is ignored); returns offsets[n+1] with
    offsets[n] = total."""
    dev = require_hip(flags)
    n = int(flags.numel()) - 1
    out = torch.empty_like(flags)
    ws_bytes = int(_ffi.lib().spamd_scan_ws_bytes(n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _ffi.call("spamd_exclusive_scan", n, ptr(flags), ptr(out), ptr(ws), ws_bytes, stream_ptr(dev))
    return out


def new_flags(n, dev):
    """int64[n+1] flag buffer for flag_* -> exclusive_scan -> compact."""
    return torch.empty(n + 1, dtype=torch.int64, device=dev)


def flag_heads(keys):
    dev = require_hip(keys)
    f = new_flags(keys.numel(), dev)
    _ffi.call("spamd_flag_heads", keys.numel(), ptr(keys), ptr(f), stream_ptr(dev))
    return f


def flag_ne_bits(data, fill_value):
    """flags[i] = data[i] is not bit-identical to fill_value (reference `equivalent` without
    `loose`, _utils.py:448-452)."""
    dev = require_hip(data)
    f = new_flags(data.numel(), dev)
    lo, hi = _fill_words(fill_value, np_dtype(data.dtype))
    _ffi.call("spamd_flag_ne_bits", data.element_size(), data.numel(), ptr(data.contiguous()), lo, hi, ptr(f),
              stream_ptr(dev))
    return f


DENSE_NONFILL = True
DENSE_NONFILL_DIRECT = 1 << 24     # elements up to which the outputs are allocated for the worst case (12-16 bytes each) and trimmed


def dense_nonfill(flat, fill_value, numeric=False):
    """(keys, values) of the elements of a flat dense tensor that are not bit-identical to `fill_value`, keys ascending - one
    pass (csrc/prims.hip `spamd_dense_nonfill`) instead of flags + scan + iota + two compactions.  None for element sizes the
    kernel does not take (complex128) and for inputs so large that worst-case outputs would not be reasonable."""
    dev = require_hip(flat)
    n = int(flat.numel())
    if not DENSE_NONFILL or flat.element_size() not in (1, 2, 4, 8) or n == 0 or n > DENSE_NONFILL_DIRECT:
        return None
    lo, _ = _fill_words(fill_value, np_dtype(flat.dtype))
    mask = (1 << 64) - 1
    if numeric:     # `value != 0`: +0 and -0 are one value (NaN is not zero: kept, as NumPy's comparison keeps it)
        if lo != 0:
            return None
        if flat.dtype.is_floating_point:
            mask = (1 << (8 * flat.element_size() - 1)) - 1
    work = torch.empty(int(_ffi.lib().spamd_dense_nonfill_work_words(n)), dtype=torch.int64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    vals = torch.empty(n, dtype=flat.dtype, device=dev)
    _ffi.call("spamd_dense_nonfill", flat.element_size(), n, ptr(flat.contiguous()), lo, mask, ptr(work), ptr(keys), ptr(vals), stream_ptr(dev))
    count = int(work[1])
    if count * 4 < n * 3:
        return keys[:count].clone(), vals[:count].clone()
    return keys[:count], vals[:count]


def _fill_words(fill_value, npdt):
    """The fill value's bit pattern as (low 8 bytes, bytes 8..15): the second word is only non-zero for 16-byte
    elements (complex128: real part, imaginary part)."""
    raw = np.asarray(fill_value, dtype=npdt).reshape(1)
    if npdt.itemsize == 16:
        w = raw.view(np.uint64)
        return int(w[0]), int(w[1])
    return int(raw.view(f"u{npdt.itemsize}")[0]), 0


def note_zero_bits_count(data, count):
    """Remember (on the tensor, for as long as it is not written to) how many of its elements have all-zero bits — a
    producer that has just written `data` knows it for free (the SpGEMM pack kernel), and `count_eq_bits(data, 0)`, i.e.
    the prune of a zero-fill container built from it, then costs one device word instead of a pass over the data."""
    data._zero_bits_count = (count, data._version)


def known_eq_bits(data, fill_value):
    """The number of stored elements bit-identical to `fill_value` when the producer of `data` left it on the tensor
    (`note_zero_bits_count`: all-zero bits only) and the tensor was not written since; None otherwise.  No device work."""
    known = getattr(data, "_zero_bits_count", None)
    if known is None or known[1] != data._version or data.numel() == 0:
        return None
    bits, bits_hi = _fill_words(fill_value, np_dtype(data.dtype))
    return known[0] if bits == 0 and bits_hi == 0 else None


def count_eq_bits(data, fill_value):
    """Number of stored elements bit-identical to fill_value (one read-only pass)."""
    dev = require_hip(data)
    if data.numel() == 0:
        return 0
    bits, bits_hi = _fill_words(fill_value, np_dtype(data.dtype))
    known = getattr(data, "_zero_bits_count", None)
    if bits == 0 and bits_hi == 0 and known is not None and known[1] == data._version:
        return int(known[0])
    c = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_count_eq_bits", data.element_size(), data.numel(), ptr(data.contiguous()), bits, bits_hi, ptr(c),
              stream_ptr(dev))
    return int(c[0])


PRUNE_COUNT_FIRST = 1 << 22   # above this many elements a prune first counts the fill values (usually zero)


def compact(src, flags, offsets, count):
    """Stream compaction of a 1-D tensor or of every row of a 2-D [k, n] tensor."""
    dev = require_hip(src)
    n = int(src.shape[-1])
    if src.dim() == 1:
        dst = torch.empty(count, dtype=src.dtype, device=dev)
        _ffi.call("spamd_compact", src.element_size(), n, ptr(src.contiguous()), ptr(flags), ptr(offsets), ptr(dst),
                  stream_ptr(dev))
        return dst
    src = src.contiguous()
    dst = torch.empty((src.shape[0], count), dtype=src.dtype, device=dev)
    _ffi.call("spamd_compact_rows", src.element_size(), int(src.shape[0]), n, ptr(src), n, ptr(flags), ptr(offsets), ptr(dst),
              count, stream_ptr(dev))   # all rows of the [k, n] matrix in one launch
    return dst


def gather(src, perm):
    """src[..., perm] for 1-D or [k, n] tensors."""
    dev = require_hip(src, perm)
    n = int(perm.numel())
    if src.dim() == 1:
        dst = torch.empty(n, dtype=src.dtype, device=dev)
        _ffi.call("spamd_gather", src.element_size(), n, ptr(src.contiguous()), ptr(perm), ptr(dst), stream_ptr(dev))
        return dst
    src = src.contiguous()
    dst = torch.empty((src.shape[0], n), dtype=src.dtype, device=dev)
    _ffi.call("spamd_gather_rows", src.element_size(), int(src.shape[0]), n, ptr(src), int(src.shape[1]), ptr(perm), ptr(dst), n,
              stream_ptr(dev))
    return dst


def scatter_into(dst_flat, keys, src):
    dev = require_hip(dst_flat, keys, src)
    _ffi.call("spamd_scatter", src.element_size(), keys.numel(), ptr(src.contiguous()), ptr(keys), ptr(dst_flat),
              stream_ptr(dev))
    return dst_flat


def keys_to_csr(keys, R, C, idx_dtype):
    dev = require_hip(keys)
    nnz = int(keys.numel())
    indptr = torch.empty(R + 1, dtype=idx_dtype, device=dev)
    indices = torch.empty(nnz, dtype=idx_dtype, device=dev)
    _ffi.call("spamd_keys_to_csr", code_of(idx_dtype), nnz, ptr(keys), R, C, ptr(indptr), ptr(indices), stream_ptr(dev))
    return indptr, indices


def csr_to_keys(indptr, indices, R, C):
    dev = require_hip(indptr, indices)
    (indptr, indices), it = _unify_index(indptr.contiguous(), indices.contiguous())
    nnz = int(indices.numel())
    keys = torch.empty(nnz, dtype=torch.int64, device=dev)
    _ffi.call("spamd_csr_to_keys", code_of(it), R, nnz, ptr(indptr), ptr(indices), C, ptr(keys), stream_ptr(dev))
    return keys


def rows_to_indptr(rows, R):
    """int64 indptr of sorted row ids (`cumsum(bincount(coords[0]))`, reference _common.py:452-458)."""
    dev = require_hip(rows)
    if not index_dtype_ok(rows):
        rows = rows.to(torch.int64)
    indptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_rows_to_indptr", code_of(rows.dtype), rows.numel(), ptr(rows.contiguous()), R, ptr(indptr),
              stream_ptr(dev))
    return indptr


_CODE_T = {torch.float32: _ffi.F32, torch.float64: _ffi.F64, torch.int32: _ffi.I32, torch.int64: _ffi.I64,
           torch.bool: _ffi.U8, torch.uint8: _ffi.U8}


def convert(t, dtype):
    """astype on the device between float32/float64/int32/int64/bool, and from any of those or a complex type to
    complex64/complex128 (`spamd_cplx_convert`; complex -> real discards a part and is not a device conversion)."""
    dtype = torch_dtype(dtype)
    if t.dtype == dtype:
        return t
    dev = require_hip(t)
    if dtype in _COMPLEX_CODE and (t.dtype in _CODE_T or t.dtype in _COMPLEX_CODE):
        out = torch.empty(t.shape, dtype=dtype, device=dev)
        _ffi.call("spamd_cplx_convert", _CODE_T.get(t.dtype, _COMPLEX_CODE.get(t.dtype)), _COMPLEX_CODE[dtype], t.numel(),
                  ptr(t.contiguous()), ptr(out), stream_ptr(dev))
        return out
    if t.dtype not in _CODE_T or dtype not in _CODE_T:
        raise TypeError(f"hip backend cannot convert {t.dtype} -> {dtype}")
    out = torch.empty(t.shape, dtype=dtype, device=dev)
    _ffi.call("spamd_convert", _CODE_T[t.dtype], _CODE_T[dtype], t.numel(), ptr(t.contiguous()), ptr(out),
              stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------
# the rest of the `_dot_*` kernel family (reference _common.py:758-1158), built on the kernels above
# ---------------------------------------------------------------------------------------------
def csx_swap_2d(data, indices, indptr, n_major, n_minor):
    """Re-compress a 2-D compressed matrix along its other axis (CSR <-> CSC): returns (data, indices, indptr) with
    n_minor + 1 pointers.  The input is ordered by (major, minor), so a STABLE sort on the minor index alone gives
    (minor, major) order: ceil(log2(n_minor)) key bits instead of log2(n_major * n_minor), and the major ids and
    4-byte values ride along packed into one 8-byte payload (no permutation + gathers).
    (`_transpose` / change_compressed_axes, reference _compressed/convert.py:210-273, compressed.py:388-423)."""
    dev = require_hip(data, indices, indptr)
    nnz = int(indices.numel())
    it = indices.dtype if index_dtype_ok(indices) else torch.int64
    if nnz == 0:
        return data, indices.to(it), torch.zeros(n_minor + 1, dtype=it, device=dev)
    if data.element_size() in (4, 8) and n_major < 2 ** 31 and n_minor < 2 ** 31 and index_dtype_ok(indices) \
            and indices.dtype == indptr.dtype and not data.is_complex():
        # one library call: pack (32-bit minor key, major id | value bits), stable sort on the key, unpack + pointers
        # (8-byte values - the reference's default float64 - ride in a 16-byte payload: round 4; before, they went through a
        # 64-bit key sort with a permutation payload and two gathers: ~8 ms per 10^8 elements)
        wide = data.element_size() == 8
        ws_bytes = int((_ffi.lib().spamd_csx_swap8_ws_bytes if wide else _ffi.lib().spamd_csx_swap_ws_bytes)(nnz))
        if ws_bytes < 0:
            raise _ffi.HipBackendError(f"spamd_csx_swap_ws_bytes failed: {ws_bytes}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        new_data, new_indices = torch.empty_like(data.contiguous()), torch.empty(nnz, dtype=it, device=dev)
        new_indptr = torch.empty(n_minor + 1, dtype=it, device=dev)
        _ffi.call("spamd_csx_swap8" if wide else "spamd_csx_swap", code_of(it), int(n_major), int(n_minor), nnz, ptr(data.contiguous()), ptr(indices.contiguous()),
                  ptr(indptr.contiguous()), ptr(new_data), ptr(new_indices), ptr(new_indptr), ptr(ws), ws_bytes, stream_ptr(dev))
        return new_data, new_indices, new_indptr
    major = csr_to_keys(indptr, torch.zeros_like(indices), n_major, 1)     # major id of every stored element
    keys = convert(indices.contiguous(), torch.int64)
    if data.element_size() == 4 and n_major < 2 ** 31:
        payload = torch.stack([major.to(torch.int32), data.contiguous().view(torch.int32)], dim=1).view(torch.int64)
        keys, payload = sort_key_value(keys, payload.reshape(-1), max(n_minor - 1, 1))
        pr = payload.view(torch.int32).reshape(nnz, 2)
        new_indices = pr[:, 0].contiguous().to(it)
        new_data = pr[:, 1].contiguous().view(data.dtype)
    else:
        keys, perm = sort_keys(keys, max(n_minor - 1, 1))
        new_indices = gather(major, perm).to(it)
        new_data = gather(data, perm)
    new_indptr = rows_to_indptr(keys, n_minor).to(it)
    return new_data, new_indices, new_indptr


def _csc_to_csr(a_shape, a_data, a_indices, a_indptr):
    """(M x K) stored by columns -> CSR arrays.  Stable: within a row the columns ascend, so
    the CSR product accumulates in the same k order as the reference's column sweep."""
    M, Kd = int(a_shape[0]), int(a_shape[1])
    return csx_swap_2d(a_data, a_indices, a_indptr, Kd, M)


def dot_csc_ndarray(a_shape, b_shape, a_data, a_indices, a_indptr, b, *, exact=False):
    """C = A @ B with A stored by columns — `_dot_csc_ndarray` (reference _common.py:869-904).
    The reference scatters `out[ind, :] += v * b[i, :]` column by column; here A is re-compressed
    by rows on the device (a stable key sort) and the CSR kernel is used: same per-element
    summation order, no atomics, deterministic."""
    data, indices, indptr = _csc_to_csr(a_shape, a_data, a_indices, a_indptr)
    return dot_csr_ndarray((int(a_shape[0]), int(b_shape[1])), data, indices, indptr, b, exact=exact)


def dot_coo_ndarray(coords, data, b, out_shape, *, exact=False):
    """C = S @ B, S a row-sorted 2-D COO — `_dot_coo_ndarray` (reference _common.py:979-1014).
    Takes B itself (K x N); the reference kernel receives the transposed view."""
    M = int(out_shape[0])
    indptr = rows_to_indptr(coords[0], M)
    cols = coords[1]
    return dot_csr_ndarray(out_shape, data, cols, indptr, b, exact=exact)


def coo_transposed_csr(coords, data, Kd, N):
    """S^T compressed by rows - (data, indices, indptr) - of a 2-D COO S (Kd x N): what `dot_ndarray_coo` multiplies with.
    Depends on S alone; `_dot` keeps it with the operand between products."""
    keys = linearize(coords, (Kd, N), axis_order=(1, 0))    # col * K + row
    keys, perm = sort_keys(keys, max(Kd * N - 1, 1))
    it = coords.dtype if index_dtype_ok(coords) else torch.int64
    indptr, indices = keys_to_csr(keys, N, Kd, it)
    return gather(data, perm), indices, indptr


def dot_ndarray_coo(a, coords, data, out_shape, *, exact=False, st=None):
    """C = A @ S, A dense (M x K), S 2-D COO (K x N) — `_dot_ndarray_coo`
    (reference _common.py:1075-1103), computed as (S^T @ A^T)^T with S^T compressed by rows (`st`: that form, when the
    caller has it already)."""
    M, N = int(out_shape[0]), int(out_shape[1])
    Kd = int(a.shape[1])
    tdata, indices, indptr = st if st is not None else coo_transposed_csr(coords, data, Kd, N)
    res = dot_csr_ndarray((N, M), tdata, indices, indptr, a.t().contiguous(), exact=exact)
    return res.t()


def _sparsify(dense, struct_mask=None, numeric=False):
    """Dense 2-D tensor -> (keys, data) of the entries to store.  `struct_mask` (same shape, any
    dtype, nonzero = structurally present) restricts them; `numeric=True` keeps value != 0
    (the COO variants' `if data_curr != 0`), otherwise bit-pattern != +0 (GCXS prune)."""
    flat = dense.reshape(-1).contiguous()
    if struct_mask is None and flat.dtype in (torch.float32, torch.float64, torch.int32, torch.int64):
        fused = dense_nonfill(flat, 0, numeric=numeric)
        if fused is not None:
            return fused
    if numeric and flat.is_complex():
        flags = _complex_nonzero_flags(flat)
    elif numeric:
        from ._umath import binary_arrays

        nz = binary_arrays("not_equal", flat, torch.zeros(1, dtype=flat.dtype, device=flat.device), b_scalar=True)
        flags = flag_ne_bits(nz.view(torch.uint8), 0)
    else:
        flags = flag_ne_bits(flat, 0)
    if struct_mask is not None:
        from ._umath import binary_arrays

        sm = flag_ne_bits(struct_mask.reshape(-1).contiguous(), 0)
        flags = binary_arrays("multiply", flags, sm)
    offs = exclusive_scan(flags)
    cnt = int(offs[-1])
    n = flat.numel()
    iota = torch.empty(n, dtype=torch.int64, device=flat.device)
    _ffi.call("spamd_iota", n, ptr(iota), stream_ptr(flat.device))
    return compact(iota, flags, offs, cnt), compact(flat, flags, offs, cnt)


def _complex_nonzero_flags(flat):
    """int64 flags [n + 1] of a flat complex tensor: 1 where the value != 0, i.e. where either part is (+0 and -0 are both
    zero, NaN is not) - the real comparison over the (re, im) reals, then each pair of result bytes tested as one 16-bit word."""
    from ._umath import binary_arrays

    reals = _as_reals(flat.contiguous())
    nz = binary_arrays("not_equal", reals, torch.zeros(1, dtype=reals.dtype, device=reals.device), b_scalar=True,
                       out_bool_as=torch.uint8)
    return flag_ne_bits(nz.view(torch.int16), 0)


def _pattern_product(out_shape, a_indices, a_indptr, b, csc_shape=None):
    """Structural non-zero test of the reference's sparse-returning variants: entry (i, j) is
    stored iff some b[k, j] != 0 with k in row i of A (_common.py:796-798, 843-844)."""
    from ._umath import binary_arrays

    if b.is_complex():
        bz = _complex_nonzero_flags(b.reshape(-1))[:b.numel()]
    else:
        bz = binary_arrays("not_equal", b.reshape(-1).contiguous(), torch.zeros(1, dtype=b.dtype, device=b.device),
                           b_scalar=True)
    bz = convert(bz, torch.float32).reshape(b.shape)
    ones = torch.ones(a_indices.numel(), dtype=torch.float32, device=b.device)
    if csc_shape is None:
        return dot_csr_ndarray(out_shape, ones, a_indices, a_indptr, bz)
    return dot_csc_ndarray(csc_shape, tuple(b.shape), ones, a_indices, a_indptr, bz)


def dot_csr_ndarray_sparse(out_shape, a_data, a_indices, a_indptr, b):
    """CSR @ dense returned as CSR (data, indices, indptr[int64]) — `_dot_csr_ndarray_sparse`
    (reference _common.py:758-804) after the GCXS constructor's prune."""
    dense = dot_csr_ndarray(out_shape, a_data, a_indices, a_indptr, b, exact=True)
    mask = _pattern_product(out_shape, a_indices, a_indptr, b.to(dense.dtype) if b.dtype != dense.dtype else b)
    keys, data = _sparsify(dense, mask)
    indptr, indices = keys_to_csr(keys, int(out_shape[0]), int(out_shape[1]), torch.int64)
    return data, indices, indptr


def dot_csc_ndarray_sparse(a_shape, b_shape, a_data, a_indices, a_indptr, b):
    """CSC @ dense returned compressed by COLUMNS — `_dot_csc_ndarray_sparse`
    (reference _common.py:807-866)."""
    M, N = int(a_shape[0]), int(b_shape[1])
    dense = dot_csc_ndarray(a_shape, b_shape, a_data, a_indices, a_indptr, b, exact=True)
    mask = _pattern_product((M, N), a_indices, a_indptr, b.to(dense.dtype) if b.dtype != dense.dtype else b,
                            csc_shape=a_shape)
    keys, data = _sparsify(dense.t().contiguous(), mask.t().contiguous())  # column-major keys: col*M + row
    indptr, indices = keys_to_csr(keys, N, M, torch.int64)
    return data, indices, indptr


def dot_coo_ndarray_sparse(coords, data, b, out_shape, as_keys=False):
    """COO @ dense returned as COO (coords, data) — reference _common.py:1017-1072.  `as_keys`: (sorted linear keys, data)
    instead - the caller's container builds coordinates on demand."""
    dense = dot_coo_ndarray(coords, data, b, out_shape, exact=True)
    keys, vals = _sparsify(dense, numeric=True)
    return (keys, vals) if as_keys else (delinearize(keys, tuple(int(s) for s in out_shape), torch.int64), vals)


def dot_ndarray_coo_sparse(a, coords, data, out_shape, as_keys=False, st=None):
    """dense @ COO returned as COO — reference _common.py:1106-1158."""
    dense = dot_ndarray_coo(a, coords, data, out_shape, exact=True, st=st).contiguous()
    keys, vals = _sparsify(dense, numeric=True)
    return (keys, vals) if as_keys else (delinearize(keys, tuple(int(s) for s in out_shape), torch.int64), vals)


SPGEMM_CHUNK_PRODUCTS = 1 << 27  # products expanded/sorted at a time (bounds workspace to ~5 GB)
SPGEMM_RUN_PROBE_MIN = 1 << 13   # chunks with fewer products: even one output element holding all of them is short work
SPGEMM_RUN_DUPS_MIN = 1023       # ... and with fewer products that share their element with an earlier one there is no long run
SPGEMM_RUN_LONG = True           # False: always the one-thread-per-element sums (tests)


@functools.lru_cache(maxsize=None)
def _spgemm_vcode(dtr):
    """`code_of` the result type, None where it raises: complex values, which only the global form takes, and the types no
    kernel takes (the global form's `product_code` raises for those).  (Remembered: the route and the operands both ask.)"""
    try:
        return code_of(dtr)
    except TypeError:
        return None


class SpgemmOperands:
    """The operands of one sparse @ sparse product, prepared once (`_spgemm_operands`) and handed to every executor: the
    shape, the result type `dtr` with its value code (`_spgemm_vcode`), both value arrays cast to `dtr`, the index arrays
    contiguous and of one width `it`, the device and its stream.  The width is unified over four arrays for the small, bitmap and bucket
    kernels; `keys_index` = (a_indices, b_indices, b_indptr, their type) is the global form's width over those three alone (a
    GCXS may have int32 indices and int64 pointers: the same tensors wherever the two widths agree).  `a_rows`: the row id
    of every element of A where the caller has it (COO), else None (`_spgemm_a_rows`)."""

    __slots__ = ("n_row", "n_inner", "n_col", "dtr", "vcode", "it", "a_data", "a_indices", "a_indptr", "b_data", "b_indices",
                 "b_indptr", "keys_index", "a_rows", "dev", "s")


def _spgemm_operands(n_row, n_col, dtr, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr, a_rows=None, row_local=True):
    """SpgemmOperands of a product; `row_local` False: for the global form alone (A's pointers stay as they are, out of the
    index width)."""
    p = SpgemmOperands()
    p.n_row, p.n_inner, p.n_col, p.dtr = n_row, int(b_indptr.numel()) - 1, n_col, dtr
    p.dev = require_hip(a_data, b_data)
    p.s, p.vcode = stream_ptr(p.dev), _spgemm_vcode(dtr)
    p.a_data = a_data.to(dtr).contiguous() if a_data.dtype != dtr else a_data.contiguous()
    p.b_data = b_data.to(dtr).contiguous() if b_data.dtype != dtr else b_data.contiguous()
    a_indices, b_indices, b_indptr = a_indices.contiguous(), b_indices.contiguous(), b_indptr.contiguous()
    if not row_local:
        (p.a_indices, p.b_indices, p.b_indptr), p.it = _unify_index(a_indices, b_indices, b_indptr)
        p.a_indptr, p.keys_index = a_indptr, (p.a_indices, p.b_indices, p.b_indptr, p.it)
    else:
        (p.a_indices, p.a_indptr, p.b_indices, p.b_indptr), p.it = _unify_index(a_indices, a_indptr.contiguous(), b_indices, b_indptr)
        if p.it == torch.int64 and a_indices.dtype == b_indices.dtype == b_indptr.dtype == torch.int32:
            p.keys_index = (a_indices, b_indices, b_indptr, torch.int32)    # (A's pointers alone are wide)
        else:
            p.keys_index = (p.a_indices, p.b_indices, p.b_indptr, p.it)
    p.a_rows = a_rows
    return p


def _spgemm_a_rows(p):
    """The row id of every element of A (int64): the caller's, else from A's pointers.  One product asks once: the global
    form for all of A, or the bucket path for its heavy rows."""
    if p.a_rows is not None:
        return convert(p.a_rows.contiguous(), torch.int64)
    return csr_to_keys(p.a_indptr, torch.zeros_like(p.a_indices, dtype=p.a_indptr.dtype), p.n_row, 1)


def _spgemm_keys(p, part=None):
    """Expand-sort-compress over row chunks; returns (keys, data) sorted by row*n_col + col with
    every output element summed in the reference's order.  `part` = (a_data, a_indices, a_rows) of the elements of A to
    take, at the width of `p.it` (the heavy rows of the bucket path); None: all of A, at the width of `p.keys_index`."""
    from ._reduce import segment_reduce

    n_row, n_col, dtr, dev, s = p.n_row, p.n_col, p.dtr, p.dev, p.s
    vcode = product_code(dtr)
    if part is None:
        a_data, a_rows, b_data, (a_indices, b_indices, b_indptr, it) = p.a_data, _spgemm_a_rows(p), p.b_data, p.keys_index
    else:
        (a_data, a_indices, a_rows), b_data, b_indices, b_indptr, it = part, p.b_data, p.b_indices, p.b_indptr, p.it
    nnz_a = int(a_indices.numel())
    out_keys, out_vals = [], []
    if nnz_a == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=dtr, device=dev)
    cnt = torch.empty(nnz_a + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spgemm_count", code_of(it), 0, nnz_a, ptr(a_indices), ptr(b_indptr), ptr(cnt), s)
    offs_all = exclusive_scan(cnt)
    total = int(offs_all[-1])
    # chunk boundaries on A elements so that each chunk expands <= SPGEMM_CHUNK_PRODUCTS products;
    # a chunk always ends on a ROW boundary of A so that no output element is split
    p = 0
    row_ends = None
    while p < nnz_a:
        if total - int(offs_all[p]) <= SPGEMM_CHUNK_PRODUCTS:
            q = nnz_a
        else:
            target = int(offs_all[p]) + SPGEMM_CHUNK_PRODUCTS
            q = int(torch.searchsorted(offs_all, torch.tensor([target], device=dev), right=True)[0]) - 1
            q = max(q, p + 1)
            # advance q to the end of the row that element q-1 belongs to
            r = int(a_rows[q - 1])
            q = int(torch.searchsorted(a_rows, torch.tensor([r], device=dev), right=True)[0])
        P = int(offs_all[q]) - int(offs_all[p])
        if P:
            offs = (offs_all[p:q + 1] - offs_all[p]).contiguous()
            keys = torch.empty(P, dtype=torch.int64, device=dev)
            vals = torch.empty(P, dtype=dtr, device=dev)
            _ffi.call("spamd_spgemm_expand", vcode, code_of(it), p, q - p, ptr(a_data), ptr(a_indices), ptr(a_rows),
                      ptr(b_data), ptr(b_indices), ptr(b_indptr), ptr(offs), P, n_col, ptr(keys), ptr(vals), s)
            if vals.element_size() > 8:     # complex128: the pair sort moves 4- and 8-byte values; sort a permutation, gather
                keys, perm = sort_keys(keys, max(n_row * n_col - 1, 1))
                vals = gather(vals, perm)
            else:
                keys, vals = sort_key_value(keys, vals, max(n_row * n_col - 1, 1))
            heads = flag_heads(keys)
            ho = exclusive_scan(heads)
            c = int(ho[-1])
            summed = None
            if P >= SPGEMM_RUN_PROBE_MIN and P - c >= SPGEMM_RUN_DUPS_MIN and dtr in _CODE_T and dtr != torch.bool:
                # one thread per output element adds its products left to right (the reference's `sums[j] += ...` order, bit for
                # bit) - and walks alone when an element has 5 x 10^4 of them (the diagonal element of a hub row in a @ a.T:
                # 10.5 ms of a 15 ms product, tools/r06/spgemm_hub.py).  When the scan of the head flags shows a window of 1024
                # products without a head (`has_long_run`: P / 1024 words read; P - c products share their element with an
                # earlier one - fewer than a long run's, and there is none), the grouped reduce adds the runs - any length,
                # streaming speed, re-associated: 1e-12 / 1e-5 relative.
                from ._reduce import group_reduce, has_long_run

                if SPGEMM_RUN_LONG and has_long_run(ho):
                    summed = group_reduce(keys, 1, vals, "add", key_bound=max(n_row * n_col, 1), sync=False)[1][:c]
            out_vals.append(summed if summed is not None else segment_reduce(vals, heads, ho, c, "add", sequential=True))
            out_keys.append(compact(keys, heads, ho, c))
        p = q
    if not out_keys:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=dtr, device=dev)
    return (torch.cat(out_keys), torch.cat(out_vals)) if len(out_keys) > 1 else (out_keys[0], out_vals[0])


SPGEMM_ROW_LOCAL = True  # tuning hook: False = always the global expand-sort-compress


SPGEMM_STATS = {}   # last product: its route, rows, rows left to the global form (diagnostics for the benches; `_spgemm` writes it)
SPGEMM_BITMAP = True            # wide rows of a matrix with <= 2^20 columns: csrc/spgemm_bitmap.hip (rows written in place)
SPGEMM_BITMAP_MIN_MEAN = 1300   # mean products per row from which the per-row bitmap scan (n_col / 8 bytes of LDS) pays: measured
#                                 at n_col = 10^6, 60000 rows (tools/r04/spgemm_sweep.py; ms buckets / bitmap), round 6 (the bitmap
#                                 kernel of round 5): 400 products per row 1.07 / 2.31, 900: 1.79 / 2.40, 1296: 2.51 / 2.51,
#                                 1600: 2.77 / 2.53, 2025: 3.09 / 2.59, 4096: 6.48 / 3.08, 6400: 8.02 / 3.84, 10^4: 14.0 / 5.34
#                                 (round 4, when 1536 was chosen: 900: 1.91 / 2.55, 2025: 3.36 / 2.89, 10^4: 13.95 / 6.45)
SPGEMM_BITMAP_MAX_DUPS = 120    # expected products per row that share an output element with an earlier one (list of 512)


_BITMAP_UNSUPPORTED = set()    # (device index, split form?) whose launch the library refused once
_BITMAP_REFUSAL_CODES = (1, 2, 9, 701)   # hipError_t values that mean "not with these resources", not "the device faulted"


def _spgemm_bitmap(p, parts, total):
    """C = A @ B by csrc/spgemm_bitmap.hip: ((data, int64 indices, int64 indptr), seen), the triple None when a row (or part
    of a row) exceeded the kernel's limits or the library refuses this form on this device (the caller then tries the next
    form); `seen` = what the attempt leaves for SPGEMM_STATS.  `parts` = 1: whole rows, one workgroup per CU; > 1: column
    ranges, two workgroups per CU.  The result buffers are allocated for every product (an upper bound of the result's
    length) and trimmed: a view when at least 3/4 of them are used."""
    n_row, dev = p.n_row, p.dev
    if (dev.index, parts > 1) in _BITMAP_UNSUPPORTED:
        return None, {}
    out_idx = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    out_val = torch.empty(max(total, 1), dtype=p.dtr, device=dev)
    out_ptr = torch.empty(n_row + 1, dtype=torch.int64, device=dev)
    work = torch.empty(n_row * parts + 32, dtype=torch.int64, device=dev)
    bsplit = torch.empty(max(p.n_inner * (parts - 1), 1), dtype=p.it, device=dev) if parts > 1 else None
    try:
        _ffi.call("spamd_spgemm_bitmap", p.vcode, code_of(p.it), n_row, p.n_inner, p.n_col, parts, ptr(p.a_indptr), ptr(p.a_indices),
                  ptr(p.a_data), ptr(p.b_indptr), ptr(p.b_indices), ptr(p.b_data), ptr(bsplit) if bsplit is not None else None,
                  ptr(work), ptr(out_ptr), ptr(out_idx), ptr(out_val), p.s)
    except _ffi.HipBackendError as e:
        # the launch itself was REFUSED - a negative SPAMD_E* from the range / LDS checks, or the runtime declining the 160 KB
        # LDS opt-in or the occupancy query on a part with less (hipErrorInvalidValue 1, hipErrorOutOfMemory 2,
        # hipErrorLaunchOutOfResources 701, hipErrorInvalidConfiguration 9): this form is not available on this device -
        # remembered, and the next form (or the bucket kernels) takes the product.  Any other hipError_t is a device fault
        # (an illegal address from a bad operand, a hung queue): never masked, as in _umath._on_device.
        code = getattr(e, "code", 0)
        if code > 0 and code not in _BITMAP_REFUSAL_CODES:
            raise
        _BITMAP_UNSUPPORTED.add((dev.index, parts > 1))
        return None, {"bitmap_refused": 1}
    failed, zeros, nnz = (int(v) for v in torch.cat([work[1:3], out_ptr[-1:]]).tolist())   # ONE read-back
    seen = {}
    if os.environ.get("SPAMD_BMK_PROF"):     # (-DBMK_PROF builds of csrc/spgemm_bitmap.hip: cycles per phase, thread 0 of every workgroup)
        seen["phase_cycles"] = work[4:20].tolist()
    if failed:
        seen["bitmap_failed"] = 1
        return None, seen
    if nnz * 4 < total * 3:
        out_idx, out_val = out_idx[:nnz].clone(), out_val[:nnz].clone()
    else:
        out_idx, out_val = out_idx[:nnz], out_val[:nnz]
    note_zero_bits_count(out_val, zeros)
    return (out_val, out_idx, out_ptr), seen


SPGEMM_BITMAP_SPLIT = True   # tuning hook: False = only the wide form (whole rows, one workgroup per CU); "first" = the split form first


def _spgemm_bitmap_forms(vcode, n_col, max_prod):
    """The forms of the bitmap kernel to try for this product, best first: a list of `parts` values (1 = wide).  The wide
    form wins where both apply (config-5 share: 13.2 against 14.6 ms with two parts: every part repeats the row's staging,
    scans and look-back with half the threads); the split form is what takes matrices of more than 2^20 columns and rows of
    more than 16384 products."""
    lim = _ffi.lib().spamd_spgemm_bitmap_limits
    forms = []
    if max_prod <= lim(vcode, 0) and n_col <= lim(vcode, 2) and max_prod * max_prod <= 2 * n_col * SPGEMM_BITMAP_MAX_DUPS:
        forms.append(1)
    split_prod, split_cols = int(lim(vcode, 4)), int(lim(vcode, 5))
    if SPGEMM_BITMAP_SPLIT and split_prod and split_cols and (not forms or SPGEMM_BITMAP_SPLIT == "first"):
        parts = max(2, -(-n_col // split_cols))
        # a part holds ~1 / parts of a row's products (uniform columns: + a few standard deviations)
        while parts <= 64 and max_prod / parts + 4 * (max_prod / parts) ** 0.5 + 64 > split_prod:
            parts += 1
        if parts <= 64 and max_prod * max_prod <= 2 * n_col * parts * (SPGEMM_BITMAP_MAX_DUPS // 2):
            forms.insert(0, parts)
    return forms


SPGEMM_SMALL = True
SPGEMM_SMALL_SECOND = True
SPGEMM_SMALL_MAX_CELLS = 1 << 22     # n_row x n_col of the result: its upper-bound buffers (12-16 B per cell) stay below 64 MB
SPGEMM_SMALL_MAX_NNZ = 1 << 16       # stored elements of A (a wave walks its row's elements one after the other): beyond this the
                                     # kernels that spread a row's products over a workgroup have enough work to pay their set-up


SPGEMM_SMALL_MAX_BUFFER = 1 << 30    # entries of the second chance's result buffers (12-16 bytes each)


def _spgemm_small_second(vcode, n_row, n_col, total):
    """Once the row products are known: is this a product for the dense-accumulator kernel after all?  (Round 6,
    tools/r06/spgemm_small_second.py.)  When the result is dense-ish - at least one product per cell of the result - the bucket
    kernel's rows overflow their buckets (a column collects many products) and are redone by the global expand-sort-compress,
    and the bitmap kernel parks too many repeated columns: 3000 x 3000 with 300 elements per row took 28.6 ms, 100000 x 3000
    with 100 per row 91 ms - 1.1 and 7.3 ms with a wave per row over an LDS accumulator, bit-identical.  Below one product
    per cell the accumulator kernel still wins while four waves share a workgroup (rows of at most ~4000 float32 / ~2000
    float64 columns) from a quarter product per cell; with one wave per workgroup or sparser results the other kernels do."""
    if not (SPGEMM_SMALL and SPGEMM_SMALL_SECOND and total and n_row < 2 ** 31):
        return False
    if n_col > int(_ffi.lib().spamd_spgemm_small_max_cols(vcode)) or min(n_row * n_col, total) > SPGEMM_SMALL_MAX_BUFFER:
        return False
    fill = total / (n_row * n_col)
    es = 8 if vcode in (code_of(torch.float64), code_of(torch.int64)) else 4
    four_waves = ((64 * 1024) // 4 - 32) * 8 // (8 * es + 1)       # (sm_max_cols(4), csrc/spgemm_small.hip)
    return fill >= 1.0 or (n_col <= four_waves and fill >= 0.25)


def _spgemm_small_fits(vcode, n_row, n_col):
    """Whether csrc/spgemm_small.hip takes a result of this shape at all (a zero-width result: the kernel's argument check
    refuses n_col <= 0; the general path returns the empty matrix)."""
    return vcode is not None and n_row != 0 and n_col != 0 and n_col <= int(_ffi.lib().spamd_spgemm_small_max_cols(vcode))


def _spgemm_route(n_row, n_col, nnz_a, dtr, products=None):
    """The one choice of kernel for sparse @ sparse: the steps to try in order, each of which may decline (`_spgemm` then
    takes the next one) - ("small", bound), ("probe",), ("bitmap", parts), ("buckets",), ("global",) - from plain numbers:
    the result's shape, the stored elements of A, the result type and, once the row-product probe has run, `products` =
    (total, max_prod, max_arow).  Pure but for the SPGEMM_* switches, read at the call, and the library's host-only limits.

    Before the probe (`products` None): the first chance of the one-launch kernel where the result and A are small; then
    ("probe",) when it is worth launching, else ("global",) - the row-local, small and bitmap kernels are real-only (the global
    expand-sort-compress has complex values, and the TypeError of a type no kernel takes), and they have no rows to walk
    (`n_row` 0) or no room for the column in their keys (`n_col` >= 2^31 - 1).  After it: the second chance of the small
    kernel (`_spgemm_small_second`, its buffers bounded by `total`), the forms of the bitmap kernel where the mean row has
    SPGEMM_BITMAP_MIN_MEAN products and no row of A is longer than the kernel stages (`_spgemm_bitmap_forms`), the bucket
    kernels, the global form.  What only the device can tell - a `failed` word, a refused launch, mostly heavy rows - is a
    decline of the executor, not a rule here."""
    if not SPGEMM_ROW_LOCAL:
        return (("global",),)
    vcode = _spgemm_vcode(dtr)
    if products is None:
        steps = ()
        if SPGEMM_SMALL and n_row * n_col <= SPGEMM_SMALL_MAX_CELLS and nnz_a <= SPGEMM_SMALL_MAX_NNZ and _spgemm_small_fits(vcode, n_row, n_col):
            steps = (("small", None),)
        return steps + ((("global",),) if vcode is None or n_col >= 2 ** 31 - 1 or n_row == 0 else (("probe",),))
    total, max_prod, max_arow = products
    steps = []
    if _spgemm_small_second(vcode, n_row, n_col, total):
        steps.append(("small", total))
    if SPGEMM_BITMAP and total and max_arow <= _ffi.lib().spamd_spgemm_bitmap_limits(vcode, 1) and total >= SPGEMM_BITMAP_MIN_MEAN * n_row:
        steps += [("bitmap", parts) for parts in _spgemm_bitmap_forms(vcode, n_col, max_prod)]
    return (*steps, ("buckets",), ("global",))


def _spgemm_small_run(p, bound=None):
    """csrc/spgemm_small.hip: the whole product in one launch and one read-back (the reference's own benchmark sizes,
    benchmarks/test_benchmark_coo.py:9-40, are launch-bound on the general path: 230-300 us against ~70).  None when a row
    is outside its limits or B is not canonical (the caller takes the general path); the shape is the caller's to check
    (`_spgemm_small_fits`: the route does).
    `bound`: an upper bound of the result's length below its cells (the products, on the second chance)."""
    n_row, n_col, dev = p.n_row, p.n_col, p.dev
    cells = n_row * n_col if bound is None else min(n_row * n_col, int(bound))     # (the result holds at most one element per product)
    out_idx = torch.empty(cells, dtype=torch.int64, device=dev)
    out_val = torch.empty(cells, dtype=p.dtr, device=dev)
    head = torch.empty(2 * n_row + 8, dtype=torch.int64, device=dev)      # [work (n_row + 4) | out_indptr (n_row + 1)]: one buffer, one read-back
    work, out_ptr = head[: n_row + 4], head[n_row + 4: 2 * n_row + 5]
    _ffi.call("spamd_spgemm_small", p.vcode, code_of(p.it), n_row, n_col, ptr(p.a_indptr), ptr(p.a_indices), ptr(p.a_data),
              ptr(p.b_indptr), ptr(p.b_indices), ptr(p.b_data), ptr(work), ptr(out_ptr), ptr(out_idx), ptr(out_val), p.s)
    failed, zeros, nnz = read_words(head[1:4])      # ONE read-back (three adjacent words, through pinned host memory)
    if failed:
        return None
    out_idx, out_val = (out_idx[:nnz].clone(), out_val[:nnz].clone()) if nnz * 4 < cells * 3 else (out_idx[:nnz], out_val[:nnz])
    note_zero_bits_count(out_val, zeros)
    return out_val, out_idx, out_ptr


def _spgemm_probe(p):
    """The products of every output row (csrc/spgemm_rows.hip): (prod[n_row + 1], their exclusive scan, total, max_prod,
    max_arow) - one launch, one scan, the two maxima through pinned memory and the total."""
    prod = torch.empty(p.n_row + 1, dtype=torch.int64, device=p.dev)
    maxes = torch.empty(2, dtype=torch.int64, device=p.dev)
    _ffi.call("spamd_spgemm_row_products", code_of(p.it), p.n_row, ptr(p.a_indptr), ptr(p.a_indices), ptr(p.b_indptr), ptr(prod),
              ptr(maxes), p.s)
    prod_off = exclusive_scan(prod)
    max_prod, max_arow = read_words(maxes)
    return prod, prod_off, int(prod_off[-1]), max_prod, max_arow


def _spgemm_classify(p, prod, cap, nnz_row):
    """(flags[n_row + 1], rows, their products, rows heavy only by their A length) - csrc/spgemm_rows.hip"""
    flags = new_flags(p.n_row, p.dev)
    counts = torch.empty(3, dtype=torch.int64, device=p.dev)
    _ffi.call("spamd_spgemm_classify_rows", code_of(p.it), p.n_row, ptr(prod), ptr(p.a_indptr), ptr(nnz_row) if nnz_row is not None else 0,
              cap, ptr(flags), ptr(counts), p.s)
    return (flags, *[int(v) for v in counts.tolist()])


def _spgemm_merge_heavy(p, flags, n_heavy, prod_off, tmp_cols, tmp_vals, nnz_row):
    """The `n_heavy` rows that `flags` marks, computed by the global form over their elements of A and copied into the
    bucket kernels' scratch (`tmp_cols` / `tmp_vals` at `prod_off`, their lengths into `nnz_row`)."""
    dev, s, n_row = p.dev, p.s, p.n_row
    nA = int(p.a_indices.numel())
    iota = torch.empty(max(n_row, nA) + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_iota", int(iota.numel()), ptr(iota), s)
    heavy_rows = compact(iota[:n_row], flags, exclusive_scan(flags), n_heavy)
    a_rows = _spgemm_a_rows(p)
    eflags = new_flags(nA, dev)
    _ffi.call("spamd_gather", 8, nA, ptr(flags), ptr(a_rows), ptr(eflags), s)
    eflags[nA:] = 0
    eoff = exclusive_scan(eflags)
    sel = compact(iota[:nA], eflags, eoff, int(eoff[-1]))               # A elements of those rows
    hkeys, hvals = _spgemm_keys(p, (gather(p.a_data, sel), gather(p.a_indices, sel), gather(a_rows, sel)))
    hptr, hidx = keys_to_csr(hkeys, n_row, p.n_col, torch.int64)
    _ffi.call("spamd_spgemm_unpack", p.vcode, n_heavy, ptr(heavy_rows.contiguous()), ptr(hptr),
              ptr(hidx), ptr(hvals.contiguous()), ptr(prod_off), ptr(tmp_cols), ptr(tmp_vals), ptr(nnz_row), s)


def _spgemm_buckets(p, prod, prod_off, total, max_prod, max_arow):
    """Row-local SpGEMM (csrc/spgemm_rows.hip): ((data, int64 indices, int64 indptr) of A @ B, the rows it left to the
    global form).  Rows too heavy for LDS are computed by the global expand-sort-compress and merged in; None when most
    of the work is in such rows (the caller then uses the global form throughout)."""
    n_row, dev, s = p.n_row, p.dev, p.s
    cap = int(_ffi.lib().spamd_spgemm_rows_capacity(p.vcode, p.n_col, max_arow))
    if max_prod > cap or max_arow > cap:
        # rows too heavy for LDS (products, or A elements to stage) go through the global expand-sort-compress
        _, n_heavy, heavy_products, n_arow_only = _spgemm_classify(p, prod, cap, None)
        if n_heavy * 4 > n_row or heavy_products * 4 > total * 3 or n_arow_only:
            return None  # mostly heavy (or rows heavy only by their A length): the global form throughout
    tmp_cols = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    tmp_vals = torch.empty(max(total, 1), dtype=p.dtr, device=dev)
    nnz_row = torch.zeros(n_row + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spgemm_rows", p.vcode, code_of(p.it), n_row, p.n_col, ptr(p.a_indptr), ptr(p.a_indices), ptr(p.a_data),
              ptr(p.b_indptr), ptr(p.b_indices), ptr(p.b_data), ptr(prod_off), min(max_prod, cap), max_arow, ptr(tmp_cols),
              ptr(tmp_vals), ptr(nnz_row), s)
    # rows above the capacity were skipped, rows with a column of more than 64 products were declined (nnz_row = -1):
    # both are computed by the global form and copied into the scratch
    flags, n_heavy, _, _ = _spgemm_classify(p, prod, cap, nnz_row)
    if n_heavy:
        _spgemm_merge_heavy(p, flags, n_heavy, prod_off, tmp_cols, tmp_vals, nnz_row)
    out_ptr = exclusive_scan(nnz_row)
    nnz = int(out_ptr[-1])
    out_idx = torch.empty(nnz, dtype=torch.int64, device=dev)
    out_val = torch.empty(nnz, dtype=p.dtr, device=dev)
    zeros = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spgemm_pack", p.vcode, n_row, ptr(prod_off), ptr(out_ptr), ptr(tmp_cols), ptr(tmp_vals), ptr(out_idx),
              ptr(out_val), ptr(zeros), s)
    note_zero_bits_count(out_val, zeros)
    return (out_val, out_idx, out_ptr), n_heavy


def _spgemm(n_row, n_col, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr, a_rows=None, row_local_only=False):
    """A @ B along `_spgemm_route`: ((data, int64 indices, int64 indptr), None) from the first row-local step that delivers,
    else (None, (keys, data)) from the global form - or (None, None) with `row_local_only`.  A is given by its pointers, by
    the row id of every element (`a_rows`, of a COO: its pointers are built when a row-local step wants them) or by both.
    The only writer of SPGEMM_STATS: `route` = small/first | small/second | bitmap | buckets | global is what delivered;
    `kernel`, `rows`, `heavy_or_declined` (and `parts`) with a row-local delivery - `kernel` = "buckets" also when the bucket
    path hands the whole product to the global form; `max_prod`, `max_arow`, `products` once the probe has run; the bitmap
    kernel's `bitmap_failed` (since the probe), `bitmap_refused`, `phase_cycles`."""
    dtr = torch_dtype(dot_dtype(a_data.dtype, b_data.dtype))
    nnz_a = int(a_data.numel())
    steps = _spgemm_route(n_row, n_col, nnz_a, dtr)
    row_local = steps[0][0] != "global"
    if not row_local and row_local_only:
        return None, None
    if row_local and a_indptr is None:
        a_indptr = rows_to_indptr(a_rows, n_row)
    p = _spgemm_operands(n_row, n_col, dtr, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr, a_rows, row_local)
    probe = None
    while steps:
        step, steps = steps[0], steps[1:]
        kind, arg = step[0], step[1:]
        if kind == "probe":
            probe = _spgemm_probe(p)
            SPGEMM_STATS.update(max_prod=probe[3], max_arow=probe[4], products=probe[2])
            SPGEMM_STATS.pop("bitmap_failed", None)
            steps = _spgemm_route(n_row, n_col, nnz_a, dtr, probe[2:])
        elif kind == "small":
            try:
                res = _spgemm_small_run(p, arg[0])
            except torch.OutOfMemoryError:       # (its buffers hold min(cells, products) entries: the other kernels need less)
                if arg[0] is None:
                    raise
                res = None
            if res is not None:
                SPGEMM_STATS.update(kernel="small", rows=n_row, heavy_or_declined=0, route="small/first" if arg[0] is None else "small/second")
                return res, None
        elif kind == "bitmap":
            res, seen = _spgemm_bitmap(p, arg[0], probe[2])
            for key, value in seen.items():
                SPGEMM_STATS[key] = value if key == "phase_cycles" else SPGEMM_STATS.get(key, 0) + value
            if res is not None:
                SPGEMM_STATS.update(rows=n_row, heavy_or_declined=0, kernel="bitmap", parts=arg[0], route="bitmap")
                return res, None
        elif kind == "buckets":
            SPGEMM_STATS["kernel"] = "buckets"
            out = _spgemm_buckets(p, *probe)
            if out is not None:
                SPGEMM_STATS.update(rows=n_row, heavy_or_declined=out[1], route="buckets")
                return out[0], None
        elif not row_local_only:
            keys = _spgemm_keys(p)
            SPGEMM_STATS["route"] = "global"
            return None, keys
    return None, None


def _spgemm_small(n_row, n_col, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr):
    """The one-launch kernel alone, whatever the route's switches say (a test calls it): (data, int64 indices, int64 indptr),
    or None when the operands are outside its limits or B is not canonical.  Writes no statistics."""
    dtr = torch_dtype(dot_dtype(a_data.dtype, b_data.dtype))
    if not _spgemm_small_fits(_spgemm_vcode(dtr), n_row, n_col):
        return None
    return _spgemm_small_run(_spgemm_operands(n_row, n_col, dtr, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr))


def _spgemm_rows(n_row, n_col, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr):
    """The row-local steps of `_spgemm` alone: (data, int64 indices, int64 indptr) of A @ B from the first of the small,
    bitmap and bucket kernels that delivers; None when the route is the global form's or every step declined (the caller
    then uses the global form throughout)."""
    return _spgemm(n_row, n_col, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr, row_local_only=True)[0]


def dot_csr_csr(out_shape, a_data, b_data, a_indices, b_indices, a_indptr, b_indptr):
    """CSR @ CSR -> (data, indices, indptr) with int64 indices — `_dot_csr_csr`
    (reference _common.py:639-717).  Explicit zeros are kept (the GCXS constructor prunes)."""
    n_row, n_col = int(out_shape[0]), int(out_shape[1])
    res, keys = _spgemm(n_row, n_col, a_data, a_indices, a_indptr, b_data, b_indices, b_indptr)
    if res is not None:
        return res
    indptr, indices = keys_to_csr(keys[0], n_row, n_col, torch.int64)
    return keys[1], indices, indptr


def dot_coo_coo(out_shape, a_coords, b_coords, a_data, b_data, n_inner):
    """COO @ COO -> (coords[2, nnz] int64, data), sorted — `_dot_coo_coo` + the indptr
    construction of reference _common.py:450-475,907-976.  `n_inner` = a.shape[1] = b.shape[0]."""
    n_row, n_col = int(out_shape[0]), int(out_shape[1])
    b_indptr = rows_to_indptr(b_coords[0], int(n_inner))
    res, keys = _spgemm(n_row, n_col, a_data, a_coords[1], None, b_data, b_coords[1], b_indptr, a_rows=a_coords[0])
    if res is not None:
        keys = csr_to_keys(res[2], res[1], n_row, n_col), res[0]
    return delinearize(keys[0], (n_row, n_col), torch.int64), keys[1]


SDDMM_PANEL_BYTES = 3 << 20     # Bt rows of one column panel: what stays in a 4 MiB L2 next to the streamed operands
SDDMM_PANEL_MIN_NNZ = 1 << 18   # below this the kernel is launch-bound either way
SDDMM_PANEL_GAIN = 0.75         # share of a gathered Bt row that the panel order saves (the rest: scattered output, streams)


class SddmmPanels:
    """Column-panel order of a mask, or of a subset of its stored elements (csrc/sddmm.hip, spamd_sddmm_panels):
    `pos` = the elements' positions in the mask, stably sorted by column panel; `rows`/`cols` = their coordinates in
    that order.  Depends on the coordinates and the panel width only: cached on the mask by `sparse_amd.sddmm`."""

    __slots__ = ("pos", "rows", "cols", "width", "count", "nnz", "chunk", "xstate", "xmax", "_vals", "_vals_key", "row_runs")

    def values(self, s_orig, s_data):
        """`s_data` (= `s_orig` in the accumulation dtype) in panel order; kept for as long as the same, unmodified
        `s_orig` is passed."""
        key = (s_orig.data_ptr(), s_orig._version, s_orig.dtype, s_data.dtype)
        if self._vals_key != key:
            self._vals, self._vals_key = gather(s_data, self.pos), key
        return self._vals


SDDMM_HALF_DTYPES = (torch.bfloat16, torch.float16)       # the 16-bit float operand types: fp32 accumulate, matrix-core tiles
SDDMM_DTYPES = SDDMM_HALF_DTYPES + (torch.float32, torch.float64)


def sddmm_code(dt):
    """C-ABI code of an SDDMM operand type: what `code_of` knows plus float16, which only the SDDMM kernels take.  Kept apart
    from `code_of` (and from `product_code`), whose TypeError for float16 is the "no device kernel for this dtype" probe of
    the other layers."""
    dt = dt if isinstance(dt, torch.dtype) else torch_dtype(dt)
    if dt not in SDDMM_DTYPES:
        raise TypeError(f"sddmm supports bfloat16/float16/float32/float64 dense operands, got {dt}")
    return _ffi.F16 if dt is torch.float16 else code_of(dt)


def sddmm_complex_code(dt):
    """C-ABI code of a complex SDDMM operand type (`spamd_sddmm_complex`): complex64 / complex128 and nothing else.  A lookup
    of its own, next to `product_code` and `sddmm_code`: `SDDMM_DTYPES` stays the list of the real kernels' types."""
    dt = dt if isinstance(dt, torch.dtype) else torch_dtype(dt)
    if dt not in _COMPLEX_CODE:
        raise TypeError(f"complex sddmm supports complex64/complex128 dense operands, got {dt}")
    return _COMPLEX_CODE[dt]


def sddmm_has_panels(dtype, Kd):
    """Does the column-panel order have a kernel for rows of `Kd` elements of `dtype` (spamd_sddmm_panels; for complex types
    the row-cached kernel of spamd_sddmm_complex)?"""
    try:
        dtype = dtype if isinstance(dtype, torch.dtype) else torch_dtype(dtype)
        if dtype in _COMPLEX_CODE:
            return bool(_ffi.lib().spamd_sddmm_complex_has_rowcache(_COMPLEX_CODE[dtype], int(Kd)))
        code = sddmm_code(dtype)
    except (TypeError, KeyError):
        return False
    return bool(_ffi.lib().spamd_sddmm_has_panels(code, int(Kd)))


SDDMM_PAD_MIN_NNZ = 200_000     # samples from which padding the inner dimension to a row-cached kernel's row length pays the two copies
_SDDMM_ROW_BYTES = (256, 512, 768, 1024, 1536, 2048, 3072, 4096)      # rows the row-cached / panel kernels are instantiated for


def sddmm_pad_inner(a, bt, nnz):
    """(a, bt) with the inner dimension zero-padded to the next row length the row-cached kernels have, when that is at most
    1.5x the rows' own length (round 6, tools/r06/sddmm_k_sweep.py: K = 96 or 100 in float32, 192 in bfloat16 - 384-byte rows -
    ran through the generic gather, 0.61 / 0.85 ms at config 4's mask, without a panel order; as 512-byte rows 0.38 / 0.33 ms
    plus two copies of ~0.03 ms).  Zeros add nothing to a dot product: the sums are those of the padded kernels' lane order,
    in the mask's own order and in panel order alike."""
    if a.dtype not in SDDMM_DTYPES or a.dim() != 2 or nnz < SDDMM_PAD_MIN_NNZ:
        return a, bt
    esz, k = a.element_size(), int(a.shape[1])
    if k == 0 or sddmm_has_panels(a.dtype, k):
        return a, bt
    rb = -(-k * esz // 16) * 16
    want = next((w for w in _SDDMM_ROW_BYTES if w >= rb), None)
    if want is None or want * 2 > rb * 3:
        return a, bt
    pad = want // esz - k
    return torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(bt, (0, pad))


def sddmm_panel_width(bt):
    """Bt rows per panel, or 0 when Bt fits the L2 as a whole or its K has no row-cached kernel (no panel order)."""
    row_bytes = int(bt.shape[1]) * bt.element_size()
    if row_bytes == 0 or int(bt.shape[0]) * row_bytes <= SDDMM_PANEL_BYTES:
        return 0
    if not sddmm_has_panels(bt.dtype, bt.shape[1]):
        return 0
    if SDDMM_TWO_PASS and not bt.is_complex():
        # rows of 1 KB run as two passes over 512-byte halves (round 5): a panel is sized for the half-rows
        row_bytes = int(_ffi.lib().spamd_sddmm_panel_row_bytes(sddmm_code(bt.dtype), int(bt.shape[1]))) or row_bytes
    if SDDMM_XCD_PANELS and int(bt.shape[0]) * row_bytes >= 8 * SDDMM_PANEL_BYTES:
        # XCD-private panels: a multiple of eight panels of at most 7/6 of the panel size (3.5 MiB), so that every XCD owns the same number
        # (measured at config 4: 16 panels of 6250 rows 0.357 ms private vs 0.390 shared; 17 panels of 6144 rows 0.402 vs 0.396)
        per_xcd = -(-int(bt.shape[0]) * row_bytes // (8 * (SDDMM_PANEL_BYTES * 7 // 6)))
        return max(-(-int(bt.shape[0]) // (8 * per_xcd)), 64)
    return max(SDDMM_PANEL_BYTES // row_bytes, 64)


def sddmm_panels_pay(n, a, bt, width):
    """Column-panel order or the mask's own order for `n` stored elements?  In the mask's order every element fetches
    its Bt row (K * itemsize bytes) through the fabric; in panel order the Bt rows come from the L2, but A is streamed
    once per panel and Bt once per XCD, whatever n is (measured at config 4's shapes: 10^7 elements 0.40 vs 0.70 ms,
    3 * 10^6 elements 0.33 vs 0.21 ms)."""
    if not width or n < SDDMM_PANEL_MIN_NNZ:
        return False
    row_bytes = int(bt.shape[1]) * bt.element_size()
    panels = -(-int(bt.shape[0]) // int(width))
    fixed = panels * int(a.shape[0]) * row_bytes + 8 * int(bt.shape[0]) * row_bytes
    return n * row_bytes * SDDMM_PANEL_GAIN > fixed


SDDMM_TILE_EQUIV = 410      # a 32 x 32 tile product costs what the sampled kernel spends on this many samples INSIDE a dense tile
SDDMM_REST_PENALTY = 2.5    # left-over samples per sample gained that the split may cost (they leave the panel order)


def sddmm_tiles_pay(plan, a, bt, width):
    """Dense tiles on the matrix cores + the rest sampled, or everything sampled?  Measured at K = 256 bf16
    (tools/sddmm_crossover.py, bench_paths A9_mfma_*): a tile product takes ~9 ns whatever the tile holds, the sampled
    kernel ~0.022 ns per sample inside a dense tile (A and Bt rows are shared), so the tiles gain
    n_dense - 410 * ntiles samples' worth of time; the left-over samples, run on their own, cost ~0.10 instead of
    ~0.045 ns each when the whole mask would have taken the panel order (both scale with the row length alike)."""
    ntiles = int(plan.tiles.numel())
    gain = plan.n_dense_samples - SDDMM_TILE_EQUIV * ntiles
    if ntiles == 0 or gain <= 0:
        return False
    nrest = int(plan.rest.numel())
    if sddmm_panels_pay(plan.nnz, a, bt, width) and not sddmm_panels_pay(nrest, a, bt, width):
        return gain > SDDMM_REST_PENALTY * nrest
    return True


SDDMM_TWO_PASS = True     # rows of exactly 1 KB in two launches over 512-byte halves and half-row panels (False: the row-cached kernel on whole rows, rounds 2-4)
SDDMM_XCD_PANELS = True   # panels are private to an XCD (workgroup b serves XCD b % 8: the placement MI355X is observed to use;
                          # only speed depends on it); False: every XCD walks every panel


def sddmm_panels(coords, shape, width, subset=None, xcd=None):
    """Panel order of the mask's stored elements, or of those listed in `subset` (int64 positions, ascending).  With `xcd`
    (default SDDMM_XCD_PANELS, and only when there are at least 8 panels) the order is XCD-major: panel p belongs to XCD
    p % 8, and `xstate` holds where each XCD's elements start."""
    dev = require_hip(coords)
    rows, cols = coords[0].contiguous(), coords[1].contiguous()
    if not index_dtype_ok(rows):
        rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    p = SddmmPanels()
    p.nnz = int(rows.numel())
    if subset is not None:
        rows, cols = gather(rows, subset), gather(cols, subset)
    n = int(rows.numel())
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    npanels = (int(shape[1]) - 1) // int(width) + 1
    xcd = SDDMM_XCD_PANELS if xcd is None else xcd
    per_xcd = -(-npanels // 8) if xcd and npanels >= 8 else 0
    _ffi.call("spamd_sddmm_panel_keys", code_of(cols.dtype), n, ptr(cols), int(width), per_xcd, ptr(keys), stream_ptr(dev))
    skeys, perm = sort_keys(keys, max(8 * per_xcd - 1 if per_xcd else npanels - 1, 1))
    p.pos = perm if subset is None else gather(subset, perm)
    p.rows, p.cols, p.width, p.count, p.chunk = gather(rows, perm), gather(cols, perm), int(width), n, 0
    p.xstate, p.xmax = None, 0
    # runs of equal rows in the panel order (one small read-back at plan time): 256 consecutive elements hold about
    # 256 * row_runs / count + 1 distinct A rows - what the panel kernel's LDS slots are sized for (`_sddmm_row_slots`)
    p.row_runs = int((p.rows[1:] != p.rows[:-1]).sum().item()) + 1 if n > 0 else 0
    if per_xcd:
        # first element of every (XCD, panel) key in the sorted order -> the nine boundaries of the XCDs' ranges
        first = rows_to_indptr(skeys, 8 * per_xcd)[::per_xcd].contiguous()
        host = first.cpu().numpy()                       # (plan time: one small read-back for the launch grid)
        p.xstate, p.xmax = first, int(np.max(np.diff(host)))
    p._vals = p._vals_key = None
    return p


def _sddmm_row_slots(panels, row_bytes, idx_bytes):
    """LDS slots for A rows per 256-element workgroup of the panel kernel (`chunk` of spamd_sddmm_panels): enough for the
    distinct rows such a workgroup meets - a row without a slot is fetched from memory and waited for on the spot - but not
    past three workgroups per CU.  (Round 6, tools/r06/sddmm_cap_sweep.py at config 4's mask: 768-byte rows, 61 distinct
    rows per workgroup: 32 slots - the kernel's own default, 24 KB - 0.82 ms, 52: 1.00, 64: 0.59, 72-96: 0.64, 128: 1.07;
    512-byte rows, 41 distinct: 44-72 slots 0.324, 80-96: 0.356; 256-byte rows, 21 distinct: 48-72 slots 0.172, 96 - the
    default - 0.199.)"""
    if panels.chunk or not panels.count or row_bytes >= 1024:
        return int(panels.chunk)
    expected = 256.0 * panels.row_runs / panels.count + 1.0
    default = max(16, (24 << 10) // row_bytes)                # (the kernel's own choice: 24 KB of rows, launch_panel)
    three = (160 * 1024 // 3 - 2048 - 1024 - 2 * 256 * idx_bytes - 16) // row_bytes    # (- 2 KB: LDS is handed out in blocks; 65 slots of 768 bytes already leave two workgroups per CU)
    if expected + 2 > default:                                 # rows without a slot would be the rule
        return max(16, min(int(1.3 * expected) + 8, three, 256))
    if default > 64 and 1.3 * expected + 8 <= 64:              # short rows: 64 slots instead of 96 (0.172 against 0.199 ms)
        return 64
    return 0


def _sddmm_panels_into(panels, s_orig, s_data, a, bt, out):
    """The elements of `panels` (all of the mask or a subset), written to their positions in `out`."""
    if a.is_complex():
        # the row-cached kernel in panel order for every row length it has: no half-row passes, no LDS slots
        _ffi.call("spamd_sddmm_complex", sddmm_complex_code(a.dtype), code_of(panels.rows.dtype), panels.count, ptr(panels.rows),
                  ptr(panels.cols), ptr(panels.values(s_orig, s_data)), ptr(a), a.stride(0), ptr(bt), bt.stride(0),
                  int(a.shape[1]), ptr(out), ptr(panels.pos), int(panels.chunk),
                  ptr(panels.xstate) if panels.xstate is not None else None, int(panels.xmax), stream_ptr(out.device))
        return
    part = None
    row_bytes = int(a.shape[1]) * a.element_size()
    if SDDMM_TWO_PASS and row_bytes == 1024:
        part = torch.empty(panels.count, dtype=out.dtype, device=out.device)     # (first-half sums, panel order)
        row_bytes = 512
    slots = _sddmm_row_slots(panels, row_bytes, panels.rows.element_size())
    _ffi.call("spamd_sddmm_panels", sddmm_code(a.dtype), code_of(out.dtype), code_of(panels.rows.dtype), panels.count,
              ptr(panels.rows), ptr(panels.cols), ptr(panels.pos), ptr(panels.values(s_orig, s_data)), ptr(a), a.stride(0),
              ptr(bt), bt.stride(0), int(a.shape[1]), slots, ptr(panels.xstate) if panels.xstate is not None else None,
              int(panels.xmax), ptr(part) if part is not None else None, ptr(out), stream_ptr(out.device))


def sddmm_coo(coords, s_data, a, bt, panels=None):
    """out[n] = s[n] * <a[i_n, :], bt[j_n, :]> for a 2-D COO mask — the sampled product the
    reference writes as `s * (a @ b)` (examples/sddmm_example.py:51-52).  `panels` (SddmmPanels of the same
    mask) selects the column-panel order."""
    dev = require_hip(coords, s_data, a, bt)
    nnz = int(s_data.numel())
    if a.dtype != bt.dtype:
        raise TypeError("a and bt must share a dtype")
    cplx = a.is_complex()
    in_code = sddmm_complex_code(a.dtype) if cplx else sddmm_code(a.dtype)       # (TypeError for any other operand type)
    if cplx:
        # mask values of any real or complex type become the operands' complex type on the device (spamd_cplx_convert)
        sdt = a.dtype
        s_orig, s_data = s_data, convert(s_data.contiguous(), sdt).contiguous()
    else:
        if s_data.is_complex():
            raise TypeError("complex mask values over real operands: multiply the unit-mask product by them (sparse_amd.sddmm does)")
        sdt = torch.float64 if a.dtype == torch.float64 else torch.float32
        s_orig, s_data = s_data, s_data.to(sdt).contiguous()
    a, bt = a.contiguous(), bt.contiguous()
    if a.shape[1] != bt.shape[1]:
        raise ValueError("shape-mismatch for sum")
    esz = a.element_size()
    if (a.shape[1] * esz) % 16:
        pad = (16 - (a.shape[1] * esz) % 16) // esz  # row pitch must be 16-byte aligned
        a = torch.nn.functional.pad(a, (0, pad))
        bt = torch.nn.functional.pad(bt, (0, pad))
    if a.data_ptr() % 16:      # the kernels load 16-byte vectors: a view at an odd storage offset is copied once
        a = a.clone()
    if bt.data_ptr() % 16:
        bt = bt.clone()
    rows, cols = coords[0].contiguous(), coords[1].contiguous()
    if not index_dtype_ok(rows):
        rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    out = torch.empty(nnz, dtype=sdt, device=dev)
    if panels is not None and nnz and panels.nnz == nnz and panels.count == nnz and sddmm_has_panels(a.dtype, a.shape[1]):
        _sddmm_panels_into(panels, s_orig, s_data, a, bt, out)
        return out
    if cplx:
        _ffi.call("spamd_sddmm_complex", in_code, code_of(rows.dtype), nnz, ptr(rows), ptr(cols), ptr(s_data), ptr(a), a.stride(0),
                  ptr(bt), bt.stride(0), int(a.shape[1]), ptr(out), None, 0, None, 0, stream_ptr(dev))
        return out
    _ffi.call("spamd_sddmm", in_code, code_of(sdt), code_of(rows.dtype), nnz, ptr(rows), ptr(cols),
              ptr(s_data), ptr(a), a.stride(0), ptr(bt), bt.stride(0), int(a.shape[1]), ptr(out), stream_ptr(dev))
    return out


SDDMM_TILE_THRESHOLD = 512     # samples per 32 x 32 mask tile from which the matrix-core tile product is clearly the cheaper one (tools/sddmm_crossover.py, profiles/r02_sddmm_crossover.txt: 1.5x at 512, 2.3x at 1024, break-even ~150 against the panel-order sampled kernel but ~400 against the sampled kernel on a dense tile)
SDDMM_MFMA_MIN_SHARE = 0.05    # (sddmm_coo_mfma without `force`) below this share of samples in dense tiles it declines


class SddmmPlan:
    """Per-mask dispatch between the matrix-core tile kernel and the sampled kernel (csrc/sddmm_mfma.hip):
    `tiles` = runs (in `seg_start`) of the tiles that take the MFMA path, `rest` = sample indices left to the sampled
    kernel.  Depends on the coordinates only: cached on the mask by `sparse_amd.sddmm`."""

    __slots__ = ("keys", "perm", "seg_start", "tiles", "rest", "tile_cols", "n_dense_samples", "nnz", "threshold")


def sddmm_plan(coords, shape, threshold=None):
    dev = require_hip(coords)
    threshold = SDDMM_TILE_THRESHOLD if threshold is None else int(threshold)
    rows, cols = coords[0].contiguous(), coords[1].contiguous()
    if not index_dtype_ok(rows):
        rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    nnz = int(rows.numel())
    ts = int(_ffi.lib().spamd_sddmm_tile_size())
    tile_rows, tile_cols = -(-int(shape[0]) // ts), -(-int(shape[1]) // ts)
    p = SddmmPlan()
    p.nnz, p.tile_cols, p.threshold = nnz, tile_cols, threshold
    s = stream_ptr(dev)
    keys = torch.empty(nnz, dtype=torch.int64, device=dev)
    _ffi.call("spamd_sddmm_tile_keys", code_of(rows.dtype), nnz, ptr(rows), ptr(cols), tile_cols, ptr(keys), s)
    p.keys, p.perm = sort_keys(keys, max(tile_rows * tile_cols - 1, 1))
    heads = flag_heads(p.keys)
    hoff = exclusive_scan(heads)
    nseg = int(hoff[-1])
    iota = torch.empty(nnz + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_iota", nnz + 1, ptr(iota), s)
    seg_start = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
    if nseg:
        _ffi.call("spamd_compact", 8, nnz, ptr(iota), ptr(heads), ptr(hoff), ptr(seg_start), s)
    seg_start[nseg:] = nnz   # (one 8-byte fill: the end of the last run)
    p.seg_start = seg_start
    tflag, sflag = new_flags(nseg, dev), new_flags(nnz, dev)
    _ffi.call("spamd_sddmm_tile_classify", nseg, ptr(seg_start), threshold, ptr(tflag), ptr(sflag), s)
    toff, soff = exclusive_scan(tflag), exclusive_scan(sflag)
    ntile, nrest = int(toff[-1]), int(soff[-1])
    p.tiles = compact(iota[:nseg].contiguous(), tflag, toff, ntile) if nseg else torch.empty(0, dtype=torch.int64, device=dev)
    p.rest = compact(p.perm, sflag, soff, nrest)
    p.n_dense_samples = nnz - nrest
    return p


def sddmm_coo_mfma(plan, coords, shape, s_data, a, bt, out=None, force=False, rest_panels=None):
    """SDDMM with per-tile dispatch (bf16 or float16 operands): dense tiles on the matrix cores, the rest through the sampled
    kernel (in column-panel order when `rest_panels` = sddmm_panels(..., subset=plan.rest) is given).  Returns None
    when the plan leaves (almost) everything to the sampled kernel and `force` is not set."""
    dev = require_hip(coords, s_data, a, bt)
    if a.dtype not in SDDMM_HALF_DTYPES or bt.dtype != a.dtype:
        raise TypeError("the matrix-core SDDMM path takes bfloat16 or float16 operands, both of one type")
    in_code = sddmm_code(a.dtype)
    Kd = int(a.shape[1])
    if Kd % 16 or Kd == 0:
        return None
    if not force and plan.n_dense_samples < SDDMM_MFMA_MIN_SHARE * plan.nnz:
        return None
    a, bt = a.contiguous(), bt.contiguous()
    if a.data_ptr() % 16 or bt.data_ptr() % 16:
        return None     # the tile kernel loads 16-byte operand fragments (a view at an odd storage offset): sampled kernel
    s_orig, s_data = s_data, s_data.to(torch.float32).contiguous()
    rows, cols = coords[0].contiguous(), coords[1].contiguous()
    if not index_dtype_ok(rows):
        rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    if out is None:
        out = torch.empty(plan.nnz, dtype=torch.float32, device=dev)
    s = stream_ptr(dev)
    _ffi.call("spamd_sddmm_mfma_tiles_typed", in_code, code_of(rows.dtype), int(plan.tiles.numel()), ptr(plan.tiles), ptr(plan.seg_start),
              ptr(plan.keys), ptr(plan.perm), plan.tile_cols, int(shape[0]), int(shape[1]), ptr(rows), ptr(cols), ptr(s_data),
              ptr(a), a.stride(0), ptr(bt), bt.stride(0), Kd, ptr(out), s)
    nrest = int(plan.rest.numel())
    if nrest and rest_panels is not None and rest_panels.count == nrest and rest_panels.nnz == plan.nnz and \
            sddmm_has_panels(a.dtype, Kd):
        _sddmm_panels_into(rest_panels, s_orig, s_data, a, bt, out)
    elif nrest:
        sub = torch.empty(nrest, dtype=torch.float32, device=dev)
        rr, cc, ss = gather(rows, plan.rest), gather(cols, plan.rest), gather(s_data, plan.rest)
        _ffi.call("spamd_sddmm", in_code, code_of(torch.float32), code_of(rr.dtype), nrest, ptr(rr), ptr(cc), ptr(ss),
                  ptr(a), a.stride(0), ptr(bt), bt.stride(0), Kd, ptr(sub), s)
        scatter_into(out, plan.rest, sub)
    return out


def sddmm_fold_strides(mask_lead, op_lead, what="a"):
    """Per-axis strides of an operand's batch ordinal under an N-D mask: `mask_lead` = the mask's leading shape, `op_lead` =
    the leading shape the operand HAS (right-aligned against it, NumPy's matmul rule - except that the mask's leading shape
    is the result's, so an operand axis must be 1 or the mask's size and the operand may not have more axes).  A broadcast
    axis has stride 0.  Returns (strides, number of batches of the operand)."""
    mask_lead, op_lead = tuple(int(d) for d in mask_lead), tuple(int(d) for d in op_lead)
    if len(op_lead) > len(mask_lead):
        raise ValueError(f"sddmm: `{what}` has more leading axes {op_lead} than the mask {mask_lead}")
    full = (1,) * (len(mask_lead) - len(op_lead)) + op_lead
    strides, run = [0] * len(full), 1
    for d in range(len(full) - 1, -1, -1):
        if full[d] != 1 and full[d] != mask_lead[d]:
            raise ValueError(f"sddmm: leading axes {op_lead} of `{what}` do not broadcast to the mask's {mask_lead}")
        if full[d] != 1:
            strides[d] = run
            run *= full[d]
    return strides, run


def sddmm_fold(coords, nlead, a_strides, b_strides, M, N, rows_total, cols_total):
    """[2, nnz] = (rows', cols') of an N-D mask's stored elements for the 2-D SDDMM kernels (csrc/sddmm_batch.hip): one launch,
    int32 when `rows_total` = Ba * M and `cols_total` = Bb * N fit, else int64."""
    dev = require_hip(coords)
    coords = coords.contiguous()
    if not index_dtype_ok(coords):
        coords = coords.to(torch.int64)
    nnz = int(coords.shape[1])
    odt = torch.int32 if max(int(rows_total), int(cols_total)) < 2 ** 31 else torch.int64
    out = torch.empty((2, nnz), dtype=odt, device=dev)       # [rows'; cols']: what the 2-D kernels take as `coords`
    if nnz == 0:
        return out
    arr = _ct.c_int64 * max(int(nlead), 1)
    _ffi.call("spamd_sddmm_batch_fold", code_of(coords.dtype), code_of(odt), int(nlead), nnz, ptr(coords), int(coords.stride(0)),
              arr(*[int(x) for x in a_strides]), arr(*[int(x) for x in b_strides]), int(M), int(N), ptr(out[0]), ptr(out[1]),
              stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------
# what the wrappers of the segment walkers share (DESIGN.md "The shared segment walk")
# ---------------------------------------------------------------------------------------------
def _seg_forms(what, form, chunk, short_max, longest, default_chunk, default_short_max, kind, name="form"):
    """(chunk, short_max) of a call with the forced `form` (None: the defaults; "long": pieces of 64 unless a chunk is given;
    "wide" and "long": no sub-groups), or the error of a form that cannot take the `longest` segment"""
    chunk = (64 if form == "long" else default_chunk) if chunk is None else int(chunk)
    short_max = (default_short_max if short_max is None else int(short_max)) if form in (None, "short") else 0
    if form == "short" and longest > 64 or form == "wide" and longest > chunk:
        raise ValueError(f"{what}: {name} {form!r} does not take a {kind} of {longest} elements")
    return chunk, short_max


def _seg_scale(scale, dt):
    """(has_scale, the scale rounded to the data type once) for the C entries"""
    return (0, 0.0) if scale is None else (1, float(np.asarray(scale).astype(np_dtype(dt))))


def _seg_workspace(entry, dev, *args):
    """(workspace or None, its size) as the C entry `entry` (a spamd_*_ws_bytes) sizes it"""
    ws_bytes = int(getattr(_ffi.lib(), entry)(*args))
    if ws_bytes < 0:
        raise _ffi.HipBackendError(f"{entry} failed: {ws_bytes}")
    return (torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None), ws_bytes


# ---------------------------------------------------------------------------------------------
# MTTKRP (csrc/mttkrp.hip)
# ---------------------------------------------------------------------------------------------
MTTKRP_MAX_NDIM = 8      # MTTKRP_MAX_NDIM of csrc/mttkrp.hip
# Elements of a row piece (a sub-group of lanes sums one piece sequentially; longer rows are cut and joined in piece order).
# A tuning constant of the Python side only: the kernel takes it as an argument.  Chosen with tools/mttkrp_time.py (MI355X,
# 10^6 stored elements, R = 32, float32, ms per call, median of 5 rounds of 20 calls, spread below 2 %):
#   chunk                     256     512     1024    2048    4096    8192
#   ONE row of 10^6           1.341   0.743   0.519   0.549   0.851   1.587     short pieces: the join's chain of piece sums
#   2000 rows of ~500         0.101   0.111   0.101   0.101   0.101   0.101     (only 256 cuts these rows at all)
# 1024 is the best of the sweep for the long row and costs the short rows nothing; the first guess, 2048, was 6 % behind.
MTTKRP_CHUNK = 1024


class MttkrpPlan:
    """The stored elements of a COO grouped by coords[mode]: `rowptr` (int64[shape[mode] + 1]) bounds each row's positions
    in plan order, `perm` (int64[nnz]) maps a plan position to a stored position - stable, i.e. ascending within a row -
    or is None when the stored order is the plan order (mode 0 of a canonical COO)."""

    __slots__ = ("mode", "perm", "rowptr")

    def __init__(self, mode, perm, rowptr):
        self.mode, self.perm, self.rowptr = mode, perm, rowptr


def mttkrp_plan(coords, shape, mode):
    """MttkrpPlan of `coords` ([ndim, nnz], canonical: sorted C-order, no duplicates) for `mode`."""
    require_hip(coords)
    nrows = int(shape[mode])
    if mode == 0:
        return MttkrpPlan(0, None, rows_to_indptr(coords[0], nrows))
    keys = coords[mode].to(torch.int64).contiguous()         # (memory plumbing: the sort takes int64 keys)
    skeys, perm = sort_keys(keys, max(nrows - 1, 0))          # stable: stored order within a row
    return MttkrpPlan(mode, perm, rows_to_indptr(skeys, nrows))


def mttkrp_coo(coords, data, shape, factors, mode, plan, *, chunk=None, exact=False):
    """out[i, r] = sum_{n: coords[mode][n] == i} data[n] * prod_{d != mode} factors[d][coords[d][n], r]  (spamd_mttkrp):
    `data` and the used `factors` (2-D device tensors, last axis contiguous) are float32 or all float64, `plan` an
    MttkrpPlan of the same coordinates and mode.  Returns the dense [shape[mode], R] device tensor."""
    ndim, nnz = int(coords.shape[0]), int(coords.shape[1])
    used = [factors[d] for d in range(ndim) if d != mode]
    dev = require_hip(coords, data, plan.rowptr, plan.perm, *used)
    dt = data.dtype
    if dt not in (torch.float32, torch.float64) or any(f.dtype != dt for f in used):
        raise TypeError("mttkrp: data and factors must all be float32 or all float64")
    R = int(used[0].shape[1])
    nrows = int(shape[mode])
    chunk = MTTKRP_CHUNK if chunk is None else int(chunk)
    out = torch.empty((nrows, R), dtype=dt, device=dev)
    coords = coords.contiguous()
    if not index_dtype_ok(coords):
        coords = coords.to(torch.int64)
    keep = []      # factors copied because their last axis is strided: alive until the launch is queued
    fptr, pitch = [0] * ndim, [0] * ndim
    for d in range(ndim):
        if d == mode:
            continue
        f = factors[d]
        if f.shape[1] > 1 and f.stride(1) != 1 or f.shape[0] > 1 and f.stride(0) < R:
            f = f.contiguous()
            keep.append(f)
        fptr[d], pitch[d] = ptr(f), max(int(f.stride(0)), R) if f.shape[0] > 1 else R
    ws, ws_bytes = _seg_workspace("spamd_mttkrp_ws_bytes", dev, code_of(dt), nnz, R, chunk)
    _ffi.call("spamd_mttkrp", code_of(dt), code_of(coords.dtype), ndim, int(mode), nnz, R, ptr(coords), int(coords.stride(0)) if nnz else 0,
              ptr(data.contiguous()), (_ct.c_void_p * ndim)(*fptr), _harr64(pitch), ptr(plan.perm), ptr(plan.rowptr), nrows, chunk,
              ptr(ws), ws_bytes, ptr(out), R, _ffi.EXACT_MULADD if exact else 0, stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------
# softmax over stored elements (csrc/softmax.hip)
# ---------------------------------------------------------------------------------------------
SOFTMAX_GROUPS = (8, 16, 32, 64)
SOFTMAX_MAX_CHUNK = 1024     # SOFTMAX_MAX_CHUNK of csrc/softmax.hip: a wave holds a group of that many elements in registers
SOFTMAX_FORMS = ("short", "wide", "long")
# SOFTMAX_CHUNK is part of the order contract for groups longer than it (pieces of that many elements, include/sparse_amd.h
# A14) and of no shorter group; SOFTMAX_SHORT_MAX (groups of at most that many elements go to a sub-group of lanes, longer
# ones to a whole wave) and SOFTMAX_GROUP (the sub-group's width) never change a bit.  Chosen with tools/softmax_time.py
# --sweep (MI355X, float32, ms per kernel call through this wrapper, median of 5 rounds of 20 calls, spread below 2 %), one
# parameter at a time: (a) CSR graph of 2^17 nodes, mean degree 32; (b) one hub row of 10^6 among 2^16 rows of 8; (c) COO
# batch 16 x 2048 x 2048, 32 per row:
#   group          8       16      32      64
#     (a)        0.0127  0.0143  0.0196  0.0303     fewer lanes per group = more values per lane and fewer shuffle steps
#     (b)        0.0964  0.0972  0.0998  0.1045
#     (c)        0.0084  0.0082  0.0083  0.0087
#   short_max      0       16      32      64       (0 = every group a whole wave)
#     (a)        0.0985  0.1077  0.0816  0.0192
#     (c)        0.0907  0.0938  0.0590  0.0087
#   chunk          64      128     256     512     1024
#     (b)        0.926   0.478   0.252   0.147   0.0997    short pieces: more windows to search, longer chains of piece sums
SOFTMAX_CHUNK = 1024
SOFTMAX_SHORT_MAX = 64
SOFTMAX_GROUP = 8


def softmax_segments(segptr, perm, data, max_len, *, scale=None, group=None, chunk=None, form=None, short_max=None):
    """softmax of every segment of `data` (spamd_softmax): `segptr` (int32 | int64 [nseg + 1], ascending from 0 to nnz) bounds
    the groups' positions in plan order, `perm` (int64[nnz] or None) maps a plan position to a stored position, `data` is
    float32 or float64, `max_len` the longest group's length.  Returns a new tensor in the stored order of `data`.
    `scale`: None or a real scalar (rounded to the data type once).  `form` forces a kernel form, for tests and sweeps:
    "short" (sub-groups of `group` lanes; every group has at most 64 elements), "wide" (a wave per group; at most `chunk`
    elements), "long" (a wave per group up to `chunk`, default 64 here, pieces beyond); `short_max` moves the length at which
    the default hands a group from a sub-group to a wave (sweeps)."""
    dev = require_hip(segptr, perm, data)
    dt = data.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError("softmax: data must be float32 or float64")
    if not index_dtype_ok(segptr) or (perm is not None and perm.dtype != torch.int64):
        raise TypeError("softmax: segptr must be int32 or int64 and perm int64")
    nnz, nseg, max_len = int(data.numel()), int(segptr.numel()) - 1, int(max_len)
    if form not in (None,) + SOFTMAX_FORMS:
        raise ValueError(f"softmax: form must be one of {SOFTMAX_FORMS} or None, got {form!r}")
    chunk, short_max = _seg_forms("softmax", form, chunk, short_max, max_len, SOFTMAX_CHUNK, SOFTMAX_SHORT_MAX, "group")
    group = SOFTMAX_GROUP if group is None else int(group)
    out = torch.empty_like(data, memory_format=torch.contiguous_format)
    ws, ws_bytes = _seg_workspace("spamd_softmax_ws_bytes", dev, code_of(dt), nnz, chunk) if max_len > chunk else (None, 0)
    _ffi.call("spamd_softmax", code_of(dt), code_of(segptr.dtype), nseg, nnz, ptr(segptr.contiguous()), ptr(perm),
              ptr(data.contiguous()), *_seg_scale(scale, dt), group, short_max, chunk, max_len, ptr(ws), ws_bytes, ptr(out),
              stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------
# sparse attention (csrc/attention.hip)
# ---------------------------------------------------------------------------------------------
ATTENTION_GROUPS = SOFTMAX_GROUPS
ATTENTION_FORMS = SOFTMAX_FORMS
# ATTENTION_CHUNK is part of the order contract for rows longer than it (include/sparse_amd.h A15: the pieces of the softmax
# sum and of the output) and of no shorter row: a multiple of 64, at most SOFTMAX_MAX_CHUNK.  ATTENTION_SHORT_MAX and
# ATTENTION_GROUP never change a bit.  Chosen with tools/attention_time.py --sweep (MI355X, float32, ms per kernel call through
# this wrapper, median of 5 rounds of 20 calls, spread below 1 %), one parameter at a time: (a) CSR graph of 2^17 nodes, mean
# degree 32, D = Dv = 64; (b) the same graph, 8 heads of D = Dv = 16; (c) one hub row of 10^6 among 2^16 rows of 8, D = Dv = 64:
#   group          8       16      32      64
#     (a)        0.300   0.284   0.305   0.514      16: four accumulators a lane at D = 64, four shuffle steps, four waves a SIMD
#     (b)        1.888   1.538   2.205   3.992
#   short_max      0       16      32      64       (0 = every row a whole wave)
#     (a)        1.351   1.358   1.036   0.284
#     (b)        4.693   4.716   3.775   1.539
#   chunk          64      128     256     512     1024
#     (c)        7.90    4.07    2.25    1.48    1.28
ATTENTION_CHUNK = SOFTMAX_CHUNK
ATTENTION_SHORT_MAX = 64
ATTENTION_GROUP = 16


def _rows3(t, dev):
    """(tensor [H, rows, width] whose last axis is contiguous, row pitch, head stride) of a dense operand [..., rows, width]: a
    view where the strides allow it, else one copy (a strided last axis, rows that overlap, leading axes that do not fold)"""
    rows, width = int(t.shape[-2]), int(t.shape[-1])
    H = 1
    for n in t.shape[:-2]:
        H *= int(n)
    if width > 1 and t.stride(-1) != 1 or rows > 1 and t.stride(-2) < width:
        t = t.contiguous()
    t3 = t.reshape(H, rows, width)             # (a view when the leading axes fold into one stride, else the one copy)
    if width > 1 and t3.stride(2) != 1 or rows > 1 and t3.stride(1) < width or H > 1 and t3.stride(0) < 0:
        t3 = t3.contiguous()
    pitch = int(t3.stride(1)) if rows > 1 else width
    head = int(t3.stride(0)) if H > 1 else 0
    return t3, pitch, head


def _bias2(bias, lead, H, nnz, dt, what):
    """(tensor, head stride in elements) of a bias in CSR order: [nnz] - shared, stride 0 - or lead + [nnz], viewed as (H, nnz)
    with its own head stride where the strides allow it (a slice of a wider tensor is not copied), else one copy"""
    if bias.dtype != dt:
        raise TypeError(f"{what}: the bias must have the type of the operands ({dt}), got {bias.dtype}")
    shape = tuple(int(n) for n in bias.shape)
    if shape == (nnz,):
        return bias.contiguous(), 0
    if shape != tuple(int(n) for n in lead) + (nnz,):
        raise ValueError(f"{what}: the bias must have the shape ({nnz},) or {tuple(lead) + (nnz,)}, got {shape}")
    b2 = bias.reshape(H, nnz)                    # (a view when the leading axes fold into one stride, else the one copy)
    if nnz > 1 and b2.stride(1) != 1 or H > 1 and b2.stride(0) < nnz:
        b2 = b2.contiguous()
    return b2, (int(b2.stride(0)) if H > 1 else 0)


def _dropout_args(dropout, seed, what):
    """(rate, the 64 bits of the seed as a signed integer) of a kernel-level dropout, or None for no dropout (None or 0: the
    seed is then ignored)"""
    if dropout is None or float(dropout) == 0.0:
        return None
    rate = float(dropout)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"{what}: the dropout must lie in [0, 1), got {dropout!r}")
    if seed is None:
        raise ValueError(f"{what}: a dropout above 0 needs a seed (there is no hidden generator)")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{what}: the seed must lie in [0, 2^64), got {seed}")
    return rate, seed - (1 << 64) if seed >= 1 << 63 else seed


def attention_keep(nnz, heads, dropout, seed, device, *, pos0=0, head0=0):
    """bool [heads, nnz]: the keep decisions of attention dropout for the stored (CSR) positions pos0 .. pos0 + nnz - 1 of the
    heads head0 .. head0 + heads - 1 (spamd_attention_keep: the device code the attention kernels call)"""
    nnz, heads = int(nnz), int(heads)
    out = torch.empty((heads, nnz), dtype=torch.uint8, device=device)
    require_hip(out)
    dz = _dropout_args(dropout, seed, "attention_keep")
    rate, sd = (0.0, 0) if dz is None else dz
    _ffi.call("spamd_attention_keep", nnz, heads, int(pos0), int(head0), rate, sd, ptr(out), stream_ptr(out.device))
    return out.view(torch.bool)


def attention_rows(indptr, indices, svals, q, k, v, max_len, *, scale=None, group=None, chunk=None, form=None, short_max=None,
                   bias=None, dropout=None, seed=None):
    """out[h] = softmax_over_stored(scale * (s * (q[h] @ k[h].T))) @ v[h] for the CSR mask (`svals`, `indices`, `indptr`: M + 1
    int32 | int64 pointers) (spamd_attention).  `q` [..., M, D], `k` [..., N, D], `v` [..., N, Dv] are device tensors of the
    type of `svals` (float32 or float64) with the same leading axes; `max_len` is the longest row's length.  Returns the
    dense [..., M, Dv] tensor.  `form` forces a kernel form, for tests and sweeps: "short" (sub-groups of `group` lanes; every
    row has at most 64 elements), "wide" (a wave per row; at most `chunk` elements), "long" (a wave per row up to `chunk`,
    default 64 here, pieces beyond); `short_max` moves the length at which a row goes from a sub-group to a wave (sweeps).
    `bias`: None, or a device tensor of that type in the order of `svals`, [nnz] (every head shares it) or [..., nnz], added to
    the scores after the scale (spamd_attention_bias).  `dropout`: None, or a rate in [0, 1) with a `seed` in [0, 2^64): the
    probabilities are dropped and rescaled by the counter-based decision of (seed, head, stored position)
    (spamd_attention_dropout); None or 0 reaches the entries without it."""
    dev = require_hip(indptr, indices, svals, q, k, v)
    dz = _dropout_args(dropout, seed, "attention")
    dt = svals.dtype
    if dt not in (torch.float32, torch.float64) or any(t.dtype != dt for t in (q, k, v)):
        raise TypeError("attention: the mask values, q, k and v must all be float32 or all float64")
    if not index_dtype_ok(indptr) or indices.dtype != indptr.dtype:
        raise TypeError("attention: indptr and indices must both be int32 or both int64")
    lead = tuple(q.shape[:-2])
    if tuple(k.shape[:-2]) != lead or tuple(v.shape[:-2]) != lead:
        raise ValueError("attention: q, k and v must have the same leading axes")
    M, D, N, Dv = int(q.shape[-2]), int(q.shape[-1]), int(k.shape[-2]), int(v.shape[-1])
    if int(k.shape[-1]) != D or int(v.shape[-2]) != N or int(indptr.numel()) != M + 1:
        raise ValueError("attention: shape mismatch between the mask, q, k and v")
    nnz, max_len = int(svals.numel()), int(max_len)
    if form not in (None,) + ATTENTION_FORMS:
        raise ValueError(f"attention: form must be one of {ATTENTION_FORMS} or None, got {form!r}")
    chunk, short_max = _seg_forms("attention", form, chunk, short_max, max_len, ATTENTION_CHUNK, ATTENTION_SHORT_MAX, "row")
    group = ATTENTION_GROUP if group is None else int(group)
    q3, qp, qh = _rows3(q, dev)
    k3, kp, kh = _rows3(k, dev)
    v3, vp, vh = _rows3(v, dev)
    H = int(q3.shape[0])
    out = torch.empty(lead + (M, Dv), dtype=dt, device=dev)
    ws, ws_bytes = _seg_workspace("spamd_attention_ws_bytes", dev, code_of(dt), nnz, H, Dv, chunk) if max_len > chunk else (None, 0)
    b2, bh = (None, 0)
    if bias is not None:
        require_hip(indptr, bias)
        b2, bh = _bias2(bias, lead, H, nnz, dt, "attention")      # (nnz == 0: no pointer, which the entry takes for no bias - rightly)
    # one argument list; the entry - plain, with a bias, with dropout - takes what it knows of the middle
    if dz is not None:
        entry, mods = "spamd_attention_dropout", (ptr(b2), bh, dz[0], dz[1], 0)
    elif bias is not None:
        entry, mods = "spamd_attention_bias", (ptr(b2), bh)
    else:
        entry, mods = "spamd_attention", ()
    _ffi.call(entry, code_of(dt), code_of(indptr.dtype), M, N, nnz, H, D, Dv, ptr(indptr.contiguous()), ptr(indices.contiguous()),
              ptr(svals.contiguous()), ptr(q3), qp, qh, ptr(k3), kp, kh, ptr(v3), vp, vh, *_seg_scale(scale, dt), group, short_max, chunk,
              max_len, *mods, ptr(ws), ws_bytes, ptr(out), stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------
# the backward pass of sparse attention (csrc/attention_grad.hip)
# ---------------------------------------------------------------------------------------------
# The chunk of the backward pass is part of its order contract for rows AND columns longer than it (include/sparse_amd.h A16) and
# must be the forward's for the probabilities to carry the forward's bits: it IS `ATTENTION_CHUNK` (`attention_grad_chunk`).  The
# widths and ATTENTION_GRAD_SHORT_MAX never change a bit.  Chosen with tools/attention_grad_time.py --sweep (MI355X, float32, ms
# per call of `attention_grad_rows`, median of 5 rounds of 20 calls, spread below 1 %), one parameter at a time around 16 / 16 /
# 64 / 1024: (a) CSR graph of 2^17 nodes, mean degree 32, D = Dv = 64; (b) the same graph, 8 heads of D = Dv = 16; (c) one hub row
# of 10^6 among 2^16 rows of 8, D = Dv = 64; (c') its transpose, one hub column:
#   group (row pass)   8       16      32      64
#     (a)            0.920   0.901   0.950   1.275     16 is the forward's width, and the narrowest that parks no scalar in a
#     (b)            5.180   5.128   6.066   8.634     vector lane (DESIGN A16, resource table)
#   col_group          8       16      32      64
#     (a)            0.914   0.900   0.890   0.879     the column pass only gathers: wider sub-groups hold fewer accumulators a
#     (b)            5.196   5.133   4.994   5.088     lane; 32 is the best at (b) and within 1.3 % of the best at (a)
#     (c)            2.292   2.295   2.379   2.611     (10^6 columns of one or two elements: reported only)
#   short_max          0       16      32      64      (0 = every row and column a whole wave)
#     (a)            2.784   2.808   2.192   0.901
#     (b)           12.566  12.622  10.110   5.131
#   chunk              64      128     256     512     1024
#     (c)            9.87    5.40    3.17    2.31    2.29
#     (c')          14.34    7.04    4.28    2.79    2.57
ATTENTION_GRAD_SHORT_MAX = 64
ATTENTION_GRAD_GROUP = 16
ATTENTION_GRAD_COL_GROUP = 32


def attention_grad_chunk():
    return ATTENTION_CHUNK


def attention_grad_rows(indptr, indices, svals, colptr, colperm, colrows, q, k, v, g, max_row, max_col, *, scale=None, group=None,
                        col_group=None, chunk=None, form=None, short_max=None, bias=None, want_dbias=False, dropout=None,
                        seed=None):
    """(dq, dk, dv) of `attention_rows` for the gradient `g` [..., M, Dv] of its result (spamd_attention_grad).  With a `bias`
    (as in `attention_rows`: spamd_attention_grad_bias) the probabilities are the biased forward's and the result is
    (dq, dk, dv, dbias): dbias [..., nnz] in the order of `svals`, always per head, or None unless `want_dbias`.  The mask and
    q, k, v are as there; `colptr` (N + 1, the type of `indptr`), `colperm` (int64[nnz]) and `colrows` (nnz, the type of
    `indptr`) are the column grouping: the stored positions of every column in stored order and their row ids; `max_row` and
    `max_col` the longest row and column.  `form` forces a kernel form on BOTH passes, for tests and sweeps: "short"
    (sub-groups of `group` / `col_group` lanes; at most 64 elements a row and a column), "wide" (a wave each; at most `chunk`),
    "long" (a wave up to `chunk`, default 64 here, pieces beyond); `short_max` moves the length at which a row or column goes
    from a sub-group to a wave (sweeps).  `dropout` and `seed` are those of `attention_rows`: the decisions are recomputed, so
    the backward drops what the forward dropped (spamd_attention_grad_dropout); None or 0 reaches the entries without it."""
    dev = require_hip(indptr, indices, svals, colptr, colperm, colrows, q, k, v, g)
    dz = _dropout_args(dropout, seed, "attention_grad")
    dt = svals.dtype
    if dt not in (torch.float32, torch.float64) or any(t.dtype != dt for t in (q, k, v, g)):
        raise TypeError("attention_grad: the mask values, q, k, v and g must all be float32 or all float64")
    if not index_dtype_ok(indptr) or any(t.dtype != indptr.dtype for t in (indices, colptr, colrows)) or colperm.dtype != torch.int64:
        raise TypeError("attention_grad: indptr, indices, colptr and colrows must all be int32 or all int64, colperm int64")
    lead = tuple(q.shape[:-2])
    if any(tuple(t.shape[:-2]) != lead for t in (k, v, g)):
        raise ValueError("attention_grad: q, k, v and g must have the same leading axes")
    M, D, N, Dv = int(q.shape[-2]), int(q.shape[-1]), int(k.shape[-2]), int(v.shape[-1])
    nnz, max_row, max_col = int(svals.numel()), int(max_row), int(max_col)
    if int(k.shape[-1]) != D or int(v.shape[-2]) != N or int(indptr.numel()) != M + 1 or tuple(g.shape[-2:]) != (M, Dv) \
            or int(colptr.numel()) != N + 1 or int(colperm.numel()) != nnz or int(colrows.numel()) != nnz:
        raise ValueError("attention_grad: shape mismatch between the mask, the column grouping, q, k, v and g")
    if form not in (None,) + ATTENTION_FORMS:
        raise ValueError(f"attention_grad: form must be one of {ATTENTION_FORMS} or None, got {form!r}")
    chunk, short_max = _seg_forms("attention_grad", form, chunk, short_max, max(max_row, max_col), attention_grad_chunk(),
                                  ATTENTION_GRAD_SHORT_MAX, "row or column")
    group = ATTENTION_GRAD_GROUP if group is None else int(group)
    col_group = ATTENTION_GRAD_COL_GROUP if col_group is None else int(col_group)
    q3, qp, qh = _rows3(q, dev)
    k3, kp, kh = _rows3(k, dev)
    v3, vp, vh = _rows3(v, dev)
    g3, gp, gh = _rows3(g, dev)
    H = int(q3.shape[0])
    dq = torch.empty(lead + (M, D), dtype=dt, device=dev)
    dk = torch.empty(lead + (N, D), dtype=dt, device=dev)
    dv = torch.empty(lead + (N, Dv), dtype=dt, device=dev)
    ws, ws_bytes = _seg_workspace("spamd_attention_grad_ws_bytes", dev, code_of(dt), nnz, H, D, Dv, chunk)
    b2, bh, dbias = None, 0, None
    if bias is not None:
        require_hip(indptr, bias)
        b2, bh = _bias2(bias, lead, H, nnz, dt, "attention_grad")
        # every element is written by the row pass, which the entry skips only when dq, dk and dv are all empty (D = Dv = 0: z = 0)
        if want_dbias:
            dbias = (torch.zeros if D == 0 and Dv == 0 else torch.empty)(lead + (nnz,), dtype=dt, device=dev)
    # one argument list; the entry - plain, with a bias, with dropout - takes what it knows of the middle
    if dz is not None:
        entry, mods = "spamd_attention_grad_dropout", (ptr(b2), bh, ptr(dbias), dz[0], dz[1], 0)
    elif bias is not None:
        entry, mods = "spamd_attention_grad_bias", (ptr(b2), bh, ptr(dbias))
    else:
        entry, mods = "spamd_attention_grad", ()
    _ffi.call(entry, code_of(dt), code_of(indptr.dtype), M, N, nnz, H, D, Dv, ptr(indptr.contiguous()), ptr(indices.contiguous()),
              ptr(svals.contiguous()), ptr(colptr.contiguous()), ptr(colperm.contiguous()), ptr(colrows.contiguous()), ptr(q3), qp, qh,
              ptr(k3), kp, kh, ptr(v3), vp, vh, ptr(g3), gp, gh, *_seg_scale(scale, dt), group, col_group, short_max, chunk, max_row,
              max_col, *mods, ptr(ws), ws_bytes, ptr(dq), ptr(dk), ptr(dv), stream_ptr(dev))
    return (dq, dk, dv) if bias is None else (dq, dk, dv, dbias)


# ---------------------------------------------------------------------------------------------
# semiring products sparse @ dense (csrc/semiring_spmm.hip)
# ---------------------------------------------------------------------------------------------
SEMIRING_ADDS = ("min", "max")
SEMIRING_MULS = ("plus", "times")
SEMIRING_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
SEMIRING_GROUPS = (8, 16, 32, 64)
SEMIRING_FORMS = ("rows", "lanes", "long")
SEMIRING_MAX_CHUNK = 1 << 30     # SR_MAX_CHUNK of csrc/semiring_spmm.hip
# None of these changes a bit of the result (include/sparse_amd.h A17: the rule is associative over any in-order split).
# SEMIRING_LANES_MAX_N: results of at most that many columns run the lanes ALONG the rows ("lanes"), wider ones give every lane
# 16 bytes of output columns ("rows").  SEMIRING_CHUNK: rows longer than it are cut into pieces ("long").  The sub-group width
# defaults to the narrowest that covers the result's columns with 16 bytes a lane ("rows") or that takes a mean row in one trip
# of four elements a lane ("lanes").  Chosen with tools/semiring_time.py --sweep (MI355X, float32, ms per call of this wrapper,
# median of 5 rounds of 20 calls, the alternatives taking turns in one process, min-max spread below 4 %), run with these
# defaults in place: (a) CSR graph of 2^17 nodes, mean degree 32, N = 64, max.times; (b) the same graph, N = 1, min.plus with an
# init; (c) one hub row of 10^6 among 2^16 rows of 8, N = 16, max.times:
#   group            8       16      32      64
#     (a) rows     0.2050  0.1665  0.2304  0.3732     16 lanes x 16 bytes = the 64 columns: the default's choice
#     (b) lanes    0.0259  0.0287  0.0423  0.0732     8 lanes x 4 elements = a mean row: the default's choice
#     (b) rows     0.0614  0.0948  0.1590  0.2735     (the other form at each size, for the record)
#     (a) lanes    0.5751  1.1970  2.2296  3.6593
#   N (graph of (a))   1       2       3       4       5       6       8       16      (each form at its default width)
#     rows           0.0629  0.0609  0.0616  0.0708  0.0651  0.0702  0.0842  0.0938
#     lanes          0.0261  0.0304  0.0395  0.0453  0.0570  0.0665  0.0858  0.1659
#       lanes lead by 2.4 x at 1 and still 1.56 x at 4, by 12 % at 5 and 5 % at 6, and lose from 8 on (7: not measured).  The cut-off
#       is 4: up to there the lead is large; the small one at 5 and 6 is that of one graph of one degree and one value type
#   chunk            64      256     512     1024    2048    4096    16384
#     (c)          1.5966  0.4367  0.2555  0.1809  0.1684  0.2384  0.7973    short pieces: more windows; long ones: too few waves
SEMIRING_LANES_MAX_N = 4
SEMIRING_CHUNK = 2048


def _semiring_group(narrow, N, itemsize, nnz, M):
    """the default sub-group width: "rows" - the narrowest whose lanes, 16 bytes of columns each, cover the N columns; "lanes" -
    the narrowest that takes a mean row in one trip of four elements a lane"""
    want = -(-nnz // max(4 * M, 1)) if narrow else -(-N * itemsize // 16)
    return next((g for g in SEMIRING_GROUPS if g >= want), 64)


def _pitched2(t):
    """(2-D tensor whose last axis is contiguous, row pitch in elements): a view where the strides allow it, else one copy"""
    rows, width = int(t.shape[0]), int(t.shape[1])
    if width > 1 and t.stride(1) != 1 or rows > 1 and t.stride(0) < width:
        t = t.contiguous()
    return t, (int(t.stride(0)) if rows > 1 else width)


def semiring_spmm(indptr, indices, vals, b, max_len, *, add, mul, init=None, return_arg=False, form=None, group=None, chunk=None):
    """out[i, j] = (min | max) over the stored (i, k) of vals[i, k] (+ | *) b[k, j] for the CSR matrix (`vals`, `indices`, `indptr`:
    M + 1 int32 | int64 pointers) (spamd_semiring_spmm).  `b` [K, N] or [K] is a device tensor of the type of `vals` (float32,
    float64, int32 or int64; any strides: a row pitch is passed through), `init` None or a tensor of the result's shape and
    type that every output starts from (it is only read), `max_len` the longest row's length.  Returns the dense [M, N] or [M]
    tensor; with `return_arg` (out, arg), arg int64: the k that was picked, -1 for the init or an empty row.
    `form` forces a kernel form, for tests and sweeps: "rows" (`group` lanes own a row, 16 bytes of columns a lane), "lanes"
    (`group` lanes run along a row, per output element) - both without pieces unless a `chunk` is given -, "long" (pieces of
    `chunk`, default 64 here, for the rows longer than it); `group` and `chunk` never change a bit."""
    if add not in SEMIRING_ADDS or mul not in SEMIRING_MULS:
        raise ValueError(f"semiring_spmm: add must be one of {SEMIRING_ADDS} and mul one of {SEMIRING_MULS} (the semirings min.plus, "
                         f"min.times, max.plus and max.times), got add={add!r}, mul={mul!r}")
    if form not in (None,) + SEMIRING_FORMS:
        raise ValueError(f"semiring_spmm: form must be one of {SEMIRING_FORMS} or None, got {form!r}")
    if group is not None and group not in SEMIRING_GROUPS:
        raise ValueError(f"semiring_spmm: group must be one of {SEMIRING_GROUPS} or None, got {group!r}")
    if chunk is not None and (int(chunk) != chunk or chunk < 64 or chunk > SEMIRING_MAX_CHUNK or chunk % 64):
        raise ValueError(f"semiring_spmm: chunk must be a multiple of 64 in 64 .. {SEMIRING_MAX_CHUNK} or None, got {chunk!r}")
    dt = b.dtype
    if dt not in SEMIRING_DTYPES or vals.dtype != dt or (init is not None and init.dtype != dt):
        raise TypeError("semiring_spmm: the values, b and the init must all be float32, float64, int32 or int64 - one type")
    if not index_dtype_ok(indptr) or indices.dtype != indptr.dtype:
        raise TypeError("semiring_spmm: indptr and indices must both be int32 or both int64")
    if b.ndim not in (1, 2):
        raise ValueError(f"semiring_spmm: b must have 1 or 2 dimensions, got {b.ndim}")
    M, K, nnz, max_len = int(indptr.numel()) - 1, int(b.shape[0]), int(vals.numel()), int(max_len)
    out_shape = (M,) if b.ndim == 1 else (M, int(b.shape[1]))
    if M < 0 or int(indices.numel()) != nnz or (nnz and K == 0):
        raise ValueError("semiring_spmm: shape mismatch between the CSR arrays and b")
    if init is not None and tuple(int(n) for n in init.shape) != out_shape:
        raise ValueError(f"semiring_spmm: the init must have the result's shape {out_shape}, got {tuple(init.shape)}")
    dev = require_hip(indptr, indices, vals, b, init)
    N = out_shape[1] if b.ndim == 2 else 1
    if M == 0 or N == 0 or nnz == 0:      # nothing to fold: the init, or the identity of the add - no launch
        if init is not None:
            out = init.clone(memory_format=torch.contiguous_format)
        else:
            lim = torch.finfo(dt) if dt.is_floating_point else torch.iinfo(dt)
            top = float("inf") if dt.is_floating_point else lim.max
            out = torch.full(out_shape, (top if add == "min" else (-top if dt.is_floating_point else lim.min)), dtype=dt, device=dev)
        return (out, torch.full(out_shape, -1, dtype=torch.int64, device=dev)) if return_arg else out
    narrow = N <= SEMIRING_LANES_MAX_N if form in (None, "long") else form == "lanes"
    chunk = (64 if form == "long" else SEMIRING_CHUNK if form is None else SEMIRING_MAX_CHUNK) if chunk is None else int(chunk)
    group = _semiring_group(narrow, N, b.element_size(), nnz, M) if group is None else int(group)
    b2, ldb = _pitched2(b if b.ndim == 2 else b.unsqueeze(1))
    i2, ldi = (None, N) if init is None else _pitched2(init if b.ndim == 2 else init.unsqueeze(1))
    out = torch.empty((M, N), dtype=dt, device=dev)
    arg = torch.empty((M, N), dtype=torch.int64, device=dev) if return_arg else None
    ws, ws_bytes = _seg_workspace("spamd_semiring_spmm_ws_bytes", dev, code_of(dt), nnz, N, chunk, int(return_arg)) if max_len > chunk else (None, 0)
    _ffi.call("spamd_semiring_spmm", code_of(dt), code_of(indptr.dtype), SEMIRING_ADDS.index(add), SEMIRING_MULS.index(mul), M, K, N,
              nnz, ptr(indptr.contiguous()), ptr(indices.contiguous()), ptr(vals.contiguous()), ptr(b2), ldb, ptr(i2), ldi,
              int(narrow), group, chunk, max_len, ptr(ws), ws_bytes, ptr(out), N, ptr(arg), N, stream_ptr(dev))
    out, arg = out.reshape(out_shape), (arg.reshape(out_shape) if return_arg else None)
    return (out, arg) if return_arg else out


# ---- the backward pass (csrc/semiring_grad.hip) ----
SEMIRING_GRAD_COL_FORMS = ("short", "wide", "long")
SEMIRING_GRAD_COL_GROUPS = (1,) + SEMIRING_GROUPS      # 1: a lane owns all outputs of a column (results of at most 4 columns)
SEMIRING_GRAD_LANE_MAX_N = 4                           # SG_LANE_MAX_N of csrc/semiring_grad.hip
# None of these changes a bit of da or dinit; db depends on `chunk` alone (include/sparse_amd.h A18: the piece rule is part of
# the order, as in A16).  Chosen with tools/semiring_grad_time.py --sweep (MI355X, float32, ms per call of this wrapper, median of
# 5 rounds of 20 calls, the alternatives taking turns in one process, min-max spread below 2 %; one parameter at a time, the
# others at A16's column defaults - col_group 32, short_max 64, chunk 1024 - and A17's width rule for the element pass): (a) CSR
# graph of 2^17 nodes, mean degree 32, N = 64, max.times; (b) the same graph, N = 1, min.plus with an init; (c) one hub COLUMN of
# 10^6 among 10^6 rows, N = 16, max.times:
#   group (element pass alone)      8       16      32      64
#     (a)                         0.1439  0.1920  0.3131  0.5463     8 lanes x 8 accumulators: the narrowest wins at every size,
#     (b)                         0.0748  0.1157  0.2144  0.4082     more elements in flight per wave
#     (c)                         0.0677  0.0880  0.1555  0.2822
#   col_group (column pass alone)   1       8       16      32      64
#     (a)                                 0.6038  0.4995  0.4993  0.5735     16 lanes x 16 bytes = the 64 columns
#     (b)                         0.0397  0.1185  0.1962  0.3444  0.6005     a lane per column: 3 x the narrowest sub-group
#     (c)                                 0.5556  0.5674  0.5834  0.6130     (the hub column's pieces dominate)
#   short_max (column pass alone)   0       8       16      32      64
#     (a)                         0.5869  0.5867  0.5915  0.5891  0.4994
#     (b)                         0.6026  0.6023  0.6065  0.3740  0.0398
#     (c)                         0.6085  0.5822  0.5830  0.5831  0.5831
#   chunk (column pass alone)       64      256     512     1024    2048    4096    16384
#     (c)                         4.954   1.390   0.795   0.583   0.669   1.116   4.118     short pieces: more windows; long: too few waves
# Shipped: group 8; col_group 1 for results of at most 4 columns, else the narrowest sub-group whose lanes, 16 bytes of columns
# each, cover the N columns (A17's rule for its rows form: 16 at (a), 8 at (c) - the fastest or within 0.1 % of it at both);
# short_max 64 and chunk 1024 (A16's).
SEMIRING_GRAD_GROUP = 8
SEMIRING_GRAD_SHORT_MAX = ATTENTION_GRAD_SHORT_MAX
SEMIRING_GRAD_CHUNK = 1024
SEMIRING_GRAD_STATS = {}      # the passes of the last call that reached the entry (tests): {"da", "db", "dinit"} -> bool


def _semiring_grad_col_group(N, itemsize):
    """the default width of the column pass: a lane per column for results of at most 4 columns, else A17's rule for the rows form"""
    return 1 if N <= SEMIRING_GRAD_LANE_MAX_N else _semiring_group(False, N, itemsize, 0, 1)


def semiring_grad(indptr, indices, vals, colptr, colperm, colrows, b, arg, g, max_col, *, mul, want=(True, True, False),
                  col_form=None, group=None, col_group=None, short_max=None, chunk=None):
    """(da, db, dinit) of `semiring_spmm` for the gradient `g` of its result and the forward's `arg` (spamd_semiring_grad): da
    [nnz] in the order of `vals`, db of the shape of `b`, dinit of the shape of `g`; `want` = (da?, db?, dinit?) - an output that
    is not wanted is None and its pass is not launched.  The CSR matrix, `b` and `mul` are those of `semiring_spmm` (float32 /
    float64 only); `arg` is int64, `arg` and `g` have the result's shape, any strides.  `colptr` (K + 1, the type of `indptr`),
    `colperm` (int64[nnz]) and `colrows` (nnz, the type of `indptr`) are the column grouping of `attention_grad_rows`, `max_col`
    the longest column; all four may be None when db is not wanted.  For "plus" `vals` is not read.
    `col_form` forces a form on the column pass, for tests and sweeps: "short" (sub-groups of `col_group` lanes; at most 64
    elements a column), "wide" (a wave each; at most `chunk`), "long" (a wave up to `chunk`, default 64 here, pieces beyond);
    `short_max` moves the length at which a column goes from a sub-group to a wave; `group` is the width of the element pass,
    `col_group` 1 gives a lane a whole column's outputs (N <= 4)."""
    if mul not in SEMIRING_MULS:
        raise ValueError(f"semiring_grad: mul must be one of {SEMIRING_MULS}, got {mul!r}")
    if col_form not in (None,) + SEMIRING_GRAD_COL_FORMS:
        raise ValueError(f"semiring_grad: col_form must be one of {SEMIRING_GRAD_COL_FORMS} or None, got {col_form!r}")
    if group is not None and group not in SEMIRING_GROUPS:
        raise ValueError(f"semiring_grad: group must be one of {SEMIRING_GROUPS} or None, got {group!r}")
    if col_group is not None and col_group not in SEMIRING_GRAD_COL_GROUPS:
        raise ValueError(f"semiring_grad: col_group must be one of {SEMIRING_GRAD_COL_GROUPS} or None, got {col_group!r}")
    if short_max is not None and (int(short_max) != short_max or short_max < 0 or short_max > 64):
        raise ValueError(f"semiring_grad: short_max must lie in 0 .. 64 or be None, got {short_max!r}")
    if chunk is not None and (int(chunk) != chunk or chunk < 64 or chunk > SEMIRING_MAX_CHUNK or chunk % 64):
        raise ValueError(f"semiring_grad: chunk must be a multiple of 64 in 64 .. {SEMIRING_MAX_CHUNK} or None, got {chunk!r}")
    want_da, want_db, want_di = (bool(w) for w in want)
    dt = b.dtype
    if dt in (torch.int32, torch.int64):
        raise TypeError("semiring_grad: min / max of integers has no gradient here - the values, b and g must be float32 or float64")
    if dt not in (torch.float32, torch.float64) or vals.dtype != dt or g.dtype != dt:
        raise TypeError("semiring_grad: the values, b and g must all be float32 or all float64 - one type")
    if arg.dtype != torch.int64:
        raise TypeError(f"semiring_grad: arg must be int64, got {arg.dtype}")
    if not index_dtype_ok(indptr) or indices.dtype != indptr.dtype:
        raise TypeError("semiring_grad: indptr and indices must both be int32 or both int64")
    if want_db and (colptr is None or colperm is None or colrows is None or colptr.dtype != indptr.dtype
                    or colrows.dtype != indptr.dtype or colperm.dtype != torch.int64):
        raise TypeError("semiring_grad: db needs the column grouping: colptr and colrows of the type of indptr, colperm int64")
    if b.ndim not in (1, 2):
        raise ValueError(f"semiring_grad: b must have 1 or 2 dimensions, got {b.ndim}")
    M, K, nnz = int(indptr.numel()) - 1, int(b.shape[0]), int(vals.numel())
    out_shape = (M,) if b.ndim == 1 else (M, int(b.shape[1]))
    N = out_shape[1] if b.ndim == 2 else 1
    if M < 0 or int(indices.numel()) != nnz or (nnz and K == 0):
        raise ValueError("semiring_grad: shape mismatch between the CSR arrays and b")
    if tuple(int(n) for n in arg.shape) != out_shape or tuple(int(n) for n in g.shape) != out_shape:
        raise ValueError(f"semiring_grad: arg and g must have the result's shape {out_shape}, got {tuple(arg.shape)} and {tuple(g.shape)}")
    if want_db and (int(colptr.numel()) != K + 1 or int(colperm.numel()) != nnz or int(colrows.numel()) != nnz):
        raise ValueError("semiring_grad: shape mismatch between the column grouping, the CSR arrays and b")
    max_col = int(max_col or 0)
    chunk, short_max = _seg_forms("semiring_grad", col_form, chunk, short_max, max_col if want_db else 0, SEMIRING_GRAD_CHUNK,
                                  SEMIRING_GRAD_SHORT_MAX, "column", name="col_form")
    if col_group is None:
        col_group = _semiring_grad_col_group(N, b.element_size())
    elif col_group == 1 and N > SEMIRING_GRAD_LANE_MAX_N:
        raise ValueError(f"semiring_grad: col_group 1 takes results of at most {SEMIRING_GRAD_LANE_MAX_N} columns, got {N}")
    group = SEMIRING_GRAD_GROUP if group is None else int(group)
    dev = require_hip(indptr, indices, vals, b, arg, g, *((colptr, colperm, colrows) if want_db else ()))
    SEMIRING_GRAD_STATS.clear()
    SEMIRING_GRAD_STATS.update(da=False, db=False, dinit=False)
    if M == 0 or N == 0 or nnz == 0 or K == 0:      # nothing is credited: no launch
        return (torch.zeros(nnz, dtype=dt, device=dev) if want_da else None,
                torch.zeros(tuple(b.shape), dtype=dt, device=dev) if want_db else None,
                g.clone(memory_format=torch.contiguous_format) if want_di else None)
    if not (want_da or want_db or want_di):
        return None, None, None
    times = mul == "times"
    b2, ldb = _pitched2(b if b.ndim == 2 else b.unsqueeze(1)) if times and want_da else (None, N)
    a2, lda = _pitched2(arg if b.ndim == 2 else arg.unsqueeze(1))
    g2, ldg = _pitched2(g if b.ndim == 2 else g.unsqueeze(1))
    da = torch.empty(nnz, dtype=dt, device=dev) if want_da else None
    db = torch.empty((K, N), dtype=dt, device=dev) if want_db else None
    di = torch.empty((M, N), dtype=dt, device=dev) if want_di else None
    ws, ws_bytes = _seg_workspace("spamd_semiring_grad_ws_bytes", dev, code_of(dt), nnz, N, chunk) if want_db and max_col > chunk else (None, 0)
    cp, cm, cr = (colptr.contiguous(), colperm.contiguous(), colrows.contiguous()) if want_db else (None, None, None)
    SEMIRING_GRAD_STATS.update(da=want_da, db=want_db, dinit=want_di)
    _ffi.call("spamd_semiring_grad", code_of(dt), code_of(indptr.dtype), SEMIRING_MULS.index(mul), M, K, N, nnz, ptr(indptr.contiguous()),
              ptr(indices.contiguous()), ptr(vals.contiguous()) if times and want_db else None, ptr(cp), ptr(cm), ptr(cr), ptr(b2), ldb,
              ptr(a2), lda, ptr(g2), ldg, group, col_group, short_max, chunk, max_col if want_db else 0, ptr(ws), ws_bytes, ptr(da),
              ptr(db), N, ptr(di), N, stream_ptr(dev))
    return da, (db.reshape(tuple(b.shape)) if want_db else None), (di.reshape(out_shape) if want_di else None)


# ---------------------------------------------------------------------------------------------
# masked SpGEMM (csrc/masked_spgemm.hip)
# ---------------------------------------------------------------------------------------------
MASKED_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
MASKED_GROUPS = (8, 16, 32, 64)
MASKED_MAX_CAP = 2048        # MSG_MAX_CAP of csrc/masked_spgemm.hip
# Tuning constants of the Python side only (the kernel takes them as arguments; none of them changes a bit of the result):
# MASKED_GROUP lanes walk one column of B together, a row of A of at most MASKED_CAP entries is searched in LDS (4 waves x
# cap x 4 or 8 bytes per workgroup), a wave owns MASKED_WINDOW consecutive mask elements.  Chosen with
# tools/masked_matmul_time.py --sweep (MI355X, symmetric graph of 2^17 nodes, mean degree 32, s = a = b, float32, 32-bit
# indices, ms per kernel call, median of 5 rounds of 20 calls, spread below 1 %), one parameter at a time around 16 / 256 / 256:
#   group    8: 0.687   16: 0.739   32: 0.906   64: 1.152
#   cap      1: 1.461   64 .. 512: 0.739   1024: 0.978   2048: 1.767      (1 = every search in global memory)
#   window  64: 0.921  128: 0.730  256: 0.739   512: 0.897  1024: 0.939  4096: 3.165
# and jointly group 8 | 16 x cap 64 | 128 | 256 x window 256 | 1024: cap makes no difference below 1024, window 1024 costs
# 26-27 %, group 8 is 7 % ahead of 16 on this graph (columns of ~32 entries); 16 is kept for longer columns (DESIGN A13, open).
MASKED_GROUP = 16
MASKED_CAP = 256
MASKED_WINDOW = 256


def masked_spgemm(shape, s_csr, a_csr, b_csc, *, group=None, cap=None, window=None, exact=False):
    """out[e] = m[e] * sum over common k of A[i, k] * B[k, j] at every stored position e = (i, j) of the mask, in the mask's
    CSR order (spamd_masked_spgemm; the order contract is in include/sparse_amd.h, A13).  `shape` = (M, N, K); `s_csr`,
    `a_csr`: (data, indices, indptr) compressed by rows, `b_csc`: the same compressed by columns (the CSR triplet of B^T);
    the three value arrays have one of MASKED_DTYPES.  Returns the values; the number of all-zero-bit results is left on
    them (`note_zero_bits_count`)."""
    M, N, Kd = (int(v) for v in shape)
    (s_val, s_idx, s_ptr), (a_val, a_idx, a_ptr), (b_val, b_idx, b_ptr) = s_csr, a_csr, b_csc
    dev = require_hip(s_val, s_idx, s_ptr, a_val, a_idx, a_ptr, b_val, b_idx, b_ptr)
    dt = s_val.dtype
    if dt not in MASKED_DTYPES or a_val.dtype != dt or b_val.dtype != dt:
        raise TypeError("masked_spgemm: the three value arrays must share one of float32, float64, int32, int64")
    group = MASKED_GROUP if group is None else int(group)
    cap = MASKED_CAP if cap is None else int(cap)
    window = MASKED_WINDOW if window is None else int(window)
    if group not in MASKED_GROUPS:
        raise ValueError(f"group must be one of {MASKED_GROUPS}, got {group}")
    if not 1 <= cap <= MASKED_MAX_CAP:
        raise ValueError(f"cap must be in 1 .. {MASKED_MAX_CAP}, got {cap}")
    if window < 1:
        raise ValueError(f"window must be positive, got {window}")
    if s_ptr.numel() != M + 1 or a_ptr.numel() != M + 1 or b_ptr.numel() != N + 1:
        raise ValueError("masked_spgemm: pointer arrays do not match the shapes")
    idx, it = _unify_index(*[t.contiguous() for t in (s_ptr, s_idx, a_ptr, a_idx, b_ptr, b_idx)])
    s_ptr, s_idx, a_ptr, a_idx, b_ptr, b_idx = idx
    nnz = int(s_idx.numel())
    out = torch.empty(nnz, dtype=dt, device=dev)
    zeros = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_masked_spgemm", code_of(dt), code_of(it), M, N, Kd, nnz, ptr(s_ptr), ptr(s_idx), ptr(s_val.contiguous()),
              ptr(a_ptr), ptr(a_idx), ptr(a_val.contiguous()), ptr(b_ptr), ptr(b_idx), ptr(b_val.contiguous()), group, cap, window,
              ptr(out), ptr(zeros), _ffi.EXACT_MULADD if exact else 0, stream_ptr(dev))
    note_zero_bits_count(out, zeros)
    return out


# ---------------------------------------------------------------------------------------------
# inspector/executor SpMM (csrc/spmm_tiled.hip)
# ---------------------------------------------------------------------------------------------
def tiled_params(dtype=torch.float32):
    """(rows per group, B rows per tile, groups per workgroup, entries per block, slack blocks, max tiles of the
    direct inspector, columns per panel) for float32 / float64 values."""
    v = [_ct.c_int(0) for _ in range(7)]
    _ffi.call("spamd_spmm_tiled_params", code_of(_tiled_layout_dtype(torch_dtype(dtype))), *[_ct.byref(x) for x in v])
    return tuple(x.value for x in v)


TILED_DTYPES = (torch.float32, torch.float64, torch.int32)


def _tiled_layout_dtype(dtype):
    """int32 values travel in the float32 layout (the inspector only moves value bits; the executor's int32 variant does
    the arithmetic: SPAMD_TILED_INT32)"""
    return torch.float32 if dtype == torch.int32 else dtype

_TOUCH_OVERRIDE = int(__import__("os").environ.get("SPARSE_AMD_TILED_TOUCH", "0"))   # tuning hook: lines prefetched per list


TILED_ONE_PASS_INSPECTOR = True   # False: the two-pass builder (count, scan, fill) - kept for cross-checks


class TiledLayout(tuple):
    """(blocks, blk_off, value dtype) + `mean_blocks` = mean 64-byte blocks per (row group, tile) list, which the
    launcher turns into the executor's prefetch width without reading anything back from the device, + `group_ends`:
    blk_off holds tiles + 1 entries per row group (the one-pass inspector's form) instead of one running array"""

    def __new__(cls, blocks, blk_off, dtype, mean_blocks, group_ends=False, pending=None, rowmap=None, groups=None):
        self = super().__new__(cls, (blocks, blk_off, dtype))
        self.mean_blocks = mean_blocks
        self.group_ends = group_ends
        self.pending = pending   # device word of a one-pass layout whose "unsorted column indices" verdict was not read yet
        self.rowmap = rowmap     # balanced layout (round 5): the row of every slot of every group, int32[groups * rows_per_group + 16]
        self.groups = groups
        return self


class UnsortedColumns(ValueError):
    """A one-pass tiled layout built with `defer_check=True` turned out to come from rows with unsorted column indices:
    the layout (and the product just computed from it) is invalid; rebuild with `force_sort=True`."""


def csr_tiled_layout(a_data, a_indices, a_indptr, M, Kd, force_sort=False, dtype=None, defer_check=False, balance=None):
    """Inspector: the K-tiled block stream of a CSR matrix used by `dot_csr_ndarray_tiled`, for float32 or float64
    values (`dtype`, default: a_data's if it is one of them, else float32).
    Returns (blocks int32[(total_blocks + slack) * 16], blk_off int32[nseg + 1], value dtype).
    Sorted column indices and a moderate K take the direct one-pass builder (count + fill in one launch, row groups
    independent of each other; the stream is then allocated for its upper bound, groups start at closed-form offsets
    with zeroed blocks between them, and blk_off is int32[groups * (tiles + 1)]: `TiledLayout.group_ends`);
    anything else the general key-sort recipe.  The one-pass builder reports unsorted column indices in a device word;
    with `defer_check` that word is not read here (no host wait between the inspector and the first product):
    `dot_csr_ndarray_tiled` reads it after enqueueing its first product and raises `UnsortedColumns`.
    `balance` (round 5, skewed row lengths): None = decide - with `defer_check` the test itself is deferred as well (the natural
    layout is built, the heaviest row group's size travels with the "unsorted" word and is read behind the first product,
    which then marks the layout `rebalance` for its owner: no host wait on the common, unskewed path), without it the
    statistics are read here; True = build the balanced layout if the operand is skewed at all, reading here; False = never."""
    dev = require_hip(a_data, a_indices, a_indptr)
    if dtype is None:
        dtype = a_data.dtype if a_data.dtype in TILED_DTYPES else torch.float32
    dtype = torch_dtype(dtype)
    vc = code_of(_tiled_layout_dtype(dtype))
    rg, kb, gpb, epb, slack, direct_max, _ = tiled_params(dtype)
    nnz = int(a_data.numel())
    ntiles = -(-Kd // kb)
    groups = -(-(-(-M // rg)) // gpb) * gpb
    nseg = groups * ntiles
    s = stream_ptr(dev)
    vals = a_data.to(dtype).contiguous()
    if dtype == torch.int32:
        vals = vals.view(torch.float32)
    if not index_dtype_ok(a_indices) or a_indices.dtype != a_indptr.dtype:
        a_indices, a_indptr = a_indices.to(torch.int64), a_indptr.to(torch.int64)

    def finish(blk_off, fill):
        total = int(blk_off[-1])
        if total >= 2 ** 31:
            raise ValueError("tiled SpMM layout: more than 2^31 blocks")
        blocks = torch.empty((total + slack) * 16, dtype=torch.int32, device=dev)
        fill(blk_off, total, blocks)
        return TiledLayout(blocks, convert(blk_off, torch.int32), dtype, total / max(nseg, 1))

    may_balance = (ntiles <= direct_max and not force_sort and TILED_ONE_PASS_INSPECTOR and TILED_BALANCE and balance is not False
                   and nnz >= TILED_BALANCE_MIN_NNZ and 0 < M < 2 ** 31)
    if may_balance and (balance or not defer_check):
        lay = _balanced_tiled_layout(vals, a_indices.contiguous(), a_indptr.contiguous(), M, Kd, dtype, nnz, defer_check, dev, s)
        if lay is not None:
            return lay
        may_balance = False      # (measured here: not skewed)
    if ntiles <= direct_max and not force_sort and TILED_ONE_PASS_INSPECTOR:
        # one pass over A (csrc/spmm_tiled.hip `tl_inspect_kernel`): count, fill and padding in a single launch with no
        # dependence between row groups (a group's first block is a closed-form upper bound from the row pointers); the
        # stream is allocated for its upper bound, so nothing waits for a total
        ic = code_of(a_indices.dtype)
        ind, ptr_ = a_indices.contiguous(), a_indptr.contiguous()
        upper = -(-nnz // epb) + nseg
        if upper < 2 ** 31:
            blocks = torch.empty((upper + slack) * 16, dtype=torch.int32, device=dev)
            blk_off = torch.empty(groups * (ntiles + 1), dtype=torch.int32, device=dev)
            state = torch.empty(9, dtype=torch.int64, device=dev)       # [0] unsorted columns; [1..8] = the skew statistics' eight words ([7] = heaviest natural group)
            _ffi.call("spamd_spmm_tiled_inspect", vc, ic, M, Kd, ptr(vals), ptr(ind), ptr(ptr_), ptr(state), ptr(blk_off),
                      ptr(blocks), s)
            if defer_check:
                lay = TiledLayout(blocks, blk_off, dtype, nnz / epb / max(nseg, 1) + 0.5, group_ends=True, pending=state)
                if may_balance:
                    # the skew test rides along: the heaviest natural group (one thread per group) lands in state[7]
                    _ffi.call("spamd_spmm_tiled_map_stats", ic, M, Kd, 32, ptr(ptr_), None, None, ptr(state) + 8, s)
                    lay.skew_mean = nnz * rg / max(M, 1)
                return lay
            if int(state[0]) == 0:      # (sorted column indices everywhere)
                return TiledLayout(blocks, blk_off, dtype, nnz / epb / max(nseg, 1) + 0.5, group_ends=True)
    elif ntiles <= direct_max and not force_sort:
        nblk = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        ic = code_of(a_indices.dtype)
        ind, ptr_ = a_indices.contiguous(), a_indptr.contiguous()
        _ffi.call("spamd_spmm_tiled_count", vc, ic, M, Kd, ptr(ind), ptr(ptr_), ptr(nblk), ptr(flags), s)
        blk_off = exclusive_scan(nblk)
        if int(flags[0]) == 0:
            return finish(blk_off, lambda bo, total, blocks: _ffi.call(
                "spamd_spmm_tiled_fill", vc, ic, M, Kd, ptr(vals), ptr(ind), ptr(ptr_), ptr(bo), total, ptr(blocks), s))
    rc = csr_to_keys(a_indptr, a_indices, M, Kd)
    tk = torch.empty_like(rc)
    _ffi.call("spamd_spmm_tiled_keys", nnz, ptr(rc), Kd, ptr(tk), s)
    del rc
    tk, vals = sort_key_value(tk, vals, max(nseg * rg * kb - 1, 1))
    seg_start = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
    nblk = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spmm_tiled_lists", vc, nnz, ptr(tk), M, Kd, ptr(seg_start), ptr(nblk), s)
    return finish(exclusive_scan(nblk), lambda bo, total, blocks: _ffi.call(
        "spamd_spmm_tiled_pack", vc, nnz, ptr(tk), ptr(vals), ptr(seg_start), ptr(bo), total, ptr(blocks), s))


TILED_BALANCE = True            # skewed row lengths: a balanced (row-mapped) layout instead of consecutive rows per wave
TILED_BALANCE_MIN_NNZ = 1 << 20
TILED_BALANCE_SKEW = 1.6        # natural layout kept while its heaviest row group holds at most this x the mean group
TILED_BALANCE_CAPMUL = 2        # cap = the power of two >= this x the mean 35-row group (rows above cap / 2 get a group of their own)
TILED_BALANCE_STATS = {}        # the last decision (tests, benches)


def _balanced_tiled_layout(vals, ind, ptr_, M, Kd, dtype, nnz, defer_check, dev, s):
    """The block stream of a SKEWED matrix (csrc/spmm_tiled.hip, `tl_map_*`): rows sorted by length, heavy rows given
    groups of their own (or shared by 2 / 4 / 8 / 16), a workgroup's 16 groups equally heavy, rows read and stored
    through a row map.  Returns None when the natural layout is balanced enough (its heaviest 35-row group at most
    TILED_BALANCE_SKEW x the mean: uniform `random` matrices measure ~1.1) - one small read-back decides.  Measured on a Zipf
    matrix of config 2's size (bench row A1_powerlaw): natural layout 3.5 ms per product, balanced see DESIGN.md."""
    rg, kb, gpb, epb, slack, direct_max, _ = tiled_params(dtype)
    ntiles = -(-Kd // kb)
    ic, vc = code_of(ind.dtype), code_of(_tiled_layout_dtype(dtype))
    mean_group = nnz * rg / max(M, 1)
    cap = 32
    while cap < TILED_BALANCE_CAPMUL * mean_group:
        cap *= 2
    stats = torch.empty(8, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spmm_tiled_map_stats", ic, M, Kd, cap, ptr(ptr_), None, None, ptr(stats), s)    # statistics only: 4-8 B per row
    st = stats.tolist()                                   # (the one read-back of the decision)
    skew = st[6] / max(mean_group, 1.0)
    TILED_BALANCE_STATS.update(cap=cap, class_rows=st[:6], natural_max_group=st[6], skew=skew, balanced=False)
    if skew <= TILED_BALANCE_SKEW:
        return None
    keys = torch.empty(M, dtype=torch.int64, device=dev)
    rows = torch.empty(M, dtype=torch.int32, device=dev)
    _ffi.call("spamd_spmm_tiled_map_stats", ic, M, Kd, cap, ptr(ptr_), ptr(keys), ptr(rows), ptr(stats), s)      # + the sort's keys and payload, rows per class
    st = stats.tolist()
    TILED_BALANCE_STATS.update(class_rows=st[:6])
    counts = _harr64(st[:6])
    groups = int(_ffi.lib().spamd_spmm_tiled_map_groups(counts))
    nseg = groups * ntiles
    upper = -(-nnz // epb) + nseg
    if groups <= 0 or upper >= 2 ** 31:
        return None
    keys, rows = sort_key_value(keys, rows, max(Kd, 1))  # longest rows first (stable): neighbours in a workgroup are equally long
    rowmap = torch.empty(groups * rg + 16, dtype=torch.int32, device=dev)
    gload = torch.empty(groups + 1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spmm_tiled_map_build", ic, M, cap, ptr(ptr_), ptr(rows), counts, ptr(rowmap), ptr(gload), s)
    vstart = exclusive_scan(gload)
    blocks = torch.empty((upper + slack) * 16, dtype=torch.int32, device=dev)
    blk_off = torch.empty(groups * (ntiles + 1), dtype=torch.int32, device=dev)
    state = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spmm_tiled_inspect_mapped", vc, ic, M, Kd, groups, ptr(vals), ptr(ind), ptr(ptr_), ptr(rowmap), ptr(vstart),
              ptr(state), ptr(blk_off), ptr(blocks), s)
    TILED_BALANCE_STATS.update(balanced=True, groups=groups)
    lay = TiledLayout(blocks, blk_off, dtype, nnz / epb / max(nseg, 1) + 0.5, group_ends=True, pending=state if defer_check else None,
                      rowmap=rowmap, groups=groups)
    if not defer_check and int(state[0]) != 0:
        return None          # unsorted column indices: the caller's key-sort recipe (natural layout)
    return lay


def csc_tiled_layout(a_data, a_indices, a_indptr, M, Kd, dtype=None):
    """The one-pass inspector for a CSC operand (`a_indices` = row indices, `a_indptr` = Kd + 1 column pointers): the same
    block stream as `csr_tiled_layout(..., defer_check=True)` of the CSR twin would give the executor, without building the
    twin (late round 4: the reference-default tall operand paid 4.3 ms of CSC -> CSR at config 2's size before its first
    product).  Returns None when the shape is outside the one-pass builder (more than `direct_max` tiles).  Rows that do
    not ascend inside a column are reported like unsorted columns are: the layout's `pending` word, read behind the first
    product (`UnsortedColumns`; the lists are then empty and the caller converts to CSR)."""
    dev = require_hip(a_data, a_indices, a_indptr)
    if dtype is None:
        dtype = a_data.dtype if a_data.dtype in TILED_DTYPES else torch.float32
    dtype = torch_dtype(dtype)
    rg, kb, gpb, epb, slack, direct_max, _ = tiled_params(dtype)
    nnz = int(a_data.numel())
    ntiles = -(-Kd // kb)
    groups = -(-(-(-M // rg)) // gpb) * gpb
    nseg = groups * ntiles
    upper = -(-nnz // epb) + nseg
    if ntiles > direct_max or upper >= 2 ** 31 or groups == 0 or not TILED_ONE_PASS_INSPECTOR:
        return None
    if not index_dtype_ok(a_indices) or a_indices.dtype != a_indptr.dtype:
        a_indices, a_indptr = a_indices.to(torch.int64), a_indptr.to(torch.int64)
    vals = a_data.to(dtype).contiguous()
    if dtype == torch.int32:
        vals = vals.view(torch.float32)
    blocks = torch.empty((upper + slack) * 16, dtype=torch.int32, device=dev)
    blk_off = torch.empty(groups * (ntiles + 1), dtype=torch.int32, device=dev)
    split = torch.empty(int(_ffi.lib().spamd_spmm_tiled_inspect_csc_ws(M, Kd)), dtype=torch.int32, device=dev)   # (workspace)
    state = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.call("spamd_spmm_tiled_inspect_csc", code_of(_tiled_layout_dtype(dtype)), code_of(a_indices.dtype), M, Kd, ptr(vals),
              ptr(a_indices.contiguous()), ptr(a_indptr.contiguous()), ptr(split), ptr(state), ptr(blk_off), ptr(blocks),
              stream_ptr(dev))
    return TiledLayout(blocks, blk_off, dtype, nnz / epb / max(nseg, 1) + 0.5, group_ends=True, pending=state)


def dot_csr_ndarray_tiled(layout, out_shape, Kd, b, out=None, exact=False):
    """Executor: C = A @ B from the tiled layout; `exact` = separate multiply and add (the reference's arithmetic) instead
    of one FMA per term.  B provides whole column panels (float32: 128 columns, float64: 64; `b.shape[1]` a multiple of
    that, zero-padded by the caller); `out_shape[1]` may be narrower than B (any width since late round 4): the last panel
    then stores its leading columns only - no padded result, no slice afterwards."""
    blocks, blk_off, dtype = layout
    M, N = int(out_shape[0]), int(b.shape[1])
    Nout = int(out_shape[1])
    panel = 64 if dtype == torch.float64 else 128
    if N % panel or not (N - panel < Nout <= N):
        raise ValueError(f"tiled executor: B has {N} columns (whole {panel}-column panels expected), result {Nout}")
    last_cols = (Nout - (N - panel)) % panel    # 0 = the whole last panel
    dev = require_hip(blocks, blk_off, b)
    if b.dtype != dtype:
        raise TypeError(f"tiled layout holds {dtype} values, B is {b.dtype}")
    b = b.contiguous()
    if out is None:
        out = torch.empty((M, Nout), dtype=dtype, device=dev)
    # prefetch hint: ~1.5 x the mean number of 64-byte blocks per (row group, tile) list
    lists = max(int(blk_off.numel()) - 1, 1)
    mean_blocks = getattr(layout, "mean_blocks", None) or (int(blocks.numel()) // 16) / lists
    hint = min(64, max(6, int(1.5 * mean_blocks) + 3))
    if _TOUCH_OVERRIDE:
        hint = _TOUCH_OVERRIDE
    ends = _ffi.TILED_GROUP_ENDS if getattr(layout, "group_ends", False) else 0
    ints = _ffi.TILED_INT32 if dtype == torch.int32 else 0
    flags = (_ffi.EXACT_MULADD if exact and not ints else 0) | ends | ints | (hint << 8) | (last_cols << 16)
    rowmap = getattr(layout, "rowmap", None)
    if rowmap is not None:
        _ffi.call("spamd_spmm_tiled_mapped", code_of(_tiled_layout_dtype(dtype)), M, int(layout.groups), Kd, N, ptr(blocks), ptr(blk_off),
                  ptr(rowmap), ptr(b), N, ptr(out), Nout, flags, stream_ptr(dev))
    else:
        _ffi.call("spamd_spmm_tiled", code_of(_tiled_layout_dtype(dtype)), M, Kd, N, ptr(blocks), ptr(blk_off), ptr(b), N, ptr(out), Nout,
                  flags, stream_ptr(dev))
    pending = getattr(layout, "pending", None)
    if pending is not None:   # first product of a layout built with defer_check: the verdict is read now, behind the launch
        layout.pending = None
        words = pending.tolist()
        mean = getattr(layout, "skew_mean", None)
        if mean and len(words) >= 8 and words[7] > TILED_BALANCE_SKEW * max(mean, 1.0):
            layout.rebalance = True       # (the product just enqueued is correct; the owner rebuilds a balanced layout for the next ones)
        if int(words[0]) != 0:
            raise UnsortedColumns("tiled layout built from rows with unsorted column indices")
    return out

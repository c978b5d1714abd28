"""Structural invariants of the result containers, checked on the host.

A dense image does not show the order of the stored elements, a duplicate whose partner holds a zero, a stale `_keys`, a wrong
row pointer or a wrong cached count - and those are what the next kernel trusts without looking (`COO._from_sorted_keys`,
`has_duplicates=False, sorted=True`, `GCXS((data, indices, indptr))`, `note_zero_bits_count`, the layouts of
`_dot.DERIVED_CACHES`).  Two layers:

* `check_coo_arrays` / `check_gcxs_arrays`: NumPy only, no device.  Each raises `AssertionError` whose message starts with the
  name of the violated rule (the `RULE_*` constants) and gives the first offending position.
* `assert_canonical(x, pruned=False)`: copies the buffers of a `COO` / `GCXS` to the host, calls the above and then checks the
  hidden state that is present (`_keys`, lazily derived coordinates, the zero-bit note on the value tensor, the derived layouts
  whose stamp is still current).  It leaves the container as it found it and returns how many containers it checked.
"""
import numpy as np

# ---- rule names (the first word of every message) ---------------------------------------------------------------------------
RULE_COO_LAYOUT = "coo.layout"                # coords is [ndim, nnz], data is [nnz]
RULE_COO_INDEX_DTYPE = "coo.index_dtype"      # int32 or int64, and the one asked for
RULE_COO_BOUNDS = "coo.bounds"                # 0 <= coords[d] < shape[d]
RULE_COO_ORDER = "coo.order"                  # C-order linear keys strictly increasing (sorted AND duplicate-free)
RULE_COO_KEYS_DTYPE = "coo.keys_dtype"        # cached keys are int64[nnz]
RULE_COO_KEYS = "coo.keys"                    # cached keys equal the host's keys
RULE_COO_LAZY_COORDS = "coo.lazy_coords"      # coordinates derived from the keys equal np.unravel_index of them
RULE_PRUNED = "pruned"                        # no stored value bit-identical to the fill value
RULE_GCXS_LAYOUT = "gcxs.layout"              # one pointer more than compressed rows; 1-D arrays store no pointers
RULE_GCXS_PTR_FIRST = "gcxs.indptr[0]"        # indptr[0] == 0
RULE_GCXS_PTR_MONOTONE = "gcxs.indptr_monotone"
RULE_GCXS_PTR_LAST = "gcxs.indptr[-1]"        # indptr[-1] == len(data) == len(indices)
RULE_GCXS_BOUNDS = "gcxs.index_bounds"        # 0 <= index < product of the uncompressed extents
RULE_GCXS_ROW_ORDER = "gcxs.row_order"        # indices strictly increasing inside every row
RULE_GCXS_WIDTH = "gcxs.index_width"          # the widths `_gcxs.unified_index_dtype` defines
RULE_ZERO_NOTE = "zero_bits_note"             # the count a producer left on the value tensor
RULE_DERIVED = "derived"                      # a cached layout whose stamp is still current


def _fail(rule, what, pos=None):
    raise AssertionError(f"{rule}: {what}" + ("" if pos is None else f" (first at position {pos})"))


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _prod(values):
    p = 1
    for v in values:
        p *= int(v)
    return p


def same_bits(a, b):
    """element-wise bit equality of two arrays of one dtype and shape (NaN payloads and the sign of zero count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def eq_bits(data, value):
    """boolean [n]: which elements of `data` are bit-identical to `value` (cast to data's dtype)"""
    data = np.ascontiguousarray(data)
    n, size = data.shape[0], data.dtype.itemsize
    pattern = np.frombuffer(np.asarray(value).astype(data.dtype).tobytes(), dtype=np.uint8)
    if n == 0:
        return np.zeros(0, dtype=bool)
    return (data.view(np.uint8).reshape(n, size) == pattern[None, :]).all(axis=1)


def host_keys(coords, shape):
    """C-order linear keys on the host: int64, or Python integers (an object array) where prod(shape) could pass 2^63"""
    coords = np.asarray(coords)
    nnz = coords.shape[1] if coords.ndim == 2 else 0
    wide = _prod(shape) >= 2 ** 63
    keys = np.zeros(nnz, dtype=object if wide else np.int64)
    for d, extent in enumerate(shape):
        keys = keys * int(extent) + (coords[d].astype(object) if wide else coords[d].astype(np.int64))
    return keys


def _check_pruned(data, fill_value):
    hit = eq_bits(data, fill_value)
    if hit.any():
        _fail(RULE_PRUNED, f"a stored value is bit-identical to the fill value {fill_value!r}", _first(hit))


def check_coo_arrays(coords, data, shape, fill_value, keys=None, index_dtype=None, pruned=False):
    coords, data = np.asarray(coords), np.asarray(data)
    shape = tuple(int(s) for s in shape)
    if data.ndim != 1:
        _fail(RULE_COO_LAYOUT, f"data has {data.ndim} dimensions")
    if coords.ndim != 2 or coords.shape != (len(shape), data.shape[0]):
        _fail(RULE_COO_LAYOUT, f"coords has shape {coords.shape}, expected {(len(shape), data.shape[0])}")
    if coords.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        _fail(RULE_COO_INDEX_DTYPE, f"coordinates are {coords.dtype}")
    if index_dtype is not None and coords.dtype != np.dtype(index_dtype):
        _fail(RULE_COO_INDEX_DTYPE, f"coordinates are {coords.dtype}, the container says {np.dtype(index_dtype)}")
    nnz = data.shape[0]
    for d, extent in enumerate(shape):
        bad = (coords[d] < 0) | (coords[d] >= extent)
        if bad.any():
            _fail(RULE_COO_BOUNDS, f"coordinate {int(coords[d][_first(bad)])} on axis {d} of extent {extent}", _first(bad))
    want = host_keys(coords, shape)
    if nnz > 1:
        bad = np.asarray(want[1:] <= want[:-1], dtype=bool)
        if bad.any():
            k = _first(bad)
            _fail(RULE_COO_ORDER, f"key {want[k + 1]} follows {want[k]}: " + ("duplicate" if want[k + 1] == want[k] else "unsorted"), k + 1)
    if keys is not None:
        keys = np.asarray(keys)
        if keys.dtype != np.dtype(np.int64) or keys.shape != (nnz,):
            _fail(RULE_COO_KEYS_DTYPE, f"cached keys are {keys.dtype}{list(keys.shape)}, expected int64[{nnz}]")
        bad = np.asarray(keys.astype(want.dtype) != want, dtype=bool)
        if bad.any():
            k = _first(bad)
            _fail(RULE_COO_KEYS, f"cached key {keys[k]}, the coordinates give {want[k]}", k)
    if pruned:
        _check_pruned(data, fill_value)


def _np_of_torch_dtype(t):
    import torch

    return np.dtype({torch.int32: np.int32, torch.int64: np.int64}[t])


def _torch_of_np_dtype(d):
    import torch

    return {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}.get(np.dtype(d))


def check_gcxs_arrays(data, indices, indptr, shape, compressed_axes, fill_value, pruned=False):
    from sparse_amd._gcxs import unified_index_dtype

    data, indices, indptr = np.asarray(data), np.asarray(indices), np.asarray(indptr)
    shape = tuple(int(s) for s in shape)
    if data.ndim != 1 or indices.ndim != 1 or indptr.ndim != 1:
        _fail(RULE_GCXS_LAYOUT, f"data / indices / indptr have {data.ndim} / {indices.ndim} / {indptr.ndim} dimensions")
    if compressed_axes is None:          # a 1-D array stores its coordinates in `indices` and no pointers
        if len(shape) != 1 or indptr.size:
            _fail(RULE_GCXS_LAYOUT, f"no compressed axes for shape {shape} with {indptr.size} pointers")
        rows, cols = 1, shape[0]
        ptr = np.array([0, indices.shape[0]], dtype=np.int64)
        if data.shape[0] != indices.shape[0]:
            _fail(RULE_GCXS_PTR_LAST, f"len(data) = {data.shape[0]}, len(indices) = {indices.shape[0]}")
    else:
        compressed_axes = tuple(int(c) for c in compressed_axes)
        rows = _prod(shape[c] for c in compressed_axes)
        cols = _prod(shape[d] for d in range(len(shape)) if d not in compressed_axes)
        if indptr.shape[0] != rows + 1:
            _fail(RULE_GCXS_LAYOUT, f"{indptr.shape[0]} pointers for {rows} compressed rows (expected {rows + 1})")
        ptr = indptr.astype(np.int64)
        if ptr[0] != 0:
            _fail(RULE_GCXS_PTR_FIRST, f"indptr[0] = {int(ptr[0])}", 0)
        bad = ptr[1:] < ptr[:-1]
        if bad.any():
            k = _first(bad)
            _fail(RULE_GCXS_PTR_MONOTONE, f"indptr[{k + 1}] = {int(ptr[k + 1])} < indptr[{k}] = {int(ptr[k])}", k + 1)
        if not int(ptr[-1]) == data.shape[0] == indices.shape[0]:
            _fail(RULE_GCXS_PTR_LAST, f"indptr[-1] = {int(ptr[-1])}, len(data) = {data.shape[0]}, len(indices) = {indices.shape[0]}")
    ti = _torch_of_np_dtype(indices.dtype)
    if ti is None:
        _fail(RULE_GCXS_WIDTH, f"indices are {indices.dtype}")
    want = _np_of_torch_dtype(unified_index_dtype(ti, int(data.shape[0])))
    if indices.dtype != want or (compressed_axes is not None and indptr.dtype != want):
        _fail(RULE_GCXS_WIDTH, f"indices {indices.dtype}, indptr {indptr.dtype}; one width, {want}, is expected")
    bad = (indices < 0) | (indices >= cols)
    if bad.any():
        _fail(RULE_GCXS_BOUNDS, f"index {int(indices[_first(bad)])} in a row of length {cols}", _first(bad))
    if indices.shape[0] > 1:
        bad = indices[1:] <= indices[:-1]
        starts = ptr[1:-1]                     # the first element of a row may be anything against the row before
        starts = starts[(starts > 0) & (starts < indices.shape[0])]
        bad[starts - 1] = False
        if bad.any():
            k = _first(bad)
            _fail(RULE_GCXS_ROW_ORDER, f"index {int(indices[k + 1])} follows {int(indices[k])} inside one row", k + 1)
    if pruned:
        _check_pruned(data, fill_value)


# ---- host forms used by the adapters -------------------------------------------------------------------------------------------
def gcxs_rows(indptr, n):
    """row number of every stored element of a compressed layout"""
    ptr = np.asarray(indptr).astype(np.int64)
    return np.repeat(np.arange(ptr.shape[0] - 1, dtype=np.int64), np.diff(ptr)) if ptr.size else np.zeros(n, dtype=np.int64)


def host_csr(rows, cols, data, n_rows):
    """(data, indices, indptr) in CSR order of elements given by rows / cols (any order, no duplicates)"""
    order = np.lexsort((cols, rows))
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=ptr[1:])
    return data[order], cols[order], ptr


def _npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _check_zero_note(data_t, data):
    note = getattr(data_t, "_zero_bits_count", None)
    if note is None or note[1] != data_t._version:
        return
    have = int(eq_bits(data, np.zeros((), dtype=data.dtype)).sum()) if data.size else 0
    if int(note[0]) != have:
        _fail(RULE_ZERO_NOTE, f"the value tensor carries a count of {int(note[0])} all-zero-bit elements, the host counts {have}")


def _check_triplet(what, got, want):
    gd, gi, gp = (_npy(t) for t in got)
    wd, wi, wp = want
    if not np.array_equal(gp.astype(np.int64), wp):
        _fail(RULE_DERIVED, f"{what}: row pointers differ", _first(gp.astype(np.int64) != wp) if gp.shape == wp.shape else None)
    if not np.array_equal(gi.astype(np.int64), wi):
        _fail(RULE_DERIVED, f"{what}: column indices differ", _first(gi.astype(np.int64) != wi) if gi.shape == wi.shape else None)
    if not same_bits(gd, wd):
        _fail(RULE_DERIVED, f"{what}: values differ")


def _check_tdot_views(x, coords, data):
    """each cached `tensordot` form against transpose(...).reshape(...) of the same elements; returns containers checked"""
    n = 0
    for (axes, vshape), v in (x.__dict__.get("_tdot_views") or {}).items():
        if v is not x:                            # (the identity permutation + the array's own shape gives the array itself)
            n += assert_canonical(v)
        tshape = tuple(x.shape[a] for a in axes)
        size = _prod(tshape)
        vshape = tuple(int(s) if s != -1 else size // max(1, _prod(t for t in vshape if t != -1)) for s in vshape)
        if tuple(v.shape) != vshape:
            _fail(RULE_DERIVED, f"_tdot_views[{axes}, {vshape}] has shape {tuple(v.shape)}")
        if size <= 1 << 22:
            dense = np.full(x.shape, x.fill_value, dtype=data.dtype)
            dense[tuple(coords)] = data
            if not same_bits(np.asarray(v.todense()), dense.transpose(axes).reshape(vshape)):
                _fail(RULE_DERIVED, f"_tdot_views[{axes}, {vshape}] is not transpose + reshape of the array")
        else:                                     # too large for a dense image: the same comparison on the stored elements
            keys = host_keys(coords[list(axes)], tshape)
            order = np.argsort(keys, kind="stable")
            vc = v.tocoo() if hasattr(v, "indptr") else v
            if not np.array_equal(host_keys(_npy(vc.coords), vshape), keys[order]) or not same_bits(_npy(vc.data), data[order]):
                _fail(RULE_DERIVED, f"_tdot_views[{axes}, {vshape}] is not transpose + reshape of the array")
    return n


def assert_canonical(x, pruned=False):
    """Check one `COO` / `GCXS` (see the module docstring); returns the number of containers checked (the array itself plus
    the cached 2-D forms it holds)."""
    from sparse_amd import COO, GCXS
    from sparse_amd import _dot

    assert isinstance(x, (COO, GCXS)), type(x)
    current = x.__dict__.get("_derived_stamp") == _dot._stamp(x)      # (read before anything below touches the container)
    shape = tuple(int(s) for s in x.shape)
    data = _npy(x.data)
    checked = 1
    if isinstance(x, COO):
        lazy = x.__dict__.get("_coords") is None
        keys_t = getattr(x, "_keys", None)
        if lazy and keys_t is None:
            _fail(RULE_COO_LAYOUT, "neither coordinates nor keys")
        keys = None if keys_t is None else _npy(keys_t)
        try:
            coords = _npy(x.coords)
        finally:
            if lazy:
                x.__dict__["_coords"] = None                          # leave the container as it was found
        if x.nnz != data.shape[0]:
            _fail(RULE_COO_LAYOUT, f"nnz = {x.nnz} with {data.shape[0]} values")
        if _torch_of_np_dtype(coords.dtype) is not None and _torch_of_np_dtype(coords.dtype) != x._index_dtype:
            _fail(RULE_COO_INDEX_DTYPE, f"coordinates are {coords.dtype}, the container says {x._index_dtype}")
        check_coo_arrays(coords, data, shape, x.fill_value, keys=keys, index_dtype=coords.dtype, pruned=pruned)
        if lazy and shape:
            want = np.stack(np.unravel_index(keys, shape)) if keys.size else np.zeros((len(shape), 0), dtype=np.int64)
            if not np.array_equal(coords.astype(np.int64), want):
                _fail(RULE_COO_LAZY_COORDS, "coordinates derived from the keys differ from np.unravel_index",
                      _first((coords.astype(np.int64) != want).any(axis=0)))
        _check_zero_note(x.data, data)
        if current:
            view = x.__dict__.get("_csr_view")
            if view is not None:
                if len(shape) != 2:
                    _fail(RULE_DERIVED, f"_csr_view on a {len(shape)}-D array")
                _check_triplet("_csr_view", view, host_csr(coords[0].astype(np.int64), coords[1].astype(np.int64), data, shape[0]))
            checked += _check_tdot_views(x, coords.astype(np.int64), data)
        return checked
    indices, indptr = _npy(x.indices), _npy(x.indptr)
    if len(shape) == 0:                          # a 0-d array: at most one stored element, no index structure
        if data.shape[0] > 1 or indptr.size:
            _fail(RULE_GCXS_LAYOUT, f"0-d array with {data.shape[0]} stored elements and {indptr.size} pointers")
        if pruned:
            _check_pruned(data, x.fill_value)
        return checked
    check_gcxs_arrays(data, indices, indptr, shape, x.compressed_axes, x.fill_value, pruned=pruned)
    _check_zero_note(x.data, data)
    if current:
        if len(shape) == 1:
            rows, (R, C) = np.zeros(data.shape[0], dtype=np.int64), (1, shape[0])
        else:
            rows, (R, C) = gcxs_rows(indptr, data.shape[0]), x._compressed_shape
        cols = indices.astype(np.int64)
        k2 = x.__dict__.get("_keys2d")
        if k2 is not None:
            if k2[0] is None:
                _fail(RULE_DERIVED, "_keys2d says the keys do not ascend strictly")
            got = _npy(k2[0])
            if got.dtype != np.int64 or not np.array_equal(got, rows * C + cols):
                _fail(RULE_DERIVED, "_keys2d differs from row * C + column")
        twin = x.__dict__.get("_csr_twin")
        if twin is not None:
            if len(shape) != 2 or x.compressed_axes != (1,):
                _fail(RULE_DERIVED, f"_csr_twin on compressed_axes {x.compressed_axes} of a {len(shape)}-D array")
            _check_triplet("_csr_twin", twin, host_csr(cols, rows, data, shape[0]))
        if x.__dict__.get("_tdot_views"):
            order = x._axis_order if len(shape) > 1 else [0]
            rc = np.stack(np.unravel_index(rows * C + cols, tuple(shape[a] for a in order))) if data.size else \
                np.zeros((len(shape), 0), dtype=np.int64)
            nat = np.empty_like(rc)
            nat[order] = rc
            checked += _check_tdot_views(x, nat, data)
    return checked

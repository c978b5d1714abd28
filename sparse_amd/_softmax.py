"""softmax over the stored elements of a sparse array as one fused kernel (csrc/softmax.hip): the step between the scores
`sddmm` gives at a mask's stored positions and the `matmul` that follows.  The container API cannot write it - `exp` of a
sparse array turns the fill value into 1, `x.max(axis=1)` counts the fill value 0 - and the reference has no function for it;
`torch.sparse.softmax` has the same meaning."""
from numbers import Real

import numpy as np
import torch

from . import _kernels as K
from ._coo import COO
from ._gcxs import GCXS
from ._utils import normalize_axis


class SoftmaxPlan:
    """The stored elements grouped for one axis tuple: `segptr` (int32 | int64 [nseg + 1]) bounds each non-empty group's
    positions in plan order (for a 2-D GCXS over its uncompressed axis it is `indptr` itself, empty rows included), `perm`
    (int64[nnz]) maps a plan position to a stored position - stable, i.e. stored order within a group - or is None when
    the stored order is the plan order.  `max_len`: the longest group."""

    __slots__ = ("segptr", "perm", "max_len")

    def __init__(self, segptr, perm, max_len):
        self.segptr, self.perm, self.max_len = segptr, perm, max_len


def _max_len(segptr):
    return int((segptr[1:] - segptr[:-1]).max()) if segptr.numel() > 1 else 0


def _own_width(x, segptr):
    """the segment pointers at the array's own index width, as every other entry point takes its index arrays"""
    width = x._index_dtype if isinstance(x, COO) else x.indices.dtype
    return segptr.to(torch.int32) if width == torch.int32 and x.nnz < 2 ** 31 else segptr


def _build_plan(x, axis):
    kept = tuple(a for a in range(x.ndim) if a not in axis)
    dev, nnz = x.device, x.nnz
    if isinstance(x, GCXS) and x.ndim >= 2 and kept == tuple(x.compressed_axes):
        # the kept axes are the compressed ones: a compressed row (a column of a CSC) is a group as it is stored
        return SoftmaxPlan(x.indptr, None, _max_len(x.indptr))
    order = kept + axis
    n_cols = 1
    for a in axis:
        n_cols *= x.shape[a]
    perm = None
    if not kept:                                                         # one group: the keys say nothing
        return SoftmaxPlan(_own_width(x, torch.tensor([0, nnz], dtype=torch.int64, device=dev)), None, nnz)
    if isinstance(x, COO):       # (from the coordinates when they exist: they are what the stamp watches)
        keys = x.linear_loc() if x.__dict__.get("_coords") is None else K.linearize(x.coords, x.shape)
    else:
        from ._convert import gcxs_natural_keys

        keys = gcxs_natural_keys(x)                                      # in storage order, whatever the layout
    from ._reduce import _scalar_dev
    from ._umath import binary_arrays

    # the group of every stored element: its key with the kept axes leading, without the digits of the normalised axes
    gk = binary_arrays("floor_divide_i64", K.permute_keys(keys, x.shape, order), _scalar_dev(n_cols, torch.int64, dev),
                       b_scalar=True)
    if K.keys_check(gk)[0]:      # (a canonical COO over its trailing axes, a GCXS over its uncompressed ones: grouped already)
        gk, perm = K.sort_keys(gk, max(x.size // max(n_cols, 1) - 1, 1))     # stable: stored order within a group
    heads = K.flag_heads(gk)
    offs = K.exclusive_scan(heads)
    count = int(offs[-1])
    iota = torch.empty(nnz, dtype=torch.int64, device=dev)
    K._ffi.call("spamd_iota", nnz, K.ptr(iota), K.stream_ptr(dev))
    segptr = torch.cat([K.compact(iota, heads, offs, count), _scalar_dev(nnz, torch.int64, dev)])   # non-empty groups only
    return SoftmaxPlan(_own_width(x, segptr), perm, _max_len(segptr))


def _like(x, data):
    """a container with the stored structure of `x` and the values `data`; the index buffers are shared, as by `x * 2`"""
    fill = np.dtype(K.np_dtype(data.dtype)).type(0)
    if isinstance(x, GCXS):
        return GCXS((data, x.indices, x.indptr), shape=x.shape, compressed_axes=x.compressed_axes, fill_value=fill)
    out = COO._from_sorted_keys(x._keys, data, x.shape, fill, x._index_dtype)
    out.__dict__["_coords"] = x.__dict__.get("_coords")
    return out


def _coord_stamp(x):
    """identity + version of the index buffers alone (`_dot._stamp` without the values), by name; a COO's coordinates count
    only once they exist (they are split off its keys on first use, which changes no grouping)"""
    bufs = {"indices": x.indices, "indptr": x.indptr} if isinstance(x, GCXS) else \
        {"coords": x.__dict__.get("_coords"), "keys": getattr(x, "_keys", None)}
    return {k: (t.data_ptr(), int(t.numel()), int(t._version)) for k, t in bufs.items() if t is not None}


def _stamp_holds(old, new):
    """every buffer the plans were built under is still the same; a buffer that did not exist then says nothing"""
    return all(new.get(k) == v for k, v in old.items())


def _check_arguments(dtype, ndim, axis, scale):
    """the checks that need no array: value type, axes and scale; returns the sorted tuple of normalised axes"""
    if ndim < 1:
        raise ValueError("softmax needs an array of at least 1 dimension")
    kind, size = np.dtype(dtype).kind, np.dtype(dtype).itemsize
    if kind == "c" or (kind == "f" and size not in (4, 8)) or kind not in "fiub":
        raise TypeError(f"softmax: values of type {np.dtype(dtype)} are not supported (complex and 16-bit values are not; "
                        "float32, float64, integer and boolean are)")
    if scale is not None and (not isinstance(scale, (Real, np.integer, np.floating)) or isinstance(scale, (bool, np.bool_))):
        raise TypeError("softmax: scale must be None or a real scalar")
    axis = normalize_axis(axis, ndim)
    if axis is None:
        raise ValueError("axis None not understood: name the axes to normalise over")
    axis = tuple(sorted(axis)) if isinstance(axis, tuple) else (axis,)
    if len(set(axis)) != len(axis):
        raise ValueError(f"repeated axis in {axis}")
    if not axis:
        raise ValueError("softmax needs at least one axis")
    return axis


def softmax(x, axis=-1, *, scale=None):
    """softmax of `scale * x` over `axis`, taken over the STORED elements: an unstored position counts as minus infinity
    and stays unstored.  The result equals `scipy.special.softmax` of the dense array with -inf at every unstored position,
    read back at the stored positions (the meaning of `torch.sparse.softmax`).

    `x`: a COO or GCXS of at least one dimension with a zero fill value; float32 or float64 values, integer and boolean
    values are converted to float64 on the device; complex and 16-bit values raise TypeError.  `axis`: an int or a tuple of
    ints (negative values count from the end); the normalisation runs over those axes jointly, once per index of the
    remaining axes (a group).  `scale`: None or a real scalar; `t = scale * x` is one multiplication in the result type, and
    the maximum is taken of `t` (a negative scale is legal).

    Returns an array of the container type, shape, index width, compressed axes and exact stored structure of `x` - the
    same coordinates in the same order, so it lines up element for element with the mask it came from.  Stored zeros take
    part as the value 0, results that underflow to 0 stay stored, the fill value stays 0, a group without stored elements
    stays empty (it is not NaN).  A group that holds a NaN or a +inf is NaN throughout, and so is a group whose every
    element is -inf; a -inf beside finite values gives +0.0.

    The order of every operation is fixed (include/sparse_amd.h, A14; groups longer than `_kernels.SOFTMAX_CHUNK` are summed
    in pieces of that many elements): the same bits on every call, no atomics.  The grouping of the stored elements is
    built once per axis tuple and kept on the array."""
    from ._utils import check_zero_fill_value

    if not isinstance(x, (COO, GCXS)):
        raise TypeError(f"softmax needs a COO or GCXS array, got {type(x).__name__}")
    axis = _check_arguments(x.dtype, x.ndim, axis, scale)
    check_zero_fill_value(x)
    dt = torch.float32 if x.dtype == np.float32 else torch.float64
    data = K.convert(x.data, dt)
    if isinstance(x, COO):
        x.linear_loc()           # (the keys exist from here on: the stamp below and the result share them)
    if x.nnz == 0 or x.size == 0:
        return _like(x, data.clone() if data is x.data else data)
    # Two things drop the plans.  Their own stamp, over the index buffers alone: the grouping depends on nothing else, so
    # `x.data *= 2` followed by another softmax reuses them.  And `_dot.drop_derived`, because the name is in
    # `_dot.DERIVED_CACHES`: a replaced buffer forgets them with the MTTKRP plans - and so does any OTHER operation that
    # validates the array's derived layouts after a write to the values (`matmul`, `sddmm`, `mttkrp`: their stamp covers the
    # values).  That costs one rebuild and never a wrong result.
    stamp = _coord_stamp(x)
    plans = x.__dict__.get("_softmax_plan")
    if plans is None or not _stamp_holds(plans["stamp"], stamp):
        plans = x.__dict__["_softmax_plan"] = {"stamp": stamp}
    else:
        plans["stamp"].update(stamp)
    plan = plans.get(axis)
    if plan is None:
        plan = plans[axis] = _build_plan(x, axis)
    return _like(x, K.softmax_segments(plan.segptr, plan.perm, data, plan.max_len, scale=scale))

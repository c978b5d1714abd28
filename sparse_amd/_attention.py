"""Sparse attention as one fused kernel (csrc/attention.hip): the scores `sddmm` gives at a mask's stored positions, the
`softmax` over them and the `matmul` by `v`, for one or many heads over one shared 2-D mask - graph attention, sparse
transformers, neighbourhood attention.  The three-call expression

    matmul(softmax(sddmm(s, q, bt=k), scale=c), v)

writes the scores once and reads them three times, builds its plans on two arrays and cannot share a mask between heads."""
import numpy as np
import torch

from . import _device as dev
from . import _kernels as K
from ._coo import COO
from ._gcxs import GCXS

_OPERAND_DTYPES = (torch.float32, torch.float64)
_NP_OPERAND = {np.dtype("float32"): torch.float32, np.dtype("float64"): torch.float64}


def _check_operands(s_shape, q, k, v):
    """the checks of q, k and v that need no device: kinds, types, head axes and shapes; returns (torch dtype, leading axes)"""
    dts = []
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, (np.ndarray, torch.Tensor)):
            raise TypeError(f"sparse_attention: `{name}` must be a NumPy array or a torch tensor, got {type(t).__name__}")
        if t.ndim < 2:
            raise ValueError(f"sparse_attention: `{name}` needs at least 2 dimensions, got {t.ndim}")
        dts.append(t.dtype if isinstance(t, torch.Tensor) else _NP_OPERAND.get(t.dtype, t.dtype))
    if len(set(dts)) != 1 or dts[0] not in _OPERAND_DTYPES:
        raise TypeError("sparse_attention: q, k and v must be all float32 or all float64 (mixed, 16-bit and complex operands "
                        f"are not supported), got {[str(t) for t in dts]}")
    lead = tuple(int(n) for n in q.shape[:-2])
    if tuple(int(n) for n in k.shape[:-2]) != lead or tuple(int(n) for n in v.shape[:-2]) != lead:
        raise ValueError(f"sparse_attention: the leading (head) axes of q, k and v must be identical (no broadcasting), got "
                         f"{tuple(q.shape[:-2])}, {tuple(k.shape[:-2])}, {tuple(v.shape[:-2])}")
    M, N = int(s_shape[0]), int(s_shape[1])
    D = int(q.shape[-1])
    if int(q.shape[-2]) != M or int(k.shape[-2]) != N or int(v.shape[-2]) != N or int(k.shape[-1]) != D:
        raise ValueError(f"shape-mismatch for sparse_attention: s {tuple(s_shape)}, q {tuple(q.shape)}, k {tuple(k.shape)}, "
                         f"v {tuple(v.shape)}; expected (M, N), (..., M, D), (..., N, D), (..., N, Dv)")
    return dts[0], lead


def _csr_of_mask(s):
    """(data, indices, indptr) the kernel reads: a row-compressed GCXS's own arrays untouched, else the memoised CSR form"""
    from ._dot import _csr_triplet

    if isinstance(s, GCXS) and s.compressed_axes == (0,):
        return s.data, s.indices, s.indptr
    return _csr_triplet(s)


def _longest_row(s, indptr):
    """the longest row's length: state of the pattern alone, kept on the array under a stamp of its index buffers (as
    `_softmax_plan`); it only picks the kernel forms"""
    from ._softmax import _coord_stamp, _max_len, _stamp_holds

    stamp = _coord_stamp(s)
    plan = s.__dict__.get("_attention_plan")
    if plan is None or not _stamp_holds(plan["stamp"], stamp) or plan["indptr"] is not indptr:
        plan = s.__dict__["_attention_plan"] = {"stamp": stamp, "indptr": indptr, "max_len": _max_len(indptr)}
    else:
        plan["stamp"].update(stamp)
    return plan["max_len"]


def sparse_attention(s, q, k, v, *, scale=None):
    """`softmax_over_stored(scale * (s * (q @ k.T))) @ v` for every head, in one fused kernel.

    `s`: a 2-D COO or GCXS (either compressed axis) of shape (M, N) with a zero fill value; float32, float64, integer or
    boolean values, converted to the result type on the device; complex and 16-bit values raise TypeError.  `q` (..., M, D),
    `k` (..., N, D), `v` (..., N, Dv): NumPy arrays or torch tensors (any strides), all float32 or all float64 - the result
    type.  The leading axes are the heads: absent, or identical on all three (no broadcasting); every head uses the same
    mask.  `scale`: None or a real scalar, rounded to the result type once.

    Returns the dense (..., M, Dv) result: a torch device tensor if any of q, k, v was a torch tensor, else an ndarray.  An
    unstored position of `s` counts as minus infinity; a row without stored elements gives a row of +0.0, not NaN.  Stored
    zeros of `s`, and scores that come out 0, take part as the value 0 - UNLIKE `matmul(softmax(sddmm(s, q, bt=k),
    scale=scale), v)`, where `sddmm` prunes every score of +0.0 and the softmax then counts it as minus infinity.  A row
    whose scores hold a NaN or +inf, or only -inf, is NaN throughout its output row.

    The order of every operation is fixed (include/sparse_amd.h, A15; rows longer than `_kernels.ATTENTION_CHUNK` are summed in
    pieces of that many elements): the same bits on every call, no atomics, and the probabilities carry the bits `softmax`
    gives for the same scores.  The kernel reads the mask's CSR form - a row-compressed GCXS's own arrays, else the form the
    array memoises for its products, so a second call converts nothing."""
    from ._softmax import _check_arguments
    from ._utils import check_zero_fill_value

    if not isinstance(s, (COO, GCXS)):
        raise TypeError(f"sparse_attention needs a COO or GCXS mask, got {type(s).__name__}")
    if s.ndim != 2:
        raise ValueError(f"sparse_attention needs a 2-D mask, `s` has {s.ndim} dimensions (every head shares one 2-D mask)")
    _check_arguments(s.dtype, 2, -1, scale)
    check_zero_fill_value(s)
    dt, lead = _check_operands(s.shape, q, k, v)
    torch_out = any(isinstance(t, torch.Tensor) for t in (q, k, v))
    M, Dv = int(s.shape[0]), int(v.shape[-1])
    if s.nnz == 0 or M == 0 or Dv == 0 or 0 in lead:
        out = torch.zeros(lead + (M, Dv), dtype=dt, device=s.device)
        return out if torch_out else dev.to_numpy(out)
    data, indices, indptr = _csr_of_mask(s)
    max_len = _longest_row(s, indptr)
    dq, dk, dv = (dev.to_device(t, s.device) for t in (q, k, v))
    out = K.attention_rows(indptr, indices, K.convert(data, dt), dq, dk, dv, max_len, scale=scale)
    return out if torch_out else dev.to_numpy(out)

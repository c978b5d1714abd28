"""Semiring products sparse @ dense whose "add" is min or max (csrc/semiring_spmm.hip): max / min neighbourhood aggregation with
its arg-max (GraphSAGE pooling, PNA, EdgeConv), and the tropical products - one Bellman-Ford relaxation is `min.plus`, Viterbi
`max.plus`, most-reliable path `max.times`.  Every other product of the library aggregates with a sum; the broadcasting
expression `(a[:, :, None] + b[None]).min(axis=1)` counts an unstored position as the value 0 instead of as absent, and the
torch expression `scatter_reduce(..., "amin")` over the materialised (nnz, N) products writes and re-reads them and gives no arg."""
import numpy as np
import torch

from . import _device as dev
from . import _kernels as K
from ._coo import COO
from ._gcxs import GCXS

_NP_RESULT = {np.dtype("float32"): torch.float32, np.dtype("float64"): torch.float64, np.dtype("int32"): torch.int32,
              np.dtype("int64"): torch.int64}
_SEMIRINGS = "min.plus, min.times, max.plus and max.times"


def _dense_dtype(t):
    return t.dtype if isinstance(t, torch.Tensor) else _NP_RESULT.get(t.dtype, t.dtype)


def _check_sparse(a):
    """the checks of `a` that need no device: container, dimensions and fill value"""
    from ._utils import check_zero_fill_value

    if not isinstance(a, (COO, GCXS)):
        raise TypeError(f"semiring_matmul needs a COO or GCXS array on the left, got {type(a).__name__}")
    if a.ndim != 2:
        raise ValueError(f"semiring_matmul needs a 2-D sparse array, `a` has {a.ndim} dimensions")
    check_zero_fill_value(a)


def _check_arguments(a_shape, a_dtype, b, add, mul, init):
    """the checks that need no device: the semiring, the kinds, types and shapes of `b` and `init`; returns the torch result type"""
    if add not in K.SEMIRING_ADDS or mul not in K.SEMIRING_MULS:
        raise ValueError(f"semiring_matmul: add must be one of {K.SEMIRING_ADDS} and mul one of {K.SEMIRING_MULS} - the semirings "
                         f"{_SEMIRINGS} -, got add={add!r}, mul={mul!r}")
    for name, t in (("b", b),) + ((("init", init),) if init is not None else ()):
        if not isinstance(t, (np.ndarray, torch.Tensor)):
            raise TypeError(f"semiring_matmul: `{name}` must be a NumPy array or a torch tensor, got {type(t).__name__}")
    dt = _dense_dtype(b)
    if dt not in K.SEMIRING_DTYPES:
        raise TypeError(f"semiring_matmul: `b` must be float32, float64, int32 or int64 - its type is the result type -, got {dt} "
                        "(complex and 16-bit values are not supported)")
    adt, bdt = np.dtype(a_dtype), K.np_dtype(dt)
    if adt.kind == "c" or (adt.kind == "f" and adt.itemsize < 4) or not (adt.kind == "b" or np.can_cast(adt, bdt, "same_kind")):
        raise TypeError(f"semiring_matmul: the values of `a` ({adt}) cannot be converted to the type of `b` ({bdt}): complex and 16-bit "
                        "values are not supported, and float values do not go into an integer `b`")
    if b.ndim not in (1, 2):
        raise ValueError(f"semiring_matmul: `b` must have 1 or 2 dimensions (K,) or (K, N), got {b.ndim} (batched operands are not supported)")
    M, Kd = int(a_shape[0]), int(a_shape[1])
    if int(b.shape[0]) != Kd:
        raise ValueError(f"shape-mismatch for semiring_matmul: a {tuple(a_shape)}, b {tuple(b.shape)}; expected (M, K) and (K, N) or (K,)")
    out_shape = (M,) + tuple(int(n) for n in b.shape[1:])
    if init is not None:
        if _dense_dtype(init) != dt:
            raise TypeError(f"semiring_matmul: `init` must have the type of `b` ({dt}; it is not converted), got {_dense_dtype(init)}")
        if tuple(int(n) for n in init.shape) != out_shape:
            raise ValueError(f"shape-mismatch for semiring_matmul: `init` {tuple(init.shape)} is not the shape of the result {out_shape}")
    return dt


def semiring_matmul(a, b, *, add="min", mul="plus", init=None, return_arg=False):
    """`out[i, j] = add over the STORED (i, k) of  a[i, k] mul b[k, j]`, in one fused kernel: `add` is "min" or "max", `mul` is
    "plus" or "times".  An unstored position of `a` is absent - it does not count as the value 0 -, a stored zero takes part
    as the value 0.

    `a`: a 2-D COO or GCXS (either compressed axis) of shape (M, K) with a zero fill value.  `b`: a NumPy array or torch
    tensor of shape (K, N) or (K,), any strides; its type is the result type: float32, float64, int32 or int64.  The values of
    `a` are converted to it on the device when `np.can_cast(a.dtype, b.dtype, "same_kind")` holds (boolean values always);
    complex or 16-bit values, or float values into an integer `b`, raise TypeError.  `init`: None, or a dense array or tensor of
    the result's shape and type: the value every output starts from (GraphBLAS `accum`; `init=d` fuses the outer `min(d, ...)`
    of a Bellman-Ford step).  It is not modified.

    Returns the dense (M, N) or (M,) result - an ndarray if `b` (and `init`, if given) are ndarrays, else a device tensor; with
    `return_arg=True`, `(out, arg)`, `arg` int64 of the shape of `out`.

    For output (i, j) of a "min" semiring ("max" mirrored), with row i's stored elements e = 0 .. n - 1 in CSR stored order and
    `t_e = a[i, k_e] + b[k_e, j]` (or `*`; one operation, integers wrap): the result is the element `np.argmin` picks in the
    sequence `[init[i, j]]` (if given) `+ [t_0 .. t_{n-1}]` - the first NaN if there is one, else the first element that attains
    the minimum; -0.0 and +0.0 compare equal, so the first of them wins and keeps its sign.  `out` is its value, `arg` its
    `k_e`, or -1 when the init was picked.  A row without stored elements gives `init[i, j]`, or without an init the identity of
    `add` (+inf / -inf, the integer type's max / min), with arg -1.

    The rule is associative over any in-order split, so the result does not depend on the kernel form or the launch geometry
    (include/sparse_amd.h, A17): the same bits on every call, no atomics.  The kernel reads the CSR form of `a` - a row-compressed
    GCXS's own arrays, else the form the array memoises for its products, so a second call converts nothing."""
    from ._attention import _csr_of_mask, _longest_row

    _check_sparse(a)
    dt = _check_arguments(a.shape, a.dtype, b, add, mul, init)
    numpy_out = isinstance(b, np.ndarray) and (init is None or isinstance(init, np.ndarray))
    device = a.device
    if a.nnz == 0 or a.size == 0:
        indptr = torch.zeros(int(a.shape[0]) + 1, dtype=torch.int64, device=device)
        indices, data, max_len = indptr[:0], torch.zeros(0, dtype=dt, device=device), 0
    else:
        data, indices, indptr = _csr_of_mask(a)
        max_len = _longest_row(a, indptr)
    res = K.semiring_spmm(indptr, indices, K.convert(data, dt), dev.to_device(b, device), max_len, add=add, mul=mul,
                          init=None if init is None else dev.to_device(init, device), return_arg=return_arg)
    if not numpy_out:
        return res
    return (dev.to_numpy(res[0]), dev.to_numpy(res[1])) if return_arg else dev.to_numpy(res)

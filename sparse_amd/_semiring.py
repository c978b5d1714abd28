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
    return _semiring_matmul(a, b, add, mul, init, return_arg, None)


def _semiring_matmul(a, b, add, mul, init, return_arg, values):
    """`semiring_matmul`; `values`: None, or a device tensor aligned with `a.data` (the caller's order) that takes the place of the
    stored values"""
    from ._attention import _bias_in_csr_order, _csr_of_mask, _longest_row

    _check_sparse(a)
    dt = _check_arguments(a.shape, a.dtype if values is None else _values_dtype(values), b, add, mul, init)
    numpy_out = isinstance(b, np.ndarray) and (init is None or isinstance(init, np.ndarray))
    device = a.device
    if a.nnz == 0 or a.size == 0:
        indptr = torch.zeros(int(a.shape[0]) + 1, dtype=torch.int64, device=device)
        indices, data, max_len = indptr[:0], torch.zeros(0, dtype=dt, device=device), 0
    else:
        data, indices, indptr = _csr_of_mask(a)
        max_len = _longest_row(a, indptr)
        if values is not None:
            data = _bias_in_csr_order(a, values)
    res = K.semiring_spmm(indptr, indices, K.convert(data, dt), dev.to_device(b, device), max_len, add=add, mul=mul,
                          init=None if init is None else dev.to_device(init, device), return_arg=return_arg)
    if not numpy_out:
        return res
    return (dev.to_numpy(res[0]), dev.to_numpy(res[1])) if return_arg else dev.to_numpy(res)


# ---- the backward pass (csrc/semiring_grad.hip) ------------------------------------------------------------------------------------
def _values_dtype(values):
    return K.np_dtype(values.dtype) if isinstance(values, torch.Tensor) else np.dtype(values.dtype)


def _check_values(a, values, what):
    """the checks of `values` that need no device: kind and alignment with `a.data`"""
    if values is None:
        return
    if not isinstance(values, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{what}: `values` must be a NumPy array or a torch tensor, got {type(values).__name__}")
    if tuple(int(n) for n in values.shape) != (int(a.nnz),):
        raise ValueError(f"shape-mismatch for {what}: `values` {tuple(values.shape)} is not aligned with `a.data` ({int(a.nnz)},)")


def _check_grad_arguments(a, b, arg, grad, mul, values):
    """the checks of `semiring_matmul_grad` that need no device; returns the torch result type"""
    _check_sparse(a)
    _check_values(a, values, "semiring_matmul_grad")
    if isinstance(b, (np.ndarray, torch.Tensor)) and _dense_dtype(b) in (torch.int32, torch.int64):
        raise TypeError("semiring_matmul_grad: `b` is an integer array, and min / max of integers has no gradient here - the result "
                        "type must be float32 or float64")
    dt = _check_arguments(a.shape, a.dtype if values is None else _values_dtype(values), b, "min", mul, None)
    out_shape = (int(a.shape[0]),) + tuple(int(n) for n in b.shape[1:])
    for name, t in (("arg", arg), ("grad", grad)):
        if not isinstance(t, (np.ndarray, torch.Tensor)):
            raise TypeError(f"semiring_matmul_grad: `{name}` must be a NumPy array or a torch tensor, got {type(t).__name__}")
        if tuple(int(n) for n in t.shape) != out_shape:
            raise ValueError(f"shape-mismatch for semiring_matmul_grad: `{name}` {tuple(t.shape)} is not the shape of the forward's "
                             f"result {out_shape}")
    if _dense_dtype(arg) != torch.int64:
        raise TypeError(f"semiring_matmul_grad: `arg` must be int64 (the forward's arg), got {arg.dtype}")
    if _dense_dtype(grad) != dt:
        raise TypeError(f"semiring_matmul_grad: `grad` must have the type of `b` ({dt}; it is not converted), got {_dense_dtype(grad)}")
    return dt


def semiring_matmul_grad(a, b, arg, grad, *, mul="plus", values=None, with_init=False):
    """The gradient of `semiring_matmul(a, b, add=.., mul=mul, init=.., return_arg=True)`: `(da, db)` for `grad`, the gradient of
    its result, and `arg`, the arg it returned; with `with_init=True`, `(da, db, dinit)`.  Only `arg` is needed, not the add.

    `a`, `b` and the conversion of the values are those of `semiring_matmul`; the result type is float32 or float64 - an integer
    `b` raises TypeError: min / max of integers has no gradient here.  `arg`: an int64 array or tensor of the result's shape.
    `grad`: the result's shape and type, any strides.  `values`: None, or an array or tensor `(nnz,)` aligned with `a.data` that
    takes the place of the stored values (the values the forward ran with).  Returns `da` `(nnz,)`, the gradient with respect to
    the stored values in the order of `a.data` - the caller's order for a column-compressed GCXS too -, `db` of the shape of `b`
    and `dinit` of the result's shape: ndarrays if `b`, `arg`, `grad` (and `values`) are all ndarrays, else device tensors.

    Output (i, j) with `arg[i, j] == -1` - the init or the identity was picked - credits no element: `dinit[i, j] = grad[i, j]`.
    Otherwise it credits the stored elements of row i whose inner index is `arg[i, j]`: exactly one in an array without duplicate
    coordinates (every COO the library builds, every canonical GCXS); with duplicates every one is credited.  For "plus" the
    credited `a` element and `b[k, j]` both take `grad[i, j]`; for "times" the element takes `grad[i, j] * b[k, j]` and `b[k, j]`
    takes `a[i, k] * grad[i, j]`.  This is the subgradient `torch.max(dim=..)` takes: on a tie the element the forward picked
    gets everything.  `arg` is only compared with stored indices, never used as an address: a value that is no index of its row
    credits nothing.

    The order of every operation is fixed (include/sparse_amd.h, A18): `da` sums its row's hits by 64 accumulators over the
    columns, `db` sums each column's stored elements in stored order - the same bits on every call, no atomics.  The column
    grouping is the memoised plan `sparse_attention_grad` uses: pattern-only state, a second call builds nothing.  An empty `a`,
    or M, N or K of 0, gives zeros and `dinit = grad` without a launch."""
    return _semiring_grad(a, b, arg, grad, mul, values, (True, True, bool(with_init)))[:3 if with_init else 2]


def _semiring_grad(a, b, arg, grad, mul, values, want):
    """`semiring_matmul_grad` for the outputs `want` = (da?, db?, dinit?): None stands for the others, whose pass is not launched"""
    from ._attention import _bias_in_csr_order, _bias_order, _column_grouping, _csr_of_mask

    dt = _check_grad_arguments(a, b, arg, grad, mul, values)
    numpy_out = all(isinstance(t, np.ndarray) for t in (b, arg, grad) + (() if values is None else (values,)))
    device = a.device
    tb, targ, tg = (dev.to_device(t, device) for t in (b, arg, grad))
    if a.nnz == 0 or a.size == 0:
        outs = (torch.zeros(int(a.nnz), dtype=dt, device=device) if want[0] else None,
                torch.zeros(tuple(tb.shape), dtype=dt, device=device) if want[1] else None,
                tg.clone(memory_format=torch.contiguous_format) if want[2] else None)
    else:
        data, indices, indptr = _csr_of_mask(a)
        if values is not None:
            data = _bias_in_csr_order(a, values)
        plan = _column_grouping(a, indices, indptr) if want[1] else {"colptr": None, "colperm": None, "colrows": None, "max_col": 0}
        outs = K.semiring_grad(indptr, indices, K.convert(data, dt), plan["colptr"], plan["colperm"], plan["colrows"], tb, targ, tg,
                               plan["max_col"], mul=mul, want=want)
        order = _bias_order(a) if want[0] else None
        if order is not None:      # back to the caller's order
            outs = (K.gather(outs[0], order["inv"]),) + outs[1:]
    return tuple(None if t is None else dev.to_numpy(t) for t in outs) if numpy_out else outs


class _SemiringMatmul(torch.autograd.Function):
    """forward: the fused call of `semiring_matmul` with the arg; backward: `semiring_matmul_grad` for the inputs that need one"""

    @staticmethod
    def forward(ctx, a, add, mul, b, init, values):
        ctx.a, ctx.mul, ctx.has = a, mul, (init is not None, values is not None)
        out, arg = _semiring_matmul(a, b.detach(), add, mul, None if init is None else init.detach(), True,
                                    None if values is None else values.detach())
        ctx.save_for_backward(b, arg, *(() if values is None else (values,)))
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad, _grad_arg):
        b, arg = ctx.saved_tensors[:2]
        values = ctx.saved_tensors[2] if ctx.has[1] else None
        need = ctx.needs_input_grad
        want = (bool(need[5]), bool(need[3]), bool(need[4]))
        da, db, dinit = _semiring_grad(ctx.a, b, arg, grad, ctx.mul, values, want) if any(want) else (None, None, None)
        if da is not None:
            da = da.to(device=values.device, dtype=values.dtype)      # (values of another float type were converted on the way in)
        if db is not None:
            db = db.to(b.device)
        if dinit is not None:
            dinit = dinit.to(grad.device)
        return None, None, None, db, dinit, da


def semiring_matmul_autograd(a, b, *, add="min", mul="plus", init=None, values=None, return_arg=False):
    """`semiring_matmul(a, b, add=add, mul=mul, init=init, return_arg=return_arg)` as a differentiable torch function: the forward
    is that fused call with the arg - the same bits -, the backward is `semiring_matmul_grad`.  `b` and `init` are torch tensors
    (float32 or float64); `values`: None, or a torch tensor `(nnz,)` aligned with `a.data` that takes the place of the stored
    values - differentiable edge weights.  `b`, `init` and `values` are the differentiable inputs: one that does not require a
    gradient gets None, and the pass that would serve only it is not launched.  The array `a` itself gets no gradient, and `arg`
    is marked non-differentiable.  On a tie the element the forward picked gets the whole gradient (A18)."""
    for name, t in (("b", b),) + ((("init", init),) if init is not None else ()) + ((("values", values),) if values is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"semiring_matmul_autograd: `{name}` must be a torch tensor, got {type(t).__name__}")
    _check_sparse(a)
    _check_values(a, values, "semiring_matmul_autograd")
    if b.dtype in (torch.int32, torch.int64):
        raise TypeError("semiring_matmul_autograd: `b` is an integer tensor, and min / max of integers has no gradient here")
    _check_arguments(a.shape, a.dtype if values is None else _values_dtype(values), b, add, mul, init)
    out, arg = _SemiringMatmul.apply(a, add, mul, b, init, values)
    return (out, arg) if return_arg else out

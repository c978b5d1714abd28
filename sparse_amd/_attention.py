"""Sparse attention as one fused kernel (csrc/attention.hip): the scores `sddmm` gives at a mask's stored positions, the
`softmax` over them and the `matmul` by `v`, for one or many heads over one shared 2-D mask - graph attention, sparse
transformers, neighbourhood attention.  The three-call expression

    matmul(softmax(sddmm(s, q, bt=k), scale=c), v)

writes the scores once and reads them three times, builds its plans on two arrays and cannot share a mask between heads."""
import numbers
import operator

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


def _check_bias(bias, dt, lead, nnz, what="sparse_attention"):
    """the checks of a bias that need no device: kind, type (no silent conversion) and shape"""
    if bias is None:
        return
    if not isinstance(bias, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{what}: `bias` must be a NumPy array or a torch tensor of one value per stored element of `s` (a sparse "
                        f"or other array is not accepted), got {type(bias).__name__}")
    bdt = bias.dtype if isinstance(bias, torch.Tensor) else _NP_OPERAND.get(bias.dtype, bias.dtype)
    if bdt != dt:
        raise TypeError(f"{what}: `bias` must have the type of q, k and v ({dt}; it is not converted), got {bdt}")
    shape = tuple(int(n) for n in bias.shape)
    if shape != (nnz,) and shape != lead + (nnz,):
        raise ValueError(f"shape-mismatch for {what}: `bias` {shape} is neither ({nnz},) - one value per stored element, shared by "
                         f"the heads - nor {lead + (nnz,)}")


def _check_dropout(dropout, seed, what="sparse_attention"):
    """the checks of `dropout` and `seed`, which need no device: (rate, seed) for a rate above 0, else (None, None) - `dropout`
    None or 0 is the call without it, and the seed is then ignored"""
    if dropout is None:
        return None, None
    if isinstance(dropout, (bool, np.bool_)) or not isinstance(dropout, numbers.Real):
        raise TypeError(f"{what}: `dropout` must be None or a real number in [0, 1), got {type(dropout).__name__}")
    rate = float(dropout)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"{what}: `dropout` must lie in [0, 1) - the probability that a stored element is dropped -, got {dropout!r}")
    if rate == 0.0:
        return None, None
    if seed is None:
        raise ValueError(f"{what}: `dropout` above 0 needs a `seed` (an int in [0, 2^64)): there is no hidden global generator, "
                         "training code passes a new seed per step")
    if isinstance(seed, (bool, np.bool_)):
        raise TypeError(f"{what}: `seed` must be an int in [0, 2^64), got {type(seed).__name__}")
    try:
        sd = operator.index(seed)
    except TypeError:
        raise TypeError(f"{what}: `seed` must be an int in [0, 2^64), got {type(seed).__name__}") from None
    if not 0 <= sd < 1 << 64:
        raise ValueError(f"{what}: `seed` must lie in [0, 2^64), got {sd}")
    return rate, sd


def _bias_order(s):
    """None when the order of `s.data` - the caller's - is the CSR order the kernel reads (a COO, a row-compressed GCXS); for a
    column-compressed GCXS the plan {"perm": CSR position -> caller's position, "inv": caller's position -> CSR position}: the
    stable re-compression that makes the CSR twin, applied to the positions as data.  Pattern-only state, kept on the array
    under a stamp of its index buffers as `_attention_plan` is"""
    from ._softmax import _coord_stamp, _stamp_holds

    if not (isinstance(s, GCXS) and s.compressed_axes != (0,)):
        return None
    stamp = _coord_stamp(s)
    plan = s.__dict__.get("_attention_bias_perm")
    if plan is None or not _stamp_holds(plan["stamp"], stamp):
        pos = torch.arange(s.nnz, dtype=torch.int64, device=s.device)
        perm = K._csc_to_csr(s.shape, pos, s.indices, s.indptr)[0]
        plan = s.__dict__["_attention_bias_perm"] = {"stamp": stamp, "perm": perm, "inv": K.sort_keys(perm, max(s.nnz - 1, 1))[1]}
    else:
        plan["stamp"].update(stamp)
    return plan


def _bias_in_csr_order(s, bias):
    """the bias on the mask's device in the order the kernel reads: untouched where that is the caller's order, else gathered
    through the memoised permutation, once"""
    b = dev.to_device(bias, s.device)
    order = _bias_order(s)
    if order is None:
        return b
    return K.gather(b.reshape(-1, s.nnz), order["perm"]).reshape(b.shape)


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


def sparse_attention(s, q, k, v, *, scale=None, bias=None, dropout=None, seed=None):
    """`dropout(softmax_over_stored(scale * (s * (q @ k.T)) + bias)) @ v` for every head, in one fused kernel.

    `s`: a 2-D COO or GCXS (either compressed axis) of shape (M, N) with a zero fill value; float32, float64, integer or
    boolean values, converted to the result type on the device; complex and 16-bit values raise TypeError.  `q` (..., M, D),
    `k` (..., N, D), `v` (..., N, Dv): NumPy arrays or torch tensors (any strides), all float32 or all float64 - the result
    type.  The leading axes are the heads: absent, or identical on all three (no broadcasting); every head uses the same
    mask.  `scale`: None or a real scalar, rounded to the result type once.

    `bias`: None, or one additive value per stored element - an edge encoding, a relative-position bias -: a NumPy array or
    torch tensor of the operands' type (it is not converted; any strides) of shape `(s.nnz,)`, shared by the heads, or
    `lead + (s.nnz,)`, one per head.  It is aligned with the array the caller holds: element `i` belongs to `s.data[i]` - to
    `s.coords[:, i]` of a COO, to `s.indices[i]` inside its compressed slice of a GCXS of either axis.  It is added to the
    score after the scale, `t = scale * (s * (q . k)) + bias`, one add rounded once (A15), so a bias of +0.0 changes no bit.  A
    bias of -inf gives that stored element the probability +0.0 in that head: per-head masks over one shared pattern (a row
    of one head whose elements are all -inf is NaN, as below; trailing -inf elements of a row of at most `ATTENTION_CHUNK`
    elements give the bits of the mask without them).  A sparse array or a dense (M, N) array is not accepted.

    `dropout`: None, or a real number in [0, 1): the probability that a stored element's attention probability is dropped.  A
    kept probability is multiplied by `1 / (1 - dropout)` (rounded to the result type once), a dropped one counts as +0.0 - it
    still takes part in the sum, so a row whose elements are all dropped is +0.0.  `seed`: an int in [0, 2^64), required when
    `dropout > 0`: there is no hidden global generator, training code passes a new seed per step.  The decision is a
    counter-based generator (Philox4x32-10) keyed by (seed, head, stored position in CSR order): the same seed gives the same
    bits on every call, in every kernel form, and a COO, a CSR and a CSC of one pattern drop the same edges;
    `sparse_attention_keep_mask` returns the decisions.  `dropout` None or 0 is the call without it (the seed is ignored).

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
    _check_bias(bias, dt, lead, int(s.nnz))
    rate, sd = _check_dropout(dropout, seed)
    torch_out = any(isinstance(t, torch.Tensor) for t in (q, k, v))
    M, Dv = int(s.shape[0]), int(v.shape[-1])
    if s.nnz == 0 or M == 0 or Dv == 0 or 0 in lead:
        out = torch.zeros(lead + (M, Dv), dtype=dt, device=s.device)
        return out if torch_out else dev.to_numpy(out)
    data, indices, indptr = _csr_of_mask(s)
    max_len = _longest_row(s, indptr)
    dq, dk, dv = (dev.to_device(t, s.device) for t in (q, k, v))
    db = None if bias is None else _bias_in_csr_order(s, bias)
    if rate is None:
        out = K.attention_rows(indptr, indices, K.convert(data, dt), dq, dk, dv, max_len, scale=scale, bias=db)
    else:
        out = K.attention_rows(indptr, indices, K.convert(data, dt), dq, dk, dv, max_len, scale=scale, bias=db, dropout=rate, seed=sd)
    return out if torch_out else dev.to_numpy(out)


def sparse_attention_keep_mask(s, lead=(), *, dropout, seed):
    """The keep decisions of `sparse_attention(s, q, k, v, dropout=dropout, seed=seed)` for operands whose leading (head) axes
    are `lead`: a bool torch tensor of shape `lead + (s.nnz,)` on the mask's device, True where the stored element is kept.
    It is aligned with `s.data` exactly as `bias` is - element `i` belongs to `s.data[i]`, for a column-compressed GCXS too -
    and comes from the device code the attention kernels call.  `dropout` of None or 0 keeps everything."""
    if not isinstance(s, (COO, GCXS)):
        raise TypeError(f"sparse_attention_keep_mask needs a COO or GCXS mask, got {type(s).__name__}")
    if s.ndim != 2:
        raise ValueError(f"sparse_attention_keep_mask needs a 2-D mask, `s` has {s.ndim} dimensions")
    if isinstance(lead, (bool, np.bool_)):
        raise TypeError("sparse_attention_keep_mask: `lead` must be an int or a tuple of ints")
    try:
        lead = (operator.index(lead),) if not isinstance(lead, (tuple, list, torch.Size)) else tuple(operator.index(n) for n in lead)
    except TypeError:
        raise TypeError("sparse_attention_keep_mask: `lead` must be an int or a tuple of ints, the leading (head) axes") from None
    if any(n < 0 for n in lead):
        raise ValueError(f"sparse_attention_keep_mask: `lead` must not be negative, got {lead}")
    rate, sd = _check_dropout(dropout, seed, "sparse_attention_keep_mask")
    nnz, H = int(s.nnz), int(np.prod(lead, dtype=np.int64))
    if rate is None or nnz == 0 or H == 0:
        return torch.ones(lead + (nnz,), dtype=torch.bool, device=s.device)
    keep = K.attention_keep(nnz, H, rate, sd, s.device)
    order = _bias_order(s)
    if order is not None:      # the decisions are made at CSR positions: back to the caller's order
        k8 = keep.view(torch.uint8)      # (the row gather takes at most 65535 rows a call)
        keep = torch.cat([K.gather(k8[h0:h0 + 65535], order["inv"]) for h0 in range(0, H, 65535)]).view(torch.bool)
    return keep.reshape(lead + (nnz,))


# ---- the backward pass (csrc/attention_grad.hip) -------------------------------------------------------------------------------------
def _build_grad_plan(indices, indptr, shape):
    """the column grouping of a CSR pattern, from the key and index primitives: (colptr [N + 1] and colrows [nnz] at the width of
    `indptr`, colperm int64[nnz], the longest column).  The sort is stable, so a column's elements keep their stored order"""
    from ._reduce import _scalar_dev
    from ._softmax import _max_len
    from ._umath import binary_arrays

    M, N = int(shape[0]), int(shape[1])
    dev_ = indices.device
    rows = binary_arrays("floor_divide_i64", K.csr_to_keys(indptr, indices, M, N), _scalar_dev(N, torch.int64, dev_), b_scalar=True)
    cols, colperm = K.sort_keys(K.convert(indices, torch.int64), max(N - 1, 1))
    colptr = K.rows_to_indptr(cols, N)
    max_col = _max_len(colptr)
    colrows = K.gather(rows, colperm)
    return K.convert(colptr, indptr.dtype), colperm, K.convert(colrows, indptr.dtype), max_col


def _column_grouping(s, indices, indptr):
    """`_build_grad_plan` of the mask, kept on the array under a stamp of its index buffers as `_attention_plan` is"""
    from ._softmax import _coord_stamp, _stamp_holds

    stamp = _coord_stamp(s)
    plan = s.__dict__.get("_attention_grad_plan")
    if plan is None or not _stamp_holds(plan["stamp"], stamp) or plan["indptr"] is not indptr:
        colptr, colperm, colrows, max_col = _build_grad_plan(indices, indptr, s.shape)
        plan = s.__dict__["_attention_grad_plan"] = {"stamp": stamp, "indptr": indptr, "colptr": colptr, "colperm": colperm,
                                                     "colrows": colrows, "max_col": max_col}
    else:
        plan["stamp"].update(stamp)
    return plan


def sparse_attention_grad(s, q, k, v, grad, *, scale=None, bias=None, dropout=None, seed=None):
    """The gradient of `sparse_attention(s, q, k, v, scale=scale, bias=bias, dropout=dropout, seed=seed)`: `(dq, dk, dv)` for
    `grad`, the gradient of its result, in one fused backward pass (two passes over the mask, no atomics); with a `bias`,
    `(dq, dk, dv, dbias)`.

    `s`, `q`, `k`, `v` and `scale` are those of `sparse_attention`: the same masks, operand kinds, strides, head axes and
    errors.  `grad` (..., M, Dv): a NumPy array or torch tensor of the operands' type and head axes (any strides).  Returns
    `dq` (..., M, D), `dk` (..., N, D) and `dv` (..., N, Dv): ndarrays if all four operands are ndarrays, else torch device
    tensors.  The gradient with respect to the mask values is not computed.

    `bias` is that of `sparse_attention`: the same kinds, shapes, alignment with `s.data` and errors; the probabilities are
    recomputed with it, the forward's bits.  `dbias` (..., nnz) is the derivative with respect to the biased score,
    `z_i = p_i * (e_i - delta)` (A16), in the order of `s.data` - the caller's order for a column-compressed mask too.  It is
    always per head, also for a shared bias (whose gradient is its sum over the head axes), so that it is covered by the
    order contract: written once per element by the row pass, no atomics.  Where the bias is -inf, p = +0.0 and dbias is 0.

    `dropout` and `seed` are those of `sparse_attention`: the same kinds, ranges and errors.  The keep decisions are recomputed
    from the seed, not stored: with the forward's `dropout` and `seed` the backward drops what the forward dropped.  A dropped
    element gets no gradient through `v` (`dv` takes the dropped-and-rescaled probability) and enters `delta` as 0 (A16).

    A row without stored elements has a `dq` row of +0.0, a column without stored elements `dk` and `dv` rows of +0.0.  A
    row whose forward row is NaN has a NaN `dq` row and hands NaN to the `dk` / `dv` rows of its columns.

    The order of every operation is fixed (include/sparse_amd.h, A16): the probabilities are recomputed with the forward's
    bits, `dk` and `dv` sum each column's stored elements in stored order - the same bits on every call.  The column grouping
    of the mask is pattern-only state, built once and kept on the array; a second call converts and builds nothing."""
    return _attention_grad(s, q, k, v, grad, scale, bias, True, dropout, seed)


def _attention_grad(s, q, k, v, grad, scale, bias, want_dbias, dropout=None, seed=None):
    """`sparse_attention_grad`; `want_dbias` False leaves dbias out of the row pass and returns None in its place"""
    from ._softmax import _check_arguments
    from ._utils import check_zero_fill_value

    if not isinstance(s, (COO, GCXS)):
        raise TypeError(f"sparse_attention needs a COO or GCXS mask, got {type(s).__name__}")
    if s.ndim != 2:
        raise ValueError(f"sparse_attention needs a 2-D mask, `s` has {s.ndim} dimensions (every head shares one 2-D mask)")
    _check_arguments(s.dtype, 2, -1, scale)
    check_zero_fill_value(s)
    dt, lead = _check_operands(s.shape, q, k, v)
    if not isinstance(grad, (np.ndarray, torch.Tensor)):
        raise TypeError(f"sparse_attention_grad: `grad` must be a NumPy array or a torch tensor, got {type(grad).__name__}")
    gdt = grad.dtype if isinstance(grad, torch.Tensor) else _NP_OPERAND.get(grad.dtype, grad.dtype)
    if gdt != dt:
        raise TypeError(f"sparse_attention_grad: `grad` must have the type of q, k and v ({dt}), got {gdt}")
    M, N, D, Dv = int(s.shape[0]), int(s.shape[1]), int(q.shape[-1]), int(v.shape[-1])
    if tuple(int(n) for n in grad.shape) != lead + (M, Dv):
        raise ValueError(f"shape-mismatch for sparse_attention_grad: `grad` {tuple(grad.shape)} is not the shape of the forward's "
                         f"result {lead + (M, Dv)}")
    _check_bias(bias, dt, lead, int(s.nnz), "sparse_attention_grad")
    rate, sd = _check_dropout(dropout, seed, "sparse_attention_grad")
    drop = {} if rate is None else {"dropout": rate, "seed": sd}
    torch_out = any(isinstance(t, torch.Tensor) for t in (q, k, v, grad))
    if s.nnz == 0 or 0 in lead:
        outs = tuple(torch.zeros(lead + shp, dtype=dt, device=s.device) for shp in ((M, D), (N, D), (N, Dv)))
        if bias is not None:
            outs += (torch.zeros(lead + (int(s.nnz),), dtype=dt, device=s.device) if want_dbias else None,)
    else:
        data, indices, indptr = _csr_of_mask(s)
        max_row = _longest_row(s, indptr)
        plan = _column_grouping(s, indices, indptr)
        tq, tk, tv, tg = (dev.to_device(t, s.device) for t in (q, k, v, grad))
        db = None if bias is None else _bias_in_csr_order(s, bias)
        outs = K.attention_grad_rows(indptr, indices, K.convert(data, dt), plan["colptr"], plan["colperm"], plan["colrows"], tq, tk,
                                     tv, tg, max_row, plan["max_col"], scale=scale, bias=db, want_dbias=want_dbias, **drop)
        order = None if bias is None else _bias_order(s)
        if order is not None and outs[3] is not None:      # back to the caller's order
            outs = outs[:3] + (K.gather(outs[3].reshape(-1, int(s.nnz)), order["inv"]).reshape(outs[3].shape),)
    return outs if torch_out else tuple(None if t is None else dev.to_numpy(t) for t in outs)


class _SparseAttention(torch.autograd.Function):
    """forward: the fused call of `sparse_attention`; backward: `sparse_attention_grad` (no gradient for the mask or the scale)"""

    @staticmethod
    def forward(ctx, s, scale, q, k, v, bias, dropout=None, seed=None):
        ctx.s, ctx.scale, ctx.has_bias = s, scale, bias is not None
        ctx.drop = {} if dropout is None else {"dropout": dropout, "seed": seed}      # the backward drops what the forward dropped
        if bias is None:
            ctx.save_for_backward(q, k, v)
            return sparse_attention(s, q.detach(), k.detach(), v.detach(), scale=scale, **ctx.drop)
        ctx.save_for_backward(q, k, v, bias)
        return sparse_attention(s, q.detach(), k.detach(), v.detach(), scale=scale, bias=bias.detach(), **ctx.drop)

    @staticmethod
    def backward(ctx, grad):
        need = ctx.needs_input_grad
        if not ctx.has_bias:
            q, k, v = ctx.saved_tensors
            dq, dk, dv = sparse_attention_grad(ctx.s, q, k, v, grad, scale=ctx.scale, **ctx.drop)
            return None, None, dq if need[2] else None, dk if need[3] else None, dv if need[4] else None, None, None, None
        q, k, v, bias = ctx.saved_tensors
        dq, dk, dv, dbias = _attention_grad(ctx.s, q, k, v, grad, ctx.scale, bias, need[5], **ctx.drop)
        if need[5] and dbias.dim() > bias.dim():      # a bias shared by the heads: the one sum outside the written order
            dbias = torch.sum(dbias, dim=tuple(range(dbias.dim() - 1)))
        return (None, None, dq if need[2] else None, dk if need[3] else None, dv if need[4] else None, dbias if need[5] else None,
                None, None)


def sparse_attention_autograd(s, q, k, v, *, scale=None, bias=None, dropout=None, seed=None):
    """`sparse_attention(s, q, k, v, scale=scale, bias=bias)` as a differentiable torch function: the forward is that fused call
    - the same bits -, the backward is `sparse_attention_grad`.  `q`, `k` and `v` are torch tensors; the mask `s` and `scale`
    get no gradient, and an operand that does not require one gets None.

    `bias`: None or a torch tensor as in `sparse_attention` (aligned with `s.data`, added after the scale, -inf masks an
    element for a head); it is a differentiable input.  Its gradient is `dbias` of `sparse_attention_grad`; for a bias of
    shape `(nnz,)` shared by several heads it is `torch.sum` of `dbias` over the head axes - this one sum is outside the
    written order of A16 (torch chooses its order).  `dbias` is not computed when the bias does not require a gradient.

    `dropout` and `seed` are those of `sparse_attention` (neither gets a gradient).  The function saves them and hands them to
    the backward, which recomputes the keep decisions: the backward drops what the forward dropped."""
    for name, t in (("q", q), ("k", k), ("v", v)) + ((("bias", bias),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"sparse_attention_autograd: `{name}` must be a torch tensor, got {type(t).__name__}")
    rate, sd = _check_dropout(dropout, seed, "sparse_attention_autograd")
    return _SparseAttention.apply(s, scale, q, k, v, bias, rate, sd)

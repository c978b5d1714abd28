"""sparse_attention, sparse_attention_grad and sparse_attention_autograd with an additive bias, on the device
(spamd_attention_bias in csrc/attention.hip, spamd_attention_grad_bias in csrc/attention_grad.hip).

Yardsticks, from tests/attention_bias_cases.py:
  * `attention_bias_restated` / `grad_bias_restated` - A15 and A16 with the one add `t_i = t_i + b_i` after the scale and
    `dbias_i = z_i`, written in NumPy - in the result type, BIT FOR BIT (any NaN equals any NaN);
  * the calls without a bias: a bias of +0.0 changes no bit, and `bias=None` is the old entry;
  * every kernel form, sub-group width and layout against every other, bit for bit;
  * torch.autograd.gradcheck at torch's own default tolerances."""
import functools

import numpy as np
import pytest
import torch

import attention_bias_cases as bc
import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNKS = (64, 128, None)          # None: the default, `_kernels.ATTENTION_CHUNK`, on `attention_cases.SHORT_LENGTHS`
LEAD = (2,)


def _chunk(monkeypatch, chunk):
    from sparse_amd import _kernels as K

    if chunk is not None:
        monkeypatch.setattr(K, "ATTENTION_CHUNK", chunk)
    return K.ATTENTION_CHUNK


def _coo(indptr, indices, vals, shape, idx=None, **kw):
    import sparse_amd

    kw = dict(dict(has_duplicates=False, sorted=True), **kw)
    return sparse_amd.COO(ac.coords_of(indptr, indices), vals, shape=shape, idx_dtype=idx, device=DEV, **kw)


def _csr(indptr, indices, vals, shape):
    import sparse_amd

    return sparse_amd.GCXS((vals, indices, indptr), shape=shape, compressed_axes=(0,), device=DEV)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _dev(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs)


def _same(got, want):
    return len(got) == len(want) and all(sc.same_bits(_np(a), b) for a, b in zip(got, want))


@pytest.fixture
def spy(monkeypatch):
    """records the bias every `attention_rows` and `attention_grad_rows` call was given"""
    from sparse_amd import _kernels as K

    seen = []
    for name in ("attention_rows", "attention_grad_rows"):
        real = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _real=real, **kw: seen.append(kw.get("bias")) or _real(*a, **kw))
    return seen


# ---- the listed lengths in every layout ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lengths_case(chunk, dtype, columns=False):
    """the listed lengths of one chunk (None: SHORT_LENGTHS at the default chunk) as the row - or, `columns`, the column - lengths
    of one mask; two heads, D = 17, Dv = 5, a scale, a bias per head.  Restated once: the forward and the gradient with the
    per-head bias, and those of head 1 with head 0's bias (the shared bias)"""
    lengths = ac.SHORT_LENGTHS if chunk is None else sc.listed_lengths(chunk)
    ck = 1024 if chunk is None else chunk
    indptr, indices, vals, shape = (gc.transposed_mask if columns else ac.csr_mask)(240 + ck, lengths, dtype)
    q, k, v = ac.operands(241 + ck, shape, 17, 5, dtype, lead=LEAD)
    g = gc.grad_operand(242 + ck, shape, 5, dtype, lead=LEAD)
    bias = bc.bias_of(243 + ck, len(indices), dtype, lead=LEAD)
    out = bc.attention_bias_heads(indptr, indices, vals, q, k, v, ck, 0.3, bias)
    grads = bc.grad_bias_heads(indptr, indices, vals, q, k, v, g, ck, 0.3, bias)
    out1 = bc.attention_bias_restated(indptr, indices, vals, q[1], k[1], v[1], ck, 0.3, bias[0])[0]
    grads1 = bc.grad_bias_restated(indptr, indices, vals, q[1], k[1], v[1], g[1], ck, 0.3, bias[0])
    out_sh = np.stack([out[0], out1])
    grads_sh = tuple(np.stack([a[0], b]) for a, b in zip(grads, grads1))
    for a in (indptr, indices, vals, q, k, v, g, bias, out, out_sh) + grads + grads_sh:
        a.setflags(write=False)
    return indptr, indices, vals, shape, q, k, v, g, bias, out, grads, out_sh, grads_sh


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_listed_lengths_bit_for_bit_in_every_layout(dtype, idx, chunk, monkeypatch, spy):
    """forward and backward, per-head and shared bias, NumPy and torch operands; the short / wide switch at 64 / 65, the wide /
    long switch at chunk / chunk + 1, rows of 2 and 5 pieces, empty rows first, last and in runs"""
    import sparse_amd

    case = _lengths_case(chunk, np.dtype(dtype))
    _chunk(monkeypatch, chunk)
    indptr, indices, vals, shape, q, k, v, g, bias, out, grads, out_sh, grads_sh = case
    ptr_i, ind_i = indptr.astype(idx), indices.astype(idx)
    nnz = len(indices)

    def check(s, b_head, b_shared, order=None):
        """`order`: the caller's order of `s.data` as positions of the canonical order (dbias comes back in it)"""
        got = sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=b_head)
        assert isinstance(got, np.ndarray) and sc.same_bits(got, out)
        assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=b_shared), out_sh)
        for b, want in ((b_head, grads), (b_shared, grads_sh)):
            gr = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=b)
            assert len(gr) == 4 and gr[3].shape == LEAD + (nnz,) and all(isinstance(a, np.ndarray) for a in gr)
            assert _same(gr[:3], want[:3])
            assert sc.same_bits(gr[3], want[3] if order is None else want[3][..., order])

    # a canonical COO
    coo = _coo(ptr_i, ind_i, vals, shape, idx)
    check(coo, bias, bias[0])
    # a row-compressed GCXS: the caller's order is the kernel's, a device bias is passed through untouched
    x = _csr(ptr_i, ind_i, vals, shape)
    check(x, bias, bias[0])
    tb, = _dev(bias)
    tq, tk, tv, tg = _dev(q, k, v, g)
    tout = sparse_amd.sparse_attention(x, tq, tk, tv, scale=0.3, bias=tb)
    assert spy[-1] is tb and isinstance(tout, torch.Tensor) and sc.same_bits(_np(tout), out)
    tgr = sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg, scale=0.3, bias=tb)
    assert spy[-1] is tb and all(isinstance(t, torch.Tensor) and t.is_cuda for t in tgr) and _same(tgr, grads)
    tout = sparse_amd.sparse_attention(coo, tq, tk, tv, scale=0.3, bias=tb)
    assert spy[-1] is tb and sc.same_bits(_np(tout), out)
    # a column-compressed GCXS: the caller's order is by (column, row); the bias and dbias are in it
    xc = coo.asformat("gcxs", compressed_axes=(1,))
    order = gc.column_order(indptr, indices)[0]
    assert np.array_equal(_np(xc.data), vals[order])
    check(xc, np.ascontiguousarray(bias[..., order]), np.ascontiguousarray(bias[0][order]), order)
    # a COO built unsorted: the array the caller holds is canonical, and so is its bias
    perm = np.random.default_rng(5).permutation(nnz)
    un = sparse_amd.COO(ac.coords_of(indptr, indices)[:, perm].astype(idx), vals[perm], shape=shape, idx_dtype=idx, device=DEV)
    assert np.array_equal(_np(un.data), vals)
    assert sc.same_bits(sparse_amd.sparse_attention(un, q, k, v, scale=0.3, bias=bias), out)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_columns_bit_for_bit(dtype, monkeypatch):
    """the listed lengths as COLUMN lengths at chunk 64: the column pass in all its forms reads the p and y of the biased rows"""
    import sparse_amd

    indptr, indices, vals, shape, q, k, v, g, bias, out, grads, out_sh, grads_sh = _lengths_case(64, np.dtype(dtype), True)
    _chunk(monkeypatch, 64)
    s = _coo(indptr, indices, vals, shape)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias), out)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias), grads)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias[0]), grads_sh)


# ---- widths and heads -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Dv", [(1, 1), (17, 5), (64, 64), (130, 65)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_widths(dtype, D, Dv):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(250, ac.SHORT_LENGTHS, dtype)
    q, k, v = ac.operands(251 + D, shape, D, Dv, dtype)
    g = gc.grad_operand(252 + Dv, shape, Dv, dtype)
    bias = bc.bias_of(253, len(indices), dtype)
    s = _coo(indptr, indices, vals, shape)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, bias=bias), bc.attention_bias_restated(indptr, indices, vals, q, k, v, 1024, None, bias)[0])
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, bias=bias), bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 1024, None, bias))


@pytest.mark.parametrize("shared", [False, True], ids=["per-head", "shared"])
@pytest.mark.parametrize("lead", [(), (3,), (2, 2)])
def test_heads(lead, shared):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(260, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(261, shape, 20, 9, np.float32, lead=lead)
    g = gc.grad_operand(262, shape, 9, np.float32, lead=lead)
    bias = bc.bias_of(263, len(indices), np.float32, None if shared else lead)
    s = _coo(indptr, indices, vals, shape)
    want = bc.attention_bias_heads(indptr, indices, vals, q, k, v, 1024, 0.5, bias)
    gwant = bc.grad_bias_heads(indptr, indices, vals, q, k, v, g, 1024, 0.5, bias)
    got = sparse_amd.sparse_attention(s, q, k, v, scale=0.5, bias=bias)
    ggot = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.5, bias=bias)
    assert got.shape == lead + (shape[0], 9) and sc.same_bits(got, want)
    assert ggot[3].shape == lead + (len(indices),) and _same(ggot, gwant)
    tq, tk, tv, tg, tb = _dev(q, k, v, g, bias)
    assert sc.same_bits(_np(sparse_amd.sparse_attention(s, tq, tk, tv, scale=0.5, bias=tb)), want)
    assert _same(sparse_amd.sparse_attention_grad(s, tq, tk, tv, tg, scale=0.5, bias=tb), gwant)
    assert sc.same_bits(_np(sparse_amd.sparse_attention(s, tq, tk, tv, scale=0.5, bias=bias)), want)          # a NumPy bias beside tensors


def test_strided_bias():
    """a slice of a wider tensor (its head stride exceeds nnz: read in place), every second element (the one copy), NumPy too"""
    import sparse_amd
    from sparse_amd import _kernels as K

    indptr, indices, vals, shape = ac.csr_mask(270, ac.SHORT_LENGTHS, np.float32)
    q, k, v = ac.operands(271, shape, 19, 7, np.float32, lead=(3,))
    g = gc.grad_operand(272, shape, 7, np.float32, lead=(3,))
    nnz = len(indices)
    bias = bc.bias_of(273, nnz, np.float32, (3,))
    s = _coo(indptr, indices, vals, shape)
    want = bc.attention_bias_heads(indptr, indices, vals, q, k, v, 1024, None, bias)
    gwant = bc.grad_bias_heads(indptr, indices, vals, q, k, v, g, 1024, None, bias)
    tq, tk, tv, tg = _dev(q, k, v, g)
    wide = torch.zeros(3, nnz + 9, device=DEV)
    wide[:, 4:4 + nnz] = torch.from_numpy(bias).to(DEV)
    b2, bh = K._bias2(wide[:, 4:4 + nnz], (3,), 3, nnz, torch.float32, "test")
    assert bh == nnz + 9 and b2.data_ptr() == wide[:, 4:].data_ptr()
    every2 = torch.zeros(3, 2 * nnz, device=DEV)
    every2[:, ::2] = torch.from_numpy(bias).to(DEV)
    for tb in (wide[:, 4:4 + nnz], every2[:, ::2]):
        assert not tb.is_contiguous()
        assert sc.same_bits(_np(sparse_amd.sparse_attention(s, tq, tk, tv, bias=tb)), want)
        assert _same(sparse_amd.sparse_attention_grad(s, tq, tk, tv, tg, bias=tb), gwant)
    big = np.zeros((3, 2 * nnz), np.float32)
    big[:, ::2] = bias
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, bias=big[:, ::2]), want)


# ---- every form against every other -------------------------------------------------------------------------------------------------
def _plan_np(indptr, indices, N):
    perm, rows, cols = gc.column_order(indptr, indices)
    return np.searchsorted(cols, np.arange(N + 1)), perm, rows


@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_groups_and_chunks_change_no_bit(dtype, idx):
    from sparse_amd import _kernels as K

    def runs(lengths, seed, variants, lead=(2,), shared=False):
        indptr, indices, vals, shape = ac.csr_mask(seed, lengths, dtype)
        q, k, v = ac.operands(seed + 1, shape, 21, 6, dtype, lead=lead)
        g = gc.grad_operand(seed + 2, shape, 6, dtype, lead=lead)
        bias = bc.bias_of(seed + 3, len(indices), dtype, None if shared else lead)
        cptr, cperm, crow = _plan_np(indptr, indices, shape[1])
        ti = lambda a, t=idx: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(t)      # noqa: E731
        csr = (ti(indptr), ti(indices), torch.from_numpy(vals).to(DEV))
        plan = (ti(cptr), ti(cperm, torch.int64), ti(crow))
        tq, tk, tv, tg, tb = _dev(q, k, v, g, bias)
        max_row, max_col = int(np.diff(indptr).max()), int(np.diff(cptr).max())
        outs = {}
        for kw in variants:
            fkw = {a: b for a, b in kw.items() if a != "col_group"}
            fwd = K.attention_rows(*csr, tq, tk, tv, max_row, scale=0.7, bias=tb, **fkw)
            bwd = K.attention_grad_rows(*csr, *plan, tq, tk, tv, tg, max_row, max_col, scale=0.7, bias=tb, want_dbias=True, **kw)
            outs[str(kw)] = [_np(fwd)] + [_np(t) for t in bwd]
        first = next(iter(outs.values()))
        assert all(_same(o, first) for o in outs.values()), [name for name, o in outs.items() if not _same(o, first)]
        nob = K.attention_grad_rows(*csr, *plan, tq, tk, tv, tg, max_row, max_col, scale=0.7, bias=tb, **variants[0])      # want_dbias False
        assert nob[3] is None and _same(nob[:3], first[1:4])
        return (indptr, indices, vals, q, k, v), g, bias, first

    def restated(case, g, bias, chunk):
        return [bc.attention_bias_heads(*case, chunk, 0.7, bias)] + list(bc.grad_bias_heads(*case, g, chunk, 0.7, bias))

    widths = [dict(group=a, col_group=b) for a, b in zip(K.ATTENTION_GROUPS, K.ATTENTION_GROUPS[::-1])]
    short = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 5]
    variants = [dict(form="short", **w) for w in widths] + [dict(form="wide", chunk=c) for c in (64, 1024)]
    variants += [dict(form="long"), dict(), dict(group=8, col_group=8), dict(group=64, col_group=64, chunk=128), dict(short_max=16),
                 dict(short_max=0, group=32, col_group=32)]
    for shared in (False, True):
        case, g, bias, got = runs(short, 271, variants, shared=shared)
        assert _same(got, restated(case, g, bias, 64))
    mid = short + [65, 100, 127, 128]
    variants = [dict(form="wide", chunk=c) for c in (128, 1024)] + [dict(chunk=c, **w) for w in widths for c in (128, 256)]
    variants += [dict(form="long", chunk=128)]
    runs(mid, 272, variants)
    long_ = mid + [129, 191, 192, 193, 64 * 5, 640]
    for chunk in (64, 128):
        variants = [dict(form="long", chunk=chunk)] + [dict(chunk=chunk, **w) for w in widths]
        case, g, bias, got = runs(long_, 273, variants, lead=(), shared=chunk == 128)
        assert _same(got, restated(case, g, bias, chunk))


# ---- a zero bias, and no bias -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_bias_has_the_bits_of_the_call_without_one(dtype, monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    indptr, indices, vals, shape = ac.csr_mask(280, sc.listed_lengths(64), dtype)
    vals[::7] = 0                                                       # scores of +0.0 and -0.0: `t + 0.0` loses the sign only
    q, k, v = ac.operands(281, shape, 17, 5, dtype, lead=(2,))
    g = gc.grad_operand(282, shape, 5, dtype, lead=(2,))
    s = _coo(indptr, indices, vals, shape)
    plain = sparse_amd.sparse_attention(s, q, k, v, scale=0.3)
    gplain = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3)
    assert len(gplain) == 3
    for zero in (np.zeros(len(indices), dtype), np.zeros((2, len(indices)), dtype)):
        assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=zero), plain)
        assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=zero)[:3], gplain)
    # bias=None goes through the wrappers to the entries without a bias
    names = []
    real = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *a: names.append(name) or real(name, *a))
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=None), plain)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=None), gplain)
    assert "spamd_attention" in names and "spamd_attention_grad" in names and not any(n.endswith("_bias") for n in names)
    del names[:]
    sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=np.zeros(len(indices), dtype))
    assert "spamd_attention_grad_bias" in names and "spamd_attention_grad" not in names


# ---- -inf: a mask per head over one shared pattern ------------------------------------------------------------------------------------
def _without(indptr, indices, vals, keep):
    """the mask without the stored elements where `keep` is False"""
    rows = ac._rows(indptr)[keep]
    ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=len(indptr) - 1)))).astype(np.int64)
    return ptr, indices[keep], vals[keep]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_neg_inf_bias_is_a_mask_per_head(dtype, monkeypatch):
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    indptr, indices, vals, shape = ac.csr_mask(290, sc.listed_lengths(64), dtype)
    H, nnz = 3, len(indices)
    q, k, v = ac.operands(291, shape, 17, 5, dtype, lead=(H,))
    g = gc.grad_operand(292, shape, 5, dtype, lead=(H,))
    bias = bc.bias_of(293, nnz, dtype, (H,), neg_inf=0.3)
    bias[:, indptr[:-1][np.diff(indptr) > 0]] = 0.25                    # every row keeps its first element in every head
    s = _coo(indptr, indices, vals, shape)
    got = sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias)
    ggot = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias)
    assert sc.same_bits(got, bc.attention_bias_heads(indptr, indices, vals, q, k, v, 64, 0.3, bias)) and np.isfinite(got).all()
    assert _same(ggot, bc.grad_bias_heads(indptr, indices, vals, q, k, v, g, 64, 0.3, bias))
    assert not ggot[3][np.isinf(bias)].any()                            # a masked element has p = +0.0, so z = 0
    for h in range(H):
        keep = np.isfinite(bias[h])
        ptr, idx, vv = _without(indptr, indices, vals, keep)
        one = sparse_amd.sparse_attention(_coo(ptr, idx, vv, shape), q[h], k[h], v[h], scale=0.3, bias=np.ascontiguousarray(bias[h][keep]))
        t = bc.attention_bias_restated(ptr, idx, vv, q[h], k[h], v[h], 64, 0.3, bias[h][keep])[1]
        want, bound = bc.other_form_bound(ptr, idx, vv, q[h], k[h], v[h], t, bias[h][keep], 0.3)
        assert (np.abs(got[h].astype(ac.LD) - one.astype(ac.LD)) <= bound).all()
        assert (np.abs(got[h].astype(ac.LD) - want) <= bound).all()
    # -inf on the trailing elements of rows of at most `chunk` elements: the bits of the mask without them
    lengths = [0, 1, 2, 9, 33, 64, 5]
    indptr, indices, vals, shape = ac.csr_mask(295, lengths, dtype)
    q, k, v = ac.operands(296, shape, 17, 5, dtype)
    g = gc.grad_operand(297, shape, 5, dtype)
    bias = bc.bias_of(298, len(indices), dtype)
    keep = np.ones(len(indices), bool)
    for r, cut in zip(range(len(lengths)), [0, 0, 1, 4, 32, 1, 2]):
        keep[indptr[r + 1] - cut:indptr[r + 1]] = False
    bias[~keep] = -np.inf
    ptr, idx, vv = _without(indptr, indices, vals, keep)
    full = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, v, scale=0.3, bias=bias)
    cut = sparse_amd.sparse_attention(_coo(ptr, idx, vv, shape), q, k, v, scale=0.3, bias=np.ascontiguousarray(bias[keep]))
    assert sc.same_bits(full, cut)
    # a row of nothing but -inf is NaN, in that head only
    bias = bc.bias_of(299, len(indices), dtype, (2,))
    bias[1, indptr[4]:indptr[5]] = -np.inf
    out = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), *ac.operands(296, shape, 17, 5, dtype, lead=(2,)), bias=bias)
    assert np.isnan(out[1, 4]).all() and np.isfinite(out[0]).all() and np.isfinite(np.delete(out[1], 4, axis=0)).all()


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per-head", "shared"])
def test_autograd_function_has_the_bits_of_both_calls(shared):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(300, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(301, shape, 12, 7, np.float32, lead=(3,))
    g = gc.grad_operand(302, shape, 7, np.float32, lead=(3,))
    bias = bc.bias_of(303, len(indices), np.float32, None if shared else (3,))
    s = _coo(indptr, indices, vals, shape)
    tq, tk, tv, tg, tb = _dev(q, k, v, g, bias)
    tq.requires_grad_()
    tb.requires_grad_()
    out = sparse_amd.sparse_attention_autograd(s, tq, tk, tv, scale=0.4, bias=tb)
    assert out.requires_grad and torch.equal(out.detach(), sparse_amd.sparse_attention(s, tq.detach(), tk, tv, scale=0.4, bias=tb.detach()))
    out.backward(tg)
    dq, dk, dv, db = sparse_amd.sparse_attention_grad(s, tq.detach(), tk, tv, tg, scale=0.4, bias=tb.detach())
    assert torch.equal(tq.grad, dq) and tk.grad is None and tb.grad.shape == tb.shape
    assert torch.equal(tb.grad, torch.sum(db, dim=0) if shared else db)
    # a bias that needs no gradient: dbias is not computed
    tq.grad = None
    sparse_amd.sparse_attention_autograd(s, tq, tk, tv, scale=0.4, bias=tb.detach()).backward(tg)
    assert torch.equal(tq.grad, dq)
    with pytest.raises(TypeError, match="torch tensor"):
        sparse_amd.sparse_attention_autograd(s, tq, tk, tv, bias=bias)


@pytest.mark.parametrize("shared", [False, True], ids=["per-head", "shared"])
def test_gradcheck(shared, monkeypatch):
    """float64, rows of 0, 1, 9 and 70 elements at chunk 64 (an empty row, the sub-group form, and two pieces), D = 3, Dv = 2, two
    heads; q, k, v and the bias all require gradients; torch's own default tolerances"""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    indptr, indices, vals, shape = ac.csr_mask(310, [0, 1, 9, 70], np.float64)
    s = _coo(indptr, indices, vals, shape)
    tq, tk, tv = (t.requires_grad_() for t in _dev(*ac.operands(311, shape, 3, 2, np.float64, lead=(2,))))
    tb = _dev(bc.bias_of(312, len(indices), np.float64, None if shared else (2,), spread=0.5))[0].requires_grad_()
    out = sparse_amd.sparse_attention_autograd(s, tq, tk, tv, scale=0.7, bias=tb)
    assert torch.equal(out.detach(), sparse_amd.sparse_attention(s, tq.detach(), tk.detach(), tv.detach(), scale=0.7, bias=tb.detach()))
    assert torch.autograd.gradcheck(lambda a, b, c, d: sparse_amd.sparse_attention_autograd(s, a, b, c, scale=0.7, bias=d), (tq, tk, tv, tb))


# ---- caches -----------------------------------------------------------------------------------------------------------------------------
def test_second_call_builds_no_plan_and_no_permutation(monkeypatch):
    import sparse_amd
    from sparse_amd import _attention, _dot, _kernels as K

    assert "_attention_bias_perm" in _dot.DERIVED_CACHES
    swaps = []
    real = K._csc_to_csr
    monkeypatch.setattr(K, "_csc_to_csr", lambda *a: swaps.append(1) or real(*a))
    indptr, indices, vals, shape = ac.csr_mask(320, ac.SHORT_LENGTHS + [1500], np.float32)
    q, k, v = ac.operands(321, shape, 16, 8, np.float32)
    g = gc.grad_operand(322, shape, 8, np.float32)
    bias = bc.bias_of(323, len(indices), np.float32)
    order = gc.column_order(indptr, indices)[0]
    tq, tk, tv, tg = _dev(q, k, v, g)
    want = bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 1024, None, bias)
    xc = _coo(indptr, indices, vals, shape).asformat("gcxs", compressed_axes=(1,))
    tb, = _dev(bias[order])
    first = sparse_amd.sparse_attention_grad(xc, tq, tk, tv, tg, bias=tb)
    n = len(swaps)
    assert 1 <= n <= 2                                                  # the twin and the permutation
    perm, plan, gplan = xc._attention_bias_perm, xc._attention_plan, xc._attention_grad_plan
    # the caller's position j holds the canonical element order[j]: CSR position -> caller's position is the inverse of `order`
    assert np.array_equal(_np(perm["perm"]), np.argsort(order)) and np.array_equal(_np(perm["inv"]), order)
    second = sparse_amd.sparse_attention_grad(xc, tq, tk, tv, tg, bias=tb)
    sparse_amd.sparse_attention(xc, tq, tk, tv, bias=tb)
    assert len(swaps) == n and xc._attention_bias_perm is perm and xc._attention_plan is plan and xc._attention_grad_plan is gplan
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert _same(first[:3], want[:3]) and sc.same_bits(_np(first[3]), want[3][order])
    # a COO and a row-compressed GCXS have no permutation
    for x in (_coo(indptr, indices, vals, shape), _csr(indptr, indices, vals, shape)):
        assert _same(sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg, bias=bias), want) and "_attention_bias_perm" not in x.__dict__
    # other index buffers (the same pattern in new tensors): the plans are built again
    xc.indices = xc.indices.clone()
    xc.indptr = xc.indptr.clone()
    third = sparse_amd.sparse_attention_grad(xc, tq, tk, tv, tg, bias=tb)
    assert xc._attention_bias_perm is not perm and xc._attention_grad_plan is not gplan and len(swaps) > n
    assert all(torch.equal(a, b) for a, b in zip(first, third))

"""Attention dropout on the device: spamd_attention_keep, spamd_attention_dropout (csrc/attention.hip) and
spamd_attention_grad_dropout (csrc/attention_grad.hip) through `sparse_attention`, `sparse_attention_grad`,
`sparse_attention_autograd` and `sparse_attention_keep_mask`.

Yardsticks, from tests/attention_dropout_cases.py:
  * `keep_restated` - Philox4x32-10 in NumPy - byte for byte;
  * `attention_dropout_restated` / `grad_dropout_restated` - A15 and A16 with pd_i and ed_i, written in NumPy - in the result
    type, BIT FOR BIT (any NaN equals any NaN);
  * the calls without dropout: `dropout=0.0` and `dropout=None` reach the old entries and have their bits;
  * every kernel form, sub-group width and layout against every other, bit for bit;
  * torch.autograd.gradcheck at torch's own default tolerances."""
import functools

import numpy as np
import pytest
import torch

import attention_bias_cases as bc
import attention_cases as ac
import attention_dropout_cases as dc
import attention_grad_cases as gc
import softmax_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNKS = (64, 128, None)          # None: the default, `_kernels.ATTENTION_CHUNK`, on `attention_cases.SHORT_LENGTHS`
LEAD = (2,)
SEED_A, SEED_B = 0xDEADBEEFCAFEF00D, (1 << 63) + 12345      # both halves non-zero


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


# ---- the decisions by themselves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos0,head0,seed", [(0, 0, 7), ((1 << 32) - 500, 0, SEED_A), (1 << 40, 0, SEED_A), (0, (1 << 32) - 1, SEED_B),
                                             ((1 << 40) + 3, (1 << 33) + 1, (1 << 64) - 1)])
def test_keep_kernel_byte_for_byte(pos0, head0, seed):
    """positions, heads and seeds whose high words are not zero: the only places where a dropped high word shows"""
    from sparse_amd import _kernels as K

    for rate in (0.0, 0.1, 0.6):
        got = K.attention_keep(1000, 3, rate, seed, DEV, pos0=pos0, head0=head0)
        assert got.dtype == torch.bool and got.shape == (3, 1000)
        assert np.array_equal(_np(got.view(torch.uint8)), dc.keep_restated(1000, 3, rate, seed, pos0, head0).astype(np.uint8))
    if pos0 >> 32 or head0 >> 32:      # the restatement itself sees the high words
        low = dc.keep_restated(1000, 3, 0.6, seed, pos0 & 0xFFFFFFFF, head0 & 0xFFFFFFFF)
        assert (dc.keep_restated(1000, 3, 0.6, seed, pos0, head0) != low).any()


# ---- the listed lengths in every layout ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lengths_case(chunk, dtype, columns=False):
    """the listed lengths of one chunk (None: SHORT_LENGTHS at the default chunk) as the row - or, `columns`, the column - lengths
    of one mask; two heads, D = 17, Dv = 5.  Restated once: A - rate 0.1, a scale, a bias per head; B - rate 0.6, neither"""
    lengths = ac.SHORT_LENGTHS if chunk is None else sc.listed_lengths(chunk)
    ck = 1024 if chunk is None else chunk
    indptr, indices, vals, shape = (gc.transposed_mask if columns else ac.csr_mask)(340 + ck, lengths, dtype)
    q, k, v = ac.operands(341 + ck, shape, 17, 5, dtype, lead=LEAD)
    g = gc.grad_operand(342 + ck, shape, 5, dtype, lead=LEAD)
    bias = bc.bias_of(343 + ck, len(indices), dtype, lead=LEAD)
    out_a = dc.attention_dropout_heads(indptr, indices, vals, q, k, v, ck, 0.3, bias, 0.1, SEED_A)
    grads_a = dc.grad_dropout_heads(indptr, indices, vals, q, k, v, g, ck, 0.3, bias, 0.1, SEED_A)
    out_b = dc.attention_dropout_heads(indptr, indices, vals, q, k, v, ck, None, None, 0.6, SEED_B)
    grads_b = dc.grad_dropout_heads(indptr, indices, vals, q, k, v, g, ck, None, None, 0.6, SEED_B)[:3]
    for a in (indptr, indices, vals, q, k, v, g, bias, out_a, out_b) + grads_a + grads_b:
        a.setflags(write=False)
    return indptr, indices, vals, shape, q, k, v, g, bias, out_a, grads_a, out_b, grads_b


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_listed_lengths_bit_for_bit_in_every_layout(dtype, idx, chunk, monkeypatch):
    """forward and backward, with a bias and a scale at rate 0.1 and with neither at rate 0.6, NumPy and torch operands; the
    short / wide switch at 64 / 65, the wide / long switch at chunk / chunk + 1, rows of 2 and 5 pieces, empty rows; a COO, a
    CSR, a CSC and a COO built unsorted of one pattern give identical bits, the CSC's dbias and keep mask in the caller's order"""
    import sparse_amd

    case = _lengths_case(chunk, np.dtype(dtype))
    _chunk(monkeypatch, chunk)
    indptr, indices, vals, shape, q, k, v, g, bias, out_a, grads_a, out_b, grads_b = case
    ptr_i, ind_i = indptr.astype(idx), indices.astype(idx)
    nnz = len(indices)
    keep_b = dc.keep_restated(nnz, 2, 0.6, SEED_B)

    def check(s, b_head, order=None):
        """`order`: the caller's order of `s.data` as positions of the canonical order (dbias and the keep mask come in it)"""
        got = sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=b_head, dropout=0.1, seed=SEED_A)
        assert isinstance(got, np.ndarray) and sc.same_bits(got, out_a)
        assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, dropout=0.6, seed=SEED_B), out_b)
        gr = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=b_head, dropout=0.1, seed=SEED_A)
        assert len(gr) == 4 and gr[3].shape == LEAD + (nnz,) and all(isinstance(a, np.ndarray) for a in gr)
        assert _same(gr[:3], grads_a[:3])
        assert sc.same_bits(gr[3], grads_a[3] if order is None else grads_a[3][..., order])
        gr = sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.6, seed=SEED_B)
        assert len(gr) == 3 and _same(gr, grads_b)
        mask = sparse_amd.sparse_attention_keep_mask(s, LEAD, dropout=0.6, seed=SEED_B)
        assert mask.dtype == torch.bool and mask.shape == LEAD + (nnz,) and mask.device == torch.device(DEV)
        assert np.array_equal(_np(mask), keep_b if order is None else keep_b[..., order])

    coo = _coo(ptr_i, ind_i, vals, shape, idx)
    check(coo, bias)
    x = _csr(ptr_i, ind_i, vals, shape)
    check(x, bias)
    tq, tk, tv, tg, tb = _dev(q, k, v, g, bias)
    tout = sparse_amd.sparse_attention(x, tq, tk, tv, scale=0.3, bias=tb, dropout=0.1, seed=SEED_A)
    assert isinstance(tout, torch.Tensor) and sc.same_bits(_np(tout), out_a)
    tgr = sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg, scale=0.3, bias=tb, dropout=0.1, seed=SEED_A)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tgr) and _same(tgr, grads_a)
    xc = coo.asformat("gcxs", compressed_axes=(1,))
    order = gc.column_order(indptr, indices)[0]
    assert np.array_equal(_np(xc.data), vals[order])
    check(xc, np.ascontiguousarray(bias[..., order]), order)
    perm = np.random.default_rng(5).permutation(nnz)
    un = sparse_amd.COO(ac.coords_of(indptr, indices)[:, perm].astype(idx), vals[perm], shape=shape, idx_dtype=idx, device=DEV)
    assert np.array_equal(_np(un.data), vals)
    check(un, bias)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_columns_bit_for_bit(dtype, monkeypatch):
    """the listed lengths as COLUMN lengths at chunk 64: the column pass in all its forms reads the pd and y of the row pass"""
    import sparse_amd

    indptr, indices, vals, shape, q, k, v, g, bias, out_a, grads_a, out_b, grads_b = _lengths_case(64, np.dtype(dtype), True)
    _chunk(monkeypatch, 64)
    s = _coo(indptr, indices, vals, shape)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias, dropout=0.1, seed=SEED_A), out_a)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias, dropout=0.1, seed=SEED_A), grads_a)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, dropout=0.6, seed=SEED_B), out_b)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.6, seed=SEED_B), grads_b)


# ---- widths and heads -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Dv", [(1, 1), (17, 5), (64, 64), (130, 65)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_widths(dtype, D, Dv):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(350, ac.SHORT_LENGTHS, dtype)
    q, k, v = ac.operands(351 + D, shape, D, Dv, dtype)
    g = gc.grad_operand(352 + Dv, shape, Dv, dtype)
    s = _coo(indptr, indices, vals, shape)
    rate = 0.1 if D in (1, 64) else 0.6
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, dropout=rate, seed=5),
                        dc.attention_dropout_restated(indptr, indices, vals, q, k, v, 1024, None, None, rate, 5)[0])
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=rate, seed=5),
                 dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 1024, None, None, rate, 5)[:3])


@pytest.mark.parametrize("kind", ["none", "per-head", "shared"])
@pytest.mark.parametrize("lead", [(), (3,), (2, 2)])
def test_heads(lead, kind):
    """the head's number is its index in the flattened leading axes; without a bias, with one per head, with a shared one"""
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(360, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(361, shape, 20, 9, np.float32, lead=lead)
    g = gc.grad_operand(362, shape, 9, np.float32, lead=lead)
    bias = None if kind == "none" else bc.bias_of(363, len(indices), np.float32, None if kind == "shared" else lead)
    rate, scale = (0.6, 0.5) if kind != "shared" else (0.1, None)
    s = _coo(indptr, indices, vals, shape)
    want = dc.attention_dropout_heads(indptr, indices, vals, q, k, v, 1024, scale, bias, rate, SEED_A)
    gwant = dc.grad_dropout_heads(indptr, indices, vals, q, k, v, g, 1024, scale, bias, rate, SEED_A)[:3 if bias is None else 4]
    got = sparse_amd.sparse_attention(s, q, k, v, scale=scale, bias=bias, dropout=rate, seed=SEED_A)
    ggot = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale, bias=bias, dropout=rate, seed=SEED_A)
    assert got.shape == lead + (shape[0], 9) and sc.same_bits(got, want) and _same(ggot, gwant)
    mask = sparse_amd.sparse_attention_keep_mask(s, lead, dropout=rate, seed=SEED_A)
    H = int(np.prod(lead, dtype=np.int64))
    assert mask.shape == lead + (len(indices),) and np.array_equal(_np(mask).reshape(H, -1), dc.keep_restated(len(indices), H, rate, SEED_A))
    if len(lead) == 1:
        assert np.array_equal(_np(sparse_amd.sparse_attention_keep_mask(s, lead[0], dropout=rate, seed=SEED_A)), _np(mask))
    tq, tk, tv, tg = _dev(q, k, v, g)
    tb = None if bias is None else _dev(bias)[0]
    assert sc.same_bits(_np(sparse_amd.sparse_attention(s, tq, tk, tv, scale=scale, bias=tb, dropout=rate, seed=SEED_A)), want)
    assert _same(sparse_amd.sparse_attention_grad(s, tq, tk, tv, tg, scale=scale, bias=tb, dropout=rate, seed=SEED_A), gwant)


# ---- every form against every other -------------------------------------------------------------------------------------------------
def _plan_np(indptr, indices, N):
    perm, rows, cols = gc.column_order(indptr, indices)
    return np.searchsorted(cols, np.arange(N + 1)), perm, rows


@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_groups_and_chunks_change_no_bit(dtype, idx):
    from sparse_amd import _kernels as K

    def runs(lengths, seed, variants, lead=(2,), biased=True, rate=0.6, restate=None):
        """every variant against the first; `restate`: a chunk at which the first is held to the restatement too"""
        indptr, indices, vals, shape = ac.csr_mask(seed, lengths, dtype)
        q, k, v = ac.operands(seed + 1, shape, 21, 6, dtype, lead=lead)
        g = gc.grad_operand(seed + 2, shape, 6, dtype, lead=lead)
        bias = bc.bias_of(seed + 3, len(indices), dtype, lead) if biased else None
        cptr, cperm, crow = _plan_np(indptr, indices, shape[1])
        ti = lambda a, t=idx: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(t)      # noqa: E731
        csr = (ti(indptr), ti(indices), torch.from_numpy(vals).to(DEV))
        plan = (ti(cptr), ti(cperm, torch.int64), ti(crow))
        tq, tk, tv, tg = _dev(q, k, v, g)
        tb = _dev(bias)[0] if biased else None
        max_row, max_col = int(np.diff(indptr).max()), int(np.diff(cptr).max())
        outs = {}
        for kw in variants:
            fkw = {a: b for a, b in kw.items() if a != "col_group"}
            fwd = K.attention_rows(*csr, tq, tk, tv, max_row, scale=0.7, bias=tb, dropout=rate, seed=SEED_B, **fkw)
            bwd = K.attention_grad_rows(*csr, *plan, tq, tk, tv, tg, max_row, max_col, scale=0.7, bias=tb, want_dbias=True, dropout=rate,
                                        seed=SEED_B, **kw)
            outs[str(kw)] = [_np(fwd)] + [_np(t) for t in bwd]
        first = next(iter(outs.values()))
        assert all(_same(o, first) for o in outs.values()), [name for name, o in outs.items() if not _same(o, first)]
        if restate is not None:
            want = [dc.attention_dropout_heads(indptr, indices, vals, q, k, v, restate, 0.7, bias, rate, SEED_B)]
            want += list(dc.grad_dropout_heads(indptr, indices, vals, q, k, v, g, restate, 0.7, bias, rate, SEED_B))
            assert _same(first, want[:len(first)])

    widths = [dict(group=a, col_group=b) for a, b in zip(K.ATTENTION_GROUPS, K.ATTENTION_GROUPS[::-1])]
    short = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 5]
    variants = [dict(form="short", **w) for w in widths] + [dict(form="wide", chunk=c) for c in (64, 1024)]
    variants += [dict(form="long"), dict(), dict(group=8, col_group=8), dict(group=64, col_group=64, chunk=128), dict(short_max=16),
                 dict(short_max=0, group=32, col_group=32)]
    for biased, rate in ((True, 0.6), (False, 0.1)):
        runs(short, 371, variants, biased=biased, rate=rate, restate=64)
    mid = short + [65, 100, 127, 128]
    variants = [dict(form="wide", chunk=c) for c in (128, 1024)] + [dict(chunk=c, **w) for w in widths for c in (128, 256)]
    variants += [dict(form="long", chunk=128)]
    runs(mid, 372, variants)
    long_ = mid + [129, 191, 192, 193, 64 * 5, 640]
    for chunk in (64, 128):
        variants = [dict(form="long", chunk=chunk)] + [dict(chunk=chunk, **w) for w in widths]
        runs(long_, 373, variants, lead=(), biased=chunk == 128, rate=0.1 if chunk == 128 else 0.6, restate=chunk)


# ---- no dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_dropout_reaches_the_entries_without_it(dtype, monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    indptr, indices, vals, shape = ac.csr_mask(380, sc.listed_lengths(64), dtype)
    q, k, v = ac.operands(381, shape, 17, 5, dtype, lead=(2,))
    g = gc.grad_operand(382, shape, 5, dtype, lead=(2,))
    bias = bc.bias_of(383, len(indices), dtype)
    s = _coo(indptr, indices, vals, shape)
    plain = sparse_amd.sparse_attention(s, q, k, v, scale=0.3)
    gplain = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3)
    biased = sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias)
    gbiased = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias)
    names = []
    real = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *a: names.append(name) or real(name, *a))
    for kw in (dict(dropout=None), dict(dropout=0.0, seed=None), dict(dropout=0, seed=3), dict(dropout=None, seed=3), dict(dropout=np.float32(0))):
        assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, **kw), plain)
        assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, **kw), gplain)
        assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias, **kw), biased)
        assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias, **kw), gbiased)
    assert {"spamd_attention", "spamd_attention_grad", "spamd_attention_bias", "spamd_attention_grad_bias"} <= set(names)
    assert not any("dropout" in n or "keep" in n for n in names)
    assert _np(sparse_amd.sparse_attention_keep_mask(s, (2,), dropout=0.0, seed=None)).all() and not any("keep" in n for n in names)
    del names[:]
    sparse_amd.sparse_attention(s, q, k, v, dropout=0.5, seed=1)
    sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.5, seed=1)
    assert "spamd_attention_dropout" in names and "spamd_attention_grad_dropout" in names and "spamd_attention" not in names
    # the new C entries at rate 0 have those bits too (the Python layers never send a rate of 0 there: made to, here)
    del names[:]
    monkeypatch.setattr(K, "_dropout_args", lambda dropout, seed, what: (0.0, 0))
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3), plain)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3), gplain)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, scale=0.3, bias=bias), biased)
    assert _same(sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.3, bias=bias), gbiased)
    assert names.count("spamd_attention_dropout") == 2 and names.count("spamd_attention_grad_dropout") == 2


def test_more_heads_than_one_launch():
    """65 537 heads over a 2 x 2 mask, D = Dv = 1: the head's number goes on across the launches of 65 535 heads - head 65 536
    has its own decisions, not head 1's or head 0's"""
    import sparse_amd

    H, rate, seed = 65537, 0.6, 21
    indptr, indices = np.array([0, 2, 4]), np.array([0, 1, 0, 1])
    vals = np.array([1.0, -0.5, 0.75, 1.25], np.float32)
    rng = np.random.default_rng(390)
    q, k, v, g = (rng.standard_normal((H, 2, 1)).astype(np.float32) for _ in range(4))
    keep = dc.keep_restated(4, H, rate, seed)
    assert (keep[65536] != keep[0]).any() and (keep[65536] != keep[1]).any() and (keep[65535] != keep[0]).any()      # (chosen on the CPU)
    s = _coo(indptr, indices, vals, (2, 2))
    tq, tk, tv, tg = _dev(q, k, v, g)
    mask = sparse_amd.sparse_attention_keep_mask(s, (H,), dropout=rate, seed=seed)
    assert np.array_equal(_np(mask), keep)
    out = _np(sparse_amd.sparse_attention(s, tq, tk, tv, dropout=rate, seed=seed))
    grads = [_np(t) for t in sparse_amd.sparse_attention_grad(s, tq, tk, tv, tg, dropout=rate, seed=seed)]
    # a row is +0.0 exactly where both its elements are dropped (p > 0 and v != 0 everywhere)
    assert np.array_equal(out[:, :, 0] == 0, ~keep.reshape(H, 2, 2).any(axis=2))
    for h in (0, 1, 2, 65534, 65535, 65536):
        want = dc.attention_dropout_restated(indptr, indices, vals, q[h], k[h], v[h], 1024, None, None, rate, seed, head=h)[0]
        gwant = dc.grad_dropout_restated(indptr, indices, vals, q[h], k[h], v[h], g[h], 1024, None, None, rate, seed, head=h)[:3]
        assert sc.same_bits(out[h], want) and _same([a[h] for a in grads], gwant), h


def test_a_second_seed():
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(400, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = _dev(*ac.operands(401, shape, 16, 8, np.float32, lead=(2,)))
    g, = _dev(gc.grad_operand(402, shape, 8, np.float32, lead=(2,)))
    s = _coo(indptr, indices, vals, shape)
    one = sparse_amd.sparse_attention(s, q, k, v, dropout=0.1, seed=1)
    gone = sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.1, seed=1)
    assert torch.equal(one, sparse_amd.sparse_attention(s, q, k, v, dropout=0.1, seed=1))
    assert all(torch.equal(a, b) for a, b in zip(gone, sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.1, seed=1)))
    m1 = sparse_amd.sparse_attention_keep_mask(s, (2,), dropout=0.1, seed=1)
    m2 = sparse_amd.sparse_attention_keep_mask(s, (2,), dropout=0.1, seed=2)
    assert not torch.equal(m1, m2) and (dc.keep_restated(len(indices), 2, 0.1, 1) != dc.keep_restated(len(indices), 2, 0.1, 2)).any()
    two = sparse_amd.sparse_attention(s, q, k, v, dropout=0.1, seed=2)
    assert not torch.equal(one, two)
    assert not torch.equal(gone[2], sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.1, seed=2)[2])


def test_keep_mask_against_the_result():
    """seed 2 at rate 0.6 keeps, of the positions 0 .. 7 of head 0, position 5 alone (chosen on the CPU): a row of 5 that is
    dropped entirely is +0.0, a row of 3 with one element kept is c * p_kept * v[col] to the bit, and dv has no contribution
    where the mask is False"""
    import sparse_amd

    dtype = np.dtype(np.float32)
    indptr, indices, vals, shape = ac.csr_mask(410, [5, 3], dtype, ncols=12)
    q, k, v = ac.operands(411, shape, 9, 4, dtype)
    g = gc.grad_operand(412, shape, 4, dtype)
    s = _coo(indptr, indices, vals, shape)
    mask = _np(sparse_amd.sparse_attention_keep_mask(s, dropout=0.6, seed=2))
    assert mask.shape == (8,) and mask.tolist() == [False] * 5 + [True, False, False]
    out = sparse_amd.sparse_attention(s, q, k, v, dropout=0.6, seed=2)
    p = ac.attention_restated(indptr, indices, vals, q, k, v, 1024)[2]
    c = dc.c_of(0.6, dtype)
    assert (out[0] == 0).all() and not np.signbit(out[0]).any()
    assert sc.same_bits(out[1], sc._fma(dtype)(np.broadcast_to(p[5] * c, (4,)), v[indices[5]], np.zeros(4, dtype)).astype(dtype))
    dq, dk, dv = sparse_amd.sparse_attention_grad(s, q, k, v, g, dropout=0.6, seed=2)
    want_dv = np.zeros_like(v)
    want_dv[indices[5]] = sc._fma(dtype)(np.broadcast_to(p[5] * c, (4,)), g[1], np.zeros(4, dtype))
    assert sc.same_bits(dv, want_dv) and (dq[0] == 0).all()
    # one row, all but one element dropped, in the wave form too: seed 1 at rate 0.96 keeps one of 70 (chosen on the CPU)
    n, seed = 70, 1
    keep = dc.keep_restated(n, 1, 0.96, seed)[0]
    assert keep.sum() == 1
    indptr, indices, vals, shape = ac.csr_mask(413, [n], dtype)
    q, k, v = ac.operands(414, shape, 9, 4, dtype)
    s = _coo(indptr, indices, vals, shape)
    assert np.array_equal(_np(sparse_amd.sparse_attention_keep_mask(s, dropout=0.96, seed=seed)), keep)
    p = ac.attention_restated(indptr, indices, vals, q, k, v, 1024)[2]
    i = int(np.flatnonzero(keep)[0])
    want = sc._fma(dtype)(np.broadcast_to(p[i] * dc.c_of(0.96, dtype), (4,)), v[indices[i]], np.zeros(4, dtype)).astype(dtype)
    assert sc.same_bits(sparse_amd.sparse_attention(s, q, k, v, dropout=0.96, seed=seed)[0], want)


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("biased", [False, True], ids=["no-bias", "bias"])
def test_autograd_function_has_the_bits_of_both_calls(biased):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(420, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(421, shape, 12, 7, np.float32, lead=(3,))
    g = gc.grad_operand(422, shape, 7, np.float32, lead=(3,))
    s = _coo(indptr, indices, vals, shape)
    tq, tk, tv, tg = _dev(q, k, v, g)
    tb = _dev(bc.bias_of(423, len(indices), np.float32, (3,)))[0].requires_grad_() if biased else None
    tq.requires_grad_()
    tv.requires_grad_()
    kw = dict(scale=0.4, dropout=0.6, seed=SEED_A)
    out = sparse_amd.sparse_attention_autograd(s, tq, tk, tv, bias=tb, **kw)
    db = None if tb is None else tb.detach()
    assert out.requires_grad and torch.equal(out.detach(), sparse_amd.sparse_attention(s, tq.detach(), tk, tv.detach(), bias=db, **kw))
    assert not torch.equal(out.detach(), sparse_amd.sparse_attention(s, tq.detach(), tk, tv.detach(), bias=db, scale=0.4))
    out.backward(tg)
    grads = sparse_amd.sparse_attention_grad(s, tq.detach(), tk, tv.detach(), tg, bias=db, **kw)
    assert torch.equal(tq.grad, grads[0]) and tk.grad is None and torch.equal(tv.grad, grads[2])      # the backward drops what the forward dropped
    if biased:
        assert torch.equal(tb.grad, grads[3])
    with pytest.raises(ValueError, match="no hidden global generator"):
        sparse_amd.sparse_attention_autograd(s, tq, tk, tv, dropout=0.5)


@pytest.mark.parametrize("rate,biased", [(0.6, True), (0.1, False)])
def test_gradcheck(rate, biased, monkeypatch):
    """float64, rows of 0, 1, 9 and 70 elements at chunk 64 (an empty row, the sub-group form, and two pieces), D = 3, Dv = 2, two
    heads, a fixed seed; q, k, v and the bias all require gradients; torch's own default tolerances"""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    indptr, indices, vals, shape = ac.csr_mask(430, [0, 1, 9, 70], np.float64)
    s = _coo(indptr, indices, vals, shape)
    tq, tk, tv = (t.requires_grad_() for t in _dev(*ac.operands(431, shape, 3, 2, np.float64, lead=(2,))))
    keep = dc.keep_restated(len(indices), 2, rate, 17)
    assert 0 < keep.sum() < keep.size
    if biased:
        tb = _dev(bc.bias_of(432, len(indices), np.float64, (2,), spread=0.5))[0].requires_grad_()
        fn = lambda a, b, c, d: sparse_amd.sparse_attention_autograd(s, a, b, c, scale=0.7, bias=d, dropout=rate, seed=17)   # noqa: E731
        assert torch.autograd.gradcheck(fn, (tq, tk, tv, tb))
    else:
        fn = lambda a, b, c: sparse_amd.sparse_attention_autograd(s, a, b, c, scale=0.7, dropout=rate, seed=17)               # noqa: E731
        assert torch.autograd.gradcheck(fn, (tq, tk, tv))


# ---- caches -----------------------------------------------------------------------------------------------------------------------------
def test_second_call_builds_no_plan_and_no_permutation(monkeypatch):
    import sparse_amd
    from sparse_amd import _kernels as K

    swaps = []
    real = K._csc_to_csr
    monkeypatch.setattr(K, "_csc_to_csr", lambda *a: swaps.append(1) or real(*a))
    indptr, indices, vals, shape = ac.csr_mask(440, ac.SHORT_LENGTHS + [1500], np.float32)
    q, k, v = ac.operands(441, shape, 16, 8, np.float32)
    g = gc.grad_operand(442, shape, 8, np.float32)
    order = gc.column_order(indptr, indices)[0]
    tq, tk, tv, tg = _dev(q, k, v, g)
    want = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 1024, None, None, 0.1, 9)[:3]
    xc = _coo(indptr, indices, vals, shape).asformat("gcxs", compressed_axes=(1,))
    first = sparse_amd.sparse_attention_grad(xc, tq, tk, tv, tg, dropout=0.1, seed=9)
    m1 = sparse_amd.sparse_attention_keep_mask(xc, dropout=0.1, seed=9)
    n = len(swaps)
    assert 1 <= n <= 2                                                  # the twin and the permutation
    perm, plan, gplan = xc._attention_bias_perm, xc._attention_plan, xc._attention_grad_plan
    second = sparse_amd.sparse_attention_grad(xc, tq, tk, tv, tg, dropout=0.1, seed=9)
    sparse_amd.sparse_attention(xc, tq, tk, tv, dropout=0.1, seed=9)
    m2 = sparse_amd.sparse_attention_keep_mask(xc, dropout=0.1, seed=9)
    assert len(swaps) == n and xc._attention_bias_perm is perm and xc._attention_plan is plan and xc._attention_grad_plan is gplan
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(m1, m2) and _same(first, want)
    assert np.array_equal(_np(m1), dc.keep_restated(len(indices), 1, 0.1, 9)[0][order])

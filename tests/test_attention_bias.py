"""The additive bias of sparse_attention without a GPU: the two C entries and the public keyword are in place, the argument checks
of both layers return before any launch or device, and the NumPy restatement (tests/attention_bias_cases.py) - which judges the
kernels bit for bit in tests/test_attention_bias_gpu.py - stays within its derived bounds of a longdouble computation and of a
dense float64 attention, and has the facts the order of the contract promises."""
import inspect

import numpy as np
import pytest

import attention_bias_cases as bc
import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc

WIDTHS = [(1, 1), (17, 5), (64, 64), (130, 65)]                       # `test_attention.WIDTHS`
LENGTHS = [0, 1, 2, 3, 7, 31, 63, 64, 65, 100, 128, 129, 200, 0]


def test_c_abi_and_public_keyword(hiplib):
    import sparse_amd
    from sparse_amd import _dot, _ffi, _kernels as K

    for name in ("spamd_attention_bias", "spamd_attention_grad_bias"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_attention_bias"][1]) == 32 and len(_ffi.SIGNATURES["spamd_attention_grad_bias"][1]) == 43
    assert len(_ffi.SIGNATURES["spamd_attention"][1]) == 30 and len(_ffi.SIGNATURES["spamd_attention_grad"][1]) == 40
    for f in (sparse_amd.sparse_attention, sparse_amd.sparse_attention_grad, sparse_amd.sparse_attention_autograd, K.attention_rows,
              K.attention_grad_rows):
        p = inspect.signature(f).parameters["bias"]
        assert p.default is None and p.kind is p.KEYWORD_ONLY
    assert inspect.signature(K.attention_grad_rows).parameters["want_dbias"].default is False
    assert "_attention_bias_perm" in _dot.DERIVED_CACHES


def test_argument_checks_of_the_c_entries_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch (the lists of tests/test_attention.py and
    tests/test_attention_grad.py, and bias_head = -1)"""
    from sparse_amd import _ffi

    x = 64                                                             # a pointer that is never read

    def fwd(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, short_max=64, chunk=64,
            max_len=100, ws_bytes=0, bias=None, bias_head=200):
        return hiplib.spamd_attention_bias(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, pitch, head, None, pitch, head, None,
                                           pitch, head, 0, 1.0, group, short_max, chunk, max_len, bias, bias_head, None, ws_bytes, None,
                                           None)

    def bwd(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, col_group=16, short_max=64,
            chunk=64, max_row=100, max_col=100, ws_bytes=0, bias=None, bias_head=200, dbias=None):
        return hiplib.spamd_attention_grad_bias(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, None, None, None, pitch, head,
                                                None, pitch, head, None, pitch, head, None, pitch, head, 0, 1.0, group, col_group,
                                                short_max, chunk, max_row, max_col, bias, bias_head, dbias, None, ws_bytes, None, None,
                                                None, None)

    for call, lens in ((fwd, ("max_len",)), (bwd, ("max_row", "max_col"))):
        for bias in (None, x):
            kw = dict(bias=bias)
            assert call(val=_ffi.I32, **kw) == -2 and call(val=_ffi.C64, **kw) == -2 and call(val=_ffi.F16, **kw) == -2
            assert call(val=_ffi.BF16, **kw) == -2 and call(idx=_ffi.F32, **kw) == -2 and call(idx=_ffi.U8, **kw) == -2
            for name in ("M", "N", "nnz", "H", "D", "Dv", "pitch", "head", "bias_head") + lens:
                assert call(**{name: -1}, **kw) == -1, name
            for name in lens:
                assert call(**{name: 201}, **kw) == -1
            for name in ("group",) + (("col_group",) if call is bwd else ()):
                assert call(**{name: 0}, **kw) == -1 and call(**{name: 12}, **kw) == -1 and call(**{name: 128}, **kw) == -1
            assert call(chunk=0, **kw) == -1 and call(chunk=32, **kw) == -1 and call(chunk=100, **kw) == -1 and call(chunk=2048, **kw) == -1
            assert call(short_max=-1, **kw) == -1 and call(short_max=65, **kw) == -1
            assert call(H=0, **kw) == 0                                 # nothing to do
            assert call(**kw) == -1                                     # null pointers with work to do
    assert fwd(M=0) == 0 and fwd(Dv=0) == 0 and fwd(bias_head=0, H=0) == 0
    assert bwd(D=0, Dv=0) == 0 and bwd(M=0, N=0, nnz=0, max_row=0, max_col=0, bias=x, dbias=x) == 0
    # a workspace that is too small, every pointer given: the check comes before any launch, with and without a bias
    need_f = hiplib.spamd_attention_ws_bytes(_ffi.F32, 200, 2, 6, 64)
    need_b = hiplib.spamd_attention_grad_ws_bytes(_ffi.F32, 200, 2, 5, 6, 64)
    assert need_f > 0 and need_b > 0
    for bias, dbias in ((None, None), (x, None), (x, x)):
        small_f = lambda ws, n: hiplib.spamd_attention_bias(_ffi.F32, _ffi.I64, 3, 4, 200, 2, 5, 6, x, x, x, x, 8, 64, x, 8, 64, x, 8, 64, 0, 1.0,   # noqa: E731
                                                            16, 64, 64, 100, bias, 200, ws, n, x, None)
        small_b = lambda ws, n: hiplib.spamd_attention_grad_bias(_ffi.F32, _ffi.I64, 3, 4, 200, 2, 5, 6, x, x, x, x, x, x, x, 8, 64, x, 8, 64,      # noqa: E731
                                                                 x, 8, 64, x, 8, 64, 0, 1.0, 16, 16, 64, 64, 100, 100, bias, 200, dbias, ws, n,
                                                                 x, x, x, None)
        assert small_f(x, need_f - 1) == -3 and small_f(None, need_f) == -3
        assert small_b(x, need_b - 1) == -3 and small_b(x, 0) == -3 and small_b(None, need_b) == -3


def test_python_argument_errors():
    """everything that is wrong with a bias raises before a device is touched: the checks need the mask's nnz only"""
    import torch

    import sparse_amd
    from sparse_amd._attention import _check_bias as check

    f32 = torch.float32
    for lead in ((), (3,), (2, 2)):
        for ok in (np.zeros(7, np.float32), np.zeros(lead + (7,), np.float32), torch.zeros(lead + (7,)), torch.zeros(3, 14)[..., ::2][:1].expand(lead + (7,)) if lead else torch.zeros(14)[::2]):
            check(ok, f32, lead, 7)
    check(None, f32, (3,), 7)
    check(np.zeros((2, 0)), torch.float64, (2,), 0)                    # nnz == 0: the early return still validates
    for bad in ([0.0] * 7, 1.0, "bias", (np.zeros(7, np.float32),)):
        with pytest.raises(TypeError, match="NumPy array or a torch tensor"):
            check(bad, f32, (), 7)

    class Sparse:                                                      # (any array that is neither kind: a sparse one too)
        shape, dtype = (7,), np.dtype("float32")

    with pytest.raises(TypeError, match="sparse"):
        check(Sparse(), f32, (), 7)
    for bad in (np.zeros(7), np.zeros(7, np.float16), np.zeros(7, np.int32), np.zeros(7, np.complex64), torch.zeros(7, dtype=torch.float64),
                torch.zeros(7, dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match="not converted"):
            check(bad, f32, (), 7)
    with pytest.raises(TypeError, match="not converted"):
        check(np.zeros(7, np.float32), torch.float64, (), 7)
    for lead, shape in (((), (8,)), ((), (1, 7)), ((3,), (2, 7)), ((3,), (3, 8)), ((3,), (1, 7)), ((2, 2), (4, 7)), ((2, 2), (2, 7)), ((3,), (5, 6)),
                        ((), ())):
        with pytest.raises(ValueError, match="shape-mismatch"):
            check(np.zeros(shape, np.float32), f32, lead, 7)
    with pytest.raises(ValueError, match="shape-mismatch"):
        check(np.zeros(1, np.float32), f32, (), 0)
    with pytest.raises(TypeError, match="torch tensor"):
        sparse_amd.sparse_attention_autograd(None, torch.zeros(5, 4), torch.zeros(6, 4), torch.zeros(6, 3), bias=np.zeros(3, np.float32))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D,Dv", WIDTHS)
def test_restatement_stays_within_its_bounds(dtype, D, Dv):
    """row lengths 0 to 200 at chunk 64, with a scale, a bias of 1.5 standard deviations: the biased scores against
    s scale (q . k) + b in longdouble within the derived bound, the output against the exact attention of the ROUNDED biased
    scores, and against a dense float64 softmax(scale s (q k^T) + B, -inf elsewhere) @ v within `other_form_bound` with the
    biased score bound, plus the dense value's own rounding, 4 eps"""
    indptr, indices, vals, shape = ac.csr_mask(100 + D, LENGTHS, dtype)
    q, k, v = ac.operands(200 + Dv, shape, D, Dv, dtype)
    bias = bc.bias_of(300 + D, len(indices), dtype)
    scale = D ** -0.5
    out, t, p = bc.attention_bias_restated(indptr, indices, vals, q, k, v, 64, scale, bias)
    want, bound = bc.biased_score_exact_and_bound(indptr, indices, vals, q, k, bias, scale)
    s_share = ac.share(t, want, bound)
    owant, obound, _ = ac.output_exact_and_bound(indptr, indices, t, v)
    o_share = ac.share(out, owant, obound)
    assert not np.isnan(bound).any() and not np.isnan(obound).any() and s_share <= 1 and o_share <= 1
    dense = bc.dense_attention64(indptr, indices, vals, q, k, v, bias, scale)
    _, fbound = bc.other_form_bound(indptr, indices, vals, q, k, v, t, bias, scale)
    dbound = fbound + 4 * np.finfo(np.float64).eps * np.abs(dense)
    d_share = ac.share(out, dense.astype(ac.LD), dbound)               # (the rows without an element: 0 in both, no bound)
    assert (np.abs(out.astype(ac.LD) - dense) <= dbound).all()
    assert d_share <= 1 and (out[0] == 0).all() and (out[-1] == 0).all() and not np.signbit(out[0]).any()
    print(f"attention bias restated {np.dtype(dtype)} D {D} Dv {Dv}: largest share of the biased score bound {s_share:.3f}, of the "
          f"output bound {o_share:.3f}, of the dense bound {d_share:.3f}")
    assert 0 < o_share and 0 < s_share


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_consequences_of_the_order(dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(9)
    indptr, indices, vals, shape = ac.csr_mask(30, LENGTHS, dtype)
    vals[::5] = 0                                                       # scores of +0.0 and -0.0
    q, k, v = ac.operands(31, shape, 17, 6, dtype, spread=2.0)
    g = gc.grad_operand(32, shape, 6, dtype)
    nnz = len(indices)
    # a bias of +0.0 everywhere: the bits of the restatement without a bias (`t + 0.0` changes the sign of a zero score only)
    for scale in (None, 0.4):
        plain = ac.attention_restated(indptr, indices, vals, q, k, v, 64, scale)
        zero = bc.attention_bias_restated(indptr, indices, vals, q, k, v, 64, scale, np.zeros(nnz, dtype))
        assert sc.same_bits(zero[0], plain[0]) and sc.same_bits(zero[2], plain[2]) and (zero[1] == plain[1]).all()
        assert sc.same_bits(bc.attention_bias_restated(indptr, indices, vals, q, k, v, 64, scale, None)[0], plain[0])
        gplain = gc.grad_restated(indptr, indices, vals, q, k, v, g, 64, scale)
        gzero = bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 64, scale, np.zeros(nnz, dtype))
        assert all(sc.same_bits(a, b) for a, b in zip(gzero[:3], gplain[:3]))
    assert np.signbit(plain[1]).any() and (plain[1] == 0).any() and not np.signbit(zero[1][zero[1] == 0]).any()
    # one stored element returns v[c] whatever its finite bias
    one = lambda cols, sv, b, chunk=64: bc.row_attention_bias(np.asarray(sv, dtype), np.asarray(cols), q[0], k, v, chunk, None, np.asarray(b, dtype))   # noqa: E731
    for c, b in ((0, 0.0), (7, -1e30), (200, 3e4), (3, np.finfo(dtype).max)):
        out, t, p = one([c], [rng.standard_normal()], [b])
        assert p[0] == 1 and sc.same_bits(out, v[c])
    # -inf on the trailing elements of a row of at most `chunk` elements: the bits of the shorter row
    cols = np.sort(rng.choice(shape[1], 64, replace=False))
    sv = rng.uniform(0.5, 1.5, 64)
    b = (rng.standard_normal(64) * 1.5).astype(dtype)
    for n, cut in ((2, 1), (9, 4), (33, 32), (64, 1), (64, 63)):
        bb = b[:n].copy()
        bb[n - cut:] = -np.inf
        full, short = one(cols[:n], sv[:n], bb), one(cols[:n - cut], sv[:n - cut], b[:n - cut])
        assert sc.same_bits(full[0], short[0]) and sc.same_bits(full[2][:n - cut], short[2]) and not full[2][n - cut:].any()
        assert not np.signbit(full[2][n - cut:]).any()                  # p = +0.0
    # ... -inf in the middle is a mask too (p = +0.0), but the positions after it meet other accumulators: no bit promise
    bb = b.copy()
    bb[10:20] = -np.inf
    out, t, p = one(cols, sv, bb)
    assert not p[10:20].any() and abs(p.sum() - 1) < 64 * np.finfo(dtype).eps
    # an all -inf row is NaN; so is a NaN or a +inf bias
    for bad in (np.full(5, -np.inf), [0, np.nan, 0, 0, 0], [0, 0, np.inf, 0, 0]):
        assert np.isnan(one(cols[:5], sv[:5], bad)[0]).all()
    # dbias is z: the rows of z sum to about zero (sum p (e - delta)), and a masked element has z = 0
    bias = bc.bias_of(33, nnz, dtype, neg_inf=0.2)
    bias[indptr[:-1][np.diff(indptr) > 0]] = 0.5
    z = bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 64, 0.4, bias)[3]
    assert not z[np.isinf(bias)].any() and np.isfinite(z).all() and z.any()
    sums = np.add.reduceat(z.astype(np.float64), indptr[:-1][np.diff(indptr) > 0])
    assert np.abs(sums).max() < 1000 * np.finfo(dtype).eps * np.abs(g).max() * np.abs(v).max() * 6


def test_grad_restated_against_central_differences():
    """float64: dq, dk, dv and dbias of `grad_bias_restated` against central differences of the restated forward, loss =
    sum(out * g); rows of 0, 1, 9 and 70 elements at chunk 64"""
    indptr, indices, vals, shape = ac.csr_mask(40, [0, 1, 9, 70, 3], np.float64)
    q, k, v = ac.operands(41, shape, 3, 2, np.float64)
    g = gc.grad_operand(42, shape, 2, np.float64)
    bias = bc.bias_of(43, len(indices), np.float64, spread=0.5)
    dq, dk, dv, db = bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 64, 0.7, bias)

    def loss(q_, k_, v_, b_):
        return float((bc.attention_bias_restated(indptr, indices, vals, q_, k_, v_, 64, 0.7, b_)[0] * g).sum())

    rng = np.random.default_rng(44)
    h = 1e-6
    for which, grad in enumerate((dq, dk, dv, db)):
        flat = np.flatnonzero(np.ones(grad.shape))
        for i in rng.choice(flat, min(len(flat), 25), replace=False):
            args = [q.copy(), k.copy(), v.copy(), bias.copy()]
            args[which].flat[i] += h
            up = loss(*args)
            args[which].flat[i] -= 2 * h
            num = (up - loss(*args)) / (2 * h)
            assert abs(num - grad.flat[i]) <= 1e-7 * max(1.0, abs(num)), (which, i, num, grad.flat[i])
    assert db.any() and abs(db[indptr[1]:indptr[2]]).max() == 0        # a row of one element: p = 1 whatever the bias

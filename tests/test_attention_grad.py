"""sparse_attention_grad without a GPU: the C ABI and the public surface are in place, the argument checks of both layers return
before any launch, and the NumPy restatement of the contract (tests/attention_grad_cases.py) - which judges the kernels bit for
bit in tests/test_attention_grad_gpu.py - stays within its derived bounds of the longdouble gradient, agrees with torch's
autograd of a dense attention, and has the facts the contract promises."""
import numpy as np
import pytest

import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc


def test_c_abi_public_functions_and_constants(hiplib):
    import sparse_amd
    from sparse_amd import _dot, _ffi, _kernels as K

    for name in ("spamd_attention_grad", "spamd_attention_grad_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_attention_grad"][1]) == 40 and len(_ffi.SIGNATURES["spamd_attention_grad_ws_bytes"][1]) == 6
    for name in ("sparse_attention_grad", "sparse_attention_autograd"):
        assert callable(getattr(sparse_amd, name)) and name in sparse_amd.__all__
    assert "_attention_grad_plan" in _dot.DERIVED_CACHES and "_attention_plan" in _dot.DERIVED_CACHES
    assert K.attention_grad_chunk() == K.ATTENTION_CHUNK and 0 <= K.ATTENTION_GRAD_SHORT_MAX <= 64
    assert K.ATTENTION_GRAD_GROUP in K.ATTENTION_GROUPS and K.ATTENTION_GRAD_COL_GROUP in K.ATTENTION_GROUPS
    assert callable(K.attention_grad_rows)


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch"""
    from sparse_amd import _ffi

    f = hiplib.spamd_attention_grad

    def call(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, col_group=16, short_max=64,
             chunk=64, max_row=100, max_col=100, ws_bytes=0):
        return f(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, None, None, None, pitch, head, None, pitch, head, None, pitch,
                 head, None, pitch, head, 0, 1.0, group, col_group, short_max, chunk, max_row, max_col, None, ws_bytes, None, None,
                 None, None)

    assert call(val=_ffi.I32) == -2 and call(val=_ffi.C64) == -2 and call(val=_ffi.F16) == -2 and call(val=_ffi.BF16) == -2
    assert call(idx=_ffi.F32) == -2 and call(idx=_ffi.U8) == -2
    for name in ("M", "N", "nnz", "H", "D", "Dv", "max_row", "max_col", "pitch", "head"):
        assert call(**{name: -1}) == -1, name
    assert call(max_row=201) == -1 and call(max_col=201) == -1
    for name in ("group", "col_group"):
        assert call(**{name: 0}) == -1 and call(**{name: 12}) == -1 and call(**{name: 128}) == -1
    assert call(chunk=0) == -1 and call(chunk=32) == -1 and call(chunk=100) == -1 and call(chunk=2048) == -1
    assert call(short_max=-1) == -1 and call(short_max=65) == -1
    assert call(H=0) == 0 and call(D=0, Dv=0) == 0 and call(M=0, N=0, nnz=0, max_row=0, max_col=0) == 0      # nothing to write
    assert call(M=0, Dv=0, N=0, nnz=0, max_row=0, max_col=0) == 0
    for val in (_ffi.F32, _ffi.F64):
        for idx in (_ffi.I32, _ffi.I64):
            for group in (8, 16, 32, 64):
                assert call(val=val, idx=idx, group=group, col_group=group, H=0) == 0
    assert call() == -1 and call(nnz=0, max_row=0, max_col=0) == -1           # null pointers with work to do (zeros to write)
    # a workspace that is too small, every pointer given (never read: the check comes before any launch)
    x = 64
    small = lambda ws_bytes, **kw: f(_ffi.F32, _ffi.I64, 3, 4, kw.get("nnz", 200), 2, 5, 6, x, x, x, x, x, x, x, 8, 64, x, 8, 64, x, 8, 64, x, 8,   # noqa: E731
                                     64, 0, 1.0, 16, 16, 64, 64, 100, 100, kw.get("ws", x), ws_bytes, x, x, x, None)
    need = hiplib.spamd_attention_grad_ws_bytes(_ffi.F32, 200, 2, 5, 6, 64)
    assert need > 0 and small(need - 1) == -3 and small(0) == -3 and small(need, ws=None) == -3
    ws = hiplib.spamd_attention_grad_ws_bytes
    assert ws(_ffi.F32, 0, 3, 5, 6, 64) == 0
    assert ws(_ffi.F32, 64, 3, 5, 6, 64) == 3 * 2 * 64 * 4 and ws(_ffi.F64, 1024, 8, 64, 64, 1024) == 8 * 2 * 1024 * 8      # p and y
    assert ws(_ffi.F32, 65, 1, 5, 6, 64) == (2 * 65 + 12 * 2 + 2 * 2 * 11) * 4       # + six arrays of 2 nwin, 2 nwin rows of D + Dv
    assert ws(_ffi.F64, 1000, 3, 7, 2, 128) == 3 * (2000 + 12 * 8 + 2 * 8 * 9) * 8
    assert ws(_ffi.I32, 10, 1, 1, 1, 64) == -2 and ws(_ffi.F32, 10, 1, 1, 1, 0) == -1 and ws(_ffi.F32, 10, 1, 1, 1, 96) == -1
    for bad in ((-1, 1, 1, 1), (10, -1, 1, 1), (10, 1, -1, 1), (10, 1, 1, -1)):
        assert ws(_ffi.F32, *bad, 64) == -1


def test_python_argument_errors():
    import torch

    import sparse_amd

    q, k, v, g = (np.zeros(s, np.float32) for s in ((5, 4), (6, 4), (6, 3), (5, 3)))
    for bad in (np.zeros((5, 6)), None, [[1.0]], torch.zeros(5, 6)):
        with pytest.raises(TypeError, match="COO or GCXS"):
            sparse_amd.sparse_attention_grad(bad, q, k, v, g)
    for bad in (q, None):
        with pytest.raises(TypeError, match="torch tensor"):
            sparse_amd.sparse_attention_autograd(None, bad, torch.zeros(6, 4), torch.zeros(6, 3))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
WIDTHS = [(1, 1), (17, 5), (64, 64), (130, 65)]
LENGTHS = [0, 1, 2, 3, 7, 31, 63, 64, 65, 100, 128, 129, 200, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D,Dv", WIDTHS)
def test_restatement_stays_within_its_bounds(dtype, D, Dv):
    """row lengths 0 to 200 at chunk 64 (rows of one, two and four pieces), with and without a scale: the restated dq, dk and dv
    against the longdouble gradient.  The largest shares are printed (DESIGN A16 records them)."""
    worst = np.zeros(3)
    for scale in (None, D ** -0.5):
        indptr, indices, vals, shape = ac.csr_mask(100 + D, LENGTHS, dtype)
        q, k, v = ac.operands(200 + Dv, shape, D, Dv, dtype)
        g = gc.grad_operand(300 + Dv, shape, Dv, dtype)
        got = gc.grad_restated(indptr, indices, vals, q, k, v, g, 64, scale)
        want, bounds = gc.exact_and_bounds(indptr, indices, vals, q, k, v, g, 64, scale)
        assert not any(np.isnan(b).any() for b in bounds)
        sh = gc.shares(got[:3], want, bounds)
        assert max(sh) <= 1, sh
        worst = np.maximum(worst, sh)
        assert not got[0][0].any() and not got[0][-1].any() and not np.signbit(got[0][0]).any()       # empty rows: +0.0
    print(f"attention_grad restated {np.dtype(dtype)} D {D} Dv {Dv}: largest share of the dq bound {worst[0]:.3f}, "
          f"of the dk bound {worst[1]:.3f}, of the dv bound {worst[2]:.3f}")
    assert worst[2] > 0 and (min(D, Dv) == 1 or worst[0] > 0)


def test_restatement_agrees_with_torch_autograd_of_a_dense_attention():
    """float64, 7 x 9 without an empty row: torch's autograd of softmax(scale * (smask * (q k^T)), -inf at the unstored
    positions) @ v on the CPU, within `OTHER_FORM_FACTOR` bounds plus the comparison value's own rounding, 4 eps"""
    import torch

    rng = np.random.default_rng(3)
    dense = rng.random((7, 9)) < 0.5
    dense[np.arange(7), rng.integers(0, 9, 7)] = True                   # no empty row: the dense form is finite
    dense[:, 4] = False                                                 # an empty column
    indptr = np.concatenate(([0], np.cumsum(dense.sum(axis=1))))
    indices = np.nonzero(dense)[1]
    vals = rng.uniform(0.5, 1.5, len(indices)) * rng.choice([-1, 1], len(indices))
    q, k, v = ac.operands(4, (7, 9), 6, 5, np.float64)
    g = gc.grad_operand(5, (7, 9), 5, np.float64)
    scale = 0.4
    got = gc.grad_restated(indptr, indices, vals, q, k, v, g, 64, scale)[:3]
    smask = np.zeros((7, 9))
    smask[dense] = vals
    tq, tk, tv = (torch.from_numpy(x).requires_grad_() for x in (q, k, v))
    scores = torch.where(torch.from_numpy(dense), scale * (torch.from_numpy(smask) * (tq @ tk.T)), torch.tensor(-np.inf, dtype=torch.float64))
    (torch.softmax(scores, dim=1) @ tv).backward(torch.from_numpy(g))
    want, bounds = gc.exact_and_bounds(indptr, indices, vals, q, k, v, g, 64, scale)
    eps = np.finfo(np.float64).eps
    for name, a, t, b in zip("qkv", got, (tq, tk, tv), bounds):
        other = t.grad.numpy()
        share = float((np.abs(a.astype(gc.LD) - other) / (gc.OTHER_FORM_FACTOR * b + 4 * eps * np.abs(other))).max())
        print(f"attention_grad restated against torch autograd, d{name}: largest share of the bound {share:.3f}")
        assert share <= 1
    assert not got[1][4].any() and not got[2][4].any() and np.abs(got[0]).max() > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_facts(dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(9)
    # a row of one element: p = 1, delta = e exactly, so dq[r] = +-0 and dv[c] = g[r] exactly, whatever the score
    indptr, indices, vals = np.array([0, 1, 1, 2]), np.array([2, 0]), np.array([1.25, -0.75])
    q, k, v = ac.operands(5, (3, 4), 17, 6, dtype, spread=2.0)
    g = gc.grad_operand(6, (3, 4), 6, dtype)
    dq, dk, dv, p, y = gc.grad_restated(indptr, indices, vals, q, k, v, g, 64, 0.3)
    assert (p == 1).all() and (y == 0).all() and not dq.any() and not dk.any()
    assert sc.same_bits(dv[2], g[0]) and sc.same_bits(dv[0], g[2])
    # an empty row and an empty column are +0.0
    assert not np.signbit(dq[1]).any() and not dv[[1, 3]].any() and not np.signbit(dv[[1, 3]]).any() and not np.signbit(dk[[1, 3]]).any()
    # n <= chunk is one piece in rows and columns: the chunk changes no bit; beyond it the pieces are part of the order
    ip, ix, va, shape = ac.csr_mask(11, [1, 2, 63, 64, 40, 9], dtype, ncols=64)
    q, k, v = ac.operands(12, shape, 9, 7, dtype)
    g = gc.grad_operand(13, shape, 7, dtype)
    a, b = gc.grad_restated(ip, ix, va, q, k, v, g, 64), gc.grad_restated(ip, ix, va, q, k, v, g, 1024)
    assert all(sc.same_bits(x, z) for x, z in zip(a, b))
    ip, ix, va, shape = ac.csr_mask(14, [200, 130], dtype)
    q, k, v = ac.operands(15, shape, 9, 7, dtype)
    g = gc.grad_operand(16, shape, 7, dtype)
    a, b = gc.grad_restated(ip, ix, va * 0.01, q, k, v, g, 64), gc.grad_restated(ip, ix, va * 0.01, q, k, v, g, 256)
    assert not sc.same_bits(a[0], b[0]) and np.abs(a[0] - b[0]).max() <= 64 * np.finfo(dtype).eps * np.abs(a[0]).max() * 200
    # with g = the identity (Dv = M), dv[c][r] carries exactly the bits of p(r, c): fma(p, 1, +0) and every other term adds +-0
    ip, ix, va, shape = ac.csr_mask(17, [0, 1, 5, 33, 64, 65, 130, 3], dtype)
    q, k, _ = ac.operands(18, shape, 12, 1, dtype)
    eye = np.eye(shape[0], dtype=dtype)
    v = rng.standard_normal((shape[1], shape[0])).astype(dtype)
    _, _, pf = ac.attention_restated(ip, ix, va, q, k, v, 64, 0.6)
    dq, dk, dv, p, y = gc.grad_restated(ip, ix, va, q, k, v, eye, 64, 0.6)
    rows, cols = ac.coords_of(ip, ix)
    assert sc.same_bits(p, pf) and sc.same_bits(dv[cols, rows], pf) and np.count_nonzero(dv) <= len(pf)
    # A14's NaN / inf cases: a NaN score makes its row's dq NaN and hands NaN to the dk / dv rows of its columns only
    ip, ix, va, shape = ac.csr_mask(19, [3, 4, 2], dtype, ncols=8)
    q, k, v = ac.operands(20, shape, 5, 4, dtype)
    g = gc.grad_operand(21, shape, 4, dtype)
    for bad in (np.nan, np.inf * np.sign(ac.dot64(q[1], k[ix[3:4]])[0])):
        vb = va.copy()
        vb[3] = bad                                                       # row 1, its first element
        dq, dk, dv, p, y = gc.grad_restated(ip, ix, vb, q, k, v, g, 64)
        hit = np.zeros(8, bool)
        hit[ix[3:7]] = True
        assert np.isnan(dq[1]).all() and np.isfinite(dq[[0, 2]]).all()
        assert np.isnan(dv[hit]).all() and np.isnan(dk[hit]).all() and np.isfinite(dv[~hit]).all() and np.isfinite(dk[~hit]).all()
    vb = va.copy()
    vb[3] = -np.inf * np.sign(ac.dot64(q[1], k[ix[3:4]])[0])             # -inf beside finite scores: p = +0, nothing is NaN but y_3
    dq, dk, dv, p, y = gc.grad_restated(ip, ix, vb, q, k, v, g, 64)
    assert p[3] == 0 and np.isnan(y[3]) and np.isfinite(dv).all()         # y_3 = -inf * 0


def test_restated_fma_is_exact_where_products_underflow():
    """the float64 fma of the restatement against rational arithmetic, where `softmax_cases.fma64v` leaves its domain: products
    near and below the smallest normal, results that are subnormal, exact cancellation"""
    from fractions import Fraction

    rng = np.random.default_rng(31)
    a = rng.standard_normal(400) * 10.0 ** rng.uniform(-320, -100, 400)
    b = rng.standard_normal(400) * 10.0 ** rng.uniform(-200, 5, 400)
    c = np.where(rng.random(400) < 0.5, rng.standard_normal(400) * 10.0 ** rng.uniform(-323, -290, 400), -a * b)
    got = gc._fma64_exact(a, b, c)
    want = np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert sc.same_bits(got, want) and (np.abs(a * b) < 2.0 ** -900).sum() > 100 and (want != sc.fma64v(a, b, c)).any()
    x, y, z = rng.standard_normal((3, 50))
    assert sc.same_bits(gc._fma64_exact(x, y, z), sc.fma64v(x, y, z))

"""sparse_attention without a GPU: the C ABI and the public surface are in place, the argument checks of both layers return
before any launch, and the NumPy restatement of the contract (tests/attention_cases.py) - which judges the kernels bit for bit
in tests/test_attention_gpu.py - stays within its two derived bounds of a longdouble dense attention, agrees with
scipy.special.softmax and a torch dense attention, and has the facts the contract promises."""
import numpy as np
import pytest

import attention_cases as ac
import softmax_cases as sc

F32, F64 = np.dtype("float32"), np.dtype("float64")


def test_c_abi_public_function_and_constants(hiplib):
    import sparse_amd
    from sparse_amd import _dot, _ffi, _kernels as K

    for name in ("spamd_attention", "spamd_attention_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_attention"][1]) == 30 and len(_ffi.SIGNATURES["spamd_attention_ws_bytes"][1]) == 5
    assert callable(sparse_amd.sparse_attention) and "sparse_attention" in sparse_amd.__all__
    assert "_attention_plan" in _dot.DERIVED_CACHES
    assert K.ATTENTION_CHUNK % 64 == 0 and 64 <= K.ATTENTION_CHUNK <= K.SOFTMAX_MAX_CHUNK and 0 <= K.ATTENTION_SHORT_MAX <= 64
    assert K.ATTENTION_GROUP in K.ATTENTION_GROUPS == (8, 16, 32, 64)
    assert callable(K.attention_rows)


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch"""
    from sparse_amd import _ffi

    f = hiplib.spamd_attention

    def call(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, short_max=64, chunk=64,
             max_len=100, ws_bytes=0):
        return f(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, pitch, head, None, pitch, head, None, pitch, head, 0, 1.0,
                 group, short_max, chunk, max_len, None, ws_bytes, None, None)

    assert call(val=_ffi.I32) == -2 and call(val=_ffi.C64) == -2 and call(val=_ffi.F16) == -2 and call(val=_ffi.BF16) == -2
    assert call(idx=_ffi.F32) == -2 and call(idx=_ffi.U8) == -2
    for name in ("M", "N", "nnz", "H", "D", "Dv", "max_len", "pitch", "head"):
        assert call(**{name: -1}) == -1, name
    assert call(max_len=201) == -1
    assert call(group=0) == -1 and call(group=12) == -1 and call(group=128) == -1
    assert call(chunk=0) == -1 and call(chunk=32) == -1 and call(chunk=100) == -1 and call(chunk=2048) == -1
    assert call(short_max=-1) == -1 and call(short_max=65) == -1
    assert call(M=0) == 0 and call(H=0) == 0 and call(Dv=0) == 0                # nothing to do
    for val in (_ffi.F32, _ffi.F64):
        for idx in (_ffi.I32, _ffi.I64):
            for group in (8, 16, 32, 64):
                assert call(val=val, idx=idx, group=group, M=0) == 0
    assert call() == -1 and call(nnz=0, max_len=0) == -1                      # null pointers with work to do (zeros to write)
    ws = hiplib.spamd_attention_ws_bytes
    assert ws(_ffi.F32, 64, 3, 5, 64) == 0 and ws(_ffi.F64, 1024, 8, 64, 1024) == 0
    assert ws(_ffi.F32, 65, 1, 5, 64) == (65 + 8 * 2 + 2 * 2 * 5) * 4           # scores, four arrays of 2 nwin, 2 nwin rows of Dv
    assert ws(_ffi.F64, 1000, 3, 7, 128) == 3 * (1000 + 8 * 8 + 2 * 8 * 7) * 8
    assert ws(_ffi.I32, 10, 1, 1, 64) == -2 and ws(_ffi.F32, 10, 1, 1, 0) == -1 and ws(_ffi.F32, 10, 1, 1, 96) == -1
    assert ws(_ffi.F32, -1, 1, 1, 64) == -1 and ws(_ffi.F32, 10, -1, 1, 64) == -1 and ws(_ffi.F32, 10, 1, -1, 64) == -1


# ---- the public function's argument checks (they come before anything touches a device) ---------------------------------------------
def test_python_argument_errors():
    import torch

    import sparse_amd
    from sparse_amd._attention import _check_operands as check
    from sparse_amd._softmax import _check_arguments as check_scale

    q, k, v = np.zeros((5, 4), np.float32), np.zeros((6, 4), np.float32), np.zeros((6, 3), np.float32)
    for bad in (np.zeros((5, 6)), None, [[1.0]], torch.zeros(5, 6)):
        with pytest.raises(TypeError, match="COO or GCXS"):
            sparse_amd.sparse_attention(bad, q, k, v)
    assert check((5, 6), q, k, v) == (torch.float32, ())
    assert check((5, 6), torch.zeros(2, 3, 5, 4, dtype=torch.float64), np.zeros((2, 3, 6, 4)), np.zeros((2, 3, 6, 9))) == (torch.float64, (2, 3))
    for bad in ([q, k, v.astype(np.float64)], [q.astype(np.float64), k, v], [torch.zeros(5, 4), k.astype(np.float64), v]):
        with pytest.raises(TypeError, match="all float32 or all float64"):
            check((5, 6), *bad)
    for dt in (np.float16, np.complex64, np.complex128, np.int32):
        with pytest.raises(TypeError, match="16-bit and complex"):
            check((5, 6), q.astype(dt), k.astype(dt), v.astype(dt))
    with pytest.raises(TypeError, match="16-bit and complex"):
        check((5, 6), torch.zeros(5, 4, dtype=torch.bfloat16), torch.zeros(6, 4, dtype=torch.bfloat16), torch.zeros(6, 3, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="NumPy array or a torch tensor"):
        check((5, 6), q.tolist(), k, v)
    with pytest.raises(ValueError, match="at least 2 dimensions"):
        check((5, 6), q[0], k, v)
    lead = lambda x, *n: np.zeros(n + x.shape, x.dtype)                                      # noqa: E731
    for bad in ([lead(q, 2), k, v], [lead(q, 2), lead(k, 2), lead(v, 3)], [lead(q, 2, 2), lead(k, 4), lead(v, 2, 2)],
                [lead(q, 1), lead(k, 2), lead(v, 2)]):
        with pytest.raises(ValueError, match="head"):
            check((5, 6), *bad)
    for bad in ([np.zeros((4, 4), np.float32), k, v], [q, np.zeros((7, 4), np.float32), v], [q, k, np.zeros((5, 3), np.float32)],
                [q, np.zeros((6, 5), np.float32), v], [np.zeros((5, 3), np.float32), k, v]):            # M, N of k, N of v, D, D
        with pytest.raises(ValueError, match="shape-mismatch"):
            check((5, 6), *bad)
    for bad in ("2", 1j, True, [1.0]):
        with pytest.raises(TypeError, match="scale"):
            check_scale(np.float32, 2, -1, bad)
    for dt in (np.complex64, np.float16):
        with pytest.raises(TypeError, match="complex and 16-bit"):
            check_scale(dt, 2, -1, None)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
WIDTHS = [(1, 1), (17, 5), (64, 64), (130, 65)]
LENGTHS = [0, 1, 2, 3, 7, 31, 63, 64, 65, 100, 128, 129, 200, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D,Dv", WIDTHS)
def test_restatement_stays_within_both_bounds(dtype, D, Dv):
    """row lengths 0 to 200 at chunk 64 (so rows of one, two and four pieces), with a scale, queries of 1 and 8 standard
    deviations: the restated scores against s scale (q . k) in longdouble, the restated output against the exact attention of
    the ROUNDED scores.  The largest shares are printed (DESIGN A15 records them)."""
    worst_s = worst_o = 0.0
    for spread in (1.0, 8.0):
        indptr, indices, vals, shape = ac.csr_mask(100 + D, LENGTHS, dtype)
        q, k, v = ac.operands(200 + Dv, shape, D, Dv, dtype, spread=spread)
        scale = D ** -0.5
        out, t, p = ac.attention_restated(indptr, indices, vals, q, k, v, 64, scale)
        want, bound = ac.score_exact_and_bound(indptr, indices, vals, q, k, scale)
        s_share = ac.share(t, want, bound)
        owant, obound, _ = ac.output_exact_and_bound(indptr, indices, t, v)
        o_share = ac.share(out, owant, obound)
        assert not np.isnan(obound).any() and s_share <= 1 and o_share <= 1
        worst_s, worst_o = max(worst_s, s_share), max(worst_o, o_share)
        assert (out[0] == 0).all() and (out[-1] == 0).all() and not np.signbit(out[0]).any()
    print(f"attention restated {np.dtype(dtype)} D {D} Dv {Dv}: largest share of the score bound {worst_s:.3f}, of the output bound {worst_o:.3f}")
    assert 0 < worst_o and (D == 1 or 0 < worst_s)


def test_restatement_agrees_with_scipy_and_a_torch_dense_attention():
    """float64, 7 x 9: scipy.special.softmax of the dense scores with -inf at the unstored positions, times v, and the same
    in torch on the CPU - each within the output bound plus what two score computations do to the result
    (`other_form_bound`) plus the comparison value's own rounding, 4 eps"""
    import scipy.special
    import torch

    rng = np.random.default_rng(3)
    dense = rng.random((7, 9)) < 0.5
    dense[2] = False                                                    # an empty row: +0.0 here, NaN in the dense image
    lengths = dense.sum(axis=1)
    indptr = np.concatenate(([0], np.cumsum(lengths)))
    indices = np.nonzero(dense)[1]
    vals = rng.uniform(0.5, 1.5, len(indices))
    q, k, v = ac.operands(4, (7, 9), 6, 5, np.float64)
    scale = 0.4
    out, t, _ = ac.attention_restated(indptr, indices, vals, q, k, v, 64, scale)
    smask = np.zeros((7, 9))
    smask[dense] = vals
    scores = np.where(dense, scale * (smask * (q @ k.T)), -np.inf)
    with np.errstate(all="ignore"):
        ref = np.nan_to_num(scipy.special.softmax(scores, axis=1)) @ v
    ts = torch.from_numpy(scores)
    tref = (torch.nan_to_num(torch.softmax(ts, dim=1)) @ torch.from_numpy(v)).numpy()
    want, bound = ac.other_form_bound(indptr, indices, vals, q, k, v, t, scale)
    for other in (ref, tref):
        assert (np.abs(out - other) <= (bound + 4 * np.finfo(np.float64).eps * np.abs(other)).astype(np.float64)).all()
    assert (out[2] == 0).all() and np.abs(out - ref).max() > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_facts(dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(9)
    q, k, v = ac.operands(5, (1, 300), 17, 6, dtype, spread=2.0)
    one = lambda cols, vals, kk=k, vv=v, chunk=64, scale=None: ac.row_attention(np.asarray(vals, dtype), np.asarray(cols), q[0], kk, vv, chunk, scale)   # noqa: E731
    # a row of one element returns v[c] exactly, whatever the score
    for c in (0, 7, 299):
        out, t, p = one([c], [rng.standard_normal() * 100])
        assert p[0] == 1 and sc.same_bits(out, v[c])
    # 2^k equal scores over equal v rows return that row: p = 2^-k exactly, and with entries of few significant bits (multiples
    # of 1 / 16 here) every partial sum m 2^-k v is exact, in one piece and in pieces of 64
    row = np.round(v[5] * 16) / 16
    for kk in range(0, 9):
        n = 2 ** kk
        keq, veq = np.repeat(k[3:4], 300, axis=0), np.repeat(row[None, :], 300, axis=0).astype(dtype)
        out, t, p = one(np.arange(n), np.full(n, 1.25), keq, veq, 64)
        assert (t == t[0]).all() and (p == dtype.type(2.0 ** -kk)).all() and sc.same_bits(out, veq[0])
    # an empty row is +0.0
    out, t, p = one([], [])
    assert (out == 0).all() and not np.signbit(out).any() and len(t) == 0
    # a stored zero of the mask takes part as the score 0
    out, t, p = one([1, 2, 3], [0.0, 1.0, -0.0])
    assert t[0] == 0 and t[2] == 0 and p[0] > 0 and p[2] > 0 and abs(p.sum() - 1) < 4 * np.finfo(dtype).eps
    # A14's NaN / inf cases, per row: a NaN or +inf score, or only -inf scores, make the whole output row NaN
    for vals in ([1.0, np.nan, 2.0], [1.0, np.inf * np.sign(ac.dot64(q[0], k[[2]])[0]), 2.0], [-np.inf * np.sign(ac.dot64(q[0], k[[1]])[0])]):
        out, t, p = one([1, 2, 3][:len(vals)], vals)
        assert np.isnan(out).all(), vals
    w = ac.dot64(q[0], k[[1, 2]])
    out, t, p = one([1, 2], [-np.inf * np.sign(w[0]), 1.0])              # -inf beside a finite score: p = +0, the row is v[2]
    assert p[0] == 0 and p[1] == 1 and sc.same_bits(out, v[2])
    # a negative scale is legal and equals the scaled scores' softmax
    out, t, p = one([4, 9, 30], [1.0, 2.0, 0.5], scale=-1.5)
    assert sc.same_bits(t, dtype.type(-1.5) * (np.array([1.0, 2.0, 0.5], dtype) * ac.dot64(q[0], k[[4, 9, 30]])))
    # n <= chunk is one piece: the chunk changes no bit; beyond it the pieces are part of the order
    cols = np.sort(rng.choice(300, 200, replace=False))
    vals = rng.uniform(0.5, 1.5, 200)
    for n in (1, 2, 63, 64):
        assert sc.same_bits(one(cols[:n], vals[:n], chunk=64)[0], one(cols[:n], vals[:n], chunk=1024)[0])
    assert sc.same_bits(one(cols[:128], vals[:128], chunk=128)[0], one(cols[:128], vals[:128], chunk=256)[0])
    flat = vals * 0.01                                                   # nearly uniform probabilities: every piece matters
    a, b = one(cols, flat, chunk=64)[0], one(cols, flat, chunk=256)[0]
    assert not sc.same_bits(a, b) and np.abs(a - b).max() <= 64 * np.finfo(dtype).eps * np.abs(v).max()


def test_dot_product_order():
    """D = 130: accumulator 0 takes elements 0, 64, 128, accumulator 1 takes 1, 65, 129, the others two each; the fold is
    a[l] + a[l + h], h = 32 .. 1.  Written out with the scalar fma of tests/masked_cases.py"""
    import masked_cases as mc

    rng = np.random.default_rng(12)
    for dtype, fma in ((np.float32, mc.fma32), (np.float64, mc.fma64)):
        q = rng.standard_normal(130).astype(dtype)
        k = rng.standard_normal((1, 130)).astype(dtype)
        a = [dtype(0)] * 64
        for j in range(130):
            a[j % 64] = dtype(fma(q[j], k[0, j], a[j % 64]))
        h = 32
        while h:
            a = [dtype(a[l] + a[l + h]) for l in range(h)]
            h //= 2
        assert sc.same_bits(ac.dot64(q, k), np.array(a, dtype=dtype))
        assert ac.dot64(q[:3], k[:, :3])[0] == dtype(dtype(fma(q[0], k[0, 0], dtype(0)) + fma(q[2], k[0, 2], dtype(0))) + fma(q[1], k[0, 1], dtype(0)))

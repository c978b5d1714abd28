"""Attention dropout without a GPU: the restated Philox4x32-10 gives Random123's known answers, the threshold rule and the kept
fraction hold, the three C entries and the public keywords are in place, the argument checks of both layers return before any
launch or device, and the NumPy restatement (tests/attention_dropout_cases.py) - which judges the kernels bit for bit in
tests/test_attention_dropout_gpu.py - has the bits of the restatements without dropout at rate 0 and stays within its derived
bounds of a longdouble dropout attention built on the same keep mask."""
import inspect

import numpy as np
import pytest

import attention_bias_cases as bc
import attention_cases as ac
import attention_dropout_cases as dc
import attention_grad_cases as gc
import softmax_cases as sc

WIDTHS = [(1, 1), (17, 5), (64, 64), (130, 65)]                       # `test_attention.WIDTHS`
LENGTHS = [0, 1, 2, 3, 7, 31, 63, 64, 65, 100, 128, 129, 200, 0]
SEEDS = (1, (1 << 63) + 12345, 0xDEADBEEFCAFEF00D)                    # chosen once on the CPU; the kept counts are deterministic


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's known answers for philox4x32-10, recomputed with an independent few-line integer implementation"""
    words = lambda c, k: " ".join("%08x" % int(x) for x in dc.philox4x32_10(c, k))   # noqa: E731
    assert words([0] * 4, [0] * 2) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == "d16cfe09 94fdcceb 5001e420 24126ea1"

    def plain(c, k):                                                    # Python integers, no NumPy
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = dc.M0 * c[0], dc.M1 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
            k = [(k[0] + dc.W0) & 0xFFFFFFFF, (k[1] + dc.W1) & 0xFFFFFFFF]
        return c

    rng = np.random.default_rng(5)
    cs, ks = rng.integers(0, 1 << 32, (4, 50), dtype=np.uint64), rng.integers(0, 1 << 32, (2, 50), dtype=np.uint64)
    got = np.stack(dc.philox4x32_10(cs, ks))
    for i in range(50):
        assert [int(x) for x in got[:, i]] == plain([int(x) for x in cs[:, i]], [int(x) for x in ks[:, i]])


def test_threshold_rule():
    assert dc.threshold(0.0) == 0 and dc.keep_restated(1000, 3, 0.0, 12345).all()
    assert dc.threshold(0.5) == 1 << 31
    assert dc.threshold(np.nextafter(1.0, 0.0)) < 1 << 32
    assert dc.threshold(0.1) == int(np.floor(np.float64(0.1) * 2.0 ** 32)) == 429496729
    # the counter carries all 64 bits of the position and of the head, the key all 64 of the seed
    base = dc.keep_restated(64, 1, 0.5, 3)
    assert (dc.keep_restated(64, 1, 0.5, 3, pos0=1 << 32) != base).any() and (dc.keep_restated(64, 1, 0.5, 3, head0=1 << 32) != base).any()
    assert (dc.keep_restated(64, 1, 0.5, 3 + (1 << 32)) != base).any()
    assert (dc.keep_restated(64, 2, 0.5, 3)[1] == dc.keep_restated(64, 1, 0.5, 3, head0=1)[0]).all()
    assert (dc.keep_restated(64, 1, 0.5, 3)[0, 5:] == dc.keep_restated(59, 1, 0.5, 3, pos0=5)[0]).all()


@pytest.mark.parametrize("rate", [0.1, 0.6])
@pytest.mark.parametrize("seed", SEEDS)
def test_kept_fraction(rate, seed):
    """2^16 positions of 4 heads: the kept count within 5 binomial standard deviations of n (1 - thr / 2^32)"""
    n = 4 << 16
    pk = 1 - dc.threshold(rate) / 2.0 ** 32
    kept = int(dc.keep_restated(1 << 16, 4, rate, seed).sum())
    sd = (n * pk * (1 - pk)) ** 0.5
    print(f"dropout {rate} seed {seed:#x}: kept {kept} of {n}, {(kept - n * pk) / sd:+.2f} standard deviations from the mean")
    assert abs(kept - n * pk) <= 5 * sd


# ---- both layers' interfaces ------------------------------------------------------------------------------------------------------
NEW = ("spamd_attention_dropout", "spamd_attention_grad_dropout", "spamd_attention_keep")


def test_c_abi_and_public_keywords(hiplib):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    for name in NEW:
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_attention_dropout"][1]) == 35 and len(_ffi.SIGNATURES["spamd_attention_grad_dropout"][1]) == 46
    assert len(_ffi.SIGNATURES["spamd_attention_keep"][1]) == 8
    for f in (sparse_amd.sparse_attention, sparse_amd.sparse_attention_grad, sparse_amd.sparse_attention_autograd, K.attention_rows,
              K.attention_grad_rows):
        for name in ("dropout", "seed"):
            p = inspect.signature(f).parameters[name]
            assert p.default is None and p.kind is p.KEYWORD_ONLY
    sig = inspect.signature(sparse_amd.sparse_attention_keep_mask).parameters
    assert sig["dropout"].kind is sig["dropout"].KEYWORD_ONLY and sig["seed"].kind is sig["seed"].KEYWORD_ONLY
    assert "sparse_attention_keep_mask" in sparse_amd.__all__


def test_argument_checks_of_the_c_entries_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch - the list of tests/test_attention_bias.py on the new
    entries, and the new arguments"""
    from sparse_amd import _ffi

    x = 64                                                             # a pointer that is never read

    def fwd(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, short_max=64, chunk=64,
            max_len=100, ws_bytes=0, bias=None, bias_head=200, rate=0.25, seed=7, head0=0):
        return hiplib.spamd_attention_dropout(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, pitch, head, None, pitch, head,
                                              None, pitch, head, 0, 1.0, group, short_max, chunk, max_len, bias, bias_head, rate, seed,
                                              head0, None, ws_bytes, None, None)

    def bwd(val=_ffi.F32, idx=_ffi.I64, M=3, N=4, nnz=200, H=2, D=5, Dv=6, pitch=8, head=64, group=16, col_group=16, short_max=64,
            chunk=64, max_row=100, max_col=100, ws_bytes=0, bias=None, bias_head=200, dbias=None, rate=0.25, seed=7, head0=0):
        return hiplib.spamd_attention_grad_dropout(val, idx, M, N, nnz, H, D, Dv, None, None, None, None, None, None, None, pitch, head,
                                                   None, pitch, head, None, pitch, head, None, pitch, head, 0, 1.0, group, col_group,
                                                   short_max, chunk, max_row, max_col, bias, bias_head, dbias, rate, seed, head0, None,
                                                   ws_bytes, None, None, None, None)

    for call, lens in ((fwd, ("max_len",)), (bwd, ("max_row", "max_col"))):
        for bias in (None, x):
            for rate in (0.0, 0.25):
                kw = dict(bias=bias, rate=rate)
                assert call(val=_ffi.I32, **kw) == -2 and call(val=_ffi.C64, **kw) == -2 and call(val=_ffi.F16, **kw) == -2
                assert call(val=_ffi.BF16, **kw) == -2 and call(idx=_ffi.F32, **kw) == -2 and call(idx=_ffi.U8, **kw) == -2
                for name in ("M", "N", "nnz", "H", "D", "Dv", "pitch", "head", "bias_head", "head0") + lens:
                    assert call(**{name: -1}, **kw) == -1, name
                for name in lens:
                    assert call(**{name: 201}, **kw) == -1
                for name in ("group",) + (("col_group",) if call is bwd else ()):
                    assert call(**{name: 0}, **kw) == -1 and call(**{name: 12}, **kw) == -1 and call(**{name: 128}, **kw) == -1
                assert call(chunk=0, **kw) == -1 and call(chunk=32, **kw) == -1 and call(chunk=100, **kw) == -1 and call(chunk=2048, **kw) == -1
                assert call(short_max=-1, **kw) == -1 and call(short_max=65, **kw) == -1
                assert call(H=0, **kw) == 0                             # nothing to do
                assert call(**kw) == -1                                 # null pointers with work to do
            for rate in (-0.1, 1.0, float("nan"), 1.5, float("inf"), -float("inf")):
                assert call(bias=bias, rate=rate) == -1 and call(bias=bias, rate=rate, H=0) == -1, rate
            assert call(bias=bias, head0=-1, H=0) == -1
            assert call(bias=bias, rate=float(np.nextafter(1.0, 0.0)), seed=-1, head0=(1 << 63) - 1, H=0) == 0
    assert fwd(M=0) == 0 and fwd(Dv=0) == 0 and fwd(bias_head=0, H=0) == 0
    assert bwd(D=0, Dv=0) == 0 and bwd(M=0, N=0, nnz=0, max_row=0, max_col=0, bias=x, dbias=x) == 0
    # a workspace that is too small, every pointer given: the check comes before any launch
    need_f = hiplib.spamd_attention_ws_bytes(_ffi.F32, 200, 2, 6, 64)
    need_b = hiplib.spamd_attention_grad_ws_bytes(_ffi.F32, 200, 2, 5, 6, 64)
    for bias, dbias in ((None, None), (x, None), (x, x)):
        small_f = lambda ws, n: hiplib.spamd_attention_dropout(_ffi.F32, _ffi.I64, 3, 4, 200, 2, 5, 6, x, x, x, x, 8, 64, x, 8, 64, x, 8, 64, 0,   # noqa: E731
                                                               1.0, 16, 64, 64, 100, bias, 200, 0.25, 7, 0, ws, n, x, None)
        small_b = lambda ws, n: hiplib.spamd_attention_grad_dropout(_ffi.F32, _ffi.I64, 3, 4, 200, 2, 5, 6, x, x, x, x, x, x, x, 8, 64, x, 8,       # noqa: E731
                                                                    64, x, 8, 64, x, 8, 64, 0, 1.0, 16, 16, 64, 64, 100, 100, bias, 200, dbias,
                                                                    0.25, 7, 0, ws, n, x, x, x, None)
        assert small_f(x, need_f - 1) == -3 and small_f(None, need_f) == -3
        assert small_b(x, need_b - 1) == -3 and small_b(x, 0) == -3 and small_b(None, need_b) == -3
    # the keep entry
    keep = lambda nnz=10, H=2, pos0=0, head0=0, rate=0.5, out=None: hiplib.spamd_attention_keep(nnz, H, pos0, head0, rate, 7, out, None)   # noqa: E731
    for name in ("nnz", "H", "pos0", "head0"):
        assert keep(**{name: -1}) == -1, name
    for rate in (-0.1, 1.0, float("nan")):
        assert keep(rate=rate) == -1 and keep(rate=rate, nnz=0) == -1
    assert keep() == -1 and keep(nnz=0) == 0 and keep(H=0) == 0 and keep(nnz=1 << 40, H=1 << 40, out=x) == -1


def test_python_argument_errors():
    """everything that is wrong with `dropout` or `seed` raises before a device is touched"""
    import torch

    import sparse_amd
    from sparse_amd._attention import _check_dropout as check

    assert check(None, None) == (None, None) and check(None, "ignored") == (None, None)
    assert check(0, None) == (None, None) and check(0.0, object()) == (None, None) and check(np.float32(0), -5) == (None, None)
    assert check(0.5, 0) == (0.5, 0) and check(np.float64(0.25), np.int64(9)) == (0.25, 9) and check(0.1, (1 << 64) - 1) == (0.1, (1 << 64) - 1)
    assert check(np.float32(0.5), np.uint64((1 << 64) - 1)) == (0.5, (1 << 64) - 1)
    assert check(float(np.nextafter(1.0, 0.0)), 1)[0] < 1
    for bad in (True, False, np.bool_(True), "0.5", 0.5 + 0j, np.complex64(0.5), torch.tensor(0.5), np.array(0.5), np.array([0.5]), [0.5], (0.5,)):
        with pytest.raises(TypeError, match="real number"):
            check(bad, 1)
    for bad in (-0.1, 1.0, 1, 2, float("nan"), float("inf"), -float("inf"), np.float32(1.0), -1):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            check(bad, 1)
    with pytest.raises(ValueError, match="no hidden global generator"):
        check(0.5, None)
    for bad in (1.0, "7", True, np.bool_(False), 1 + 0j, torch.tensor([1, 2]), None.__class__, [1]):
        with pytest.raises(TypeError, match="`seed` must be an int"):
            check(0.5, bad)
    for bad in (-1, 1 << 64, np.int64(-3)):
        with pytest.raises(ValueError, match=r"2\^64"):
            check(0.5, bad)
    # through a public function, with CPU tensors and no mask at all: the checks come before the mask is looked at
    s, q = None, torch.zeros(5, 4)
    with pytest.raises(ValueError, match="no hidden global generator"):
        sparse_amd.sparse_attention_autograd(s, q, torch.zeros(6, 4), torch.zeros(6, 3), dropout=0.5)
    with pytest.raises(TypeError, match="real number"):
        sparse_amd.sparse_attention_autograd(s, q, torch.zeros(6, 4), torch.zeros(6, 3), dropout="0.5", seed=1)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        sparse_amd.sparse_attention_autograd(s, q, torch.zeros(6, 4), torch.zeros(6, 3), dropout=1.0, seed=1)
    from sparse_amd import _kernels as K

    for bad, exc in ((1.0, ValueError), (-0.5, ValueError), (float("nan"), ValueError)):
        with pytest.raises(exc):
            K._dropout_args(bad, 1, "attention")
    with pytest.raises(ValueError, match="seed"):
        K._dropout_args(0.5, None, "attention")
    with pytest.raises(ValueError, match="seed"):
        K._dropout_args(0.5, 1 << 64, "attention")
    assert K._dropout_args(None, None, "a") is None and K._dropout_args(0.0, None, "a") is None
    assert K._dropout_args(0.5, (1 << 64) - 1, "a") == (0.5, -1) and K._dropout_args(0.5, 1 << 63, "a") == (0.5, -(1 << 63))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rate_zero_has_the_bits_of_the_restatements_without_dropout(dtype):
    indptr, indices, vals, shape = ac.csr_mask(30, LENGTHS, dtype)
    q, k, v = ac.operands(31, shape, 17, 6, dtype, spread=2.0)
    g = gc.grad_operand(32, shape, 6, dtype)
    bias = bc.bias_of(33, len(indices), dtype)
    assert dc.c_of(0.0, dtype) == 1
    for scale in (None, 0.4):
        plain = ac.attention_restated(indptr, indices, vals, q, k, v, 64, scale)
        zero = dc.attention_dropout_restated(indptr, indices, vals, q, k, v, 64, scale, None, 0.0, 99)
        assert sc.same_bits(zero[0], plain[0]) and sc.same_bits(zero[1], plain[1]) and sc.same_bits(zero[3], plain[2]) and zero[4].all()
        biased = bc.attention_bias_restated(indptr, indices, vals, q, k, v, 64, scale, bias)
        zero = dc.attention_dropout_restated(indptr, indices, vals, q, k, v, 64, scale, bias, 0.0, 99)
        assert sc.same_bits(zero[0], biased[0]) and sc.same_bits(zero[3], biased[2])
        gplain = gc.grad_restated(indptr, indices, vals, q, k, v, g, 64, scale)
        gzero = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 64, scale, None, 0.0, 99)
        assert all(sc.same_bits(a, b) for a, b in zip(gzero[:3], gplain[:3]))
        gbiased = bc.grad_bias_restated(indptr, indices, vals, q, k, v, g, 64, scale, bias)
        gzero = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 64, scale, bias, 0.0, 99)
        assert all(sc.same_bits(a, b) for a, b in zip(gzero, gbiased))


@pytest.mark.parametrize("rate", [0.1, 0.6])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D,Dv", WIDTHS)
def test_restatement_stays_within_its_bounds(dtype, D, Dv, rate):
    """row lengths 0 to 200 at chunk 64, with a scale: the output against the exact dropout attention of the ROUNDED scores on the
    same keep mask, dq, dk and dv against the exact dropout gradient, each within the bounds derived in
    tests/attention_dropout_cases.py - those of the files without dropout with the one extra rounding of p_i c and e_i c"""
    indptr, indices, vals, shape = ac.csr_mask(100 + D, LENGTHS, dtype)
    q, k, v = ac.operands(200 + Dv, shape, D, Dv, dtype)
    g = gc.grad_operand(400 + D, shape, Dv, dtype)
    scale, seed = D ** -0.5, SEEDS[1]
    out, t, p, pd, keep = dc.attention_dropout_restated(indptr, indices, vals, q, k, v, 64, scale, None, rate, seed)
    c = dc.c_of(rate, dtype)
    assert 0 < keep.sum() < len(keep) and (pd[~keep] == 0).all() and not np.signbit(pd[~keep]).any()
    assert sc.same_bits(pd[keep], (p * c)[keep])
    want, bound = dc.output_exact_and_bound(indptr, indices, t, v, keep, c)
    o_share = ac.share(out, want, bound)
    grads = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 64, scale, None, rate, seed)
    gwant, gbounds = dc.grad_exact_and_bounds(indptr, indices, vals, q, k, v, g, 64, keep, c, scale, t)
    g_shares = gc.shares(grads[:3], gwant, gbounds)
    print(f"attention dropout restated {np.dtype(dtype)} D {D} Dv {Dv} rate {rate}: largest share of the output bound {o_share:.3f}, "
          f"of the dq, dk, dv bounds {g_shares[0]:.3f} {g_shares[1]:.3f} {g_shares[2]:.3f}")
    assert not np.isnan(bound).any() and all(not np.isnan(b).any() for b in gbounds)
    assert 0 < o_share <= 1 and all(0 < s <= 1 for s in g_shares)
    for got, w, b in zip((out,) + grads[:3], (want,) + gwant, (bound,) + gbounds):
        assert (np.abs(got.astype(ac.LD) - w) <= b).all()
    assert (out[0] == 0).all() and not np.signbit(out[0]).any()


def test_consequences_of_the_order():
    dtype = np.dtype(np.float32)
    indptr, indices, vals, shape = ac.csr_mask(50, [5, 3, 70, 0], dtype)
    q, k, v = ac.operands(51, shape, 9, 4, dtype)
    g = gc.grad_operand(52, shape, 4, dtype)
    # seed 2 at rate 0.6 keeps, of the positions 0 .. 7 of head 0, position 5 alone (chosen on the CPU)
    keep = dc.keep_restated(8, 1, 0.6, 2)[0]
    assert keep.tolist() == [False] * 5 + [True, False, False]
    out, t, p, pd, kp = dc.attention_dropout_restated(indptr, indices, vals, q, k, v, 64, None, None, 0.6, 2)
    c = dc.c_of(0.6, dtype)
    assert (out[0] == 0).all() and not np.signbit(out[0]).any()          # a row whose elements are all dropped: +0.0
    assert sc.same_bits(out[1], sc._fma(dtype)(np.broadcast_to(p[5] * c, (4,)), v[indices[5]], np.zeros(4, dtype)).astype(dtype))
    dq, dk, dv, z = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 64, None, None, 0.6, 2)
    assert (dq[0] == 0).all() and (z[:5] == 0).all()                     # ... has ed = 0 throughout, so delta = 0 and z = 0
    only = np.setdiff1d(indices[~kp], indices[kp])                        # the columns whose elements are all dropped
    assert len(only) and (dv[only] == 0).all() and dv[np.unique(indices[kp])].any()      # ... get no dv
    # another head, another seed: other decisions
    assert (dc.keep_restated(78, 1, 0.6, 2, head0=1) != kp).any() and (dc.keep_restated(78, 1, 0.6, 3) != kp).any()


def test_grad_restated_against_central_differences():
    """float64: dq, dk, dv and dbias of `grad_dropout_restated` against central differences of the restated forward under the
    same seed, loss = sum(out * g); rows of 0, 1, 9 and 70 elements at chunk 64, rate 0.6"""
    indptr, indices, vals, shape = ac.csr_mask(40, [0, 1, 9, 70, 3], np.float64)
    q, k, v = ac.operands(41, shape, 3, 2, np.float64)
    g = gc.grad_operand(42, shape, 2, np.float64)
    bias = bc.bias_of(43, len(indices), np.float64, spread=0.5)
    dq, dk, dv, db = dc.grad_dropout_restated(indptr, indices, vals, q, k, v, g, 64, 0.7, bias, 0.6, 11)

    def loss(q_, k_, v_, b_):
        return float((dc.attention_dropout_restated(indptr, indices, vals, q_, k_, v_, 64, 0.7, b_, 0.6, 11)[0] * g).sum())

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
    assert db.any() and dv.any()

"""softmax without a GPU: the C ABI and the public surface are in place, the argument checks of both layers return before
any launch, and the NumPy restatement of the contract (tests/softmax_cases.py) - which judges the kernels bit for bit in
tests/test_softmax_gpu.py - has the exponential's facts and accuracy and agrees with scipy.special.softmax and
torch.sparse.softmax."""
import numpy as np
import pytest

import masked_cases as mc
import softmax_cases as sc

F32, F64 = np.dtype("float32"), np.dtype("float64")


def test_c_abi_public_function_and_cache_key(hiplib):
    import sparse_amd
    from sparse_amd import _dot, _ffi, _kernels as K

    for name in ("spamd_softmax", "spamd_softmax_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_softmax"][1]) == 17
    assert callable(sparse_amd.softmax) and "softmax" in sparse_amd.__all__
    assert "_softmax_plan" in _dot.DERIVED_CACHES and "_mttkrp_plan" in _dot.DERIVED_CACHES
    assert K.SOFTMAX_CHUNK % 64 == 0 and 64 <= K.SOFTMAX_CHUNK <= K.SOFTMAX_MAX_CHUNK and 0 <= K.SOFTMAX_SHORT_MAX <= 64
    assert K.SOFTMAX_GROUP in K.SOFTMAX_GROUPS == (8, 16, 32, 64)


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch"""
    from sparse_amd import _ffi

    f = hiplib.spamd_softmax

    def call(val=_ffi.F32, idx=_ffi.I64, nseg=3, nnz=200, group=16, short_max=64, chunk=64, max_len=100, ws_bytes=0):
        return f(val, idx, nseg, nnz, None, None, None, 0, 1.0, group, short_max, chunk, max_len, None, ws_bytes, None, None)

    assert call(val=_ffi.I32) == -2 and call(val=_ffi.C64) == -2 and call(val=_ffi.F16) == -2 and call(idx=_ffi.F32) == -2
    assert call(nseg=-1) == -1 and call(nnz=-1) == -1 and call(max_len=-1) == -1 and call(max_len=201) == -1
    assert call(group=0) == -1 and call(group=12) == -1 and call(group=128) == -1
    assert call(chunk=0) == -1 and call(chunk=32) == -1 and call(chunk=100) == -1 and call(chunk=2048) == -1
    assert call(short_max=-1) == -1 and call(short_max=65) == -1
    assert call(nseg=0) == 0 and call(nnz=0, max_len=0) == 0 and call(max_len=0) == 0
    assert call() == -1                                    # null pointers with work to do
    ws = hiplib.spamd_softmax_ws_bytes
    assert ws(_ffi.F32, 64, 64) == 0 and ws(_ffi.F32, 65, 64) == 8 * 2 * 4 and ws(_ffi.F64, 1000, 128) == 8 * 8 * 8
    assert ws(_ffi.I32, 10, 64) == -2 and ws(_ffi.F32, 10, 0) == -1 and ws(_ffi.F32, 10, 96) == -1 and ws(_ffi.F32, -1, 64) == -1


# ---- the exponential ---------------------------------------------------------------------------------------------------------------
def test_vector_fmas_equal_the_scalar_ones_of_masked_cases():
    """the restatement's array fmas against `masked_cases.fma32` / `fma64`, on random operands, on operands that cancel and
    on the very operands exp_det feeds them"""
    rng = np.random.default_rng(5)
    n = 1500
    for dtype, vec, scalar in ((np.float32, sc.fma32v, mc.fma32), (np.float64, sc.fma64v, mc.fma64)):
        a = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(dtype)
        b = rng.standard_normal(n).astype(dtype)
        c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 8 * np.finfo(dtype).eps)).astype(dtype)   # cancels
        k = np.rint(rng.uniform(-150, 0, n)).astype(dtype)
        d = (k * 0.6931 + rng.uniform(-0.3, 0.3, n)).astype(dtype)
        ln2_hi = dtype(sc._CONSTS[np.dtype(dtype)]["ln2_hi"])
        for x, y, z in ((a, b, c), (a, b, rng.standard_normal(n).astype(dtype)), (-k, np.full(n, ln2_hi), d),
                        (b * dtype(0.3), b * dtype(0.2), np.full(n, dtype(1.0)))):
            got = vec(x, y, z)
            want = np.array([scalar(p, q, r) for p, q, r in zip(x, y, z)], dtype=dtype)
            assert got.dtype == np.dtype(dtype) and sc.same_bits(got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exp_det_facts(dtype):
    dtype = np.dtype(dtype)
    T, fi, lo = dtype.type, np.finfo(dtype), sc._CONSTS[dtype]["lo"]
    got = sc.exp_det(np.array([0.0, -0.0, -np.inf, np.nan, lo - 1e-3 * abs(lo), 10 * lo, np.nextafter(T(lo), T(-np.inf))]), dtype)
    assert got[0] == 1 and got[1] == 1 and not np.signbit(got[:2]).any()
    assert got[2] == 0 and not np.signbit(got[2]) and np.isnan(got[3])
    assert (got[4:] == 0).all() and not np.signbit(got[4:]).any()
    # the threshold is where the exact exponential rounds to +0: below half the smallest subnormal
    assert np.exp(np.longdouble(lo)) < np.longdouble(fi.smallest_subnormal) / 2
    # a subnormal result is rounded once: where it has at most nmant - 12 bits left, the polynomial's own error (below one
    # ulp of a full significand) is below 2^-11 of the smallest subnormal, so the whole error stays within 1/2 + 2^-10 of it
    # (a second rounding could add another half); everywhere it stays within U; and the smallest subnormal is reached
    d = np.linspace(lo, float(np.log(fi.smallest_normal)), 4001).astype(dtype)
    e = sc.exp_det(d, dtype)
    assert (e >= 0).all() and (np.diff(e) >= 0).all() and e[0] == 0 and (e == fi.smallest_subnormal).any()
    err = sc.ulp_error(e, np.exp(d.astype(np.longdouble)))
    deep = e < np.ldexp(1.0, fi.minexp - 12)
    assert deep.sum() > 1000 and err[deep].max() <= 0.5 + 2.0 ** -10 and err.max() <= sc.U[dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exp_det_meets_the_measured_accuracy(dtype):
    """the seeded sample of tools/exp_det_ulp.py at a size for a second or two: float32 against float64 np.exp, float64 against
    longdouble np.exp and - 4000 arguments - mpmath.  U is the measured value rounded up to the next half ulp; at most 3"""
    import mpmath

    dtype = np.dtype(dtype)
    assert sc.U[dtype] <= sc.U_MAX and sc.U[dtype] * 2 == int(sc.U[dtype] * 2)
    rng = np.random.default_rng(11)
    d = sc.exp_arguments(rng, 400_000, dtype)
    wide = np.float64 if dtype == F32 else np.longdouble
    worst = sc.ulp_error(sc.exp_det(d, dtype), np.exp(d.astype(wide))).max()
    print(f"exp_det {dtype}: {worst:.4f} ulp over {len(d)} arguments (U = {sc.U[dtype]})")
    assert sc.U[dtype] - 0.5 < worst <= sc.U[dtype]
    d = sc.exp_arguments(rng, 4000, dtype)
    with mpmath.workprec(200):
        want = np.array([np.longdouble(mpmath.nstr(mpmath.exp(mpmath.mpf(float(v))), 25)) for v in d], dtype=np.longdouble)
    assert sc.ulp_error(sc.exp_det(d, dtype), want).max() <= sc.U[dtype]


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_scipy_and_torch_sparse_softmax():
    """float64 on a random 7 x 9 case and a 3-D one: scipy.special.softmax of the dense array with -inf at the unstored
    positions and torch.sparse.softmax on the CPU, both within the bound of the tolerance tests (tests/softmax_cases.py) plus
    the comparison value's own rounding, 4 eps"""
    import scipy.special
    import torch

    for seed, shape, nnz, axis in ((1, (7, 9), 30, 1), (2, (7, 9), 30, 0), (3, (4, 5, 6), 50, 2), (4, (4, 5, 6), 50, 0)):
        coords, data, shape = sc.random_array(seed, shape, nnz, np.float64)
        got = sc.softmax_restated(coords, data, shape, axis, 64)
        want, bound = sc.exact_and_bound(coords, data, shape, axis, use_mpmath=True)
        assert sc.bound_share(got, want, bound) <= 1
        dense = sc.dense_neg_inf(coords, data, shape)
        with np.errstate(all="ignore"):
            ref = scipy.special.softmax(dense, axis=axis)[tuple(coords)]
        ts = torch.sparse.softmax(torch.sparse_coo_tensor(torch.from_numpy(coords), torch.from_numpy(data), shape).coalesce(), axis)
        assert np.array_equal(ts.indices().numpy(), coords)
        for other in (ref, ts.values().numpy()):
            assert (np.abs(got - other) <= bound.astype(np.float64) + 4 * np.finfo(np.float64).eps * other).all()
    # an empty group stays empty, and is no NaN; the -inf image has NaN there, which is why it is read at stored positions
    coords, data, shape = sc.rows_array(5, [3, 0, 2], np.float64)
    got = sc.softmax_restated(coords, data, shape, 1, 64)
    assert len(got) == 5 and np.isfinite(got).all() and abs(got[:3].sum() - 1) < 1e-15 and abs(got[3:].sum() - 1) < 1e-15


def test_restatement_cuts_groups_into_pieces():
    """one group of chunk + 1 = 65 float32 elements: chunk 64 gives fold(e_0 .. e_63) + e_64, one piece gives accumulator 0 =
    e_0 + e_64 before the fold - different bits on this seed -, and n <= chunk is one piece whatever the chunk"""
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(65) * 3).astype(np.float32)
    cut, whole = sc.group_softmax(x, 64), sc.group_softmax(x, 128)
    e = sc.exp_det(x - x.max(), np.float32)

    def fold(a):
        a = a.copy()
        h = 32
        while h:
            a = a[:h] + a[h:2 * h]
            h //= 2
        return a[0]

    assert sc.same_bits(cut, e / (fold(e[:64]) + e[64]))
    first = e[:64].copy()
    first[0] = first[0] + e[64]
    assert sc.same_bits(whole, e / fold(first))
    assert not sc.same_bits(cut, whole) and np.abs(cut - whole).max() <= 4 * np.finfo(np.float32).eps * whole.max()
    for n in (1, 2, 63, 64):
        assert sc.same_bits(sc.group_softmax(x[:n], 64), sc.group_softmax(x[:n], 1024))
    # a short group follows the same tree: accumulators without an element are +0.0
    e3 = sc.exp_det(x[:3] - x[:3].max(), np.float32)
    assert sc.same_bits(sc.group_softmax(x[:3], 64), e3 / ((e3[0] + e3[2]) + e3[1]))
    assert sc.listed_lengths(64).count(0) >= 6 and sc.listed_lengths(64)[0] == 0 == sc.listed_lengths(64)[-1]


def test_restatement_special_values():
    inf, nan = np.inf, np.nan
    for dtype in (np.float32, np.float64):
        g = lambda *v: sc.group_softmax(np.array(v, dtype=dtype), 64)                      # noqa: E731
        assert np.isnan(g(1, nan, 3)).all() and np.isnan(g(1, inf, 3)).all() and np.isnan(g(-inf, -inf)).all()
        out = g(-inf, 0.5, 2.0)
        assert out[0] == 0 and not np.signbit(out[0]) and abs(out[1:].sum() - 1) < 4 * np.finfo(dtype).eps
        assert g(7.25)[0] == 1 and g(-0.0)[0] == 1 and (g(*[3.5] * 8) == 0.125).all() and (g(*[-2.0] * 64) == 2.0 ** -6).all()
        spread = g(0, -50, -90, -100, -103.5, -200, -740, -745.2, -2000)
        assert spread[0] == 1 and (np.diff(spread) <= 0).all() and spread[-1] == 0
        assert sc.same_bits(sc.group_softmax(np.array([1, -2, 0.5], dtype=dtype), 64, scale=-1.5),
                            g(*(dtype(-1.5) * np.array([1, -2, 0.5], dtype=dtype))))


# ---- the public function's argument checks (they come before anything touches a device) ---------------------------------------------
def test_python_argument_errors():
    """`softmax` refuses anything but a COO / GCXS first, then checks value type, axes and scale (`_check_arguments`: no array
    is needed) and the fill value"""
    import sparse_amd
    from sparse_amd._softmax import _check_arguments as check

    for bad in (np.zeros((3, 3)), None, [[1.0]]):
        with pytest.raises(TypeError, match="COO or GCXS"):
            sparse_amd.softmax(bad)
    for dt in (np.complex64, np.complex128):
        with pytest.raises(TypeError, match="complex"):
            check(dt, 2, -1, None)
    with pytest.raises(TypeError, match="16-bit"):
        check(np.float16, 2, -1, None)
    with pytest.raises(ValueError, match="at least 1 dimension"):
        check(np.float32, 0, -1, None)
    for bad in (2, -3, (0, 2)):
        with pytest.raises(ValueError, match="Invalid axis"):
            check(np.float32, 2, bad, None)
    with pytest.raises(ValueError, match="repeated"):
        check(np.float32, 2, (1, -1), None)
    with pytest.raises(ValueError, match="not understood"):
        check(np.float32, 2, 1.5, None)
    with pytest.raises(ValueError):
        check(np.float32, 2, None, None)
    with pytest.raises(ValueError, match="at least one axis"):
        check(np.float32, 2, (), None)
    for bad in ("2", 1j, True, [1.0]):
        with pytest.raises(TypeError, match="scale"):
            check(np.float32, 2, 1, bad)
    assert check(np.float32, 3, (-1, 0), 0.5) == (0, 2) and check(np.int64, 2, 1, np.float32(2)) == (1,)
    assert check(np.bool_, 1, -1, -3) == (0,) and check(np.float64, 4, 2, None) == (2,)

"""masked_matmul without a GPU: the C ABI and the public surface are in place, the fixture holds its generator's cases, the
NumPy restatement of the order contract (tests/masked_cases.py) - which judges the kernel bit for bit in
tests/test_masked_matmul_gpu.py - equals the reference's results value for value, and the argument errors that need no
device are raised."""
import importlib.util
import os

import numpy as np
import pytest

import masked_cases as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_masked_matmul_golden", os.path.join(ROOT, "tools", "gen_masked_matmul_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return mk.load_golden()


def test_c_abi_and_public_function(hiplib):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    name = "spamd_masked_spgemm"
    assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES[name][1]) == 22
    assert callable(sparse_amd.masked_matmul) and "masked_matmul" in sparse_amd.__all__
    assert K.MASKED_GROUP in K.MASKED_GROUPS and 1 <= K.MASKED_CAP <= K.MASKED_MAX_CAP and K.MASKED_WINDOW >= 1


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch (`zeros` is NULL, so nothing is cleared either)"""
    from sparse_amd import _ffi

    f = hiplib.spamd_masked_spgemm

    def call(val=_ffi.F32, idx=_ffi.I64, M=3, N=3, K=3, nnz=4, group=16, cap=64, window=8):
        return f(val, idx, M, N, K, nnz, None, None, None, None, None, None, None, None, None, group, cap, window, None, None, 0, None)

    assert call(val=_ffi.C64) == -2 and call(val=_ffi.U8) == -2 and call(idx=_ffi.F32) == -2
    assert call(M=-1) == -1 and call(N=-1) == -1 and call(K=-1) == -1 and call(nnz=-1) == -1
    assert call(group=0) == -1 and call(group=24) == -1 and call(group=128) == -1
    assert call(cap=0) == -1 and call(cap=2049) == -1 and call(window=0) == -1
    assert call(nnz=0) == 0 and call(M=0) == 0 and call(N=0) == 0
    for val in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.I64):
        for group in (8, 16, 32, 64):
            assert call(val=val, group=group, nnz=0) == 0
    assert call() == -1                                    # null pointers with work to do


def test_fixture_holds_exactly_the_generators_cases():
    names = _generator().case_names()
    assert len(names) == len(set(names))
    z = np.load(mk.GOLDEN)
    assert sorted({k.split("__")[0] for k in z.files}) == sorted(names)
    assert os.path.getsize(mk.GOLDEN) < 200 * 1024
    assert all(z[k].dtype.kind in "fiub" for k in z.files)      # arrays only


def test_fixture_covers_the_listed_ground(golden):
    assert {c["out"].dtype for c in golden.values()} == {np.dtype("float32"), np.dtype("float64"), np.dtype("int64")}
    for op in range(3):
        assert {c["formats"][op] for c in golden.values()} == {0, 1, 2}
    assert any((c["s"][1] < 0).any() and c["s"][1].dtype.kind == "f" for c in golden.values())
    assert any((np.bincount(c["a"][0][0], minlength=c["a"][2][0]) == 0).any() for c in golden.values())
    assert any((np.bincount(c["b"][0][1], minlength=c["b"][2][1]) == 0).any() for c in golden.values())
    assert any(len({c[op][1].dtype for op in "sab"}) > 1 for c in golden.values())
    for name in ("triangles_i64_coo", "triangles_i64_gcxs"):
        c = golden[name]
        a = mk.dense_of(c["a"])
        assert a.dtype == np.int64 and np.array_equal(a, a.T) and set(np.unique(a)) == {0, 1}
        assert c["out"].sum() == np.trace(np.linalg.matrix_power(a, 3)) > 0


def test_restatement_equals_every_fixture_case(golden):
    """dense images with ==: values bit-equal, signed zeros equal.  The reference's result type is the restatement's; both
    the exact and, where no rounding is involved (integers), the fused form."""
    for name, c in golden.items():
        dt = c["out"].dtype
        assert dt == np.result_type(c["s"][1].dtype, (np.zeros((), c["a"][1].dtype) * np.zeros((), c["b"][1].dtype)).dtype), name
        got = mk.dense_result(c["s"], mk.masked_restated(c["s"], c["a"], c["b"], dt))
        assert got.shape == c["out"].shape and (got == c["out"]).all(), name
        outside = mk.dense_of(c["s"]) == 0
        assert (c["out"][outside] == 0).all(), name
        if dt.kind == "i":
            fused = mk.dense_result(c["s"], mk.masked_restated(c["s"], c["a"], c["b"], dt, fused=True))
            assert (fused == c["out"]).all(), name


def test_fused_form_stays_within_the_bound_of_the_exact_value(golden):
    seen = 0.0
    for name, c in golden.items():
        dt = c["out"].dtype
        if dt.kind != "f":
            continue
        got = mk.masked_restated(c["s"], c["a"], c["b"], dt, fused=True)
        want, bound = mk.exact_and_bound(c["s"], c["a"], c["b"], dt)
        err = mk.abs_err(got, want)
        assert (err <= bound).all(), name
        seen = max(seen, float(np.max(err / np.maximum(bound, 1e-300))))
    assert 0 < seen <= 1


def test_host_fma_is_exactly_rounded():
    """cases where round(round(a * b) + c) and fma(a, b, c) differ, and a float32 case where rounding the float64 sum to
    nearest first would round twice"""
    a = np.float32(1 + 2.0 ** -12)
    assert mk.fma32(a, a, np.float32(-1)) == np.float32(2.0 ** -11 + 2.0 ** -24) != np.float32(a * a) + np.float32(-1)
    x = 1 + 2.0 ** -30
    assert mk.fma64(x, x, -1.0) == 2.0 ** -29 + 2.0 ** -60 != (x * x) - 1.0
    # p = (1 + 2^-23) * 2^-24 (1 - 2^-23) = 2^-24 - 2^-70 and c = 1 + 2^-23: p + c lies 2^-70 BELOW the midpoint of c and its
    # upper float32 neighbour, so the fma is c; float64 nearest lands on the midpoint and ties-to-even would then go UP
    p1, p2, c = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24 - 2.0 ** -47), np.float32(1 + 2.0 ** -23)
    assert float(p1) * float(p2) == 2.0 ** -24 - 2.0 ** -70
    assert np.float32(float(p1) * float(p2) + float(c)) == np.float32(1 + 2.0 ** -22)
    assert mk.fma32(p1, p2, c) == c
    assert mk.fma32(np.float32(3), np.float32(5), np.float32(-15)) == 0 and not np.signbit(mk.fma32(np.float32(3), np.float32(5), np.float32(-15)))
    assert np.isnan(mk.fma32(np.float32(np.nan), np.float32(1), np.float32(1))) and np.isnan(mk.fma64(np.inf, 0.0, 1.0))
    assert mk.fma64(np.inf, 2.0, 1.0) == np.inf


def test_restatement_order_and_empty_intersections():
    """ascending k, sequential from +0; the mask multiply last; NaN mask value over an empty intersection gives +0"""
    f = np.float32
    a = (np.array([[0, 0, 0], [1, 3, 6]]), np.array([1e8, 1.0, -1e8], f), (2, 8))
    b = (np.array([[1, 3, 5, 6], [0, 0, 0, 0]]), np.array([1.0, 1.0, 7.0, 1.0], f), (8, 2))
    s = (np.array([[0, 0, 1], [0, 1, 0]]), np.array([2.0, np.nan, np.nan], f), (2, 2))
    got = mk.masked_restated(s, a, b, f)
    assert got[0] == f(2) * ((f(0) + f(1e8)) + f(1) + f(-1e8)) == 0       # (1e8 + 1) - 1e8 in float32: the 1 is lost
    assert got[1] == 0 and not np.signbit(got[1]) and got[2] == 0           # no common k: +0 under a NaN mask value
    assert np.array_equal(mk.term_counts(s, a, b), [3, 0, 0])
    i = np.int32
    big = (np.array([[0], [0]]), np.array([2 ** 30], i), (1, 1))
    assert mk.masked_restated((big[0], np.array([3], i), (1, 1)), big, big, i)[0] == 0    # 2^60 wraps to 0 in int32


def test_argument_errors_that_need_no_device():
    import sparse_amd

    with pytest.raises(TypeError, match="sddmm"):
        sparse_amd.masked_matmul(np.ones((3, 3)), np.ones((3, 3)), np.ones((3, 3)))
    with pytest.raises(TypeError, match="sddmm"):
        sparse_amd.masked_matmul(None, None, None)

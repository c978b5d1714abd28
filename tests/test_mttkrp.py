"""MTTKRP without a GPU: the C ABI and the public surface are in place, the fixture holds its generator's cases, and the NumPy
restatement of the order contract (tests/mttkrp_cases.py) - which judges the kernel bit for bit in tests/test_mttkrp_gpu.py -
agrees with the reference's results and with float64 np.einsum."""
import importlib.util
import os

import numpy as np
import pytest

import mttkrp_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mttkrp_golden", os.path.join(ROOT, "tools", "gen_mttkrp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_c_abi_public_function_and_cache_key(hiplib):
    import sparse_amd
    from sparse_amd import _dot, _ffi

    for name in ("spamd_mttkrp", "spamd_mttkrp_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_mttkrp"][1]) == 21
    assert callable(sparse_amd.mttkrp) and "mttkrp" in sparse_amd.__all__
    assert "_mttkrp_plan" in _dot.DERIVED_CACHES


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch (type codes, sizes, ndim, mode, chunk, R == 0)"""
    from sparse_amd import _ffi

    f = hiplib.spamd_mttkrp

    def call(val=_ffi.F32, idx=_ffi.I64, ndim=3, mode=0, nnz=4, R=2, ldc=4, nrows=3, chunk=8, ldo=2):
        return f(val, idx, ndim, mode, nnz, R, None, ldc, None, None, None, None, None, nrows, chunk, None, 0, None, ldo, 0, None)

    assert call(val=_ffi.I32) == -2 and call(val=_ffi.C64) == -2 and call(idx=_ffi.F32) == -2
    assert call(nnz=-1) == -1 and call(R=-1) == -1 and call(nrows=-1) == -1
    assert call(ndim=1) == -1 and call(ndim=9) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(chunk=0) == -1 and call(ldo=1) == -1
    assert call(R=0, ldo=0) == 0 and call(nrows=0) == 0
    assert call() == -1                                    # null pointers with work to do
    ws = hiplib.spamd_mttkrp_ws_bytes
    assert ws(_ffi.F32, 100, 5, 100) == 0 and ws(_ffi.F32, 101, 5, 100) == 2 * 2 * 5 * 4 and ws(_ffi.F64, 17, 3, 8) == 2 * 3 * 3 * 8
    assert ws(_ffi.I32, 10, 5, 8) == -2 and ws(_ffi.F32, 10, 5, 0) == -1


def test_fixture_holds_exactly_the_generators_cases():
    names = _generator().case_names()
    assert len(names) == len(set(names))
    z = np.load(mc.GOLDEN)
    assert sorted({k.split("__")[0] for k in z.files}) == sorted(names)
    assert os.path.getsize(mc.GOLDEN) < 200 * 1024
    assert all(z[k].dtype.kind in "fiub" for k in z.files)      # arrays only


@pytest.fixture(scope="module")
def golden():
    return mc.load_golden()


def test_fixture_covers_the_listed_ground(golden):
    dims = {len(c["shape"]) for c in golden.values()}
    assert dims == {2, 3, 4, 5}
    for nd in (3, 4):
        assert {c["mode"] for c in golden.values() if len(c["shape"]) == nd} >= set(range(nd))
    assert {c["gcxs"] for c in golden.values()} == {True, False}
    fdts = {next(f for f in c["factors"] if f is not None).dtype for c in golden.values()}
    assert fdts == {np.dtype("float32"), np.dtype("float64")}
    assert {c["data"].dtype for c in golden.values()} >= {np.dtype("int64"), np.dtype("float32")}
    assert {next(f for f in c["factors"] if f is not None).shape[1] for c in golden.values()} == {1, 5, 25}
    assert any(1 in c["shape"] for c in golden.values())
    assert any((np.bincount(c["coords"][c["mode"]], minlength=c["shape"][c["mode"]]) == 0).any() for c in golden.values())


@pytest.mark.parametrize("chunk", [1, 3, 10 ** 9])
def test_restatement_in_float64_agrees_with_the_reference_and_einsum(golden, chunk):
    """|restated - reference| <= (n + ndim) * (eps64 + eps of the reference's result type) * sum|terms|, and twice the
    float64 bound against np.einsum (both sides are float64 sums in different orders)"""
    for name, c in golden.items():
        args = (c["coords"], c["data"], c["shape"], c["factors"], c["mode"])
        got = mc.mttkrp_restated(*args, chunk, np.float64)
        assert got.dtype == np.float64 and got.shape == c["out"].shape, name
        want = mc.mttkrp_einsum(*args)
        assert (np.abs(got - want) <= mc.bound(*args, np.float64, np.float64)).all(), name
        assert (np.abs(got - c["out"]) <= mc.bound(*args, np.float64, c["out"].dtype)).all(), name
        empty = np.bincount(c["coords"][c["mode"]], minlength=c["shape"][c["mode"]]) == 0
        assert not np.signbit(got[empty]).any() and (got[empty] == 0).all(), name


def test_restatement_cuts_rows_into_pieces():
    """float32, one row of 9 elements: chunk 4 gives ((t0+t1+t2+t3) + (t4+..+t7)) + t8 - not the sequential sum - and the
    generators build what they promise"""
    coords, data, shape = mc.rows_tensor(5, [0, 9, 1], (4, 5), 1, np.float32)
    assert shape == (4, 3, 5) and np.bincount(coords[1], minlength=3).tolist() == [0, 9, 1]
    key = np.ravel_multi_index(tuple(coords), shape)
    assert (np.diff(key) > 0).all()
    fac = mc.factors_for(5, shape, 3, np.float32, mode=1)
    seq = mc.mttkrp_restated(coords, data, shape, fac, 1, 100, np.float32)
    cut = mc.mttkrp_restated(coords, data, shape, fac, 1, 4, np.float32)
    terms = data[:, None] * fac[0][coords[0]] * fac[2][coords[2]]
    rows = np.flatnonzero(coords[1] == 1)
    t = terms[rows]
    z = np.zeros(3, np.float32)
    p0 = (((z + t[0]) + t[1]) + t[2]) + t[3]
    p1 = (((z + t[4]) + t[5]) + t[6]) + t[7]
    assert np.array_equal(cut[1], (p0 + p1) + (z + t[8]))
    s = z
    for x in t:
        s = s + x
    assert np.array_equal(seq[1], s)
    assert np.array_equal(seq[0], z) and np.array_equal(seq[2], cut[2])

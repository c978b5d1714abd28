"""Complex elementwise operations and reductions, the parts that need no GPU: the C-ABI declarations, the host-side route
tables, the committed fixture against its generator's case list, and the summation order of the device sums - restated in
Python (`_reduce.pairwise_order_sum`) and held to `np.add.reduceat` bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "complex_ew.npz")
ENTRY_POINTS = ("spamd_cplx_binary", "spamd_cplx_unary", "spamd_cplx_convert", "spamd_cplx_fill", "spamd_merge_union_complex",
                "spamd_cplx_segment_reduce", "spamd_cplx_sum_long_ws_bytes", "spamd_cplx_sum_long")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_complex_ew_golden", os.path.join(ROOT, "tools", "gen_complex_ew_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_in_header_and_ffi():
    from sparse_amd import _ffi

    syms = set(_ffi.header_symbols())
    for name in ENTRY_POINTS:
        assert name in syms and name in _ffi.SIGNATURES, name
    # the value kernels take spamd_ewise_binary's / spamd_ewise_unary's argument lists
    assert _ffi.SIGNATURES["spamd_cplx_binary"] == _ffi.SIGNATURES["spamd_ewise_binary"]
    assert _ffi.SIGNATURES["spamd_cplx_unary"] == _ffi.SIGNATURES["spamd_ewise_unary"]
    assert _ffi.SIGNATURES["spamd_cplx_convert"] == _ffi.SIGNATURES["spamd_convert"]


def test_route_tables():
    """The complex ops have tables of their own (the real tables are the conformance suite's key set); binary codes are
    the real kernels' codes; nothing outside the issue's list is in them."""
    from sparse_amd import _reduce, _trace, _umath

    assert set(_umath._CBIN) == {"add", "subtract", "multiply", "divide", "true_divide", "equal", "not_equal"}
    assert all(_umath._CBIN[k] == _umath._BIN[k] for k in _umath._CBIN)
    assert set(_umath._CUN) == {"negative", "positive", "conjugate", "conj", "square", "absolute", "abs", "real", "imag",
                                "isnan", "isinf", "isfinite"}
    for host_only in ("power", "maximum", "minimum", "greater", "less", "logical_and", "reciprocal", "sign", "exp", "sqrt"):
        assert host_only not in _umath._CBIN and host_only not in _umath._CUN
    assert "absolute" not in _trace._COMPLEX_UN      # within 4 ulp, not identical: not a traced op

    class X:
        def __init__(self, dt, fill):
            import torch

            self.data = torch.zeros(1, dtype=getattr(torch, dt))
            self.dtype = np.dtype(dt)
            self.fill_value = np.dtype(dt).type(fill)

    for dt in ("complex64", "complex128"):
        assert _reduce._complex_reducible(X(dt, 0), "add", None, {})
        assert _reduce._complex_reducible(X(dt, 2 - 1j), "add", np.dtype(dt), {})
        assert _reduce._complex_reducible(X(dt, 1), "multiply", None, {}) and _reduce._complex_reducible(X(dt, 0), "multiply", None, {})
        assert not _reduce._complex_reducible(X(dt, 1 + 0.5j), "multiply", None, {})      # np.power(fill, n_missing)
        assert not _reduce._complex_reducible(X(dt, 0), "maximum", None, {})
        assert not _reduce._complex_reducible(X(dt, 0), "add", None, {"where": None})
        assert not _reduce._complex_reducible(X(dt, 0), "add", np.float64, {})
    assert not _reduce._complex_reducible(X("float64", 0), "add", None, {})


LENGTHS = list(range(1, 200)) + [255, 256, 257, 1000, 4097, 20_000, 100_003]


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_pairwise_order_equals_reduceat(dt):
    """x0 + P(x1 ..): the order `np.add.reduceat` sums a run in, which is the order the device kernels are written to"""
    from sparse_amd._reduce import pairwise_order_sum

    rng = np.random.default_rng(7)
    for m in LENGTHS:
        x = ((rng.standard_normal(m) * 10) + 1j * rng.standard_normal(m)).astype(dt)
        want = np.add.reduceat(x, [0])[0]
        got = pairwise_order_sum(x)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (m, got, want)
    # several runs in one call: each run on its own
    x = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(dt)
    heads = [0, 1, 3, 7, 12, 77, 142, 271, 400]
    want = np.add.reduceat(x, heads)
    for g, (s, e) in enumerate(zip(heads, heads[1:] + [700])):
        assert pairwise_order_sum(x[s:e]).tobytes() == want[g].tobytes(), g


def test_fixture_holds_every_case_of_its_generator():
    gen = _generator()
    names = gen.case_names()
    assert len(names) == len(set(names))
    z = np.load(GOLD)
    have = {k.split("__")[0] for k in z.files} - {"in"}
    assert have == set(names)
    assert {k[4:] for k in z.files if k.startswith("in__")} == set(gen.inputs())
    for k in z.files:
        assert z[k].dtype.kind in "biufc", (k, z[k].dtype)       # arrays of numbers only
    for name in names:
        assert f"{name}__out" in z.files or all(f"{name}__{f}" in z.files for f in ("coords", "data", "fill", "meta")), name
    # the ground the issue asks for: every op x both types x the paths; run lengths on both sides of 4, 8, 64 and 128
    for tag in ("c64", "c128"):
        for op in gen.BINARY:
            for path in ("coo", "bcast", "scalar", "rscalar_fill", "gcxs_rows", "gcxs_cols", "mixed_real", "mixed_int"):
                assert f"{op}_{path}_{tag}" in names
        for op in gen.UNARY:
            assert {f"{op}_coo_{tag}", f"{op}_fill_{tag}", f"{op}_gcxs_{tag}"} <= set(names)
        for red in ("sum_rows", "sum_cols", "sum_all", "sum_all_keepdims", "sum_rows_fill", "mean_rows", "sum_3d_two_axes",
                    "sum_gcxs_rows", "sum_gcxs_cols", "prod_rows", "prod_fill_one"):
            assert f"{red}_{tag}" in names
        rows = z[f"in__red_coords_{tag}"][0]
        lengths = set(np.bincount(rows).tolist())
        assert {3, 4, 5, 8, 9, 64, 65, 66, 128, 129, 130} <= lengths and max(lengths) > 2000
        a, b = z[f"in__a_{tag}"], z[f"in__b_{tag}"]
        assert np.isinf(a).any() and np.isnan(a).any() and np.isinf(b).any()
        tiny = np.finfo(a.real.dtype).tiny
        assert ((np.abs(a.real) < tiny) & (a.real != 0)).any()                 # a denormal part
        both = (a != 0) & (b != 0)
        assert (np.abs(b.real[both]) < np.abs(b.imag[both])).any() and (np.abs(b.real[both]) >= np.abs(b.imag[both])).any()
        assert ((a != 0) & (b == 0)).any()                                        # a zero divisor
        assert z[f"divide_coo_{tag}__data"].dtype == a.dtype and z[f"absolute_coo_{tag}__data"].dtype == a.real.dtype
        assert z[f"equal_coo_{tag}__data"].dtype == np.dtype(bool)
    assert os.path.getsize(GOLD) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "complex_dot.npz"))

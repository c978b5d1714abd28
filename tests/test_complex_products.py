"""Complex matrix products, the parts that need no GPU: the C-ABI codes and declaration, the route of a complex
`sparse @ dense` product, the capability probe `code_of`, and the committed fixture against its generator's case list."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "complex_dot.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_complex_golden", os.path.join(ROOT, "tools", "gen_complex_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_complex_codes_in_header_and_ffi():
    from sparse_amd import _ffi

    text = open(_ffi.HEADER_PATH).read()
    codes = {name: int(val) for name, val in re.findall(r"#define\s+(SPAMD_C64|SPAMD_C128|SPAMD_U8)\s+(\d+)", text)}
    assert codes == {"SPAMD_U8": 5, "SPAMD_C64": 6, "SPAMD_C128": 7}
    assert (_ffi.U8, _ffi.C64, _ffi.C128) == (5, 6, 7)
    assert "spamd_spmm_csr_complex" in _ffi.header_symbols()
    # the argument list of spamd_spmm_csr
    assert _ffi.SIGNATURES["spamd_spmm_csr_complex"] == _ffi.SIGNATURES["spamd_spmm_csr"]


def test_code_of_still_refuses_complex():
    """`code_of` raising TypeError is the "is this a device dtype" probe of the elementwise and reduction layers, which have
    no complex kernels: the products have a lookup of their own."""
    from sparse_amd import _device, _ffi, _kernels

    for dt in (np.complex64, np.complex128, torch.complex64, torch.complex128):
        with pytest.raises(TypeError, match="is not supported by the hip backend"):
            _device.code_of(dt)
    assert _kernels.product_code(np.complex64) == _ffi.C64 and _kernels.product_code(torch.complex128) == _ffi.C128
    assert _kernels.product_code(np.float32) == _ffi.F32 and _kernels.product_code(torch.int64) == _ffi.I64
    with pytest.raises(TypeError):
        _kernels.product_code(np.float16)


@pytest.mark.parametrize("vd, bd", [("complex64", "complex64"), ("complex128", "complex128"), ("float32", "complex64"),
                                    ("complex128", "float64"), ("float64", "complex128"), ("complex64", "float32")])
@pytest.mark.parametrize("M, Kd, N, nnz", [(1_000_000, 10_000, 128, 100_000_000), (1_000_000, 10_000, 1, 100_000_000),
                                           (200_000, 3_000, 8, 2_000_000), (60, 45, 7, 400), (70_000, 512, 64, 3_000_000)])
@pytest.mark.parametrize("form", ["csr", "csc", "coo"])
def test_complex_products_take_the_plain_route(vd, bd, M, Kd, N, nnz, form):
    """No executor, no stream passes and no hub-row split for a complex value or dense type, whatever the shape"""
    from sparse_amd import _dot as D

    for exact in (False, True):
        r = D._spmm_route(M, Kd, N, nnz, getattr(torch, vd), getattr(torch, bd), form, (), 0, 1 << 20, 2 << 20, "auto", exact, True)
        assert r.kind == "spmm_csr" and r.dt is None and r.passes == 0 and r.hub_from is None and not r.count


def test_fixture_holds_every_case_of_its_generator():
    gen = _generator()
    names = gen.case_names()
    assert len(names) == len(set(names))
    z = np.load(GOLD)
    have = {k.split("__")[0] for k in z.files}
    assert have == set(names)
    for k in z.files:
        assert z[k].dtype.kind in "iufc", (k, z[k].dtype)       # arrays of numbers only
    for name in names:
        assert any(f"{name}__{f}" in z.files for f in ("out", "out_data")), name
    # the ground the issue asks for
    widths = {int(re.search(r"_n(\d+)_", n).group(1)) for n in names if n.startswith("gd_")}
    assert widths == {1, 2, 3, 7, 64, 130}
    for tag in ("c64", "c128"):
        for fmt in ("csr", "csc"):
            assert {n.rsplit("_", 1)[1] for n in names if n.startswith(f"gd_{tag}_{fmt}_")} == {"int32", "int64"}
    for n in names:
        if n.startswith("gd_"):
            ptr = z[n + "__a_indptr"]
            b = z[n + "__b"]
            assert b.dtype.kind == "c" and z[n + "__out"].dtype == b.dtype
            if int(z[n + "__a_ca"][0]) == 0:
                assert ptr[3] == ptr[4]                          # an empty row
            if b.shape[1] > 1:
                assert not b[:, 0].any()                         # an all-zero dense column
    assert os.path.getsize(GOLD) < (1 << 20)

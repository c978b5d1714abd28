"""Host side of complex SDDMM (no GPU needed): the C-ABI symbols, the dtype lookups, which row lengths have the row-cached
kernel, and the argument checks of spamd_sddmm_complex that return before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

C64_K = (32, 64, 96, 128, 192, 256, 384, 512)        # 16-byte vectors = L * KS, L in 16 | 32 | 64, KS in 1..4
C128_K = (16, 32, 48, 64, 96, 128, 192, 256)


def test_symbols_in_header_table_and_library(hiplib):
    from sparse_amd import _ffi

    for name in ("spamd_sddmm_complex", "spamd_sddmm_complex_has_rowcache"):
        assert name in _ffi.header_symbols() and name in _ffi.SIGNATURES and hasattr(hiplib, name)
    assert len(_ffi.SIGNATURES["spamd_sddmm_complex"][1]) == 17
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)


def test_complex_code_lookup_is_its_own(hiplib):
    from sparse_amd import _device, _ffi
    from sparse_amd import _kernels as K

    assert K.sddmm_complex_code(torch.complex64) == K.sddmm_complex_code(np.complex64) == _ffi.C64 == 6
    assert K.sddmm_complex_code(torch.complex128) == K.sddmm_complex_code(np.complex128) == _ffi.C128 == 7
    for dt in (torch.float32, np.float64, torch.float16, torch.bfloat16, torch.int32, np.int64, torch.bool, torch.uint8):
        with pytest.raises(TypeError, match="complex sddmm supports"):
            K.sddmm_complex_code(dt)
    # the real lookups keep refusing complex types
    for dt in (torch.complex64, torch.complex128, np.complex64):
        with pytest.raises(TypeError, match="sddmm supports"):
            K.sddmm_code(dt)
        with pytest.raises(TypeError):
            _device.code_of(dt)
    assert torch.complex64 not in K.SDDMM_DTYPES and torch.complex128 not in K.SDDMM_DTYPES


def test_has_rowcache_exactly_for_the_instantiated_row_lengths(hiplib):
    from sparse_amd import _ffi
    from sparse_amd import _kernels as K

    f = hiplib.spamd_sddmm_complex_has_rowcache
    for code, dt, ks in ((_ffi.C64, torch.complex64, C64_K), (_ffi.C128, torch.complex128, C128_K)):
        yes = [k for k in range(-2, 2100) if f(code, k)]
        assert tuple(yes) == ks
        for k in ks:
            assert K.sddmm_has_panels(dt, k)
    for k in (31, 33, 80, 1024, 0, 16):
        assert f(_ffi.C64, k) == 0 and not K.sddmm_has_panels(torch.complex64, k)
    for k in (15, 80, 512, 0, 8):
        assert f(_ffi.C128, k) == 0 and not K.sddmm_has_panels(np.complex128, k)
    for code in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.I64, _ffi.BF16, _ffi.U8, _ffi.F16, 9, -1):
        assert f(code, 64) == 0
    # the real entry points' answers for complex codes stay "no kernel"
    for code in (_ffi.C64, _ffi.C128):
        assert hiplib.spamd_sddmm_has_panels(code, 64) == 0 and hiplib.spamd_sddmm_panel_row_bytes(code, 64) == 0


def test_panel_rules_answer_for_complex_rows(hiplib):
    """The host's traffic model sizes panels by row bytes: complex64 K = 128 (1 KB rows, one pass - no half-row trick) and
    K = 32 (256-byte rows) get a width, a K without the row-cached kernel gets none, and the inner dimension is never padded."""
    from sparse_amd import _kernels as K

    bt = torch.empty((100_000, 128), dtype=torch.complex64, device="meta")
    w = K.sddmm_panel_width(bt)
    assert w == 3125          # 32 panels (four per XCD) of 3125 rows of 1 KB
    assert K.sddmm_panels_pay(10_000_000, bt, bt, w)
    short = torch.empty((100_000, 32), dtype=torch.complex64, device="meta")
    assert K.sddmm_panel_width(short) == 12500
    assert K.sddmm_panel_width(torch.empty((100_000, 100), dtype=torch.complex64, device="meta")) == 0
    assert K.sddmm_panel_width(torch.empty((1000, 128), dtype=torch.complex128, device="meta")) == 0     # fits the L2
    a = torch.zeros((4, 100), dtype=torch.complex64)
    pa, pb = K.sddmm_pad_inner(a, a, 10 * K.SDDMM_PAD_MIN_NNZ)
    assert pa is a and pb is a


def test_entry_point_returns_before_launching(hiplib):
    from sparse_amd import _ffi

    f = hiplib.spamd_sddmm_complex
    al = 4096           # (an aligned address that is never dereferenced: every call below returns at its argument checks)

    def call(val=_ffi.C64, idx=_ffi.I32, nnz=1, lda=64, ldb=64, k=64, a=al, bt=al, perm=None, s=al, out=al):
        return f(val, idx, nnz, al, al, s, a, lda, bt, ldb, k, out, perm, 0, None, 0, None)

    for code in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.I64, _ffi.BF16, _ffi.U8, _ffi.F16, 9, -1):
        assert call(val=code) == -2, code
    for code in (_ffi.F32, _ffi.U8, _ffi.C64, 9, -1):
        assert call(idx=code) == -2, code
    # row pitch off the 16-byte grid (complex64: an odd pitch), misaligned operands, negative sizes
    assert call(lda=65) == -1 and call(ldb=33) == -1
    assert call(a=al + 8) == -1 and call(bt=al + 8) == -1
    assert call(val=_ffi.C128, s=al + 8) == -1 and call(val=_ffi.C128, out=al + 8) == -1
    assert call(nnz=-1) == -1 and call(k=-1) == -1
    assert call(lda=32, k=64) == -1          # a pitch shorter than the row
    # the panel order for a row length without the row-cached kernel
    perm = (ctypes.c_int64 * 1)(0)
    assert call(k=33, lda=34, ldb=34, perm=perm) == -1 and call(val=_ffi.C128, k=80, lda=80, ldb=80, perm=perm) == -1
    # nothing to do
    assert f(_ffi.C64, _ffi.I32, 0, None, None, None, None, 0, None, 0, 64, None, None, 0, None, 0, None) == 0
    assert f(_ffi.C128, _ffi.I64, 0, None, None, None, None, 0, None, 0, 0, None, None, 0, None, 0, None) == 0

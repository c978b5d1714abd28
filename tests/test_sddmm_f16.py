"""Host side of float16 SDDMM and of the N-D mask fold (no GPU needed): the C-ABI code and symbols, the dtype lookups, the
library's answers about row-cached kernels, the fold arithmetic and the shape errors."""
import ctypes

import numpy as np
import pytest
import torch


def test_f16_code_and_symbols(hiplib):
    from sparse_amd import _ffi

    assert _ffi.F16 == 8
    header = open(_ffi.HEADER_PATH).read()
    assert "#define SPAMD_F16 8" in header
    for name in ("spamd_sddmm_mfma_tiles_typed", "spamd_sddmm_batch_fold"):
        assert name in _ffi.header_symbols() and name in _ffi.SIGNATURES and hasattr(hiplib, name)
    assert hasattr(hiplib, "spamd_sddmm_mfma_tiles")        # the bf16 form keeps its symbol


def test_f16_has_panels_exactly_where_bf16_has(hiplib):
    from sparse_amd import _ffi
    from sparse_amd import _kernels as K

    yes = 0
    for k in list(range(0, 2100)) + [4096, 4104, 8192]:
        h, b = K.sddmm_has_panels(torch.float16, k), K.sddmm_has_panels(torch.bfloat16, k)
        assert h == b, k
        assert hiplib.spamd_sddmm_panel_row_bytes(_ffi.F16, k) == hiplib.spamd_sddmm_panel_row_bytes(_ffi.BF16, k)
        yes += h
    assert yes == len(K._SDDMM_ROW_BYTES)              # K = row bytes / 2 for every instantiated row length
    for rb in K._SDDMM_ROW_BYTES:
        assert K.sddmm_has_panels(torch.float16, rb // 2)
    assert K.sddmm_has_panels(np.float16, 256) and not K.sddmm_has_panels(torch.int32, 256)
    bt = torch.empty((100_000, 256), dtype=torch.float16, device="meta")
    bb = torch.empty((100_000, 256), dtype=torch.bfloat16, device="meta")
    assert K.sddmm_panel_width(bt) == K.sddmm_panel_width(bb) == 6250
    assert K.sddmm_panels_pay(10_000_000, bt, bt, 6250) and not K.sddmm_panels_pay(3_000_000, bt, bt, 6250)
    a = torch.zeros((4, 192), dtype=torch.float16)
    pa, pb = K.sddmm_pad_inner(a, a, K.SDDMM_PAD_MIN_NNZ)
    assert pa.shape == pb.shape == (4, 256) and pa.dtype == torch.float16


def test_f16_stays_unknown_to_the_other_dtype_lookups(hiplib):
    from sparse_amd import _device, _ffi
    from sparse_amd import _kernels as K

    for dt in (np.float16, torch.float16):
        with pytest.raises(TypeError):
            _device.code_of(dt)
        with pytest.raises(TypeError):
            K.product_code(dt)
        assert K.sddmm_code(dt) == _ffi.F16
    assert K.sddmm_code(torch.bfloat16) == _ffi.BF16 and K.sddmm_code(np.float32) == _ffi.F32 and K.sddmm_code(np.float64) == _ffi.F64
    for dt in (torch.int32, np.int64, torch.complex64, torch.uint8):
        with pytest.raises(TypeError, match="sddmm supports"):
            K.sddmm_code(dt)


def test_entry_points_refuse_element_types_without_a_kernel(hiplib):
    """Argument checks that return before anything is launched (no device needed)."""
    from sparse_amd import _ffi

    for code in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.U8, _ffi.C64, 9, -1):
        rc = hiplib.spamd_sddmm_mfma_tiles_typed(code, _ffi.I32, 1, None, None, None, None, 1, 32, 32, None, None, None, None, 16,
                                                 None, 16, 16, None, None)
        assert rc == -1, code
    for code in (_ffi.I32, _ffi.I64, _ffi.U8, _ffi.C64, _ffi.C128, 9):
        assert hiplib.spamd_sddmm_has_panels(code, 256) == 0 and hiplib.spamd_sddmm_panel_row_bytes(code, 256) == 0
        perm = (ctypes.c_int64 * 1)(0)
        rc = hiplib.spamd_sddmm_panels(code, _ffi.F32, _ffi.I32, 1, None, None, perm, None, 16, 256, 16, 256, 256, 0, None, 0, None,
                                       None, None)
        assert rc < 0, code
    one = (ctypes.c_int64 * 1)(1)
    assert hiplib.spamd_sddmm_batch_fold(_ffi.I32, _ffi.F32, 1, 1, 16, 1, one, one, 4, 4, 16, 16, None) < 0      # out_dtype
    assert hiplib.spamd_sddmm_batch_fold(_ffi.I32, _ffi.I32, 15, 1, 16, 1, one, one, 4, 4, 16, 16, None) == -1   # too many axes
    assert hiplib.spamd_sddmm_batch_fold(_ffi.I32, _ffi.I32, 1, 8, 16, 4, one, one, 4, 4, 16, 16, None) == -1    # pitch < nnz
    assert hiplib.spamd_sddmm_batch_fold(_ffi.I32, _ffi.I64, 1, 0, None, 0, one, one, 4, 4, None, None, None) == 0


def _fold_numpy(coords, strides_a, strides_b, M, N):
    """The fold as csrc/sddmm_batch.hip computes it."""
    p = coords.shape[0] - 2
    ba = sum(coords[d].astype(np.int64) * strides_a[d] for d in range(p)) if p else 0
    bb = sum(coords[d].astype(np.int64) * strides_b[d] for d in range(p)) if p else 0
    return ba * M + coords[p], bb * N + coords[p + 1]


@pytest.mark.parametrize("lead, la, lb", [((3,), (3,), (3,)), ((3,), (), (3,)), ((3,), (3,), (1,)), ((3,), (), ()),
                                          ((2, 5), (2, 5), (5,)), ((2, 5), (2, 1), (1, 5)), ((2, 5), (5,), (2, 1)),
                                          ((4, 1, 3), (4, 1, 3), (3,)), ((4, 1, 3), (1, 1, 1), (4, 1, 1)), ((1, 6), (1, 6), (6,)),
                                          ((2, 3, 4), (3, 1), (2, 1, 4))])
def test_fold_strides_against_ravel_multi_index(lead, la, lb):
    """row' / col' of every position of the mask = the flat row / column index into the operand AS IT IS STORED
    (np.ravel_multi_index over the operand's own leading shape, the broadcast axes' index clamped to 0)."""
    from sparse_amd import _kernels as K

    M, N = 5, 7
    shape = lead + (M, N)
    coords = np.stack(np.unravel_index(np.arange(int(np.prod(shape))), shape)).astype(np.int64)
    sa, nba = K.sddmm_fold_strides(lead, la, "a")
    sb, nbb = K.sddmm_fold_strides(lead, lb, "b")
    assert nba == int(np.prod(la)) and nbb == int(np.prod(lb))
    rows, cols = _fold_numpy(coords, sa, sb, M, N)
    p = len(lead)
    for got, op_lead, last, extent in ((rows, la, coords[p], M), (cols, lb, coords[p + 1], N)):
        full = (1,) * (p - len(op_lead)) + tuple(op_lead)
        idx = [np.where(full[d] == 1, 0, coords[d]) for d in range(p)] + [last]
        want = np.ravel_multi_index(idx, full + (extent,))
        assert np.array_equal(got, want)
        # and the same thing said with NumPy's own broadcasting: the operand's flat row numbers, broadcast to the mask
        flat = np.arange(int(np.prod(full)) * extent).reshape(full + (extent,))
        bc = np.broadcast_to(flat, lead + (extent,))
        assert np.array_equal(got, bc[tuple(coords[d] for d in range(p)) + (last,)])


def test_fold_shape_errors():
    from sparse_amd import _kernels as K

    with pytest.raises(ValueError, match="more leading axes"):
        K.sddmm_fold_strides((3,), (2, 3), "a")
    with pytest.raises(ValueError, match="more leading axes"):
        K.sddmm_fold_strides((), (1,), "b")
    with pytest.raises(ValueError, match="do not broadcast"):
        K.sddmm_fold_strides((3,), (2,), "a")
    with pytest.raises(ValueError, match="do not broadcast"):
        K.sddmm_fold_strides((1, 4), (3, 4), "b")          # an operand may not be larger than the mask
    with pytest.raises(ValueError, match="do not broadcast"):
        K.sddmm_fold_strides((2, 4), (4, 2), "a")
    assert K.sddmm_fold_strides((), (), "a") == ([], 1)
    assert K.sddmm_fold_strides((0, 3), (0, 3), "a") == ([3, 1], 0)
    assert K.sddmm_fold_strides((2, 3), (3,), "a") == ([0, 1], 3)

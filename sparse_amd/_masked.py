"""The sparse x sparse product sampled at a sparse mask - `s * (a @ b)` with all three operands sparse, GraphBLAS's `mxm`
under a structural mask - as one fused kernel (csrc/masked_spgemm.hip).  The reference has no function for it; its example
(examples/triangles_example.py) writes

    sparse.sum(a @ a * a) / 6

which forms the whole product `a @ a`, about (mean degree) times as many stored elements as the mask keeps."""
import numpy as np
import torch

from . import _device as dev
from . import _kernels as K
from . import _settings
from ._coo import COO
from ._gcxs import GCXS

_RESULT_DTYPES = tuple(np.dtype(t) for t in ("float32", "float64", "int32", "int64"))
_OPERAND_DTYPES = _RESULT_DTYPES + (np.dtype("bool"), np.dtype("uint8"))     # what `K.convert` takes


def _csc_triplet(b):
    """(data, indices, indptr) of 2-D `b` compressed by COLUMNS - the CSR triplet of `b.T` - from what `b` memoises: a
    column-compressed GCXS is that already (its own arrays, nothing converted), a row-compressed one keeps its transposed
    view (`_t_view`, which shares its buffers and holds the re-compressed twin), a COO its transposed CSR (`_csr_of_t`)."""
    from ._dot import _csr_triplet, _validate_derived

    if isinstance(b, COO):
        b.coords      # (a COO kept as linear keys: materialising its coordinates changes the stamp, so do it first)
    _validate_derived(b)
    if isinstance(b, GCXS):
        if b.compressed_axes == (1,):
            return b.data, b.indices, b.indptr
        bt = b.__dict__.get("_t_view")
        if bt is None or bt.data is not b.data or bt.indices is not b.indices:
            bt = b.__dict__["_t_view"] = b.T
        return _csr_triplet(bt)
    st = b.__dict__.get("_csr_of_t")
    if st is None:
        st = b.__dict__["_csr_of_t"] = K.coo_transposed_csr(b.coords, b.data, int(b.shape[0]), int(b.shape[1]))
    return st


def _empty_like_mask(s, dt):
    """the result without a stored element, in the mask's format, on its device; no library call"""
    tdt, d = dev.torch_dtype(dt), s.device
    if isinstance(s, GCXS):
        it = s.indices.dtype
        return GCXS((torch.zeros(0, dtype=tdt, device=d), torch.zeros(0, dtype=it, device=d),
                     torch.zeros(int(s.shape[s.compressed_axes[0]]) + 1, dtype=it, device=d)), shape=s.shape,
                    compressed_axes=s.compressed_axes)
    return COO(torch.zeros((2, 0), dtype=torch.int64, device=d), torch.zeros(0, dtype=tdt, device=d), shape=s.shape,
               has_duplicates=False, sorted=True)


def masked_matmul(s, a, b):
    """`s * (a @ b)` for sparse `s` (M x N), `a` (M x K) and `b` (K x N), evaluated only at the stored positions of the
    mask `s`: the product `a @ b` is never formed.

    Each operand is a 2-D COO or GCXS (any mix, either compressed axis) with a zero fill value.  The result type is
    `np.result_type(s.dtype, dot_dtype(a.dtype, b.dtype))` and must be float32, float64, int32 or int64; operands of another
    real, integer or boolean type are converted to it on the device.  The result has the format (and compressed axis) of
    `s`, lives on its device, is canonical and pruned, and stores nothing outside the pattern of `s`.

    At a stored mask position (i, j) with value m the terms are the k, ascending, stored in both row i of `a` and column j
    of `b`: `acc = +0; acc = acc + a[i, k] * b[k, j]` per term, `out = m * acc`.  Under SPARSE_AMD_EXACT every operation is
    rounded on its own, otherwise a term's multiply and add are one fma (the mask multiply never is); integers wrap.  A
    position without a term stores nothing, whatever m is.  Same bits on every call; no atomics on values.  The CSR / CSC
    forms the kernel reads are the ones the operands memoise for their other products: a second call converts nothing."""
    from ._dot import _csr_triplet, _validate_derived
    from ._utils import check_zero_fill_value

    for name, x in (("s", s), ("a", a), ("b", b)):
        if not isinstance(x, (COO, GCXS)):
            raise TypeError(f"masked_matmul needs COO or GCXS operands, got {type(x).__name__} for `{name}`; for dense "
                            "`a` and `b` use sddmm(s, a, b)")
        if x.ndim != 2:
            raise ValueError(f"masked_matmul needs 2-D operands, `{name}` has {x.ndim} dimensions")
    check_zero_fill_value(s, a, b)
    M, N = int(s.shape[0]), int(s.shape[1])
    Kd = int(a.shape[1])
    if int(a.shape[0]) != M or int(b.shape[1]) != N or int(b.shape[0]) != Kd:
        raise ValueError(f"shape-mismatch for masked_matmul: s {tuple(s.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}; "
                         "expected (M, N), (M, K), (K, N)")
    dt = np.result_type(np.dtype(s.dtype), K.dot_dtype(a.dtype, b.dtype))
    for name, x in (("s", s), ("a", a), ("b", b)):
        if np.dtype(x.dtype) not in _OPERAND_DTYPES:
            raise TypeError(f"masked_matmul: `{name}` has values of type {x.dtype}; operands must be float32, float64, int32, int64, "
                            "bool or uint8 (no complex, 16-bit or 8 / 16-bit signed integer operands)")
    if dt not in _RESULT_DTYPES:
        raise TypeError(f"masked_matmul: operands of type {s.dtype}, {a.dtype}, {b.dtype} give a {dt} result; only float32, float64, "
                        "int32 and int64 results are supported (not bool-only or uint8-only operands)")
    if s.nnz == 0 or a.nnz == 0 or b.nnz == 0 or M == 0 or N == 0 or Kd == 0:
        return _empty_like_mask(s, dt)

    if isinstance(s, COO):
        sc = s
    else:  # the COO view of a GCXS mask is kept on it (as sddmm does): the result is built on its coordinates
        _validate_derived(s)
        sc = s.__dict__.get("_coo_view")
        if sc is None:
            sc = s.__dict__["_coo_view"] = s.tocoo()
    coords = sc.coords      # (materialised before the forms are taken: a COO kept as linear keys changes its stamp when it is)
    s_val, s_idx, s_ptr = _csr_triplet(sc)
    a_val, a_idx, a_ptr = _csr_triplet(a)
    b_val, b_idx, b_ptr = _csc_triplet(b)
    vals = K.masked_spgemm((M, N, Kd), (K.convert(s_val, dt), s_idx, s_ptr), (K.convert(a_val, dt), a_idx, a_ptr),
                           (K.convert(b_val, dt), b_idx, b_ptr), exact=_settings.EXACT_MULADD)
    out = COO(coords, vals, shape=(M, N), has_duplicates=False, sorted=True, prune=True)
    return out.asformat("gcxs", compressed_axes=s.compressed_axes) if isinstance(s, GCXS) else out

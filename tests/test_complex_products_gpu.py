"""Complex matrix products on the device (`matmul`, `dot`, `tensordot`, `einsum`, `@`) against the fixture the REAL
reference produced (tests/golden/complex_dot.npz, written by tools/gen_complex_golden.py), and the C ABI of
csrc/spmm_complex.hip against NumPy.

Two kinds of check:
  * exact mode (`_settings.EXACT_MULADD`): structure and values BIT-identical to the reference - the order of the sums and the
    arithmetic of a term (four rounded products, a rounded subtraction, a rounded addition, the rounded accumulate) are the
    reference's, so there is no tolerance to choose;
  * default (FMA) mode, and everything summed in tree order: element by element
        |got - want| <= (n + 4) * eps * sum_k |a_ik| |b_kj|
    with n the number of stored elements in the longest row of A (a dense A: its number of columns), eps the machine epsilon
    of the real type, the sum evaluated in float64 and `want` in the next wider complex type - the standard bound of a length-n
    complex dot product (about 2 sqrt(2) roundings for the multiply plus n for the sum, in units of eps / 2), loose by about
    2x so that FMA and tree order both fit.  No element is skipped or masked.

`einsum`: the reference's route there is another one (it multiplies the aligned operands and reduces: explicit zeros stay
stored and the sums run in another order - its own `tensordot` of the same operands differs from it in the last bit), so its
case is held to the bound in both modes and its coordinates are compared without the explicit zeros.

The csc sparse-returning variant: the reference's `_dot_csc_ndarray_sparse` sums into a float64 scratch array, which drops the
imaginary parts of complex operands, so the values it returns are not the product.  The fixture keeps its structure and
takes the values, at those coordinates, from the reference's dense-result product of the same operands - the same terms in
the same order - (tools/gen_complex_golden.py), and the test asks for those bits.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "complex_dot.npz")
WIDER = {np.dtype("complex64"): np.complex128, np.dtype("complex128"): np.clongdouble}
REAL = {np.dtype("complex64"): np.float32, np.dtype("complex128"): np.float64}
ETYPE, EINVAL = -2, -1
EXACT_MULADD, SPMM_ROWGROUP = 1, 4


@pytest.fixture(scope="module")
def sp():
    import sparse_amd

    return sparse_amd


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _names(z):
    return sorted({k.split("__")[0] for k in z.files})


def _npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# fixture cases: operands, the public call, the 2-D form the bound is evaluated on
# ---------------------------------------------------------------------------------------------------------------------
def _operand(sp, z, name, side):
    pre = f"{name}__{side}"
    if pre in z.files:
        return z[pre]
    shape = tuple(int(s) for s in z[pre + "_shape"])
    if pre + "_indptr" in z.files:
        return sp.GCXS((z[pre + "_data"], z[pre + "_indices"], z[pre + "_indptr"]), shape=shape,
                       compressed_axes=tuple(int(c) for c in z[pre + "_ca"]))
    return sp.COO(z[pre + "_coords"], z[pre + "_data"], shape=shape)


def _dense_operand(z, name, side):
    """(dense NumPy form, is it stored sparse) of an operand, from the fixture's arrays alone"""
    pre = f"{name}__{side}"
    if pre in z.files:
        return z[pre], False
    shape = tuple(int(s) for s in z[pre + "_shape"])
    data = z[pre + "_data"]
    d = np.zeros(shape, dtype=data.dtype)
    if pre + "_indptr" in z.files:
        ptr, idx = z[pre + "_indptr"].astype(np.int64), z[pre + "_indices"].astype(np.int64)
        major = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        if int(z[pre + "_ca"][0]) == 0:
            d[major, idx] = data
        else:
            d[idx, major] = data
    else:
        d[tuple(z[pre + "_coords"].astype(np.int64))] = data
    return d, True


def _call(sp, name, k, a, b):
    """the product of case `name` through the public API (the entry point varies with the case's position `k`)"""
    if name.startswith("sp_"):
        rt = sp.GCXS if ("csr" in name or "csc" in name) else sp.COO
        return sp.tensordot(a, b, axes=1, return_type=rt)
    if name.startswith("tensordot3d"):
        return sp.tensordot(a, b, axes=([1, 2], [1, 0]))
    if name.startswith("einsum"):
        return sp.einsum("ijk,kl->ijl", a, b)
    if isinstance(a, np.ndarray):       # dense @ sparse
        return (sp.matmul(a, b), b.__rmatmul__(a), sp.tensordot(a, b, axes=1), sp.dot(a, b))[k % 4]
    return (a @ b, sp.matmul(a, b), sp.dot(a, b), sp.tensordot(a, b, axes=1))[k % 4]


def _matrix_forms(z, name):
    """(A, B, n) as 2-D matrices with A @ B == the case's result (reshaped), n = stored elements in A's longest row"""
    a, a_sparse = _dense_operand(z, name, "a")
    b, _ = _dense_operand(z, name, "b")
    if name.startswith("tensordot3d"):
        a, b = a.reshape(a.shape[0], -1), b.transpose(1, 0, 2).reshape(-1, b.shape[2])
    elif name.startswith("einsum"):
        a = a.reshape(-1, a.shape[2])
    n = int(np.count_nonzero(a, axis=1).max()) if a_sparse else a.shape[1]
    return a, b, n


def _bound_terms(a, b, n, dtype):
    """(`want` in the next wider complex type, the bound in float64) of a product whose result has complex `dtype`"""
    wide, real = WIDER[np.dtype(dtype)], REAL[np.dtype(dtype)]
    want = a.astype(wide) @ b.astype(wide)
    bound = (n + 4) * float(np.finfo(real).eps) * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))
    return want, bound


def _assert_within_bound(got, a, b, n, what, terms=None, show=True):
    got = np.asarray(got)
    want, bound = terms if terms is not None else _bound_terms(a, b, n, got.dtype)
    err = np.abs(got.reshape(want.shape).astype(want.dtype) - want).astype(np.float64)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    if show:
        print(f"{what}: max |got - want| / bound = {worst:.4f}  (n = {n})")
    assert np.all(err <= bound), f"{what}: max |got - want| / bound = {worst:.4f}"


def _result_dtype(z, name):
    return (z[name + "__out"] if name + "__out" in z.files else z[name + "__out_data"]).dtype


def _check_container(sp, z, name, r):
    """type, dtype, compressed axis and - exactly - the canonical coordinates of a sparse result; returns its values in
    canonical order"""
    fmt = int(z[name + "__out_format"])
    if fmt == 2:
        assert isinstance(r, sp.COO), type(r)
        c = r
    else:
        assert isinstance(r, sp.GCXS) and r.compressed_axes == (fmt,), (type(r), getattr(r, "compressed_axes", None))
        assert _npy(r.indices).dtype.kind == "i" and _npy(r.indptr)[-1] == r.nnz
        c = r.tocoo()
    assert r.dtype == _result_dtype(z, name)
    coords, data = _npy(c.coords).astype(np.int64), _npy(c.data)
    order = np.lexsort(coords[::-1])                      # the canonical sort: first axis major
    return coords[:, order], data[order]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fma"])
def test_fixture_cases(sp, gold, exact, monkeypatch):
    """Checks 1 and 2: every fixture case through the public API - result type and dtype, exact structure, and values
    bit-identical to the reference in exact mode / within the derived bound in the default mode."""
    from sparse_amd import _settings

    monkeypatch.setattr(_settings, "EXACT_MULADD", exact)
    names = _names(gold)
    assert len(names) >= 51
    for k, name in enumerate(names):
        a, b = _operand(sp, gold, name, "a"), _operand(sp, gold, name, "b")
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)    # no NaN warning
            r = _call(sp, name, k, a, b)
        A, B, n = _matrix_forms(gold, name)
        if name + "__out" in gold.files:                  # dense result
            want = gold[name + "__out"]
            assert isinstance(r, np.ndarray), (name, type(r))
            assert r.dtype == want.dtype and r.shape == want.shape, (name, r.dtype, r.shape)
            if exact:
                assert np.array_equal(_bits(r), _bits(want)), f"{name}: not bit-identical to the reference"
            _assert_within_bound(r, A, B, n, name)
            continue
        coords, data = _check_container(sp, gold, name, r)
        wc, wd = gold[name + "__out_coords"], gold[name + "__out_data"]
        if name.startswith("einsum"):
            keep_w, keep_g = wd != 0, data != 0
            assert np.array_equal(coords[:, keep_g], wc[:, keep_w]), name
            _assert_within_bound(r.todense(), A, B, n, name)
            continue
        assert r.nnz == int(gold[name + "__out_nnz"]), (name, r.nnz)
        assert coords.shape == wc.shape and np.array_equal(coords, wc), name
        assert data.dtype == wd.dtype
        # the sparse-returning variants compute in exact mode whatever the setting; sparse x sparse has one arithmetic
        assert np.array_equal(_bits(data), _bits(wd)), f"{name}: values not bit-identical to the reference"
        _assert_within_bound(r.todense(), A, B, n, name)


def test_return_types_and_torch_operands(sp, gold, monkeypatch):
    """Every `return_type` of a complex product, for the three containers, and torch in -> torch out"""
    from sparse_amd import _settings

    monkeypatch.setattr(_settings, "EXACT_MULADD", True)
    for name in ("gd_c64_csr_n7_int64", "gd_c128_csc_n7_int64", "coo_dense_c128", "gg_csr_csr_c64", "gg_coo_coo_c128",
                 "dense_csc_c64", "dense_coo_c128"):
        a, b = _operand(sp, gold, name, "a"), _operand(sp, gold, name, "b")
        A, B, _ = _matrix_forms(gold, name)
        want = sp.tensordot(a, b, axes=1, return_type=np.ndarray)
        assert isinstance(want, np.ndarray) and want.dtype == _result_dtype(gold, name)
        if name + "__out" in gold.files:
            assert np.array_equal(_bits(want), _bits(gold[name + "__out"]))
        for rt in (sp.COO, sp.GCXS):
            r = sp.tensordot(a, b, axes=1, return_type=rt)
            assert isinstance(r, rt) and r.dtype == want.dtype
            assert np.array_equal(r.todense(), want), (name, rt)
    name = "gd_c64_csr_n64_int32"
    a = _operand(sp, gold, name, "a")
    bt = torch.from_numpy(gold[name + "__b"]).cuda()
    r = a @ bt
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.complex64
    assert np.array_equal(_bits(_npy(r)), _bits(gold[name + "__out"]))
    r = a @ bt                                       # the operand's second product with this dense type and width
    assert np.array_equal(_bits(_npy(r)), _bits(gold[name + "__out"]))


def test_products_raised_before(sp):
    """What the issue quotes: a complex product is computed, not refused"""
    rng = np.random.default_rng(3)
    d = np.where(rng.random((20, 30)) < 0.2, rng.random((20, 30)) + 1j * rng.random((20, 30)), 0)
    v = rng.random(30) + 1j * rng.random(30)
    for x in (sp.COO.from_numpy(d), sp.GCXS.from_numpy(d, compressed_axes=(0,)), sp.GCXS.from_numpy(d, compressed_axes=(1,))):
        y = x @ v                                    # a sparse Hamiltonian times a state vector
        assert y.dtype == np.complex128 and y.shape == (20,)
        assert np.allclose(y, d @ v, rtol=1e-13, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# check 3: the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _complex_csr(M, K, density, seed, cdtype, idt, long_row=None):
    from util import random_csr

    re, idx, ptr = random_csr(M, K, density, seed, dtype=np.float64, idx_dtype=idt, long_row=long_row)
    im = np.random.default_rng(seed + 1).random(len(re)) - 0.6
    return (re + 1j * im).astype(cdtype), idx, ptr


def _cdense(K, N, seed, cdtype):
    rng = np.random.default_rng(seed)
    return ((rng.random((K, N)) - 0.5) + 1j * (rng.random((K, N)) - 0.5)).astype(cdtype)


def _dev_reals(x, lead, offset_reals=0):
    """Device buffer of the reals of the 2-D complex array `x` laid out with leading dimension `lead` (complex elements),
    starting `offset_reals` reals into a fresh allocation; returns (buffer, address of the first element)."""
    real = REAL[x.dtype]
    rows = x.shape[0]
    host = np.full((max(rows, 1), lead, 2), 7.5, dtype=real)       # the padding holds a recognisable value
    host[:rows, :x.shape[1], 0], host[:rows, :x.shape[1], 1] = x.real, x.imag
    buf = torch.empty(host.size + offset_reals + 2, dtype=torch.from_numpy(host).dtype, device="cuda")
    buf[offset_reals:offset_reals + host.size] = torch.from_numpy(host.reshape(-1)).cuda()
    return buf, buf.data_ptr() + offset_reals * buf.element_size()


def _run_abi(lib, code, icode, data, idx, ptr, b, N, ldb, ldo, flags, b_off=0, out_off=0):
    M, K = len(ptr) - 1, b.shape[0]
    real = REAL[data.dtype]
    d_data = torch.from_numpy(np.ascontiguousarray(data).view(real)).cuda()
    d_idx, d_ptr = torch.from_numpy(idx).cuda(), torch.from_numpy(ptr).cuda()
    b_buf, b_addr = _dev_reals(b, ldb, b_off)
    o_buf, o_addr = _dev_reals(np.zeros((M, N), dtype=data.dtype), ldo, out_off)
    rc = lib.spamd_spmm_csr_complex(code, icode, M, K, N, d_data.data_ptr(), d_idx.data_ptr(), d_ptr.data_ptr(), b_addr, ldb,
                                    o_addr, ldo, flags, 0)
    torch.cuda.synchronize()
    assert rc == 0, rc
    host = o_buf.cpu().numpy()[out_off:out_off + M * ldo * 2].reshape(M, ldo, 2)
    assert np.all(host[:, N:, :] == 7.5), "wrote outside the result's columns"
    return (host[:, :N, 0] + 1j * host[:, :N, 1]).astype(data.dtype)


def _dense_of_csr(data, idx, ptr, K):
    d = np.zeros((len(ptr) - 1, K), dtype=data.dtype)
    d[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = data
    return d


@pytest.mark.parametrize("idt", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("cdtype, code", [(np.complex64, 6), (np.complex128, 7)], ids=["c64", "c128"])
def test_c_abi_shapes(hiplib, cdtype, code, idt):
    """`spamd_spmm_csr_complex` for every (dtype, index type): widths across the G / VEC / CH cases, padded leading
    dimensions (even and odd), a B and a result off the 16-byte grid (the 8-byte accesses), in the three modes (default,
    exact, row-group); every result within the bound, the exact mode also bit-identical to the four-products form."""
    icode = 2 if idt == np.int32 else 3
    M, K = 97, 83
    data, idx, ptr = _complex_csr(M, K, 0.2, 11, cdtype, idt)
    data = data.copy()
    ptr = ptr.copy()
    A = _dense_of_csr(data, idx.astype(np.int64), ptr.astype(np.int64), K)
    n = int(np.diff(ptr).max())
    # reals one 8-byte access apart from the 16-byte grid: one complex64 element, half a complex128 element
    off = 2 if cdtype == np.complex64 else 1
    for N in (1, 2, 3, 4, 5, 16, 33, 64, 128, 130, 512):
        b = _cdense(K, N, 100 + N, cdtype)
        terms, exact_want = _bound_terms(A, b, n, cdtype), _bits(_four_products(data, idx, ptr, b))
        layouts = [(N, N, 0, 0), (N + 2, N + 4, 0, 0), (N + 3, N + 1, 0, 0), (N, N, off, 0), (N + 2, N + 2, off, off)]
        worst = 0.0
        for ldb, ldo, b_off, out_off in layouts:
            for flags in (0, EXACT_MULADD, SPMM_ROWGROUP):
                got = _run_abi(hiplib, code, icode, data, idx, ptr, b, N, ldb, ldo, flags, b_off, out_off)
                what = f"{np.dtype(cdtype).name} N={N} ldb={ldb} ldo={ldo} off={b_off},{out_off} flags={flags}"
                _assert_within_bound(got, A, b, n, what, terms, show=False)
                worst = max(worst, float(np.max(np.abs(got.astype(terms[0].dtype) - terms[0]).astype(np.float64) / np.maximum(terms[1], 1e-300))))
                if flags == EXACT_MULADD:
                    assert np.array_equal(_bits(got), exact_want), what + ": not the four-products form"
        print(f"{np.dtype(cdtype).name} N={N}: max |got - want| / bound over layouts and modes = {worst:.4f}  (n = {n})")


def _four_products(data, idx, ptr, b):
    """the reference loop on reals: per term four rounded products, a rounded subtraction and addition, the rounded
    accumulate, k ascending (NumPy's scalar complex multiply and add)"""
    real = REAL[data.dtype]
    M, N = len(ptr) - 1, b.shape[1]
    ore, oim = np.zeros((M, N), real), np.zeros((M, N), real)
    br, bi = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
    for i in range(M):
        for k in range(int(ptr[i]), int(ptr[i + 1])):
            ar, ai, j = real(data[k].real), real(data[k].imag), int(idx[k])
            ore[i] = ore[i] + (ar * br[j] - ai * bi[j])
            oim[i] = oim[i] + (ar * bi[j] + ai * br[j])
    return (ore + 1j * oim).astype(data.dtype)


@pytest.mark.parametrize("cdtype, code", [(np.complex64, 6), (np.complex128, 7)], ids=["c64", "c128"])
def test_c_abi_long_row_and_empty_shapes(hiplib, cdtype, code):
    """A row of 10^5 stored elements (between two short ones), M = 0 and N = 0"""
    K = 100_000
    data, idx, ptr = _complex_csr(3, K, 0.0002, 5, cdtype, np.int32, long_row=1)
    assert int(np.diff(ptr).max()) == K
    A = _dense_of_csr(data, idx.astype(np.int64), ptr.astype(np.int64), K)
    for N in (1, 2, 5):
        b = _cdense(K, N, 7 + N, cdtype)
        for flags in (0, EXACT_MULADD):
            got = _run_abi(hiplib, code, 2, data, idx, ptr, b, N, N, N, flags)
            _assert_within_bound(got, A, b, K, f"long row {np.dtype(cdtype).name} N={N} flags={flags}")
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    assert hiplib.spamd_spmm_csr_complex(code, 2, 0, 5, 3, p, p, p, p, 3, p, 3, 0, 0) == 0      # M = 0
    assert hiplib.spamd_spmm_csr_complex(code, 2, 4, 5, 0, p, p, p, p, 0, p, 0, 0, 0) == 0      # N = 0
    torch.cuda.synchronize()
    assert not buf.any()


def test_c_abi_refuses_bad_arguments(hiplib):
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    call = hiplib.spamd_spmm_csr_complex
    for bad in (0, 1, 2, 3, 4, 5, 8, -1):                # the real codes, bf16, u8, unknown ones
        assert call(bad, 2, 2, 2, 2, p, p, p, p, 2, p, 2, 0, 0) == ETYPE
    for bad in (0, 1, 6, 7):                             # index types are int32 / int64
        assert call(6, bad, 2, 2, 2, p, p, p, p, 2, p, 2, 0, 0) == ETYPE
    assert call(6, 2, -1, 2, 2, p, p, p, p, 2, p, 2, 0, 0) == EINVAL
    assert call(7, 3, 2, 2, -2, p, p, p, p, 2, p, 2, 0, 0) == EINVAL
    assert call(6, 2, 2, 2, 4, p, p, p, p, 3, p, 4, 0, 0) == EINVAL      # ldb < N
    assert call(7, 2, 2, 2, 4, p, p, p, p, 4, p, 3, 0, 0) == EINVAL      # ldo < N
    assert call(6, 2, 2, 2, 2, p, p, 0, p, 2, p, 2, 0, 0) == EINVAL      # no indptr
    assert call(6, 2, 2, 2, 2, p, p, p, p + 4, 2, p, 2, 0, 0) == EINVAL  # B off the 8-byte grid
    torch.cuda.synchronize()
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------
# check 4: determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_same_product_twice_gives_the_same_bytes(cdtype):
    from sparse_amd import _kernels as K

    M, Kd = 20_000, 3_000
    data, idx, ptr = _complex_csr(M, Kd, 0.01, 21, cdtype, np.int32)
    d, i, p = (torch.from_numpy(x).cuda() for x in (data, idx, ptr))
    for N, keep in ((1, False), (2, False), (2, True), (130, False)):      # row-vector kernel; row-group kernel
        b = torch.from_numpy(_cdense(Kd, N, N, cdtype)).cuda()
        first = K.dot_csr_ndarray((M, N), d, i, p, b, keep_order=keep)
        again = K.dot_csr_ndarray((M, N), d, i, p, b, keep_order=keep)
        assert first.dtype == b.dtype
        assert torch.equal(torch.view_as_real(first), torch.view_as_real(again))


# ---------------------------------------------------------------------------------------------------------------------
# check 5: full size
# ---------------------------------------------------------------------------------------------------------------------
def _sample_rows(data, idx, ptr, M, count):
    rows = torch.from_numpy(np.random.default_rng(0).choice(M, count, replace=False)).sort().values.cuda()
    lo, hi = ptr[rows].long(), ptr[rows + 1].long()
    lens = hi - lo
    sp_ptr = torch.zeros(len(rows) + 1, dtype=torch.int64, device="cuda")
    sp_ptr[1:] = torch.cumsum(lens, 0)
    take = torch.repeat_interleave(lo - sp_ptr[:-1], lens) + torch.arange(int(sp_ptr[-1]), device="cuda")
    return rows, data[take].cpu().numpy(), idx[take].cpu().numpy().astype(np.int64), sp_ptr.cpu().numpy()


def _assert_rows_within_bound(got, sd, si, sptr, b, what):
    """the bound of the module docstring on sampled rows: `want` through scipy in complex128 for complex64 results, through
    extended-precision products summed per row for complex128 ones"""
    import scipy.sparse as sps

    R, K = len(sptr) - 1, b.shape[0]
    wide, real = WIDER[got.dtype], REAL[got.dtype]
    lens = np.diff(sptr)
    assert lens.min() > 0
    if wide is np.complex128:
        want = sps.csr_matrix((sd.astype(wide), si, sptr), shape=(R, K)) @ b.astype(wide)
    else:
        want = np.add.reduceat(sd.astype(wide)[:, None] * b.astype(wide)[si], sptr[:-1], axis=0)
    absum = sps.csr_matrix((np.abs(sd).astype(np.float64), si, sptr), shape=(R, K)) @ np.abs(b).astype(np.float64)
    bound = (int(lens.max()) + 4) * float(np.finfo(real).eps) * absum
    err = np.abs(got.astype(wide) - want).astype(np.float64)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: max |got - want| / bound = {worst:.4f}  (n = {int(lens.max())})")
    assert np.all(err <= bound), f"{what}: max |got - want| / bound = {worst:.4f}"


def test_config2_structure_with_complex_values():
    """config 2's structure (10^6 x 10^4 at 1 %) with complex64 values, N = 1 and N = 128, and complex128 values, N = 1:
    2000 sampled rows against NumPy."""
    import sparse_amd as sp

    sys.path.insert(0, os.path.dirname(HERE))
    from bench import make_csr_device

    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free: the complex128 operand, its parts and the 1 GiB result need 16")
    M, K = 1_000_000, 10_000
    re, idx, ptr = make_csr_device(M, K, 0.01, seed=0)
    g = torch.Generator(device="cuda").manual_seed(9)
    im = torch.rand(re.numel(), device="cuda", generator=g) - 0.6
    data = torch.complex(re - 0.3, im)                      # mixed signs in both parts: cancellation inside the rows
    del re, im
    b = torch.complex(torch.rand((K, 128), device="cuda", generator=g) - 0.5, torch.rand((K, 128), device="cuda", generator=g) - 0.5)
    a = sp.GCXS((data, idx, ptr), shape=(M, K), compressed_axes=(0,))
    rows, sd, si, sptr = _sample_rows(data, idx, ptr, M, 2000)
    bn = b.cpu().numpy()
    c = a @ b
    assert c.dtype == torch.complex64 and tuple(c.shape) == (M, 128)
    _assert_rows_within_bound(c[rows].cpu().numpy(), sd, si, sptr, bn, "complex64 N=128")
    del c
    y = a @ b[:, :1].contiguous()
    _assert_rows_within_bound(y[rows].cpu().numpy(), sd, si, sptr, bn[:, :1], "complex64 N=1")
    a128 = sp.GCXS((data.to(torch.complex128), idx, ptr), shape=(M, K), compressed_axes=(0,))
    del a, data
    v = b[:, :1].to(torch.complex128).contiguous()
    y = a128 @ v
    assert y.dtype == torch.complex128
    _assert_rows_within_bound(y[rows].cpu().numpy(), sd.astype(np.complex128), si, sptr, bn[:, :1].astype(np.complex128),
                              "complex128 N=1")


# ---------------------------------------------------------------------------------------------------------------------
# check 6: the NaN warning; the routes of real products
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_matmul_warns_for_nan_in_a_complex_operand(sp, cdtype, monkeypatch):
    from sparse_amd import _settings

    monkeypatch.setattr(_settings, "NAN_CHECK", True)
    monkeypatch.setattr(_settings, "NAN_WARNING", "sync")
    rng = np.random.default_rng(1)
    d = np.where(rng.random((30, 20)) < 0.3, rng.random((30, 20)) + 1j * rng.random((30, 20)), 0).astype(cdtype)
    b = _cdense(20, 5, 2, cdtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sp.GCXS.from_numpy(d) @ b                          # no NaN: no warning
    for bad in (complex(np.nan, 1), complex(1, np.nan)):        # in the real part, in the imaginary part
        dn = d.copy()
        dn[np.nonzero(dn)[0][0], np.nonzero(dn)[1][0]] = bad
        for x in (sp.GCXS.from_numpy(dn), sp.COO.from_numpy(dn)):
            with pytest.warns(RuntimeWarning, match="Nan will not be propagated in matrix multiplication"):
                x @ b
        bn = b.copy()
        bn[3, 1] = bad
        with pytest.warns(RuntimeWarning, match="Nan will not be propagated in matrix multiplication"):
            sp.GCXS.from_numpy(d) @ bn
        with pytest.warns(RuntimeWarning, match="Nan will not be propagated in matrix multiplication"):
            sp.matmul(bn.T.copy(), sp.COO.from_numpy(d.T.copy()))


_REAL_ROUTES = [
    # (M, K, N, density, container form, value dtype, the route kind this product chose before complex products existed)
    (60, 45, 7, 0.15, "csr", torch.float32, "spmm_csr"),
    (60, 45, 7, 0.15, "csr", torch.int64, "spmm_csr"),
    (40_000, 3_000, 4, 1 / 300, "csr", torch.float32, "stream"),
    (40_000, 3_000, 4, 1 / 300, "csr", torch.float64, "stream"),
    (70_000, 3_000, 128, 0.0127, "csr", torch.float32, "tiled"),
    (70_000, 3_000, 128, 0.0127, "csc", torch.float32, "tiled_csc"),
]


@pytest.mark.parametrize("M, K, N, density, form, dtype, kind", _REAL_ROUTES,
                         ids=[f"{r[6]}-{str(r[5]).replace('torch.', '')}" for r in _REAL_ROUTES])
def test_real_products_keep_their_routes(sp, M, K, N, density, form, dtype, kind):
    """One product per route kind of `_route_of`, real value types: the route chosen is the one chosen before, and the
    product is right."""
    import scipy.sparse as sps

    from bench import make_csr_device
    from sparse_amd import _dot as D

    vals, idx, ptr = make_csr_device(M, K, density, seed=3)
    vals = (vals * 8 - 3).to(dtype) if not dtype.is_floating_point else (vals - 0.3).to(dtype)
    a = sp.GCXS((vals, idx, ptr), shape=(M, K), compressed_axes=(0,))
    if form == "csc":
        a = a.change_compressed_axes((1,))
    g = torch.Generator(device="cuda").manual_seed(4)
    b = torch.rand((K, N), device="cuda", generator=g) - 0.5
    b = (b * 8).to(dtype) if not dtype.is_floating_point else b.to(dtype)
    triplet = None if D._csc_without_twin(a) else D._csr_triplet(a)
    assert D._route_of(a, b, (M, N), triplet).kind == kind
    got = (a @ b).cpu().numpy()
    ref = sps.csr_matrix((vals.cpu().numpy().astype(np.float64), idx.cpu().numpy(), ptr.cpu().numpy()), shape=(M, K))
    want = ref @ b.cpu().numpy().astype(np.float64)
    if dtype.is_floating_point:
        scale = abs(ref) @ np.abs(b.cpu().numpy()).astype(np.float64)
        assert np.all(np.abs(got - want) <= (2e-6 if dtype == torch.float32 else 1e-14) * scale + 1e-300)
    else:
        assert np.array_equal(got, want.astype(np.int64))

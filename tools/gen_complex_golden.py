"""Generate tests/golden/complex_dot.npz by RUNNING THE REAL REFERENCE on complex operands (pydata/sparse numba_backend,
imported in place through oracle/ref_loader.py, as oracle/gen_golden.py does).

    python tools/gen_complex_golden.py

TEST INFRASTRUCTURE.  Runs only where the reference tree exists; the fixture it writes is committed and pins the complex
products of the HIP path (tests/test_complex_products_gpu.py).  Fixed seeds; only arrays go into the file.  `case_names()`
lists every case the file must hold (tests/test_complex_products.py compares it with the keys present).

Layout: every case `<name>` stores its operands and the reference's result under keys `<name>__<field>`:
  sparse operands   a_data / a_indices / a_indptr / a_ca / a_shape  (GCXS)  or  a_coords / a_data / a_shape  (COO); same with b_
  dense operands    a  or  b
  dense results     out
  sparse results    out_coords / out_data (canonical COO form of the result) and out_nnz (stored elements of the container)
The one result that is not the reference's as returned: the VALUES of the csc sparse-returning variant (see `generate`).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "complex_dot.npz")

CDTYPES = (("c64", np.complex64), ("c128", np.complex128))
WIDTHS = (1, 2, 3, 7, 64, 130)
SPARSE_RETURNING = ("csr_dense", "csc_dense", "coo_dense", "dense_coo")
SPGEMM = ("csr_csr", "csc_csc", "coo_coo")


def _gd_cases():
    """(name, tag, N, compressed axis, index dtype, M, K) of the GCXS @ dense cases: every width with both compressed axes
    for the narrow results, one axis per dtype for the two wide ones (kept small: they hold most of the file's bytes)."""
    out = []
    for t, (tag, _) in enumerate(CDTYPES):
        for n, N in enumerate(WIDTHS):
            for c, ca in enumerate((0, 1)):
                if N >= 64 and (n + t + c) % 2:
                    continue
                idt = np.int32 if (n // 2 + c + t) % 2 == 0 else np.int64
                M, K = (60, 45) if N < 64 else (36, 30)
                out.append((f"gd_{tag}_{'csr' if ca == 0 else 'csc'}_n{N}_{np.dtype(idt).name}", tag, N, ca, idt, M, K))
    return out


def case_names():
    names = [c[0] for c in _gd_cases()]
    for tag, _ in CDTYPES:
        names += [f"coo_dense_{tag}", f"dense_csr_{tag}", f"dense_csc_{tag}", f"dense_coo_{tag}"]
        names += [f"sp_{v}_{tag}" for v in SPARSE_RETURNING]
        names += [f"gg_{v}_{tag}" for v in SPGEMM]
        names += [f"tensordot3d_{tag}", f"einsum_{tag}"]
    names += ["mixed_f64csr_c128dense", "mixed_c64csr_f32dense", "mixed_f32coo_c64dense", "mixed_c128csc_f64dense",
              "mixed_f64csr_c128csr"]
    return names


def _cvals(rng, shape, dtype):
    """complex (or real) values with mixed signs in both parts"""
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return ((rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)).astype(dtype)
    return (rng.random(shape) - 0.5).astype(dtype)


def _sparse_dense(rng, shape, density, dtype, empty_row=None):
    """a dense array with about `density` of its entries set"""
    d = np.where(rng.random(shape) < density, _cvals(rng, shape, dtype), 0).astype(dtype)
    if empty_row is not None:
        d[empty_row] = 0
    return d


def _dense(rng, shape, dtype, zero_col=True):
    b = _cvals(rng, shape, dtype)
    if zero_col and shape[-1] > 1:
        b[..., 0] = 0     # an all-zero dense column
    return b


def _put_sparse(cases, pre, x, sp):
    if isinstance(x, sp.GCXS):
        cases[pre + "_data"], cases[pre + "_indices"], cases[pre + "_indptr"] = x.data, x.indices, x.indptr
        cases[pre + "_ca"] = np.array(x.compressed_axes)
    else:
        cases[pre + "_coords"], cases[pre + "_data"] = x.coords, x.data
    cases[pre + "_shape"] = np.array(x.shape)


def _put_result(cases, name, r, sp):
    if isinstance(r, np.ndarray):
        cases[name + "__out"] = r
        return
    c = r.tocoo() if isinstance(r, sp.GCXS) else r
    c = sp.COO(c.coords, c.data, shape=c.shape)      # canonical: sorted, no duplicates
    cases[name + "__out_coords"], cases[name + "__out_data"] = c.coords.astype(np.int64), c.data
    cases[name + "__out_nnz"] = np.array(r.nnz)
    cases[name + "__out_format"] = np.array(2 if not isinstance(r, sp.GCXS) else r.compressed_axes[0])


def generate(sp):
    cases = {}

    def put(name, a, b, r):
        for side, x in (("a", a), ("b", b)):
            if isinstance(x, np.ndarray):
                cases[f"{name}__{side}"] = x
            else:
                _put_sparse(cases, f"{name}__{side}", x, sp)
        _put_result(cases, name, r, sp)

    dts = dict(CDTYPES)
    # --- GCXS(csr | csc) @ dense: every width, both index widths, an empty row, an all-zero dense column ----------------
    for k, (name, tag, N, ca, idt, M, K) in enumerate(_gd_cases()):
        rng = np.random.default_rng(1000 + k)
        a = sp.GCXS.from_numpy(_sparse_dense(rng, (M, K), 0.15, dts[tag], empty_row=3), compressed_axes=(ca,), idx_dtype=idt)
        assert a.indices.dtype == idt and a.data.dtype == dts[tag]
        b = _dense(rng, (K, N), dts[tag])
        put(name, a, b, sp.tensordot(a, b, axes=1))
    for t, (tag, dt) in enumerate(CDTYPES):
        rng = np.random.default_rng(2000 + t)
        # --- COO @ dense, dense @ GCXS, dense @ COO ---------------------------------------------------------------------
        x = sp.COO.from_numpy(_sparse_dense(rng, (50, 30), 0.2, dt, empty_row=3))
        b = _dense(rng, (30, 7), dt)
        put(f"coo_dense_{tag}", x, b, sp.tensordot(x, b, axes=1))
        a2 = _dense(rng, (9, 50), dt)
        for fmt, ca in (("csr", 0), ("csc", 1)):
            g = sp.GCXS.from_numpy(_sparse_dense(rng, (50, 30), 0.2, dt, empty_row=3), compressed_axes=(ca,))
            put(f"dense_{fmt}_{tag}", a2, g, sp.tensordot(a2, g, axes=1))
        put(f"dense_coo_{tag}", a2, x, sp.tensordot(a2, x, axes=1))
        # --- the four sparse-returning variants ---------------------------------------------------------------------------
        b6 = _dense(rng, (25, 6), dt)
        b6[:, 2] = 0
        for fmt, ca in (("csr", 0), ("csc", 1)):
            g = sp.GCXS.from_numpy(_sparse_dense(rng, (30, 25), 0.2, dt, empty_row=3), compressed_axes=(ca,))
            name = f"sp_{fmt}_dense_{tag}"
            put(name, g, b6, sp.tensordot(g, b6, axes=1, return_type=sp.GCXS))
            if fmt == "csc":
                # The reference's `_dot_csc_ndarray_sparse` accumulates in `sums = np.zeros(a_shape[0])`, a FLOAT64 array
                # (_common.py:835): for complex operands the imaginary parts are discarded on assignment (NumPy's
                # ComplexWarning), so the values it returns are not the product.  The structure it returns is kept; the
                # values are taken, at those coordinates, from the reference's dense-result product of the same operands
                # (`_dot_csc_ndarray`, the same terms in the same order).
                dense = sp.tensordot(g, b6, axes=1)
                wrong = cases[name + "__out_data"]
                assert np.array_equal(wrong.imag, np.zeros_like(wrong.imag)) and np.abs(wrong.real - dense[tuple(cases[name + "__out_coords"])].real).max() < 1e-5
                cases[name + "__out_data"] = dense[tuple(cases[name + "__out_coords"])]
                cases[name + "__out_data_from_dense_product"] = np.array(1)
        y = sp.COO.from_numpy(_sparse_dense(rng, (30, 25), 0.2, dt, empty_row=3))
        put(f"sp_coo_dense_{tag}", y, b6, sp.tensordot(y, b6, axes=1, return_type=sp.COO))
        a8 = _dense(rng, (8, 30), dt)
        a8[5, :] = 0
        put(f"sp_dense_coo_{tag}", a8, y, sp.tensordot(a8, y, axes=1, return_type=sp.COO))
        # --- sparse x sparse ------------------------------------------------------------------------------------------------
        da, db = _sparse_dense(rng, (30, 28), 0.12, dt, empty_row=3), _sparse_dense(rng, (28, 32), 0.12, dt)
        for fmt, ca in (("csr", 0), ("csc", 1)):
            ga, gb = sp.GCXS.from_numpy(da, compressed_axes=(ca,)), sp.GCXS.from_numpy(db, compressed_axes=(ca,))
            put(f"gg_{fmt}_{fmt}_{tag}", ga, gb, ga @ gb)
        ca_, cb_ = sp.COO.from_numpy(da), sp.COO.from_numpy(db)
        put(f"gg_coo_coo_{tag}", ca_, cb_, ca_ @ cb_)
        # --- one 3-D tensordot, one einsum ------------------------------------------------------------------------------------
        x3 = sp.COO.from_numpy(_sparse_dense(rng, (5, 6, 7), 0.3, dt))
        d3 = _dense(rng, (7, 6, 4), dt, zero_col=False)
        put(f"tensordot3d_{tag}", x3, d3, sp.tensordot(x3, d3, axes=([1, 2], [1, 0])))
        y2 = sp.COO.from_numpy(_sparse_dense(rng, (7, 8), 0.3, dt))
        put(f"einsum_{tag}", x3, y2, sp.einsum("ijk,kl->ijl", x3, y2))
    # --- mixed real x complex, both ways ----------------------------------------------------------------------------------------
    rng = np.random.default_rng(3000)
    g = sp.GCXS.from_numpy(_sparse_dense(rng, (60, 45), 0.15, np.float64, empty_row=3), compressed_axes=(0,))
    b = _dense(rng, (45, 7), np.complex128)
    put("mixed_f64csr_c128dense", g, b, sp.tensordot(g, b, axes=1))
    g = sp.GCXS.from_numpy(_sparse_dense(rng, (60, 45), 0.15, np.complex64, empty_row=3), compressed_axes=(0,))
    b = _dense(rng, (45, 7), np.float32)
    put("mixed_c64csr_f32dense", g, b, sp.tensordot(g, b, axes=1))
    x = sp.COO.from_numpy(_sparse_dense(rng, (50, 30), 0.2, np.float32))
    b = _dense(rng, (30, 2), np.complex64)
    put("mixed_f32coo_c64dense", x, b, sp.tensordot(x, b, axes=1))
    g = sp.GCXS.from_numpy(_sparse_dense(rng, (60, 45), 0.15, np.complex128), compressed_axes=(1,))
    b = _dense(rng, (45, 1), np.float64, zero_col=False)
    put("mixed_c128csc_f64dense", g, b, sp.tensordot(g, b, axes=1))
    ga = sp.GCXS.from_numpy(_sparse_dense(rng, (30, 28), 0.12, np.float64), compressed_axes=(0,))
    gb = sp.GCXS.from_numpy(_sparse_dense(rng, (28, 32), 0.12, np.complex128), compressed_axes=(0,))
    put("mixed_f64csr_c128csr", ga, gb, ga @ gb)
    return cases


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader

    if not ref_loader.available():
        raise SystemExit("the reference tree is not present: the committed fixture cannot be regenerated here")
    sp = ref_loader.load()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cases = generate(sp)
    missing = [n for n in case_names() if not any(k.startswith(n + "__") for k in cases)]
    assert not missing, missing
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **cases)
    print(f"{OUT}: {len(case_names())} cases, {len(cases)} arrays, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

"""Generate tests/golden/complex_ew.npz by RUNNING THE REAL REFERENCE (pydata/sparse numba_backend, imported in place through
oracle/ref_loader.py) on complex elementwise operations and reductions.

    python tools/gen_complex_ew_golden.py

TEST INFRASTRUCTURE.  Runs only where the reference tree exists; the fixture it writes is committed and pins the complex
elementwise / reduction paths of the HIP backend (tests/test_complex_elemwise_gpu.py replays `CASES` with `sparse_amd` on the
stored inputs).  Fixed seeds; only arrays go into the file.  `case_names()` lists every case the file must hold
(tests/test_complex_elemwise.py compares it with the keys present).

Layout: inputs under `in__<name>`; every case `<name>` stores the reference's result under `<name>__<field>`:
  dense results     out
  sparse results    coords / data (canonical COO form), fill, meta = [nnz (stored elements of the container),
                    format (2 = COO, otherwise the GCXS's first compressed axis; -1 for a 1-D GCXS), *shape]
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "complex_ew.npz")

TAGS = (("c64", np.complex64), ("c128", np.complex128))
RUN_LENGTHS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 64, 65, 66, 67, 68, 69, 128, 129, 130, 131, 137, 2301)   # stored values per row of `red`
RED_COLS = 2400

BINARY = ("add", "subtract", "multiply", "divide", "equal", "not_equal")
UNARY = ("negative", "positive", "conjugate", "square", "absolute", "real", "imag", "isnan", "isinf", "isfinite")


def _special(dt):
    """values every elementwise case sees: infinities, NaN, denormals, both branches of the division"""
    tiny = np.finfo(np.float32 if dt == np.complex64 else np.float64).tiny
    return np.array([complex(np.inf, 1), complex(-2, np.inf), complex(np.nan, 0.5), complex(tiny / 4, -tiny / 8),
                     complex(1, 3), complex(3, 1), complex(-0.0, 2), complex(2, -0.0), complex(1e-3, -1e3), complex(5, 5)], dtype=dt)


def inputs():
    I = {}
    for t, (tag, dt) in enumerate(TAGS):
        rng = np.random.default_rng(500 + t)

        def cv(shape):
            return ((rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)).astype(dt)

        sp_ = _special(dt)
        a = np.where(rng.random((6, 8)) < 0.55, cv((6, 8)), 0).astype(dt)
        b = np.where(rng.random((6, 8)) < 0.55, cv((6, 8)), 0).astype(dt)
        a[0, :], b[1, :] = sp_[:8], sp_[2:10]
        a[1, :4], b[0, 4:] = sp_[6:10], sp_[:4]
        a[5, 0] = b[5, 0] = complex(0.25, -0.5)            # equal stored values
        I[f"a_{tag}"], I[f"b_{tag}"] = a, b
        row = np.where(rng.random((1, 8)) < 0.7, cv((1, 8)), 0).astype(dt)
        I[f"row_{tag}"] = row
        I[f"dense_{tag}"] = cv((6, 8))
        I[f"x3_{tag}"] = np.where(rng.random((4, 5, 6)) < 0.5, cv((4, 5, 6)), 0).astype(dt)
        # reductions: row r of `red` holds RUN_LENGTHS[r] stored values
        coords, data = [], []
        for r, L in enumerate(RUN_LENGTHS):
            cols = np.sort(rng.choice(RED_COLS, size=L, replace=False))
            coords.append(np.stack([np.full(L, r), cols]))
            data.append(cv(L) * 3)
        I[f"red_coords_{tag}"] = np.concatenate(coords, axis=1).astype(np.int64)
        I[f"red_data_{tag}"] = np.concatenate(data)
        I[f"p_{tag}"] = np.where(rng.random((5, 7)) < 0.6, cv((5, 7)) + 1, 1).astype(dt)       # a fill value of 1
    rng = np.random.default_rng(510)
    I["real_f8"] = np.where(rng.random((6, 8)) < 0.5, rng.random((6, 8)) - 0.5, 0)
    I["real_f4"] = I["real_f8"].astype(np.float32)
    I["int_i8"] = np.where(rng.random((6, 8)) < 0.5, rng.integers(-5, 6, (6, 8)), 0).astype(np.int64)
    I["bool"] = rng.random((6, 8)) < 0.4
    return I


def _red(sp, I, tag, **kw):
    return sp.COO(I[f"red_coords_{tag}"], I[f"red_data_{tag}"], shape=(len(RUN_LENGTHS), RED_COLS), **kw)


def cases():
    """[(name, function(sp, I))]: the same functions run the reference (here) and the HIP backend (the GPU test)"""
    out = []
    for tag, dt in TAGS:
        for op in BINARY:
            f = getattr(np, op)
            out += [
                (f"{op}_coo_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"]), sp.COO.from_numpy(I[f"b_{tag}"]))),
                (f"{op}_bcast_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"]), sp.COO.from_numpy(I[f"row_{tag}"]))),
                (f"{op}_scalar_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"]), 2j)),
                (f"{op}_rscalar_fill_{tag}", lambda sp, I, f=f, tag=tag: f(1.5 - 0.5j, sp.COO.from_numpy(I[f"a_{tag}"], fill_value=0.25 + 1j))),
                (f"{op}_gcxs_rows_{tag}", lambda sp, I, f=f, tag=tag: f(sp.GCXS.from_numpy(I[f"a_{tag}"], compressed_axes=(0,)),
                                                                        sp.GCXS.from_numpy(I[f"b_{tag}"], compressed_axes=(0,)))),
                (f"{op}_gcxs_cols_{tag}", lambda sp, I, f=f, tag=tag: f(sp.GCXS.from_numpy(I[f"a_{tag}"], compressed_axes=(1,)), 0.5 + 2j)),
                (f"{op}_mixed_real_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"]),
                                                                         sp.COO.from_numpy(I["real_f4" if tag == "c64" else "real_f8"]))),
                (f"{op}_mixed_int_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I["int_i8"]), sp.COO.from_numpy(I[f"b_{tag}"]))),
            ]
        out += [
            (f"add_scalar_fill_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"a_{tag}"]) + (1 + 0.5j)),
            (f"multiply_dense_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"a_{tag}"]) * I[f"dense_{tag}"]),
            (f"multiply_dense_row_{tag}", lambda sp, I, tag=tag: I[f"dense_{tag}"][:1] * sp.COO.from_numpy(I[f"a_{tag}"])),
            (f"divide_dense_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"a_{tag}"]) / I[f"dense_{tag}"]),
            (f"multiply_bool_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"a_{tag}"]) * sp.COO.from_numpy(I["bool"])),
            (f"real_times_cscalar_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I["real_f4" if tag == "c64" else "real_f8"]) * 2j),
            (f"astype_from_real_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I["real_f8"]).astype(I[f"a_{tag}"].dtype)),
            (f"astype_other_width_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"a_{tag}"]).astype(
                np.complex128 if tag == "c64" else np.complex64)),
            (f"lambda_{tag}", lambda sp, I, tag=tag: sp.elemwise(lambda u, v: (u - v) * u + 2j, sp.COO.from_numpy(I[f"a_{tag}"]),
                                                                 sp.COO.from_numpy(I[f"b_{tag}"]))),
        ]
        for op in UNARY:
            f = getattr(np, op)
            out += [
                (f"{op}_coo_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"]))),
                (f"{op}_fill_{tag}", lambda sp, I, f=f, tag=tag: f(sp.COO.from_numpy(I[f"a_{tag}"], fill_value=-1.5 + 2j))),
                (f"{op}_gcxs_{tag}", lambda sp, I, f=f, tag=tag: f(sp.GCXS.from_numpy(I[f"b_{tag}"], compressed_axes=(1,)))),
            ]
        out += [
            (f"sum_rows_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).sum(axis=1)),
            (f"sum_cols_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).sum(axis=0)),
            (f"sum_all_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).sum()),
            (f"sum_all_keepdims_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).sum(axis=(0, 1), keepdims=True)),
            (f"sum_rows_keepdims_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).sum(axis=1, keepdims=True)),
            (f"sum_rows_fill_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag, fill_value=0.5 - 0.25j).sum(axis=1)),
            (f"mean_rows_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).mean(axis=1)),
            (f"mean_all_{tag}", lambda sp, I, tag=tag: _red(sp, I, tag).mean()),
            (f"sum_3d_two_axes_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"x3_{tag}"]).sum(axis=(0, 2))),
            (f"sum_3d_middle_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"x3_{tag}"]).sum(axis=1)),
            (f"sum_gcxs_rows_{tag}", lambda sp, I, tag=tag: sp.GCXS(_red(sp, I, tag), compressed_axes=(0,)).sum(axis=1)),
            (f"sum_gcxs_cols_{tag}", lambda sp, I, tag=tag: sp.GCXS(_red(sp, I, tag), compressed_axes=(1,)).sum(axis=0)),
            (f"sum_gcxs_all_{tag}", lambda sp, I, tag=tag: sp.GCXS.from_numpy(I[f"a_{tag}"]).sum()),
            (f"prod_rows_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"x3_{tag}"]).prod(axis=2)),
            (f"prod_fill_one_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"p_{tag}"], fill_value=1).prod(axis=1)),
            (f"prod_fill_one_all_{tag}", lambda sp, I, tag=tag: sp.COO.from_numpy(I[f"p_{tag}"], fill_value=1).prod()),
            (f"prod_runs_{tag}", lambda sp, I, tag=tag: (_red(sp, I, tag)[:, :40] * 0.5).prod(axis=0)),
        ]
    return out


def case_names():
    return [n for n, _ in cases()]


def put_result(store, name, r, sp):
    if isinstance(r, np.ndarray) or np.isscalar(r):
        store[name + "__out"] = np.asarray(r)
        return
    c = r.tocoo() if isinstance(r, sp.GCXS) else r
    c = sp.COO(c.coords, c.data, shape=c.shape, fill_value=c.fill_value)      # canonical: sorted, no duplicates
    store[name + "__coords"], store[name + "__data"] = np.asarray(c.coords).astype(np.int64), np.asarray(c.data)
    store[name + "__fill"] = np.asarray(r.fill_value)
    fmt = (r.compressed_axes[0] if r.compressed_axes else -1) if isinstance(r, sp.GCXS) else 2
    store[name + "__meta"] = np.array([r.nnz, fmt, *r.shape], dtype=np.int64)


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader

    if not ref_loader.available():
        raise SystemExit("the reference tree is not present: the committed fixture cannot be regenerated here")
    sp = ref_loader.load()
    I = inputs()
    store = {"in__" + k: v for k, v in I.items()}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for name, fn in cases():
            put_result(store, name, fn(sp, I), sp)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **store)
    print(f"{OUT}: {len(case_names())} cases, {len(store)} arrays, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

"""Generate tests/golden/masked_matmul.npz by RUNNING THE REAL REFERENCE (pydata/sparse numba_backend, imported in place
through oracle/ref_loader.py) on the expression that sparse_amd.masked_matmul fuses,

    s * (a @ b)            (examples/triangles_example.py: sparse.sum(a @ a * a) / 6)

with all three operands sparse.

    python tools/gen_masked_matmul_golden.py

TEST INFRASTRUCTURE.  Runs only where the reference tree exists; the fixture it writes is committed and pins
sparse_amd.masked_matmul (tests/test_masked_matmul.py, tests/test_masked_matmul_gpu.py).  Fixed seeds; only arrays go into the
file.  `case_names()` lists every case the file must hold.

Layout: case `<name>` stores, for each operand x of s, a, b, `<name>__x_coords` / `__x_data` / `__x_shape` (canonical COO
form), `<name>__formats` (three flags, for s, a, b: 0 COO, 1 GCXS compressed by rows, 2 GCXS compressed by columns - the
containers the reference evaluated the expression on, and the ones the tests pass) and `<name>__out` (the reference's
result, densified).  The reference also stores -0.0 at product positions outside the mask (a negative product times the
mask's +0 fill); the dense image keeps them as zeros, which compare equal."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "masked_matmul.npz")

F32, F64, I64 = np.float32, np.float64, np.int64
COO, G0, G1 = 0, 1, 2


def _cases():
    """(name, (M, K, N), (density of s, a, b), (dtype of s, a, b), (format of s, a, b), options)"""
    out = []
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        for fmts, ftag in (((COO, COO, COO), "coo"), ((G0, G0, G0), "gcxs0"), ((G1, G1, G1), "gcxs1"),
                           ((COO, G0, G1), "coo_g0_g1"), ((G1, COO, G0), "g1_coo_g0"), ((G0, G1, COO), "g0_g1_coo")):
            out.append((f"{tag}_{ftag}", (13, 17, 11), (0.5, 0.4, 0.4), (dt, dt, dt), fmts, ()))
    out += [("i64_coo", (13, 17, 11), (0.5, 0.4, 0.4), (I64, I64, I64), (COO, COO, COO), ()),
            ("i64_g0_g1_coo", (13, 17, 11), (0.5, 0.4, 0.4), (I64, I64, I64), (G0, G1, COO), ()),
            ("i64_g1_coo_g0", (9, 1, 7), (0.7, 0.8, 0.8), (I64, I64, I64), (G1, COO, G0), ()),
            ("negmask_f64_coo", (13, 17, 11), (0.6, 0.4, 0.4), (F64, F64, F64), (COO, COO, COO), ("negmask",)),
            ("negmask_f32_g1_g0_g1", (13, 17, 11), (0.6, 0.4, 0.4), (F32, F32, F32), (G1, G0, G1), ("negmask",)),
            ("emptyrows_f32_coo", (13, 17, 11), (0.6, 0.4, 0.4), (F32, F32, F32), (COO, COO, COO), ("emptyrows", "emptycols")),
            ("emptyrows_f64_g0_g0_g1", (13, 17, 11), (0.6, 0.4, 0.4), (F64, F64, F64), (G0, G0, G1), ("emptyrows", "emptycols")),
            ("mixed_i64mask_f32_f64", (13, 17, 11), (0.5, 0.4, 0.4), (I64, F32, F64), (COO, G0, G1), ()),
            ("dense_f32_coo", (6, 7, 5), (1.0, 1.0, 1.0), (F32, F32, F32), (COO, COO, COO), ()),
            ("triangles_i64_coo", (14, 14, 14), (0.0, 0.3, 0.0), (I64, I64, I64), (COO, COO, COO), ("triangles",)),
            ("triangles_i64_gcxs", (14, 14, 14), (0.0, 0.3, 0.0), (I64, I64, I64), (G0, G1, G0), ("triangles",))]
    return out


def case_names():
    return [c[0] for c in _cases()]


def _values(rng, shape, dtype, negative=True):
    if np.dtype(dtype).kind == "i":
        v = rng.integers(1, 6, shape)
        return (v * rng.choice([-1, 1], shape) if negative else v).astype(dtype)
    v = rng.random(shape) + 0.05
    return (v * rng.choice([-1, 1], shape) if negative else v).astype(dtype)


def _dense(rng, shape, density, dtype, negative=True):
    return np.where(rng.random(shape) < density, _values(rng, shape, dtype, negative), 0).astype(dtype)


def _container(sp, dense, fmt):
    if fmt == COO:
        return sp.COO.from_numpy(dense)
    return sp.GCXS.from_numpy(dense, compressed_axes=(0,) if fmt == G0 else (1,))


def generate(sp):
    cases = {}
    for k, (name, (M, Kd, N), dens, dts, fmts, opts) in enumerate(_cases()):
        rng = np.random.default_rng(7000 + k)
        if "triangles" in opts:
            up = np.triu(rng.random((M, M)) < dens[1], 1)
            a = b = s = (up | up.T).astype(dts[1])          # symmetric 0/1, empty diagonal
        else:
            s = _dense(rng, (M, N), dens[0], dts[0], negative="negmask" in opts)
            a = _dense(rng, (M, Kd), dens[1], dts[1])
            b = _dense(rng, (Kd, N), dens[2], dts[2])
            if "emptyrows" in opts:
                a[[0, 5, M - 1]] = 0
            if "emptycols" in opts:
                b[:, [1, 4, N - 1]] = 0
        ops = [_container(sp, x, f) for x, f in zip((s, a, b), fmts)]
        r = ops[0] * (ops[1] @ ops[2])
        r = r.todense() if hasattr(r, "todense") else np.asarray(r)
        assert r.shape == (M, N), (name, r.shape)
        if "triangles" in opts:
            assert int(r.sum()) == int(np.trace(np.linalg.matrix_power(a.astype(np.int64), 3))), name
        for tag, x in zip("sab", (s, a, b)):
            coo = sp.COO.from_numpy(x)
            cases[f"{name}__{tag}_coords"], cases[f"{name}__{tag}_data"] = coo.coords.astype(np.int64), coo.data
            cases[f"{name}__{tag}_shape"] = np.array(x.shape)
        cases[name + "__formats"] = np.array(fmts)
        cases[name + "__out"] = r
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

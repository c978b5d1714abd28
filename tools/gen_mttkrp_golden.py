"""Generate tests/golden/mttkrp.npz by RUNNING THE REAL REFERENCE (pydata/sparse numba_backend, imported in place through
oracle/ref_loader.py) on its own MTTKRP expression (examples/mttkrp_example.py), generalised to N modes and any kept mode:

    sparse.sum(B[..., None] * U_d[None, .., :, .., None, :] * ..., axis=every tensor axis but `mode`)

    python tools/gen_mttkrp_golden.py

TEST INFRASTRUCTURE.  Runs only where the reference tree exists; the fixture it writes is committed and pins
sparse_amd.mttkrp (tests/test_mttkrp.py, tests/test_mttkrp_gpu.py).  Fixed seeds; only arrays go into the file.
`case_names()` lists every case the file must hold.

Layout: case `<name>` stores `<name>__coords` / `__data` / `__shape` (the tensor in canonical COO form), `__gcxs` (1: the
reference evaluated the expression on the GCXS form, and the tests pass a GCXS), `__u<d>` (the factor of every dimension but
the mode), `__mode` and `__out` (the reference's result, densified)."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "mttkrp.npz")

F32, F64, I64 = np.float32, np.float64, np.int64


def _cases():
    """(name, shape, density, mode, gcxs, factor dtype, value dtype, R, emptied slices along the mode)"""
    out = [("d2_m0_coo_f64_vf64_r5", (12, 9), 0.3, 0, False, F64, F64, 5, ()),
           ("d2_m1_gcxs_f32_vf32_r1", (12, 9), 0.3, 1, True, F32, F32, 1, ())]
    for m in range(3):      # every mode of the 3-D tensor, both containers
        out.append((f"d3_m{m}_coo_f64_vf64_r25", (12, 9, 7), 0.15, m, False, F64, F64, 25, ()))
        out.append((f"d3_m{m}_gcxs_f32_vf32_r5", (12, 9, 7), 0.15, m, True, F32, F32, 5, ()))
    for m in range(4):      # every mode of the 4-D tensor; integer values
        out.append((f"d4_m{m}_coo_f32_vi64_r5", (6, 5, 4, 3), 0.2, m, False, F32, I64, 5, ()))
        out.append((f"d4_m{m}_gcxs_f64_vi64_r1", (6, 5, 4, 3), 0.2, m, True, F64, I64, 1, ()))
    out += [("d5_m2_coo_f64_vf32_r5", (4, 3, 5, 2, 3), 0.2, 2, False, F64, F32, 5, ()),
            ("d5_m4_gcxs_f32_vf32_r25", (4, 3, 5, 2, 3), 0.2, 4, True, F32, F32, 25, ())]
    for m in range(3):      # a dimension of size 1, kept and contracted
        out.append((f"one_m{m}_coo_f64_vf64_r5", (7, 1, 6), 0.4, m, False, F64, F64, 5, ()))
    out += [("empty_m0_coo_f32_vf32_r5", (12, 9, 7), 0.15, 0, False, F32, F32, 5, (0, 3, 11)),
            ("empty_m1_gcxs_f64_vf64_r25", (12, 9, 7), 0.15, 1, True, F64, F64, 25, (2, 8))]
    return out


def case_names():
    return [c[0] for c in _cases()]


def _values(rng, shape, dtype):
    if np.dtype(dtype).kind == "i":
        return (rng.integers(1, 6, shape) * rng.choice([-1, 1], shape)).astype(dtype)
    return (rng.random(shape) - 0.5).astype(dtype)


def expression(sp, B, factors, mode):
    """the example's expression for N modes: the tensor with a trailing unit axis times every factor at its own axis and
    the last one, summed over every tensor axis but `mode`"""
    ndim = B.ndim
    t = B[(slice(None),) * ndim + (None,)]
    for d in reversed(range(ndim)):       # the example multiplies by the last mode's factor first (D, then C)
        if d == mode:
            continue
        idx = [None] * ndim + [slice(None)]
        idx[d] = slice(None)
        t = t * factors[d][tuple(idx)]
    return sp.sum(t, axis=tuple(d for d in range(ndim) if d != mode))


def generate(sp):
    cases = {}
    for k, (name, shape, density, mode, gcxs, fdt, vdt, R, emptied) in enumerate(_cases()):
        rng = np.random.default_rng(4000 + k)
        dense = np.where(rng.random(shape) < density, _values(rng, shape, vdt), 0).astype(vdt)
        idx = [slice(None)] * len(shape)
        for i in emptied:
            idx[mode] = i
            dense[tuple(idx)] = 0
        coo = sp.COO.from_numpy(dense)
        B = sp.GCXS.from_numpy(dense) if gcxs else coo
        factors = [None if d == mode else ((rng.random((s, R)) + 0.25) * rng.choice([-1, 1], (s, R))).astype(fdt)
                   for d, s in enumerate(shape)]
        r = expression(sp, B, factors, mode)
        r = r.todense() if hasattr(r, "todense") else np.asarray(r)
        assert r.shape == (shape[mode], R), (name, r.shape)
        cases[name + "__coords"], cases[name + "__data"] = coo.coords.astype(np.int64), coo.data
        cases[name + "__shape"], cases[name + "__mode"], cases[name + "__gcxs"] = np.array(shape), np.array(mode), np.array(int(gcxs))
        for d, f in enumerate(factors):
            if f is not None:
                cases[f"{name}__u{d}"] = f
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

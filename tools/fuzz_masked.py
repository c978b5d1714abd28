"""Random masked_matmul(s, a, b) in exact mode against this library's own `s * (a @ b)`: dense images with equal values
(signed zeros equal, everything else in bits).  Uniform and Zipf-distributed operands (hub rows and columns), all four value
types, both index widths, COO and GCXS containers with either compressed axis, random group / cap / window through the
`_kernels` wrapper against the default's bits.
    python tools/fuzz_masked.py [seconds] [seed]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_amd as sp  # noqa: E402
from sparse_amd import _dot, _kernels as K, _masked, _settings  # noqa: E402

DEV = "cuda:0"


def operand(rng, shape, nnz, dtype, idt, zipf):
    n0, n1 = shape
    nnz = min(nnz, n0 * n1)
    if zipf:      # rows and columns drawn from a Zipf law: a few hubs hold most elements
        r = np.minimum(rng.zipf(1.3, 2 * nnz) - 1, n0 - 1)
        c = np.minimum(rng.zipf(1.3, 2 * nnz) - 1, n1 - 1)
        perm_r, perm_c = rng.permutation(n0), rng.permutation(n1)
        keys = np.unique(perm_r[r] * n1 + perm_c[c])[:nnz]
    else:
        keys = np.sort(rng.choice(n0 * n1, nnz, replace=False)) if n0 * n1 < 1 << 24 else np.unique(rng.integers(0, n0 * n1, nnz))
    if np.dtype(dtype).kind == "i":
        vals = (rng.integers(1, 100, keys.size) * rng.choice([-1, 1], keys.size)).astype(dtype)
    else:
        vals = (rng.random(keys.size) - 0.5).astype(dtype)
    x = sp.COO(np.stack([keys // n1, keys % n1]), vals, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idt, device=DEV)
    fmt = int(rng.integers(0, 3))
    return x if fmt == 0 else x.asformat("gcxs", compressed_axes=(fmt - 1,))


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    _settings.EXACT_MULADD = True
    cases = fails = 0
    t_end = time.time() + budget
    while time.time() < t_end:
        M, Kd, N = (int(rng.choice([1, 7, 64, 300, 2000])) for _ in range(3))
        dtype = [np.float32, np.float64, np.int32, np.int64][int(rng.integers(0, 4))]
        idt = np.int32 if rng.random() < 0.5 else np.int64
        zipf = rng.random() < 0.5
        dens = [float(rng.choice([0.0, 0.01, 0.1, 0.6, 1.0])) for _ in range(3)]
        s, a, b = (operand(rng, sh, int(dn * sh[0] * sh[1]), dtype, idt, zipf)
                   for sh, dn in zip(((M, N), (M, Kd), (Kd, N)), dens))
        got = sp.masked_matmul(s, a, b)
        ref = s * (a @ b)
        ok = got.dtype == ref.dtype and bool((got.todense_device() == ref.todense_device()).all()) and type(got) is type(s)
        if ok and s.nnz and a.nnz and b.nnz:
            sc = s if isinstance(s, sp.COO) else s.tocoo()
            conv = lambda t: (K.convert(t[0], got.data.dtype), t[1], t[2])      # noqa: E731
            trips = (conv(_dot._csr_triplet(sc)), conv(_dot._csr_triplet(a)), conv(_masked._csc_triplet(b)))
            base = K.masked_spgemm((M, N, Kd), *trips, exact=True)
            var = K.masked_spgemm((M, N, Kd), *trips, exact=True, group=int(rng.choice(K.MASKED_GROUPS)),
                                  cap=int(rng.choice([1, 16, 64, 1024, 2048])), window=int(rng.choice([1, 7, 64, 256, 4096])))
            ok = torch.equal(base.view(torch.uint8), var.view(torch.uint8))
        cases += 1
        if not ok:
            fails += 1
            print("MISMATCH", (M, Kd, N), dens, np.dtype(dtype).name, np.dtype(idt).name, zipf,
                  [type(x).__name__ + str(getattr(x, "compressed_axes", "")) for x in (s, a, b)], flush=True)
            if fails > 5:
                break
    print(f"fuzz_masked: {cases} cases, {fails} mismatches (seed {seed})")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()

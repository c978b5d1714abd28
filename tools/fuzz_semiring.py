"""Seeded fuzz of sparse_amd.semiring_matmul (csrc/semiring_spmm.hip) against the NumPy restatement of its contract, bit for bit
for the values (any NaN equals any NaN) and exactly for the args:

    python tools/fuzz_semiring.py [--cases 40] [--seed 0] [--max-nnz 4000]

A case draws: one of the four semirings, float32 | float64 | int32 | int64 values, 32- | 64-bit indices, a chunk of 64 .. 1024,
a form and a sub-group width (or the defaults), uniform or Zipf row lengths (hubs far beyond the chunk among many short rows), a
share of empty rows, a width N of 1 .. 70 or a 1-D b, operands of few distinct values (ties everywhere), now and then
infinities, NaNs and signed zeros, with or without an init - and a COO, a CSR or a CSC of the pattern.  Prints one line per
case; exits 1 at the first difference."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import semiring_cases as sr  # noqa: E402
import sparse_amd  # noqa: E402
from sparse_amd import _attention, _kernels as K  # noqa: E402


def lengths_of(rng, max_nnz):
    nrows = int(rng.integers(1, 120))
    if rng.random() < 0.5:
        n = rng.integers(0, int(rng.choice([4, 40, 200, 1500])) + 1, nrows)
    else:
        n = np.minimum(rng.zipf(float(rng.choice([1.2, 1.6, 2.5])), nrows), max_nnz // 2)
    n[rng.random(nrows) < rng.choice([0.0, 0.3])] = 0
    while n.sum() > max_nnz:
        n[np.argmax(n)] //= 2
    return [int(v) for v in n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-nnz", type=int, default=4000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuzz_semiring.py runs the kernels: no HIP device visible")
    for case in range(a.cases):
        rng = np.random.default_rng([a.seed, case])
        add, mul = sr.SEMIRINGS[int(rng.integers(4))]
        dtype = np.dtype(rng.choice(sr.DTYPES))
        idx = rng.choice([np.int32, np.int64])
        chunk = int(rng.choice([64, 128, 192, 512, 1024]))
        form = [None, "rows", "lanes", "long"][int(rng.integers(4))]
        group = None if rng.random() < 0.3 else int(rng.choice(K.SEMIRING_GROUPS))
        indptr, indices, vals, shape = sr.csr_mask(int(rng.integers(1 << 30)), lengths_of(rng, a.max_nnz), dtype, idx, shuffle=False)
        N = int(rng.choice([0, 1, 2, 3, 4, 5, 8, 17, 33, 70]))
        b = sr.operand(int(rng.integers(1 << 30)), (shape[1],) if N == 0 else (shape[1], N), dtype)
        init = sr.operand(int(rng.integers(1 << 30)), (shape[0],) if N == 0 else (shape[0], N), dtype) if rng.random() < 0.5 else None
        if dtype.kind == "f" and rng.random() < 0.4:
            special = [np.inf, -np.inf, np.nan, 0.0, -0.0]
            if len(vals):
                vals[rng.integers(0, len(vals), 5)] = rng.choice(special, 5)
            b.reshape(-1)[rng.integers(0, b.size, 5)] = rng.choice(special, 5)
            if init is not None:
                init.reshape(-1)[rng.integers(0, init.size, 3)] = rng.choice(special, 3)
        layout = rng.choice(["coo", "csr", "csc"])
        x = sparse_amd.COO(sr.coords_of(indptr, indices), vals, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device="cuda:0")
        if layout != "coo":
            x = x.asformat("gcxs", compressed_axes=(0,) if layout == "csr" else (1,))
        data, ind, ptr = _attention._csr_of_mask(x)
        got = K.semiring_spmm(ptr, ind, data, torch.from_numpy(b).to("cuda:0"), _attention._longest_row(x, ptr), add=add, mul=mul,
                              init=None if init is None else torch.from_numpy(init).to("cuda:0"), return_arg=True, form=form, group=group,
                              chunk=chunk)
        want = sr.semiring_restated(indptr, indices, vals, b, add, mul, init=init)
        ok = sr.same_bits(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
        print(f"case {case}: {add}.{mul} {dtype} {np.dtype(idx)} {layout} form {form} chunk {chunk} group {group} N {N} init {init is not None} "
              f"rows {shape[0]} nnz {len(vals)} longest {int(np.diff(indptr).max())}: {'same bits' if ok else 'DIFFERENT'}", flush=True)
        if not ok:
            raise SystemExit(1)


if __name__ == "__main__":
    main()

"""Seeded fuzz of sparse_amd.softmax (csrc/softmax.hip) against the NumPy restatement of its contract, bit for bit:

    python tools/fuzz_softmax.py [--cases 40] [--seed 0] [--max-nnz 40000]

A case draws: float32 | float64 values, 32- | 64-bit indices, a chunk of 64 .. 1024, a sub-group width, uniform or Zipf group
lengths (hubs far beyond the chunk among many short groups), a share of empty groups, a value spread that reaches the subnormal
results, now and then a scale, an infinity or a NaN - and either a 2-D COO over its rows, a CSR, a CSC over its rows (a
permutation) or a 3-D COO over a middle axis.  Prints one line per case; exits 1 at the first difference."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import softmax_cases as sc  # noqa: E402
import sparse_amd  # noqa: E402
from sparse_amd import _kernels as K  # noqa: E402


def lengths_of(rng, max_nnz):
    ngroups = int(rng.integers(1, 400))
    if rng.random() < 0.5:
        n = rng.integers(0, int(rng.choice([4, 40, 200, 3000])) + 1, ngroups)
    else:
        n = np.minimum(rng.zipf(float(rng.choice([1.2, 1.6, 2.5])), ngroups), max_nnz // 2)
    n[rng.random(ngroups) < rng.choice([0.0, 0.3])] = 0
    while n.sum() > max_nnz:
        n[np.argmax(n)] //= 2
    return [int(v) for v in n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-nnz", type=int, default=40000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuzz_softmax.py runs the kernels: no HIP device visible")
    for case in range(a.cases):
        rng = np.random.default_rng([a.seed, case])
        dtype = rng.choice([np.float32, np.float64])
        idx = rng.choice([np.int32, np.int64])
        K.SOFTMAX_CHUNK = int(rng.choice([64, 128, 192, 512, 1024]))
        group = K.SOFTMAX_GROUP = int(rng.choice(K.SOFTMAX_GROUPS))
        lengths = lengths_of(rng, a.max_nnz)
        coords, data, shape = sc.rows_array(int(rng.integers(1 << 30)), lengths, dtype, idx, spread=float(rng.choice([1, 10, 60, 400])))
        if len(data) and rng.random() < 0.3:
            data[rng.integers(0, len(data), 3)] = rng.choice([np.inf, -np.inf, np.nan, 0.0, -0.0], 3)
        scale = float(rng.choice([-2.0, 0.125, 3.0])) if rng.random() < 0.3 else None
        layout = rng.choice(["coo", "csr", "csc", "coo3"])
        x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device="cuda:0")
        axis = 1
        if layout in ("csr", "csc"):
            x = x.asformat("gcxs", compressed_axes=(0,) if layout == "csr" else (1,))
        elif layout == "coo3":      # the rows become axis 1 of (2, rows, cols): groups over (0, 2) mix both halves
            coords = np.stack([coords[0] % 2, coords[0], coords[1]]).astype(idx)
            order = np.lexsort((coords[2], coords[1], coords[0]))
            coords, data, shape, axis = coords[:, order], data[order], (2,) + shape, (0, 2)
            x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device="cuda:0")
        out = sparse_amd.softmax(x, axis, scale=scale)
        want = sc.softmax_restated(coords, data, shape, axis, K.SOFTMAX_CHUNK, scale)
        if layout in ("csr", "csc"):
            dense = np.zeros(shape, want.dtype)
            dense[tuple(coords)] = want
            ok = sc.same_bits(out.todense(), dense)
        else:
            ok = sc.same_bits(out.data.cpu().numpy(), want)
        print(f"case {case}: {np.dtype(dtype)} {np.dtype(idx)} {layout} chunk {K.SOFTMAX_CHUNK} group {group} scale {scale} "
              f"groups {len(lengths)} nnz {len(data)} longest {max(lengths)}: {'same bits' if ok else 'DIFFERENT'}", flush=True)
        if not ok:
            raise SystemExit(1)


if __name__ == "__main__":
    main()

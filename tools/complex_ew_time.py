"""Times of the complex elementwise operations and reductions on COO operands of 10^7 stored values (20 000 x 50 000 at 1 %),
next to the float64 form of the same call on the same structure:

    python tools/complex_ew_time.py [--reps 5] [--rounds 5] [--dtypes float64 complex64 complex128]

  x + y, x * y        two canonical arrays of one shape (the fused merge: csrc/merge.hip, csrc/merge_complex.hip)
  x * scalar, abs(x)  value kernels (csrc/ewise.hip, csrc/ewise_complex.hip)
  x.sum(axis=0)       50 000 runs of ~200 values after the kept-axis-first reordering; x.sum(): one run of 10^7

The script uses the public interface only, so the same file run in a checkout of an earlier commit measures that commit's
path for the same call (complex values: evaluated by NumPy on the host there).  A complex64 call moves the bytes of the
float64 one, a complex128 call up to twice that.  Method: device events around `reps` back-to-back calls after a warm-up of
every call, `rounds` rounds with the dtypes alternating inside a round; the median over the rounds with the min-max spread.
Prints one JSON line per operation.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_amd as sp  # noqa: E402
from bench import make_csr_device  # noqa: E402


def timed(f, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def operand(M, Kd, seed, dtype):
    re, idx, ptr = make_csr_device(M, Kd, 0.01, seed=seed, dtype=torch.float64)
    re = re - 0.3
    if dtype != "float64":
        g = torch.Generator(device="cuda").manual_seed(seed + 100)
        im = torch.rand(re.numel(), device="cuda", generator=g, dtype=torch.float64) - 0.5
        re = torch.complex(re, im).to(getattr(torch, dtype))
    return sp.GCXS((re, idx, ptr), shape=(M, Kd), compressed_axes=(0,)).tocoo()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", default=["float64", "complex64", "complex128"])
    ap.add_argument("--ops", nargs="*", default=["x + y", "x * y", "x * scalar", "abs(x)", "x.sum(axis=0)", "x.sum()"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("complex_ew_time.py measures on the GPU: no HIP device visible")
    M, Kd = 20_000, 50_000
    xs = {dt: operand(M, Kd, 1, dt) for dt in args.dtypes}
    ys = {dt: operand(M, Kd, 2, dt) for dt in args.dtypes}
    scalar = {"float64": 1.5, "complex64": 2j, "complex128": 2j}
    ops = {"x + y": lambda dt: xs[dt] + ys[dt], "x * y": lambda dt: xs[dt] * ys[dt], "x * scalar": lambda dt: xs[dt] * scalar[dt],
           "abs(x)": lambda dt: abs(xs[dt]), "x.sum(axis=0)": lambda dt: xs[dt].sum(axis=0), "x.sum()": lambda dt: xs[dt].sum()}
    for name in args.ops:
        f = ops[name]
        for dt in args.dtypes:
            f(dt)       # warm-up: code objects, allocator, plans
        times = {dt: [] for dt in args.dtypes}
        for _ in range(args.rounds):
            for dt in args.dtypes:
                times[dt].append(timed(lambda: f(dt), args.reps))
        med = {dt: statistics.median(v) for dt, v in times.items()}
        row = {"op": name, "nnz": int(xs[args.dtypes[0]].nnz), "ms": {dt: round(med[dt], 4) for dt in med},
               "ms_min_max": {dt: [round(min(v), 4), round(max(v), 4)] for dt, v in times.items()}}
        if "float64" in med:
            row["ratio_to_float64"] = {dt: round(med[dt] / med["float64"], 3) for dt in med if dt != "float64"}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

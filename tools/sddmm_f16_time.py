"""Times of `sparse_amd.sddmm` with float16 operands next to bfloat16 and to what a float16 user had to do before
(`sddmm(s, a.float(), bt=bt.float())`, the two conversions inside the timed region), and of one call over a stack of masks
next to the loop of 2-D calls it replaces:

    python tools/sddmm_f16_time.py [--reps 5] [--rounds 7] [--cases config4 block batched]

  config4   BASELINE config 4's shapes: a 100 000 x 100 000 mask of 10^7 uniform samples, K = 256 (column-panel order)
  block     2000 full 32 x 32 tiles of a 16 384 x 16 384 mask, K = 256 (the matrix-core tile path)
  batched   64 masks of 4096 x 4096 with 16 000 samples each, K = 64: one call on the 3-D mask / the loop of 64 2-D calls

The script uses the public interface only, so the same file run in a checkout of an earlier commit measures that commit's path
for the same call; a variant the checkout does not have (float16 operands, a 3-D mask) is reported as null.  Method (that of
tools/complex_ew_time.py): device events around `reps` back-to-back calls after a warm-up of every variant (plans, code
objects, allocator), `rounds` rounds with the variants alternating inside a round; the median over the rounds with the min-max
spread.  Prints one JSON line per case.
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


def timed(f, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(name, variants, reps, rounds, extra=None):
    live = {}
    for tag, f in variants.items():
        try:
            f()               # warm-up; a variant this checkout lacks raises here
            f()
            live[tag] = f
        except (TypeError, ValueError) as e:
            print(f"# {name}: {tag} not available here ({type(e).__name__}: {e})", file=sys.stderr)
    times = {tag: [] for tag in live}
    for _ in range(rounds):
        for tag, f in live.items():
            times[tag].append(timed(f, reps))
    row = {"case": name, "reps": reps, "rounds": rounds,
           "ms": {tag: round(statistics.median(times[tag]), 4) if tag in times else None for tag in variants},
           "ms_min_max": {tag: [round(min(v), 4), round(max(v), 4)] for tag, v in times.items()}}
    row.update(extra or {})
    print(json.dumps(row), flush=True)


def dtype_variants(s, M, N, Kd):
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.rand((M, Kd), device="cuda", generator=g) - 0.5
    bt = torch.rand((N, Kd), device="cuda", generator=g) - 0.5
    ah, bh = a.to(torch.float16), bt.to(torch.float16)
    ab, bb = a.to(torch.bfloat16), bt.to(torch.bfloat16)
    return {"float16": lambda: sp.sddmm(s, ah, bt=bh), "bfloat16": lambda: sp.sddmm(s, ab, bt=bb),
            "float16_widened_to_float32": lambda: sp.sddmm(s, ah.float(), bt=bh.float())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="*", default=["config4", "block", "batched"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_f16_time.py measures on the GPU: no HIP device visible")
    if "config4" in args.cases:
        M = 100_000
        s = sp.random((M, M), nnz=10_000_000, random_state=3, dtype=np.float32, idx_dtype=np.int32)
        measure("config4", dtype_variants(s, M, M, 256), args.reps, args.rounds, {"nnz": int(s.nnz), "K": 256})
        del s
    if "block" in args.cases:
        rng = np.random.default_rng(0)
        M = 16384
        tiles = rng.choice((M // 32) ** 2, 2000, replace=False)
        full = np.arange(1024)
        lin = np.sort((((tiles // (M // 32))[:, None] * 32 + full // 32).astype(np.int64) * M + (tiles % (M // 32))[:, None] * 32 + full % 32).ravel())
        s = sp.COO(np.stack([lin // M, lin % M]).astype(np.int32), rng.random(lin.size).astype(np.float32), shape=(M, M))
        measure("block", dtype_variants(s, M, M, 256), args.reps, args.rounds, {"nnz": int(s.nnz), "K": 256})
        del s
    if "batched" in args.cases:
        rng = np.random.default_rng(5)
        B, M, per, Kd = 64, 4096, 16_000, 64
        lin = np.concatenate([b * M * M + np.sort(rng.choice(M * M, per, replace=False)) for b in range(B)])
        coords = np.stack(np.unravel_index(lin, (B, M, M))).astype(np.int32)
        vals = rng.random(lin.size).astype(np.float32)
        s3 = sp.COO(coords, vals, shape=(B, M, M))
        slices = [sp.COO(coords[1:, b * per:(b + 1) * per], vals[b * per:(b + 1) * per], shape=(M, M)) for b in range(B)]
        a = (torch.rand((B, M, Kd), device="cuda") - 0.5).to(torch.bfloat16)
        bt = (torch.rand((B, M, Kd), device="cuda") - 0.5).to(torch.bfloat16)
        measure("batched", {"one_call_3d_mask": lambda: sp.sddmm(s3, a, bt=bt),
                            "loop_of_2d_calls": lambda: [sp.sddmm(slices[b], a[b], bt=bt[b]) for b in range(B)]},
                args.reps, args.rounds, {"masks": B, "nnz_per_mask": per, "K": Kd, "dtype": "bfloat16"})


if __name__ == "__main__":
    main()

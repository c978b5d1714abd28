"""Times of sparse_amd.softmax (csrc/softmax.hip) beside torch.sparse.softmax on the same device and beside a plain copy of the
same bytes (the yardstick of tools/write_bw.py: one read and one write per value):

    python tools/softmax_time.py [--reps 20] [--rounds 5] [--sweep] [--dtype float32]

  size (a)  a graph of 2^17 nodes, mean degree 32 (row lengths Poisson), 2-D GCXS over its rows: the attention-mask case
  size (b)  ONE hub row of 10^6 stored elements among 2^16 rows of 8: 2-D COO
  size (c)  a 3-D batch of masks, 16 x 2048 x 2048 with 32 stored elements per row on average, COO, softmax over the last axis
  per size: the first call (the plan is built), the call with the plan cached, torch.sparse.softmax of the same coalesced
  tensor, and `y.copy_(x)` of nnz values; --sweep adds the sub-group width, the short / wave threshold and the chunk,
  through the `_kernels` wrapper with the plan built once.

Method: device events around `reps` back-to-back calls after a warm-up, `rounds` rounds, the median with
the min-max spread.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_amd  # noqa: E402
from sparse_amd import _kernels as K, _softmax  # noqa: E402


def timed(f, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_of(f, reps, rounds):
    for _ in range(3):
        f()
    t = [timed(f, reps) for _ in range(rounds)]
    return {"ms": round(statistics.median(t), 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


def random_rows(rng, nrows, ncols, mean):
    """sorted distinct (row, column) pairs, Poisson(mean) per row before the few duplicates are dropped"""
    rows = np.repeat(np.arange(nrows), rng.poisson(mean, nrows))
    keys = np.unique(rows * ncols + rng.integers(0, ncols, len(rows)))
    return keys // ncols, keys % ncols


def build(tag, dtype, d):
    """(the array, the axis, the same elements as a coalesced torch sparse tensor)"""
    rng = np.random.default_rng(17)
    if tag == "graph":
        n = 1 << 17
        rows, cols = random_rows(rng, n, n, 32)
        ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int32)
        data = (rng.standard_normal(len(rows)) * 3).astype(dtype)
        x = sparse_amd.GCXS((data, cols.astype(np.int32), ptr), shape=(n, n), compressed_axes=(0,), device=d)
        coords, shape, axis = np.stack([rows, cols]), (n, n), 1
    elif tag == "hub":
        n, hub = (1 << 16) + 1, 10 ** 6
        lengths = np.full(n, 8)
        lengths[n // 2] = hub
        coords = np.stack([np.repeat(np.arange(n), lengths), np.concatenate([np.arange(m) * (hub // m) for m in (8, hub)])[
            np.concatenate([np.arange(8) if m == 8 else 8 + np.arange(hub) for m in lengths])]])
        data = (rng.standard_normal(coords.shape[1]) * 3).astype(dtype)
        shape, axis = (n, hub), 1
        x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, device=d)
    else:
        B, n = 16, 2048
        rows, cols = random_rows(rng, B * n, n, 32)
        coords, shape, axis = np.stack([rows // n, rows % n, cols]), (B, n, n), 2
        data = (rng.standard_normal(len(rows)) * 3).astype(dtype)
        x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, device=d)
    return x, axis, torch.sparse_coo_tensor(torch.from_numpy(coords).to(d), torch.from_numpy(data).to(d), shape, is_coalesced=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--sizes", nargs="*", default=["graph", "hub", "batch"])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    dtype = np.dtype(args.dtype)
    tiny = sparse_amd.random((8, 80), nnz=200, random_state=1, device=d).astype(dtype)
    sparse_amd.softmax(tiny, 1)                                                       # code objects
    for tag in args.sizes:
        x, axis, tx = build(tag, dtype, d)
        base = {"size": tag, "shape": x.shape, "nnz": x.nnz, "dtype": args.dtype, "format": type(x).__name__}
        first = wall_ms(lambda: sparse_amd.softmax(x, axis))
        plan = x._softmax_plan[(axis,)]
        r = rounds_of(lambda: sparse_amd.softmax(x, axis), args.reps, args.rounds)
        src, dst = x.data, torch.empty_like(x.data)
        c = rounds_of(lambda: dst.copy_(src), args.reps, args.rounds)
        line = {**base, "what": "softmax", "max_len": plan.max_len, "groups": int(plan.segptr.numel()) - 1, "permuted": plan.perm is not None,
                "first_call_wall_ms": first, "cached": r, "copy_same_bytes": c, "times_the_copy": round(r["ms"] / c["ms"], 2)}
        if not args.skip_torch:
            try:
                t = rounds_of(lambda: torch.sparse.softmax(tx, axis), max(args.reps // 4, 2), min(args.rounds, 3))
                got, ref = sparse_amd.softmax(x, axis).data, torch.sparse.softmax(tx, axis).values()
                line.update(torch_sparse_softmax=t, fused_is_faster=r["ms_min_max"][1] < t["ms_min_max"][0],
                            max_abs_diff_to_torch=float((got.double() - ref.double()).abs().max()))
            except Exception as e:      # recorded, not hidden
                line.update(torch_sparse_softmax_raises=f"{type(e).__name__}: {str(e)[:200]}")
        print(json.dumps(line), flush=True)
        if args.sweep:
            data = x.data
            run = lambda **kw: rounds_of(lambda: K.softmax_segments(plan.segptr, plan.perm, data, plan.max_len, **kw),   # noqa: E731
                                         args.reps, args.rounds)
            for g in K.SOFTMAX_GROUPS:
                print(json.dumps({**base, "what": "group", "group": g, **run(group=g)}), flush=True)
            for sm in (0, 16, 32, 64):
                print(json.dumps({**base, "what": "short_max", "short_max": sm, **run(short_max=sm)}), flush=True)
            if plan.max_len > 64:
                for chunk in (64, 128, 256, 512, 1024):
                    print(json.dumps({**base, "what": "chunk", "chunk": chunk, **run(chunk=chunk)}), flush=True)


if __name__ == "__main__":
    main()

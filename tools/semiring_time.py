"""Times of sparse_amd.semiring_matmul (csrc/semiring_spmm.hip) beside the torch expression a user would write today -
`scatter_reduce` with amin / amax over the materialised (nnz, N) products - and beside `sparse_amd.matmul` of the same operands,
the bandwidth yardstick (it moves the same operand bytes):

    python tools/semiring_time.py [--reps 20] [--rounds 5] [--sizes a b c d] [--sweep]

  size (a)  a CSR graph of 2^17 nodes, mean degree 32 (row lengths Poisson), float32, N = 64, max.times, with and without the arg
  size (b)  the same graph, N = 1, min.plus with an init (one Bellman-Ford relaxation)
  size (c)  ONE hub row of 10^6 stored elements among 2^16 rows of 8, N = 16, max.times
  size (d)  200 nodes, mean degree 4, N = 1, min.plus with an init (host-bound; reported only)
  per size the values of the fused call and of the torch expression are compared: `out` must be equal exactly (the seeded
  operands hold no zero and no NaN, so min / max of identical products has one answer).  --sweep adds the sub-group width of
  both forms, the chunk (size c) and the rows / lanes cut-off (the graph at N = 1 .. 16), through the `_kernels` wrapper.

The pass condition: at (a) and (b) `out` equals the torch expression exactly and the fused call is not slower than it; the tool
exits 1 otherwise (after printing every line).

Method: device events around `reps` back-to-back calls after a warm-up; the alternatives of one size take turns inside every one
of the `rounds` rounds, in one process; the median with the min-max spread.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_amd  # noqa: E402
from sparse_amd import _attention, _kernels as K  # noqa: E402


def timed(f, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated(fs, reps, rounds):
    """{name: {"ms": median, "ms_min_max": [min, max]}}: the alternatives take turns inside every round"""
    for f in fs.values():
        for _ in range(3):
            f()
    t = {name: [] for name in fs}
    for _ in range(rounds):
        for name, f in fs.items():
            t[name].append(timed(f, reps))
    return {name: {"ms": round(statistics.median(v), 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)]} for name, v in t.items()}


def random_rows(rng, nrows, ncols, mean):
    """sorted distinct (row, column) pairs, Poisson(mean) per row before the few duplicates are dropped"""
    rows = np.repeat(np.arange(nrows), rng.poisson(mean, nrows))
    keys = np.unique(rows * ncols + rng.integers(0, ncols, len(rows)))
    return keys // ncols, keys % ncols


def build(tag, dtype, d):
    """(the array, rows and columns of its stored elements as device tensors)"""
    rng = np.random.default_rng(17)
    if tag in ("graph", "small"):
        n, mean = (1 << 17, 32) if tag == "graph" else (200, 4)
        rows, cols = random_rows(rng, n, n, mean)
        shape = (n, n)
    else:
        n, hub = (1 << 16) + 1, 10 ** 6
        lengths = np.full(n, 8)
        lengths[n // 2] = hub
        rows = np.repeat(np.arange(n), lengths)
        cols = np.concatenate([np.arange(m) * (hub // m) for m in (8, hub)])[
            np.concatenate([np.arange(8) if m == 8 else 8 + np.arange(hub) for m in lengths])]
        shape = (n, hub)
    ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=shape[0])))).astype(np.int32)
    data = rng.uniform(0.5, 1.5, len(rows)).astype(dtype)                      # no zero, no NaN
    x = sparse_amd.GCXS((data, cols.astype(np.int32), ptr), shape=shape, compressed_axes=(0,), device=d)
    return x, torch.from_numpy(rows).to(d), torch.from_numpy(cols).to(d)


def torch_expression(rows, cols, vals, b, M, add, mul, init):
    """what a user writes today: the (nnz, N) products, then scatter_reduce over the rows; `include_self` per `init`"""
    prod = vals[:, None] * b[cols] if mul == "times" else vals[:, None] + b[cols]
    if init is None:
        base = torch.full((M, b.shape[1]), float("inf") if add == "min" else float("-inf"), dtype=b.dtype, device=b.device)
    else:
        base = init.clone()
    return base.scatter_reduce_(0, rows[:, None].expand(-1, b.shape[1]), prod, "amin" if add == "min" else "amax", include_self=True)


SIZES = {"a": ("graph", 64, "max", "times", False), "b": ("graph", 1, "min", "plus", True), "c": ("hub", 16, "max", "times", False),
         "d": ("small", 1, "min", "plus", True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["a", "b", "c", "d"], choices=sorted(SIZES))
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("semiring_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    dtype = np.dtype("float32")
    built, failed = {}, []
    for size in args.sizes:
        tag, N, add, mul, with_init = SIZES[size]
        if tag not in built:
            built.clear()
            built[tag] = build(tag, dtype, d)
        x, rows, cols = built[tag]
        M, Kd = x.shape
        rng = np.random.default_rng(18)
        b = torch.from_numpy(rng.uniform(0.5, 1.5, (Kd, N)).astype(dtype)).to(d)
        init = torch.from_numpy(rng.uniform(0.5, 40.0, (M, N)).astype(dtype)).to(d) if with_init else None
        kw = dict(add=add, mul=mul, init=init)
        base = {"size": size, "shape": x.shape, "nnz": x.nnz, "N": N, "semiring": f"{add}.{mul}", "init": with_init,
                "max_len": _attention._longest_row(x, x.indptr)}
        fs = {"fused": lambda: sparse_amd.semiring_matmul(x, b, **kw),
              "fused_with_arg": lambda: sparse_amd.semiring_matmul(x, b, return_arg=True, **kw),
              "torch_scatter_reduce": lambda: torch_expression(rows, cols, x.data, b, M, add, mul, init),
              "matmul": lambda: sparse_amd.matmul(x, b)}
        got, ref = fs["fused"](), fs["torch_scatter_reduce"]()
        r = alternated(fs, args.reps, args.rounds)
        print(json.dumps({**base, "what": "semiring_matmul", **r, "out_equals_torch_exactly": bool(torch.equal(got, ref)),
                          "fused_not_slower_than_torch": r["fused"]["ms"] <= r["torch_scatter_reduce"]["ms"],
                          "times_matmul": round(r["fused"]["ms"] / r["matmul"]["ms"], 2)}), flush=True)
        if size in ("a", "b") and not (torch.equal(got, ref) and r["fused"]["ms"] <= r["torch_scatter_reduce"]["ms"]):
            failed.append(size)
        if not args.sweep:
            continue
        vals, max_len = x.data, base["max_len"]
        run = lambda bb=b, **k2: K.semiring_spmm(x.indptr, x.indices, vals, bb, max_len, add=add, mul=mul, init=init, **k2)   # noqa: E731
        for form in ("rows", "lanes") if tag != "hub" else ():
            fg = {f"{form}_group_{g}": (lambda g=g, form=form: run(form=form, group=g)) for g in K.SEMIRING_GROUPS}
            print(json.dumps({**base, "what": f"group of {form}", **alternated(fg, args.reps, args.rounds)}), flush=True)
        if tag == "hub":
            fc = {f"chunk_{c}": (lambda c=c: run(chunk=c)) for c in (64, 256, 512, 1024, 2048, 4096, 16384)}
            print(json.dumps({**base, "what": "chunk", **alternated(fc, args.reps, args.rounds)}), flush=True)
        if size == "a":
            for n in (1, 2, 3, 4, 5, 6, 8, 16):
                bn = b[:, :n].contiguous()
                fn = {form: (lambda form=form, bn=bn: run(bn, form=form)) for form in ("rows", "lanes")}
                print(json.dumps({**base, "what": "rows / lanes cut-off", "N": n, **alternated(fn, args.reps, args.rounds)}), flush=True)

    if failed:
        raise SystemExit(f"semiring_time.py: the pass condition does not hold at size(s) {failed}")


if __name__ == "__main__":
    main()

"""Times of sparse_amd.masked_matmul (csrc/masked_spgemm.hip) next to the expression it fuses, `s * (a @ b)`, evaluated by this
library's own sparse x sparse product and elementwise multiply in the same run:

    python tools/masked_matmul_time.py [--reps 20] [--rounds 5] [--sizes a b c] [--sweep]        (tools/gpu_job.sh py ...)

  size (a)  the example's (examples/triangles_example.py): a symmetric 0/1 graph of 200 nodes, edge probability 0.2, int64,
            s = a = b
  size (b)  a symmetric random graph of 2^17 nodes, mean degree 32, float32 and int64 values, s = a = b
  size (c)  (b)'s operands under a uniform random mask with 1/64 of the stored elements of (b)'s `a`
  per size and value type: the fused call - first call (host wall time, the derived CSR / CSC forms included) and steady state -
  and the expression, first call and steady state; `fused_faster_beyond_spread` compares the slowest fused round with the
  fastest round of the expression.  --sweep: size (b), float32, through the `_kernels` wrapper: every sub-group width, `cap` and `window` one at a time
  around the defaults, then a small joint grid.

Method: device events around `reps` back-to-back calls after a warm-up, `rounds` rounds, the median with the min-max spread.
Prints one JSON line per measurement."""
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
from sparse_amd import _dot, _kernels as K, _masked  # noqa: E402


def timed(f, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_of(f, reps, rounds, warm=2):
    for _ in range(warm):
        f()
    t = [timed(f, reps) for _ in range(rounds)]
    return {"ms": round(statistics.median(t), 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


def graph(n, degree, seed, dtype, device):
    """symmetric graph without self loops: about n * degree stored elements, values 1 (integers) or U(0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    m = n * degree // 2
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    i, j = i[keep], j[keep]
    keys = np.unique(np.concatenate([i * n + j, j * n + i]))
    coords = np.stack([keys // n, keys % n])
    if np.dtype(dtype).kind == "i":
        vals = np.ones(keys.size, dtype=dtype)
    else:      # symmetric values: the value of an edge depends on its unordered pair
        lo, hi = np.minimum(coords[0], coords[1]), np.maximum(coords[0], coords[1])
        vals = (0.5 + ((lo * 2654435761 + hi * 40503) % 1000003) / 1000003).astype(dtype)
    return sparse_amd.COO(coords, vals, shape=(n, n), has_duplicates=False, sorted=True, device=device)


def uniform_mask(n, nnz, seed, dtype, device):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, n * n, nnz))
    return sparse_amd.COO(np.stack([keys // n, keys % n]), np.ones(keys.size, dtype=dtype), shape=(n, n), has_duplicates=False,
                          sorted=True, device=device)


def forget(*xs):
    for x in xs:
        _dot.drop_derived(x)


def measure(tag, s, a, b, dtype, args):
    base = {"size": tag, "dtype": np.dtype(dtype).name, "shape": list(a.shape), "nnz_s": s.nnz, "nnz_a": a.nnz, "nnz_b": b.nnz}
    fused = lambda: sparse_amd.masked_matmul(s, a, b)      # noqa: E731
    expr = lambda: s * (a @ b)                             # noqa: E731
    forget(s, a, b)
    first = wall_ms(fused)
    rf = rounds_of(fused, args.reps, args.rounds)
    print(json.dumps({**base, "what": "masked_matmul", "first_call_wall_ms": first, "steady": rf}), flush=True)
    try:
        forget(s, a, b)
        first_e = wall_ms(expr)
        got, ref = fused(), expr()
        same = bool((got.todense_device() == ref.todense_device()).all()) if a.shape[0] <= 4096 else \
            bool(got.nnz == ref.nnz and torch.equal(got.coords, ref.coords.to(got.coords.dtype)) and
                 torch.allclose(got.data.double(), ref.data.double(), rtol=1e-5))
        prod_nnz = (a @ b).nnz
        re = rounds_of(expr, max(args.reps // 10, 2), min(args.rounds, 3), warm=1)
        print(json.dumps({**base, "what": "expression", "first_call_wall_ms": first_e, "steady": re, "nnz_of_a_at_b": prod_nnz,
                          "same_values_as_fused": same, "fused_steady_ms": rf["ms"],
                          "fused_faster_beyond_spread": rf["ms_min_max"][1] < re["ms_min_max"][0]}), flush=True)
    except Exception as e:      # recorded, not hidden
        print(json.dumps({**base, "what": "expression", "raises": f"{type(e).__name__}: {str(e)[:200]}"}), flush=True)


def sweep(s, a, b, args):
    M, N, Kd = s.shape[0], s.shape[1], a.shape[1]
    trips = (_dot._csr_triplet(s), _dot._csr_triplet(a), _masked._csc_triplet(b))
    for group, cap, window in ([(g, K.MASKED_CAP, K.MASKED_WINDOW) for g in K.MASKED_GROUPS] +
                               [(K.MASKED_GROUP, c, K.MASKED_WINDOW) for c in (1, 64, 128, 256, 512, 1024, 2048)] +
                               [(K.MASKED_GROUP, K.MASKED_CAP, w) for w in (64, 128, 256, 512, 1024, 4096)] +
                               [(g, c, w) for g in (8, 16) for c in (64, 128, 256) for w in (256, 1024)]):
        r = rounds_of(lambda: K.masked_spgemm((M, N, Kd), *trips, group=group, cap=cap, window=window), args.reps, args.rounds)
        print(json.dumps({"what": "sweep", "size": "b", "group": group, "cap": cap, "window": window, **r}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_matmul_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    tiny = graph(64, 8, 1, np.float32, d)
    sparse_amd.masked_matmul(tiny, tiny, tiny)                # code objects
    if "a" in args.sizes:
        rng = np.random.default_rng(0)
        up = np.triu(rng.random((200, 200)) < 0.2, 1)
        a = sparse_amd.COO.from_numpy((up | up.T).astype(np.int64), device=d)
        measure("a", a, a, a, np.int64, args)
    n = 1 << 17
    for dtype in (np.float32, np.int64):
        if not {"b", "c"} & set(args.sizes) and not args.sweep:
            break
        a = graph(n, 32, 7, dtype, d)
        if "b" in args.sizes:
            measure("b", a, a, a, dtype, args)
        if "c" in args.sizes:
            s = uniform_mask(n, a.nnz // 64, 9, dtype, d)
            measure("c", s, a, a, dtype, args)
        if args.sweep and dtype == np.float32:
            sweep(a, a, a, args)


if __name__ == "__main__":
    main()

"""Times of sparse_amd.mttkrp (csrc/mttkrp.hip) next to the reference's expression evaluated by this library as it stands:

    python tools/mttkrp_time.py [--reps 20] [--rounds 5] [--chunks 256 512 1024 2048 4096 8192]

  size (a)  the example's (examples/mttkrp_example.py): 1000 x 1000 x 100 at density 1e-4, R = 25
  size (b)  10^6 stored elements in 2000^3, R = 32
  per size and mode: the first call (the plan is built: a sort of coords[mode] and the row pointers), then the call with the
  plan cached; once per size: `sum(B[:, :, :, None] * D[None, None, :, :] * C[None, :, None, :], axis=(1, 2))` through
  sparse_amd's own indexing, broadcast multiply and sum - or the exception it raises
  chunk sweep: size (b)'s mode 0 (2000 rows of ~500 elements: no row is cut at any chunk above 600 or so) and ONE row holding
  all 10^6 elements (every piece is a chunk), through the `_kernels` wrapper with the plan built once

Method: device events around `reps` back-to-back calls after a warm-up, `rounds` rounds, the median with the min-max
spread; the first call is host wall time around one synchronised call (it includes the plan's launches and their host work).
float32 factors on the device, float64 values in the tensor (converted per call, as the function does).  Prints one JSON
line per measurement."""
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
from sparse_amd import _kernels as K  # noqa: E402


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


def expression(B, C, D):
    """the example's line, mode 0 of a 3-D tensor"""
    return sparse_amd.sum(B[:, :, :, None] * D[None, None, :, :] * C[None, :, None, :], axis=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", type=int, nargs="*", default=[256, 512, 1024, 2048, 4096, 8192])
    ap.add_argument("--skip-expression", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mttkrp_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(3)
    sizes = {"a": ((1000, 1000, 100), None, 1e-4, 25), "b": ((2000, 2000, 2000), 10 ** 6, None, 32)}
    for tag, (shape, nnz, density, R) in sizes.items():
        x = sparse_amd.random(shape, density=density, nnz=nnz, random_state=11, device=d)
        fac = [torch.rand((s, R), device=d, generator=g, dtype=torch.float32) - 0.5 for s in shape]
        base = {"size": tag, "shape": shape, "nnz": x.nnz, "R": R}
        sparse_amd.mttkrp(sparse_amd.random((8, 8, 8), nnz=20, random_state=1, device=d), [f[:8] for f in fac], 1)   # code objects
        cached = {}
        for mode in range(3):
            x.__dict__.pop("_mttkrp_plan", None)
            first = wall_ms(lambda: sparse_amd.mttkrp(x, fac, mode))
            r = rounds_of(lambda: sparse_amd.mttkrp(x, fac, mode), args.reps, args.rounds)
            cached[mode] = r["ms"]
            print(json.dumps({**base, "what": "mttkrp", "mode": mode, "first_call_wall_ms": first, "cached": r}), flush=True)
        if not args.skip_expression:
            try:
                ref = expression(x, fac[1], fac[2])
                got = sparse_amd.mttkrp(x, fac, 0)
                refd = ref.todense() if hasattr(ref, "todense") else ref
                refd = refd if isinstance(refd, torch.Tensor) else torch.as_tensor(np.asarray(refd), device=d)
                err = float((refd.to(torch.float64) - got.to(torch.float64)).abs().max())
                r = rounds_of(lambda: expression(x, fac[1], fac[2]), max(args.reps // 10, 2), min(args.rounds, 3))
                print(json.dumps({**base, "what": "expression", "mode": 0, "result": r, "max_abs_diff_to_mttkrp": err,
                                  "mttkrp_cached_ms": cached[0], "fused_is_faster": cached[0] < r["ms_min_max"][0]}), flush=True)
            except Exception as e:      # recorded, not hidden: the library as it stands may not evaluate the expression
                print(json.dumps({**base, "what": "expression", "mode": 0, "raises": f"{type(e).__name__}: {str(e)[:200]}"}), flush=True)
        if tag == "b":
            # the chunk sweep: short rows (mode 0) and one row of everything (the tensor's elements moved into slice 0 of mode 1)
            data = K.convert(x.data, torch.float32)
            one = x.coords.clone()
            one[1] = 0
            for label, coords, mode in (("rows_of_500", x.coords, 0), ("one_row", one, 1)):
                plan = K.mttkrp_plan(coords, shape, mode)
                for chunk in args.chunks:
                    r = rounds_of(lambda: K.mttkrp_coo(coords, data, shape, fac, mode, plan, chunk=chunk), args.reps, args.rounds)
                    print(json.dumps({**base, "what": "chunk", "rows": label, "chunk": chunk, **r}), flush=True)


if __name__ == "__main__":
    main()

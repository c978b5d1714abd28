"""Times of the complex CSR x dense kernels (csrc/spmm_complex.hip) on config 2's matrix (10^6 x 10^4 at 1 %), next to the
existing float64 kernel of the same family on the same structure:

    python tools/complex_time.py [--reps 20] [--rounds 5]

  N = 1        row-vector kernels: complex64 / complex128 against float64 under SPAMD_SPMM_ROWVEC
  N = 8, 128   row-group kernels:  complex64 / complex128 against float64 under SPAMD_SPMM_ROWGROUP

A complex64 product moves exactly the bytes of a float64 one (8-byte values, the same indices, B rows of N x 8 bytes); a
complex128 product moves twice the value and B bytes.  Method: device events around `reps` back-to-back calls after a
warm-up of every shape, `rounds` rounds with the three kernels alternating inside a round; the median over the rounds is
reported with the min-max spread.  Prints one JSON line per width.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_csr_device  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="*", default=[1, 8, 128])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("complex_time.py measures on the GPU: no HIP device visible")
    M, Kd = 1_000_000, 10_000
    re, idx, ptr = make_csr_device(M, Kd, 0.01, seed=1, dtype=torch.float64)
    g = torch.Generator(device="cuda").manual_seed(2)
    im = torch.rand(re.numel(), device="cuda", generator=g, dtype=torch.float64) - 0.5
    vals = {"float64": re - 0.3, "complex64": torch.complex(re - 0.3, im).to(torch.complex64), "complex128": torch.complex(re - 0.3, im)}
    del re, im
    nnz = int(idx.numel())
    for N in args.widths:
        br = torch.rand((Kd, N), device="cuda", generator=g, dtype=torch.float64) - 0.5
        bi = torch.rand((Kd, N), device="cuda", generator=g, dtype=torch.float64) - 0.5
        bs = {"float64": br, "complex64": torch.complex(br, bi).to(torch.complex64), "complex128": torch.complex(br, bi)}
        outs = {k: torch.empty((M, N), device="cuda", dtype=v.dtype) for k, v in bs.items()}
        # the float64 kernel of the same family: row-vector for one column, row-group otherwise
        kw = {"float64": dict(rowvec=True) if N == 1 else dict(keep_order=True), "complex64": {}, "complex128": {}}
        calls = {k: (lambda k=k: K.dot_csr_ndarray((M, N), vals[k], idx, ptr, bs[k], out=outs[k], **kw[k])) for k in vals}
        for f in calls.values():       # warm-up: code objects, allocator
            for _ in range(3):
                f()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                times[k].append(timed(f, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        # bytes the algorithm needs: values + indices + pointers once, the result once (B is gathered: cache traffic, not counted)
        need = {k: nnz * (vals[k].element_size() + idx.element_size()) + (M + 1) * ptr.element_size() + M * N * outs[k].element_size()
                for k in vals}
        print(json.dumps({
            "N": N, "kernel": "row-vector" if N == 1 else "row-group",
            "ms": {k: round(med[k], 4) for k in med},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "ratio_to_float64": {k: round(med[k] / med["float64"], 3) for k in ("complex64", "complex128")},
            "byte_ratio_to_float64": {k: round(need[k] / need["float64"], 3) for k in ("complex64", "complex128")},
            "streamed_TBps": {k: round(need[k] / med[k] / 1e9, 3) for k in med},
        }), flush=True)


if __name__ == "__main__":
    main()

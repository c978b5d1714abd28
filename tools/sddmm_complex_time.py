"""Times of `sparse_amd.sddmm` with complex operands on BASELINE config 4's mask (100 000 x 100 000, 10^7 uniform samples), next
to the real call of equal row bytes and to what a complex user had to do before:

    python tools/sddmm_complex_time.py [--reps 5] [--rounds 7] [--cases rows1k short]

  rows1k   1 KB rows: complex64 K = 128 and complex128 K = 64, next to float32 K = 256 and float64 K = 128 (the same row bytes;
           their code objects are not touched by the complex kernels, so they also show the machine's drift), and the workaround:
           two real calls over concatenated [re | im] operands of inner dimension 2K - re = <[ar | ai], [br | -bi]>,
           im = <[ar | ai], [bi | br]> - plus the combine into a complex array (the operand copies are made outside the timed region)
  short    256-byte rows: complex64 K = 32 in the mask's own order and in column-panel order (the host's traffic model chooses
           between the two; here each is forced), next to float32 K = 64 as the public interface runs it

The script uses the public interface only (the element order of `short` is forced by replacing `_kernels.sddmm_panels_pay`, as
the tests do), so the same file run in a checkout of an earlier commit measures that commit's path for the same call; a variant
the checkout does not have (complex operands) is reported as null.  Method (that of tools/sddmm_f16_time.py): device events
around `reps` back-to-back calls after a warm-up of every variant (plans, code objects, allocator), `rounds` rounds with the
variants alternating inside a round; the median over the rounds with the min-max spread.  Prints one JSON line per case; run
it in two processes and compare.
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


def operands(M, N, Kd, rdt, g):
    """(a, bt) complex of real type `rdt`'s precision, and the real parts' copies the workaround needs"""
    ar, ai = (torch.rand((M, Kd), device="cuda", generator=g, dtype=rdt) - 0.5 for _ in range(2))
    br, bi = (torch.rand((N, Kd), device="cuda", generator=g, dtype=rdt) - 0.5 for _ in range(2))
    return torch.complex(ar, ai), torch.complex(br, bi), torch.cat([ar, ai], 1), torch.cat([br, -bi], 1), torch.cat([bi, br], 1)


def forced(order, f):
    """`f` with the element order of the sampled kernel forced: "own" = the mask's order, "panels" = column panels"""
    def run():
        keep = K.sddmm_panels_pay
        K.sddmm_panels_pay = (lambda n, a, bt, width: False) if order == "own" else (lambda n, a, bt, width: bool(width))
        try:
            return f()
        finally:
            K.sddmm_panels_pay = keep
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="*", default=["rows1k", "short"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_complex_time.py measures on the GPU: no HIP device visible")
    M = 100_000
    g = torch.Generator(device="cuda").manual_seed(1)
    s32 = sp.random((M, M), nnz=10_000_000, random_state=3, dtype=np.float32, idx_dtype=np.int32)
    if "rows1k" in args.cases:
        s64 = sp.COO(s32.coords, s32.data.double(), shape=s32.shape, has_duplicates=False, sorted=True)
        a, bt, a2, bre, bim = operands(M, M, 128, torch.float32, g)
        z, zt, z2, zre, zim = operands(M, M, 64, torch.float64, g)
        f32a, f32b = a2.contiguous(), bre.contiguous()            # float32 K = 256: the same 1 KB rows
        f64a, f64b = z2.contiguous(), zre.contiguous()            # float64 K = 128
        measure("rows1k", {
            "complex64_K128": lambda: sp.sddmm(s32, a, bt=bt),
            "float32_K256": lambda: sp.sddmm(s32, f32a, bt=f32b),
            "complex64_as_two_float32_calls": lambda: torch.complex(sp.sddmm(s32, a2, bt=bre).data, sp.sddmm(s32, a2, bt=bim).data),
            "complex128_K64": lambda: sp.sddmm(s64, z, bt=zt),
            "float64_K128": lambda: sp.sddmm(s64, f64a, bt=f64b),
            "complex128_as_two_float64_calls": lambda: torch.complex(sp.sddmm(s64, z2, bt=zre).data, sp.sddmm(s64, z2, bt=zim).data),
        }, args.reps, args.rounds, {"nnz": int(s32.nnz), "row_bytes": 1024})
        del a, bt, a2, bre, bim, z, zt, z2, zre, zim, f32a, f32b, f64a, f64b, s64
    if "short" in args.cases:
        a, bt, a2, bre, _ = operands(M, M, 32, torch.float32, g)
        measure("short", {
            "complex64_K32_own_order": forced("own", lambda: sp.sddmm(s32, a, bt=bt)),
            "complex64_K32_panel_order": forced("panels", lambda: sp.sddmm(s32, a, bt=bt)),
            "float32_K64": lambda: sp.sddmm(s32, a2, bt=bre),
            "float32_K64_own_order": forced("own", lambda: sp.sddmm(s32, a2, bt=bre)),
        }, args.reps, args.rounds, {"nnz": int(s32.nnz), "row_bytes": 256})


if __name__ == "__main__":
    main()

"""Times of sparse_amd.semiring_matmul_grad (csrc/semiring_grad.hip) beside the backward a user gets today - torch autograd
through `scatter_reduce(..., "amax" | "amin", include_self=True)` over the materialised (nnz, N) products - on the same device
and operands, and beside one forward `semiring_matmul` call of this library:

    python tools/semiring_grad_time.py [--reps 20] [--rounds 5] [--sizes a b c d] [--sweep]

  size (a)  a CSR graph of 2^17 nodes, mean degree 32 (row lengths Poisson), float32, N = 64, max.times: da and db
  size (b)  the same graph, N = 1, min.plus with an init: da, db and dinit
  size (c)  the hub matrix of tools/semiring_time.py TRANSPOSED - one hub COLUMN of 10^6 stored elements -, N = 16, max.times
  size (d)  200 nodes, mean degree 4, N = 1, min.plus with an init (host-bound; reported only)
  The seeded operands are random floats without zeros, and the values of the few stored elements whose products tie for an
  output's extremum are redrawn until no output has a tie (`make_tie_free`), so both compute the same gradient: the two must
  agree within 2 n eps sum|terms| per element (n terms summed in another order).  --sweep adds
  `group`, `col_group`, `short_max` and `chunk`, one parameter at a time, through the `_kernels` wrapper.

The pass condition: at (a) and (b) the two agree within the bound and the fused backward, with all requested outputs, is not
slower than torch's; the tool exits 1 otherwise (after printing every line).

Method (tools/semiring_time.py): device events around `reps` back-to-back calls after a warm-up; the alternatives of one size
take turns inside every one of the `rounds` rounds, in one process; the median with the min-max spread.  One JSON line per
measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from semiring_time import SIZES, alternated, build, torch_expression  # noqa: E402
import sparse_amd  # noqa: E402
from sparse_amd import _attention, _kernels as K  # noqa: E402


def build_transposed_hub(dtype, d):
    """the hub matrix of semiring_time.py with rows and columns swapped: a hub COLUMN (rows of at most two elements)"""
    x, rows, cols = build("hub", dtype, d)
    r, c = cols.cpu().numpy(), rows.cpu().numpy()
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    shape = (x.shape[1], x.shape[0])
    ptr = np.concatenate(([0], np.cumsum(np.bincount(r, minlength=shape[0])))).astype(np.int32)
    data = x.data.cpu().numpy()[order]
    t = sparse_amd.GCXS((data, c.astype(np.int32), ptr), shape=shape, compressed_axes=(0,), device=d)
    return t, torch.from_numpy(r).to(d), torch.from_numpy(c).to(d)


def tied_elements(x, rows, cols, b, out, init, mul):
    """(the stored elements that take part in a tie for an output's extremum, the number of such outputs): a tie is an output
    whose value is attained by more than one candidate - stored elements or the init"""
    prod = x.data[:, None] * b[cols] if mul == "times" else x.data[:, None] + b[cols]
    wins = prod == out[rows]
    count = torch.zeros_like(out).index_add_(0, rows, wins.to(out.dtype))
    if init is not None:
        count += (init == out).to(out.dtype)
    tied = count > 1
    return (wins & tied[rows]).any(1), int(tied.sum())


def make_tie_free(x, rows, cols, b, add, mul, init, seed=19):
    """redraws the values of the stored elements that take part in a tie until no output has one (random float32 products tie
    in a few outputs of millions, and on a tie torch splits the gradient while A18 gives it to the element the forward
    picked); returns the number of tied outputs met on the way"""
    gen = torch.Generator(device=x.data.device).manual_seed(seed)
    met = 0
    for _ in range(20):
        out = sparse_amd.semiring_matmul(x, b, add=add, mul=mul, init=init)
        which, n = tied_elements(x, rows, cols, b, out, init, mul)
        if n == 0:
            return met
        met += n
        x.data[which] = torch.empty(int(which.sum()), dtype=x.data.dtype, device=x.data.device).uniform_(0.5, 1.5, generator=gen)
    raise SystemExit("semiring_grad_time.py: the operands could not be made tie-free")


def within_bound(got, ref, rows, cols, vals, b, arg, g, mul):
    """do (da, db) agree with torch's within 2 n eps sum|terms| per element?  (n: the element's hits; terms: what it sums)"""
    eps = torch.finfo(g.dtype).eps
    hit = arg[rows] == cols[:, None]
    ta = (g[rows] * b[cols] if mul == "times" else g[rows]).abs() * hit
    ok_a = ((got[0] - ref[0]).abs() <= 2 * hit.sum(1) * eps * ta.sum(1)).all()
    tb = (g[rows] * vals[:, None] if mul == "times" else g[rows]).abs() * hit
    n_b = torch.zeros_like(b).index_add_(0, cols, hit.to(b.dtype))
    s_b = torch.zeros_like(b).index_add_(0, cols, tb)
    ok_b = ((got[1] - ref[1]).abs() <= 2 * n_b * eps * s_b).all()
    return bool(ok_a) and bool(ok_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["a", "b", "c", "d"], choices=sorted(SIZES))
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("semiring_grad_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    dtype = np.dtype("float32")
    built, failed = {}, []
    for size in args.sizes:
        tag, N, add, mul, with_init = SIZES[size]
        if tag not in built:
            built.clear()
            built[tag] = build_transposed_hub(dtype, d) if tag == "hub" else build(tag, dtype, d)
        x, rows, cols = built[tag]
        M, Kd = x.shape
        rng = np.random.default_rng(18)
        b = torch.from_numpy(rng.uniform(0.5, 1.5, (Kd, N)).astype(dtype)).to(d)
        init = torch.from_numpy(rng.uniform(0.5, 40.0, (M, N)).astype(dtype)).to(d) if with_init else None
        g = torch.from_numpy(rng.standard_normal((M, N)).astype(dtype)).to(d)
        ties = make_tie_free(x, rows, cols, b, add, mul, init)
        out, arg = sparse_amd.semiring_matmul(x, b, add=add, mul=mul, init=init, return_arg=True)
        plan = _attention._column_grouping(x, x.indices, x.indptr)
        base = {"size": size, "shape": x.shape, "nnz": x.nnz, "N": N, "semiring": f"{add}.{mul}", "init": with_init,
                "max_len": _attention._longest_row(x, x.indptr), "max_col": plan["max_col"], "tied_outputs_redrawn": ties}
        # torch: the graph is built once, its backward is what is timed
        tv, tb = x.data.clone().requires_grad_(), b.clone().requires_grad_()
        ti = init.clone().requires_grad_() if with_init else None
        tout = torch_expression(rows, cols, tv, tb, M, add, mul, ti)
        inputs = (tv, tb) + ((ti,) if with_init else ())
        fs = {"fused_backward": lambda: sparse_amd.semiring_matmul_grad(x, b, arg, g, mul=mul, with_init=with_init),
              "torch_autograd_backward": lambda: torch.autograd.grad(tout, inputs, g, retain_graph=True),
              "forward_with_arg": lambda: sparse_amd.semiring_matmul(x, b, add=add, mul=mul, init=init, return_arg=True)}
        got, ref = fs["fused_backward"](), fs["torch_autograd_backward"]()
        same_out = bool(torch.equal(out, tout.detach()))
        agree = within_bound(got, ref, rows, cols, x.data, b, arg, g, mul) and (not with_init or bool(torch.equal(got[2], ref[2] + 0.0)))
        r = alternated(fs, args.reps, args.rounds)
        not_slower = r["fused_backward"]["ms"] <= r["torch_autograd_backward"]["ms"]
        print(json.dumps({**base, "what": "semiring_matmul_grad", **r, "forward_equals_torch_exactly": same_out,
                          "agrees_with_torch_within_the_bound": agree, "fused_not_slower_than_torch": not_slower,
                          "forward_calls": round(r["fused_backward"]["ms"] / r["forward_with_arg"]["ms"], 2)}), flush=True)
        if size in ("a", "b") and not (agree and not_slower):
            failed.append(size)
        if not args.sweep:
            continue

        def run(want=(True, True, with_init), **kw):
            return K.semiring_grad(x.indptr, x.indices, x.data, plan["colptr"], plan["colperm"], plan["colrows"], b, arg, g,
                                   plan["max_col"], mul=mul, want=want, **kw)

        fg = {f"group_{w}": (lambda w=w: run(want=(True, False, False), group=w)) for w in K.SEMIRING_GROUPS}
        print(json.dumps({**base, "what": "group (element pass alone)", **alternated(fg, args.reps, args.rounds)}), flush=True)
        widths = [w for w in K.SEMIRING_GRAD_COL_GROUPS if w > 1 or N <= K.SEMIRING_GRAD_LANE_MAX_N]
        fc = {f"col_group_{w}": (lambda w=w: run(want=(False, True, False), col_group=w)) for w in widths}
        print(json.dumps({**base, "what": "col_group (column pass alone)", **alternated(fc, args.reps, args.rounds)}), flush=True)
        fm = {f"short_max_{m}": (lambda m=m: run(want=(False, True, False), short_max=m)) for m in (0, 8, 16, 32, 64)}
        print(json.dumps({**base, "what": "short_max (column pass alone)", **alternated(fm, args.reps, args.rounds)}), flush=True)
        if tag == "hub":
            fk = {f"chunk_{c}": (lambda c=c: run(want=(False, True, False), chunk=c)) for c in (64, 256, 512, 1024, 2048, 4096, 16384)}
            print(json.dumps({**base, "what": "chunk (column pass alone)", **alternated(fk, args.reps, args.rounds)}), flush=True)

    if failed:
        raise SystemExit(f"semiring_grad_time.py: the pass condition does not hold at size(s) {failed}")


if __name__ == "__main__":
    main()

"""Times of sparse_amd.sparse_attention_grad (csrc/attention_grad.hip) beside the composed expression through this library that
a user had to write before - in the same process, on the same inputs, a Python loop over the heads where there are several:

    P = softmax(sddmm(s, q, bt=k), scale=c);  E = sddmm(pattern, g, bt=v)
    U = P * E;  delta = U.sum(axis=1);  Z = U - P * delta[:, None];  Y = c * (s * Z)
    dq = Y @ k;  dk = Y.T @ q;  dv = P.T @ g

    python tools/attention_grad_time.py [--reps 20] [--rounds 5] [--sweep] [--sizes graph heads hub hubcol small]
                                        [--bias none|shared|head] [--dropout RATE]

  --bias shared | head: with an additive bias b (a sparse array of the mask's pattern in the composed expression, where
  P = softmax(sddmm(s, q, bt=k) * c + b) and dbias = Z is one more result), beside the fused call without a bias.
  --dropout RATE (combines with --bias): with attention dropout; the composed expression takes keep_scaled of
  tools/attention_time.py, built outside the timed region - E = sddmm(pattern, g, bt=v) * keep_scaled, dv = (P * keep_scaled).T @ g -
  beside the fused call without dropout.

  sizes (a) graph, (b) heads, (c) hub and (d) small are those of tools/attention_time.py; hubcol is the transpose of (c): ONE hub
  COLUMN of 10^6 stored elements among 2^16 columns of 8.  The hub cases are reported only.
  per size: the first fused call (wall clock: the CSR form, the longest row and the column grouping are built), the
  steady-state fused call, the kernels alone through `_kernels.attention_grad_rows`, the forward call, the composed expression
  (first call and steady state), the largest difference between the two gradients, and the derived (not counter-measured)
  bytes per stored element and head of both passes; --sweep adds the two sub-group widths, the short / wave threshold and the
  chunk one at a time.

Method: device events around `reps` back-to-back calls after a warm-up (a quarter of them for the hub cases), `rounds` rounds,
the median with the min-max spread.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_amd  # noqa: E402
from attention_time import DROPOUT_SEED, build as build_forward, make_bias, make_keep, rounds_of, wall_ms  # noqa: E402
from sparse_amd import _attention, _kernels as K  # noqa: E402


def build(tag, d):
    """(mask, pattern, q, k, v, g, scale): `attention_time.build`, transposed for `hubcol`; `pattern` is the mask with ones"""
    s, q, k, v, scale = build_forward("hub" if tag == "hubcol" else tag, d)
    if tag == "hubcol":
        s = s.T.asformat("gcxs", compressed_axes=(0,))
        q, k, v = k, q, torch.randn(q.shape[:-2] + (s.shape[1], v.shape[-1]), device=d, generator=torch.Generator(d).manual_seed(3))
    g = torch.randn(q.shape[:-2] + (s.shape[0], v.shape[-1]), device=d, generator=torch.Generator(d).manual_seed(5))
    pattern = sparse_amd.GCXS((torch.ones_like(s.data), s.indices, s.indptr), shape=s.shape, compressed_axes=(0,))
    return s, pattern, q, k, v, g, scale


def composed_head(s, pattern, q, k, v, g, scale, b=None, ks=None):
    if b is None:
        P = sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k), -1, scale=scale)
    else:
        P = sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k) * scale + b, -1)
    E = sparse_amd.sddmm(pattern, g, bt=v)
    Pd = P
    if ks is not None:
        E, Pd = E * ks, P * ks
    U = P * E
    delta = U.sum(axis=1)
    delta = delta.todense() if hasattr(delta, "todense") else delta
    Z = U - P * delta[:, None]
    Y = (s * Z) * scale
    return (sparse_amd.matmul(Y, k), sparse_amd.matmul(Y.T, q), sparse_amd.matmul(Pd.T, g)) + (() if b is None else (Z,))


def composed(s, pattern, q, k, v, g, scale, sp=None, ks=None):
    """(dq, dk, dv), and with a bias the elementwise dbias (a sparse array per head) as a fourth result"""
    if q.ndim == 2:
        return composed_head(s, pattern, q, k, v, g, scale, None if sp is None else sp[0], None if ks is None else ks[0])
    outs = [composed_head(s, pattern, q[h], k[h], v[h], g[h], scale, None if sp is None else sp[h], None if ks is None else ks[h])
            for h in range(q.shape[0])]
    return tuple(torch.stack([torch.as_tensor(o[i]) for o in outs]) for i in range(3)) + (() if sp is None else ([o[3] for o in outs],))


def traffic(s, H, D, Dv, esz, isz):
    """derived bytes per stored element and head: what each pass must read and write once (gathered rows counted per element,
    as if nothing hit a cache; index arrays shared by the heads)"""
    nnz, (M, N) = s.nnz, s.shape
    row = (isz + esz) / H + (D + Dv) * esz + D * esz + 2 * esz + (M * (D + Dv) * esz + M * D * esz) / nnz
    col = (8 + isz) / H + 2 * esz + (D + Dv) * esz + (N * (D + Dv) * esz) / nnz
    return {"row_pass_bytes_per_element_head": round(row, 1), "column_pass_bytes_per_element_head": round(col, 1)}


def bias_case(args, base, s, pattern, q, k, v, g, scale):
    """the calls with a bias, with dropout, or with both"""
    b, sp = make_bias(args.bias, s, q)
    ks = make_keep(args.dropout, s, q)
    drop = dict(dropout=args.dropout, seed=DROPOUT_SEED) if args.dropout else {}
    fused_call = lambda: sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale, bias=b, **drop)         # noqa: E731
    first = wall_ms(fused_call)
    plan, max_row = s._attention_grad_plan, s._attention_plan["max_len"]
    reps = max(args.reps // 4, 2) if base["size"] in ("hub", "hubcol") else args.reps
    fused = rounds_of(fused_call, reps, args.rounds)
    plain = rounds_of(lambda: sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale), reps, args.rounds)
    nodrop = rounds_of(lambda: sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale, bias=b), reps, args.rounds) if drop else fused
    data, indices, indptr = _attention._csr_of_mask(s)
    kernel = rounds_of(lambda: K.attention_grad_rows(indptr, indices, data, plan["colptr"], plan["colperm"], plan["colrows"], q, k, v,
                                                     g, max_row, plan["max_col"], scale=scale, bias=b, want_dbias=b is not None, **drop),
                       reps, args.rounds)
    first_c = wall_ms(lambda: composed(s, pattern, q, k, v, g, scale, sp, ks))
    comp = rounds_of(lambda: composed(s, pattern, q, k, v, g, scale, sp, ks), reps, args.rounds)
    got, ref = fused_call(), composed(s, pattern, q, k, v, g, scale, sp, ks)
    dev = q.device
    diff = [float((a.double() - torch.as_tensor(np.asarray(r) if not isinstance(r, torch.Tensor) else r).to(dev).double()).abs().max())
            for a, r in zip(got[:3], ref[:3])]
    print(json.dumps({**base, "what": "attention_grad_dropout" if drop else "attention_grad_bias", "bias": args.bias,
                      "dropout": args.dropout, "max_row": max_row, "max_col": plan["max_col"],
                      "first_call_wall_ms": first, "fused": fused, "kernels_alone": kernel, "fused_without_bias": plain,
                      "fused_without_dropout": nodrop, "bias_over_none": round(nodrop["ms"] / plain["ms"], 3),
                      "dropout_over_none": round(fused["ms"] / nodrop["ms"], 3), "composed_first_wall_ms": first_c, "composed": comp,
                      "composed_over_fused": round(comp["ms"] / fused["ms"], 2), "fused_not_slower": fused["ms"] <= comp["ms"],
                      "max_abs_diff_dq_dk_dv": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["graph", "heads", "hub", "hubcol", "small"])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--bias", choices=["none", "shared", "head"], default="none")
    ap.add_argument("--dropout", type=float, default=0.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_grad_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    warm = build("small", d)
    sparse_amd.sparse_attention_grad(warm[0], *warm[2:6], scale=warm[6])                 # code objects
    composed(*warm)
    for tag in args.sizes:
        s, pattern, q, k, v, g, scale = build(tag, d)
        H = 1 if q.ndim == 2 else int(q.shape[0])
        base = {"size": tag, "shape": s.shape, "nnz": s.nnz, "heads": H, "D": int(q.shape[-1]), "Dv": int(v.shape[-1])}
        if args.bias != "none" or args.dropout:
            bias_case(args, base, s, pattern, q, k, v, g, scale)
            continue
        fused_call = lambda: sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale)                 # noqa: E731
        first = wall_ms(fused_call)
        plan, max_row = s._attention_grad_plan, s._attention_plan["max_len"]
        hub = tag in ("hub", "hubcol")
        reps = max(args.reps // 4, 2) if hub else args.reps
        fused = rounds_of(fused_call, reps, args.rounds)
        forward = rounds_of(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale), reps, args.rounds)
        data, indices, indptr = _attention._csr_of_mask(s)
        run = lambda **kw: rounds_of(lambda: K.attention_grad_rows(indptr, indices, data, plan["colptr"], plan["colperm"],    # noqa: E731
                                                                   plan["colrows"], q, k, v, g, max_row, plan["max_col"], scale=scale,
                                                                   **kw), reps, args.rounds)
        kernel = run()
        first_c = wall_ms(lambda: composed(s, pattern, q, k, v, g, scale))
        comp = rounds_of(lambda: composed(s, pattern, q, k, v, g, scale), reps, args.rounds)
        got, ref = fused_call(), composed(s, pattern, q, k, v, g, scale)
        diff = [float((a.double() - torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b).to(d).double()).abs().max())
                for a, b in zip(got, ref)]
        print(json.dumps({**base, "what": "attention_grad", "max_row": max_row, "max_col": plan["max_col"], "first_call_wall_ms": first,
                          "fused": fused, "kernels_alone": kernel, "forward": forward,
                          "backward_over_forward": round(fused["ms"] / forward["ms"], 2), "composed_first_wall_ms": first_c,
                          "composed": comp, "composed_over_fused": round(comp["ms"] / fused["ms"], 2),
                          "fused_not_slower": fused["ms"] <= comp["ms"], "max_abs_diff_dq_dk_dv": diff,
                          **traffic(s, H, base["D"], base["Dv"], 4, indptr.element_size())}), flush=True)
        if args.sweep:
            for w in K.ATTENTION_GROUPS:
                print(json.dumps({**base, "what": "group", "group": w, **run(group=w)}), flush=True)
            for w in K.ATTENTION_GROUPS:
                print(json.dumps({**base, "what": "col_group", "col_group": w, **run(col_group=w)}), flush=True)
            for sm in (0, 16, 32, 64):
                print(json.dumps({**base, "what": "short_max", "short_max": sm, **run(short_max=sm)}), flush=True)
            if max(max_row, plan["max_col"]) > 64:
                for chunk in (64, 128, 256, 512, 1024):
                    print(json.dumps({**base, "what": "chunk", "chunk": chunk, **run(chunk=chunk)}), flush=True)


if __name__ == "__main__":
    main()

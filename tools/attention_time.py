"""Times of sparse_amd.sparse_attention (csrc/attention.hip) beside the three-call expression it fuses,

    matmul(softmax(sddmm(s, q, bt=k), scale=c), v)

through this library, in the same process, on the same inputs (the yardstick: it is what a user wrote before):

    python tools/attention_time.py [--reps 20] [--rounds 5] [--sweep] [--sizes graph heads hub small] [--bias none|shared|head]
                                   [--dropout RATE]

  --bias shared | head: the calls with an additive bias per stored element (one for all heads, or one per head), beside

    matmul(softmax(sddmm(s, q, bt=k) * c + b), v)         with b a sparse array of the mask's pattern

  and beside the fused call without a bias (`bias_over_none`, reported only).
  --dropout RATE (combines with --bias): the calls with attention dropout, beside

    matmul(softmax(sddmm(s, q, bt=k) [* c + b], ...) * keep_scaled, v)

  with keep_scaled a sparse array of the mask's pattern that holds 1 / (1 - RATE) where `sparse_attention_keep_mask` keeps
  and 0 elsewhere, built OUTSIDE the timed region (which favours the composed side), and beside the fused call without
  dropout (`dropout_over_none`, reported only).

  size (a) graph  a CSR graph of 2^17 nodes, mean degree 32 (row lengths Poisson), D = Dv = 64, float32
  size (b) heads  the same graph, H = 8 heads of D = Dv = 16, against a Python loop of the expression over the heads
  size (c) hub    ONE hub row of 10^6 stored elements among 2^16 rows of 8, D = Dv = 64 (reported only)
  size (d) small  200 nodes, mean degree 8, D = Dv = 64: host-bound
  per size: the first fused call (wall clock: the CSR form and the longest row are found), the steady-state fused call, the
  kernel alone through `_kernels.attention_rows`, the three-call expression (first call and steady state), and the largest
  difference between the two results; --sweep adds the sub-group width, the short / wave threshold and the chunk one at a time.

Method: device events around `reps` back-to-back calls after a warm-up, `rounds` rounds, the median with the min-max
spread.  Prints one JSON line per measurement."""
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


def build(tag, d):
    """(mask, q, k, v, scale): the mask a row-compressed GCXS with non-zero values, the operands device tensors"""
    rng = np.random.default_rng(17)
    H, D = (8, 16) if tag == "heads" else (1, 64)
    if tag == "hub":
        n, hub = (1 << 16) + 1, 10 ** 6
        lengths = np.full(n, 8)
        lengths[n // 2] = hub
        cols = np.concatenate([np.arange(m) * (hub // m) for m in lengths[[0, n // 2]]])[
            np.concatenate([np.arange(8) if m == 8 else 8 + np.arange(hub) for m in lengths])]
        ncols = hub
    else:
        n = 200 if tag == "small" else 1 << 17
        rows, cols = random_rows(rng, n, n, 8 if tag == "small" else 32)
        lengths, ncols = np.bincount(rows, minlength=n), n
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    data = rng.uniform(0.5, 1.5, len(cols)).astype(np.float32)
    s = sparse_amd.GCXS((data, cols.astype(np.int32), ptr), shape=(n, ncols), compressed_axes=(0,), device=d)
    lead = (H,) if H > 1 else ()
    q, k, v = (torch.from_numpy(rng.standard_normal(lead + (m, D)).astype(np.float32)).to(d) for m in (n, ncols, ncols))
    return s, q, k, v, D ** -0.5


def make_bias(mode, s, q):
    """(the bias tensor for the fused call, its sparse arrays of the mask's pattern for the composed expression: one per head)"""
    if mode == "none":
        return None, None
    H = 1 if q.ndim == 2 else int(q.shape[0])
    lead = tuple(q.shape[:-2]) if mode == "head" else ()
    b = torch.randn(lead + (s.nnz,), device=q.device, generator=torch.Generator(q.device).manual_seed(11))
    rows = b.reshape(-1, s.nnz)
    sp = [sparse_amd.GCXS((rows[h % rows.shape[0]].contiguous(), s.indices, s.indptr), shape=s.shape, compressed_axes=(0,))
          for h in range(H)]
    return b, sp


DROPOUT_SEED = 29


def make_keep(rate, s, q):
    """keep_scaled of every head: sparse arrays of the mask's pattern, 1 / (1 - rate) where the element is kept, else 0"""
    if not rate:
        return None
    lead = tuple(q.shape[:-2])
    keep = sparse_amd.sparse_attention_keep_mask(s, lead, dropout=rate, seed=DROPOUT_SEED).reshape(-1, s.nnz)
    scaled = keep.to(q.dtype) * (1.0 / (1.0 - rate))
    return [sparse_amd.GCXS((scaled[h].contiguous(), s.indices, s.indptr), shape=s.shape, compressed_axes=(0,)) for h in range(scaled.shape[0])]


def three_calls(s, q, k, v, scale, sp=None, ks=None):
    if sp is not None or ks is not None:
        def one(q, k, v, h):
            if sp is not None:
                p = sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k) * scale + sp[h], -1)
            else:
                p = sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k), -1, scale=scale)
            return sparse_amd.matmul(p if ks is None else p * ks[h], v)

        return one(q, k, v, 0) if q.ndim == 2 else torch.stack([torch.as_tensor(one(q[h], k[h], v[h], h)) for h in range(q.shape[0])])
    if q.ndim == 2:
        return sparse_amd.matmul(sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k), -1, scale=scale), v)
    return torch.stack([sparse_amd.matmul(sparse_amd.softmax(sparse_amd.sddmm(s, q[h], bt=k[h]), -1, scale=scale), v[h])
                        for h in range(q.shape[0])])


def bias_case(args, base, s, q, k, v, scale):
    """the calls with a bias, with dropout, or with both"""
    b, sp = make_bias(args.bias, s, q)
    ks = make_keep(args.dropout, s, q)
    drop = dict(dropout=args.dropout, seed=DROPOUT_SEED) if args.dropout else {}
    first = wall_ms(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale, bias=b, **drop))
    max_len = s._attention_plan["max_len"]
    reps = max(args.reps // 4, 2) if base["size"] == "hub" else args.reps
    fused = rounds_of(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale, bias=b, **drop), reps, args.rounds)
    plain = rounds_of(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale), reps, args.rounds)
    nodrop = rounds_of(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale, bias=b), reps, args.rounds) if drop else fused
    data, indices, indptr = _attention._csr_of_mask(s)
    kernel = rounds_of(lambda: K.attention_rows(indptr, indices, data, q, k, v, max_len, scale=scale, bias=b, **drop), reps, args.rounds)
    first3 = wall_ms(lambda: three_calls(s, q, k, v, scale, sp, ks))
    three = rounds_of(lambda: three_calls(s, q, k, v, scale, sp, ks), reps, args.rounds)
    got, ref = sparse_amd.sparse_attention(s, q, k, v, scale=scale, bias=b, **drop), three_calls(s, q, k, v, scale, sp, ks)
    ref = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.asarray(ref)).to(q.device)
    print(json.dumps({**base, "what": "attention_dropout" if drop else "attention_bias", "bias": args.bias, "dropout": args.dropout,
                      "max_len": max_len, "first_call_wall_ms": first,
                      "fused": fused, "kernel_alone": kernel, "fused_without_bias": plain, "fused_without_dropout": nodrop,
                      "bias_over_none": round(nodrop["ms"] / plain["ms"], 3), "dropout_over_none": round(fused["ms"] / nodrop["ms"], 3),
                      "composed_first_wall_ms": first3, "composed": three,
                      "composed_over_fused": round(three["ms"] / fused["ms"], 2), "fused_not_slower": fused["ms"] <= three["ms"],
                      "max_abs_diff": float((got.double() - ref.double()).abs().max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="*", default=["graph", "heads", "hub", "small"])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--bias", choices=["none", "shared", "head"], default="none")
    ap.add_argument("--dropout", type=float, default=0.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_time.py measures on the GPU: no HIP device visible")
    d = torch.device("cuda", 0)
    ts, tq, tk, tv, tc = build("small", d)
    sparse_amd.sparse_attention(ts, tq, tk, tv, scale=tc)                              # code objects
    three_calls(ts, tq, tk, tv, tc)
    for tag in args.sizes:
        s, q, k, v, scale = build(tag, d)
        base = {"size": tag, "shape": s.shape, "nnz": s.nnz, "heads": 1 if q.ndim == 2 else int(q.shape[0]), "D": int(q.shape[-1]),
                "Dv": int(v.shape[-1])}
        if args.bias != "none" or args.dropout:
            bias_case(args, base, s, q, k, v, scale)
            continue
        first = wall_ms(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale))
        max_len = s._attention_plan["max_len"]
        reps = max(args.reps // 4, 2) if tag == "hub" else args.reps
        fused = rounds_of(lambda: sparse_amd.sparse_attention(s, q, k, v, scale=scale), reps, args.rounds)
        data, indices, indptr = _attention._csr_of_mask(s)
        run = lambda **kw: rounds_of(lambda: K.attention_rows(indptr, indices, data, q, k, v, max_len, scale=scale, **kw),   # noqa: E731
                                     reps, args.rounds)
        kernel = run()
        first3 = wall_ms(lambda: three_calls(s, q, k, v, scale))
        three = rounds_of(lambda: three_calls(s, q, k, v, scale), reps, args.rounds)
        got, ref = sparse_amd.sparse_attention(s, q, k, v, scale=scale), three_calls(s, q, k, v, scale)
        ref = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.asarray(ref)).to(d)
        print(json.dumps({**base, "what": "attention", "max_len": max_len, "first_call_wall_ms": first, "fused": fused,
                          "kernel_alone": kernel, "three_calls_first_wall_ms": first3, "three_calls": three,
                          "three_over_fused": round(three["ms"] / fused["ms"], 2),
                          "fused_not_slower": fused["ms"] <= three["ms"],
                          "max_abs_diff": float((got.double() - ref.double()).abs().max())}), flush=True)
        if args.sweep:
            for g in K.ATTENTION_GROUPS:
                print(json.dumps({**base, "what": "group", "group": g, **run(group=g)}), flush=True)
            for sm in (0, 16, 32, 64):
                print(json.dumps({**base, "what": "short_max", "short_max": sm, **run(short_max=sm)}), flush=True)
            if max_len > 64:
                for chunk in (64, 128, 256, 512, 1024):
                    print(json.dumps({**base, "what": "chunk", "chunk": chunk, **run(chunk=chunk)}), flush=True)


if __name__ == "__main__":
    main()

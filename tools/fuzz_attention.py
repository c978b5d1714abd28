"""Seeded fuzz of sparse_amd.sparse_attention (csrc/attention.hip) against the NumPy restatement of its contract, bit for bit:

    python tools/fuzz_attention.py [--cases 40] [--seed 0] [--max-nnz 6000]

A case draws: float32 | float64 operands, 32- | 64-bit indices, a chunk of 64 .. 1024, a sub-group width, uniform or Zipf row
lengths (hubs beyond the chunk among many short rows), a share of empty rows, D and Dv of 1 .. 140, no head axis or one or two,
float, integer or boolean mask values, a query spread of 1 or 8, now and then a scale, a stored zero, an infinity or a NaN among
the mask values - and the mask as a COO, a COO built unsorted, a CSR or a CSC; the operands as NumPy arrays, device tensors or
row-strided device views; in half of the cases an additive bias, shared or per head, in the order of the array the caller holds,
with -inf entries in some; in half of the cases a dropout of 0.1 to 0.9 under a 64-bit seed (the restatement of
tests/attention_dropout_cases.py then).  Prints one line per case; exits 1 at the first difference."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attention_bias_cases as bc  # noqa: E402
import attention_dropout_cases as dc  # noqa: E402
import attention_cases as ac  # noqa: E402
import attention_grad_cases as gc  # noqa: E402
import softmax_cases as sc  # noqa: E402
import sparse_amd  # noqa: E402
from sparse_amd import _kernels as K  # noqa: E402


def lengths_of(rng, max_nnz):
    nrows = int(rng.integers(1, 120))
    if rng.random() < 0.5:
        n = rng.integers(0, int(rng.choice([4, 40, 200, 1500])) + 1, nrows)
    else:
        n = np.minimum(rng.zipf(float(rng.choice([1.2, 1.6, 2.5])), nrows), max_nnz // 2)
    n[rng.random(nrows) < rng.choice([0.0, 0.3])] = 0
    while n.sum() > max_nnz:
        n[np.argmax(n)] //= 2
    return [int(v) for v in n]


def strided(x):
    w = torch.zeros(x.shape[:-1] + (x.shape[-1] + 5,), dtype=x.dtype, device=x.device)
    w[..., 2:2 + x.shape[-1]] = x
    return w[..., 2:2 + x.shape[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-nnz", type=int, default=6000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuzz_attention.py runs the kernels: no HIP device visible")
    for case in range(a.cases):
        rng = np.random.default_rng([a.seed, case])
        dtype = rng.choice([np.float32, np.float64])
        idx = rng.choice([np.int32, np.int64])
        mdt = rng.choice([dtype, dtype, np.int32, np.int64, np.bool_])
        chunk = K.ATTENTION_CHUNK = int(rng.choice([64, 128, 192, 512, 1024]))
        group = K.ATTENTION_GROUP = int(rng.choice(K.ATTENTION_GROUPS))
        lengths = lengths_of(rng, a.max_nnz)
        D, Dv = (int(rng.choice([1, 3, 16, 17, 63, 64, 65, 128, 140])) for _ in range(2))
        lead = [(), (), (3,), (2, 2)][int(rng.integers(4))]
        indptr, indices, vals, shape = ac.csr_mask(int(rng.integers(1 << 30)), lengths, mdt, idx)
        if len(vals) and np.dtype(mdt).kind == "f" and rng.random() < 0.3:
            vals[rng.integers(0, len(vals), 3)] = rng.choice([np.inf, -np.inf, np.nan, 0.0, -0.0], 3)
        q, k, v = ac.operands(int(rng.integers(1 << 30)), shape, D, Dv, dtype, lead=lead, spread=float(rng.choice([1, 8])))
        scale = float(rng.choice([-2.0, 0.125, 3.0])) if rng.random() < 0.4 else None
        layout = rng.choice(["coo", "unsorted", "csr", "csc"])
        coords = ac.coords_of(indptr, indices).astype(idx)
        if layout == "unsorted":
            perm = rng.permutation(len(vals))
            s = sparse_amd.COO(coords[:, perm], vals[perm], shape=shape, idx_dtype=idx, device="cuda:0")
        else:
            s = sparse_amd.COO(coords, vals, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device="cuda:0")
            if layout in ("csr", "csc"):
                s = s.asformat("gcxs", compressed_axes=(0,) if layout == "csr" else (1,))
        how = rng.choice(["numpy", "torch", "strided"])
        ops = (q, k, v) if how == "numpy" else tuple(torch.from_numpy(x).to("cuda:0") for x in (q, k, v))
        if how == "strided":
            ops = tuple(strided(x) for x in ops)
        brng = np.random.default_rng([a.seed, case, 1])                     # (a stream of its own: the draws above stay as they were)
        bias = None
        if len(vals) and brng.random() < 0.5:                                # a bias in half of the cases: shared or per head, a fifth -inf
            bias = bc.bias_of(int(brng.integers(1 << 30)), len(vals), dtype, None if brng.random() < 0.5 else lead,
                              neg_inf=float(brng.choice([0.0, 0.2])))
        order = gc.column_order(indptr, indices)[0] if layout == "csc" else slice(None)      # the caller's order of `s.data`
        given = None if bias is None else np.ascontiguousarray(bias[..., order])
        if given is not None and how != "numpy":
            given = torch.from_numpy(given).to("cuda:0")
        drng = np.random.default_rng([a.seed, case, 2])                     # (a stream of its own again)
        drop = {}
        if drng.random() < 0.5:                                              # dropout in half of the cases
            drop = dict(dropout=float(drng.choice([0.1, 0.5, 0.6, 0.9])), seed=int(drng.integers(0, 1 << 64, dtype=np.uint64)))
        out = sparse_amd.sparse_attention(s, *ops, scale=scale, bias=given, **drop)
        out = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        if drop:
            want = dc.attention_dropout_heads(indptr, indices, vals, q, k, v, chunk, scale, bias, drop["dropout"], drop["seed"])
        elif bias is None:
            want = ac.attention_heads(indptr, indices, vals, q, k, v, chunk, scale)
        else:
            want = bc.attention_bias_heads(indptr, indices, vals, q, k, v, chunk, scale, bias)
        ok = sc.same_bits(out, want)
        print(f"case {case}: {np.dtype(dtype)} mask {np.dtype(mdt)} {np.dtype(idx)} {layout} {how} chunk {chunk} group {group} scale {scale} "
              f"bias {None if bias is None else bias.shape} dropout {drop.get('dropout')} D {D} Dv {Dv} heads {lead} rows {len(lengths)} nnz {len(vals)} longest {max(lengths)}: {'same bits' if ok else 'DIFFERENT'}",
              flush=True)
        if not ok:
            raise SystemExit(1)


if __name__ == "__main__":
    main()

"""Seeded fuzz of sparse_amd.semiring_matmul_grad against the restatement of include/sparse_amd.h A18
(tests/semiring_grad_cases.py), bit for bit:

    python tools/fuzz_semiring_grad.py [--cases 200] [--seed 0]

Every case draws mul, the add of the forward that makes the arg, the value type, the index width, N (1 .. 140), Zipf row lengths
- and with them Zipf column lengths: the inner indices are drawn from a Zipf law too -, an init or none, the format (COO, CSR,
CSC), the layout of b / grad / arg (contiguous, pitched, transposed, misaligned), and either the public function (default
forms) or the kernel layer with a drawn chunk, column form, short_max and widths.  Prints one line per failure and a summary;
exits 1 if a case fails."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import semiring_cases as sr  # noqa: E402
import semiring_grad_cases as sg  # noqa: E402
import sparse_amd  # noqa: E402
from sparse_amd import _attention as A, _kernels as K  # noqa: E402

DEV = "cuda:0"


def draw_pattern(rng, M, Kd):
    """CSR pattern with Zipf row lengths and Zipf-distributed inner indices (hub rows and hub columns)"""
    lengths = np.minimum(rng.zipf(1.6, M) - 1, Kd)
    weights = 1.0 / np.arange(1, Kd + 1) ** rng.choice([0.0, 0.8, 1.5])
    weights = rng.permutation(weights / weights.sum())
    cols = [np.sort(rng.choice(Kd, n, replace=False, p=weights)) for n in lengths]
    indices = (np.concatenate(cols) if M else np.zeros(0)).astype(np.int64)
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64), indices


def layout(rng, x):
    """a device tensor of the values of `x` (2-D) in a drawn layout"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    kind = rng.choice(["contiguous", "pitched", "transposed", "misaligned"])
    if kind == "contiguous" or x.ndim != 2:
        return t
    if kind == "transposed":
        return t.T.contiguous().T
    pad, off = (int(rng.integers(1, 9)), 0) if kind == "pitched" else (int(rng.integers(0, 5)), int(rng.integers(1, 4)))
    buf = torch.zeros(x.shape[0] * (x.shape[1] + pad) + off, dtype=t.dtype, device=DEV)
    view = buf[off:].reshape(x.shape[0], x.shape[1] + pad)[:, :x.shape[1]]
    view.copy_(t)
    return view


def one_case(rng):
    mul, add = rng.choice(sg.MULS), rng.choice(sr.ADDS)
    dtype = np.dtype(rng.choice([np.float32, np.float64]))
    idx = rng.choice([np.int32, np.int64])
    M, Kd = int(rng.integers(1, 40)), int(rng.integers(1, 300))
    N = int(rng.choice([1, 2, 3, 4, 5, 16, 17, 64, 65, int(rng.integers(1, 141))]))
    indptr, indices = draw_pattern(rng, M, Kd)
    vals = sr.values(rng, len(indices), dtype)
    b = sr.operand(int(rng.integers(1 << 30)), (Kd, N), dtype)
    init = sr.operand(int(rng.integers(1 << 30)), (M, N), dtype) if rng.random() < 0.5 else None
    g = rng.standard_normal((M, N)).astype(dtype)
    arg = sr.semiring_restated(indptr, indices, vals, b, add, mul, init=init)[1]
    fmt = rng.choice(["coo", "csr", "csc"])
    a = sparse_amd.COO(sr.coords_of(indptr, indices), vals, shape=(M, Kd), idx_dtype=idx, device=DEV, has_duplicates=False, sorted=True)
    order = None
    if fmt == "csr":
        a = sparse_amd.GCXS((vals, indices.astype(idx), indptr.astype(idx)), shape=(M, Kd), compressed_axes=(0,), device=DEV)
    elif fmt == "csc":
        a = a.asformat("gcxs", compressed_axes=(1,))
        order = np.lexsort((sr.coords_of(indptr, indices)[0], indices))
    tb, tg, targ = layout(rng, b), layout(rng, g), layout(rng, arg)
    what = dict(mul=mul, add=add, dtype=dtype.name, idx=np.dtype(idx).name, M=M, K=Kd, N=N, nnz=len(indices), init=init is not None, fmt=fmt)
    if rng.random() < 0.5 or len(indices) == 0:
        chunk = sg.CHUNK
        got = sparse_amd.semiring_matmul_grad(a, tb, targ, tg, mul=mul, with_init=True)
    else:
        data, ind, ptr_ = A._csr_of_mask(a)
        plan = A._column_grouping(a, ind, ptr_)
        chunk = int(rng.choice([64, 128, 1024]))
        kw = dict(chunk=chunk, short_max=int(rng.integers(0, 65)), group=int(rng.choice(K.SEMIRING_GROUPS)),
                  col_group=int(rng.choice([w for w in K.SEMIRING_GRAD_COL_GROUPS if w > 1 or N <= 4])))
        if rng.random() < 0.3:
            kw = dict(kw, col_form="long", chunk=None, short_max=None)
            chunk = 64
        what.update(kw)
        got = K.semiring_grad(ptr_, ind, K.convert(data, tb.dtype), plan["colptr"], plan["colperm"], plan["colrows"], tb, targ, tg,
                              plan["max_col"], mul=mul, want=(True, True, True), **kw)
        order = None      # the kernel layer answers in CSR order
    want = sg.grad_restated(indptr, indices, vals, b, arg, g, mul, chunk)
    want = (want[0] if order is None else want[0][order],) + want[1:]
    ok = all(sr.same_bits(t.cpu().numpy(), w) for t, w in zip(got, want))
    return ok, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuzz_semiring_grad.py runs on the GPU: no HIP device visible")
    rng = np.random.default_rng(args.seed)
    bad = 0
    for i in range(args.cases):
        ok, what = one_case(rng)
        if not ok:
            bad += 1
            print(f"FAIL case {i}: {what}", flush=True)
    print(f"fuzz_semiring_grad: {args.cases - bad} of {args.cases} cases bit-identical to the restatement (seed {args.seed})")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()

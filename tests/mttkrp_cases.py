"""MTTKRP: the order contract restated in NumPy, the float64 comparison values and the seeded case generators that
tests/test_mttkrp.py and tests/test_mttkrp_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd imports this.

`mttkrp_restated` is written from the contract in include/sparse_amd.h (A12), not from the kernel:
  a term   t = data[n]; for d ascending, d != mode: t = t * U_d[coords[d][n], r], every product rounded in `dtype`
  a row    its elements in plan order (ascending stored position) are cut into pieces of `chunk`; a piece is summed
           sequentially from +0.0, the piece sums are added in piece order; an empty row is +0.0
It covers the exact mode only (SPAMD_EXACT_MULADD: every multiply and add rounded on its own)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mttkrp.npz")


def mttkrp_restated(coords, data, shape, factors, mode, chunk, dtype):
    dtype = np.dtype(dtype)
    coords = np.asarray(coords)
    ndim, nnz = coords.shape
    mode = mode % ndim
    used = [d for d in range(ndim) if d != mode]
    R = factors[used[0]].shape[1]
    fac = {d: np.asarray(factors[d]).astype(dtype) for d in used}
    vals = np.asarray(data).astype(dtype)
    out = np.zeros((shape[mode], R), dtype=dtype)
    order = np.argsort(coords[mode], kind="stable")        # plan order: by row, stored position ascending within a row
    bounds = np.searchsorted(coords[mode][order], np.arange(shape[mode] + 1))
    for i in range(shape[mode]):
        row = order[bounds[i]:bounds[i + 1]]
        sums = []
        for p0 in range(0, len(row), chunk):
            s = np.zeros(R, dtype=dtype)                   # +0.0
            for n in row[p0:p0 + chunk]:
                t = np.full(R, vals[n], dtype=dtype)
                for d in used:
                    t = t * fac[d][coords[d][n]]
                s = s + t
            sums.append(s)
        if sums:
            total = sums[0]
            for s in sums[1:]:
                total = total + s
            out[i] = total
    return out


def dense_of(coords, data, shape, dtype=np.float64):
    x = np.zeros(shape, dtype=dtype)
    x[tuple(np.asarray(coords))] = np.asarray(data).astype(dtype)
    return x


def mttkrp_einsum(coords, data, shape, factors, mode, absolute=False):
    """float64 np.einsum of the densified tensor with the factors; `absolute`: of the absolute values (sum |terms|)"""
    ndim = len(shape)
    mode = mode % ndim
    f = (lambda a: np.abs(np.asarray(a, dtype=np.float64))) if absolute else (lambda a: np.asarray(a, dtype=np.float64))
    letters = "abcdefgh"[:ndim]
    ops, subs = [f(dense_of(coords, data, shape))], [letters]
    for d in range(ndim):
        if d != mode:
            ops.append(f(factors[d]))
            subs.append(letters[d] + "r")
    return np.einsum(",".join(subs) + "->" + letters[mode] + "r", *ops)


def longest_row(coords, shape, mode):
    c = np.asarray(coords)[mode]
    return int(np.bincount(c, minlength=shape[mode]).max()) if c.size else 0


def bound(coords, data, shape, factors, mode, dtype, other_dtype=None):
    """(n + ndim) * eps * sum|terms| per output element: the gamma_k bound of a term chain of ndim - 1 roundings and a sum
    of n terms (n = the longest row), eps of the result type `dtype`.  `other_dtype`: the type the comparison value was
    computed in, whose own error - the same bound with its eps - is added (float64 against float64: twice the bound)."""
    n = longest_row(coords, shape, mode)
    eps = float(np.finfo(dtype).eps)
    if other_dtype is not None and np.dtype(other_dtype).kind == "f":
        eps += float(np.finfo(other_dtype).eps)
    return (n + len(shape)) * eps * mttkrp_einsum(coords, data, shape, factors, mode, absolute=True)


# ---- seeded generators -------------------------------------------------------------------------------------------------------
def values(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return np.ones(n, dtype=bool)
    if dtype.kind in "iu":
        v = rng.integers(1, 6, n) * rng.choice([-1, 1], n)
        return v.astype(dtype)
    v = rng.random(n) - 0.5
    return np.where(np.abs(v) < 1e-3, 0.25, v).astype(dtype)


def random_tensor(seed, shape, nnz, val_dtype=np.float64, idx_dtype=np.int64):
    """canonical (C-order sorted, duplicate-free) coordinates [ndim, nnz] and values"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    lin = np.sort(rng.choice(size, min(nnz, size), replace=False))
    coords = np.array(np.unravel_index(lin, shape)).astype(idx_dtype).reshape(len(shape), -1)
    return coords, values(rng, coords.shape[1], val_dtype)


def rows_tensor(seed, lengths, rest, mode, val_dtype=np.float64, idx_dtype=np.int64):
    """a tensor whose slice i along `mode` holds lengths[i] stored elements; `rest` are the other dimensions' sizes in
    order.  Returns (coords, data, shape), canonical."""
    rng = np.random.default_rng(seed)
    cells = int(np.prod(rest))
    assert max(lengths) <= cells
    shape = list(rest)
    shape.insert(mode, len(lengths))
    cols = []
    for i, m in enumerate(lengths):
        lin = np.sort(rng.choice(cells, m, replace=False))
        sub = list(np.unravel_index(lin, rest))
        sub.insert(mode, np.full(m, i))
        cols.append(np.array(sub).reshape(len(shape), m))
    coords = np.concatenate(cols, axis=1)
    key = np.ravel_multi_index(tuple(coords), shape)
    coords = coords[:, np.argsort(key, kind="stable")].astype(idx_dtype)
    return coords, values(rng, coords.shape[1], val_dtype), tuple(shape)


def factors_for(seed, shape, R, dtype, mode=None):
    """one (shape[d], R) factor per dimension (None at `mode`), mixed signs, no zeros"""
    rng = np.random.default_rng(seed + 7919)
    out = []
    for d, s in enumerate(shape):
        out.append(None if d == mode else (rng.random((s, R)) + 0.25).astype(dtype) * rng.choice([-1, 1], (s, R)).astype(dtype))
    return out


# ---- the fixture (tools/gen_mttkrp_golden.py writes it by running the reference) ------------------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    names = sorted({k.split("__")[0] for k in z.files})
    cases = {}
    for name in names:
        ndim = int(z[name + "__shape"].size)
        c = {"coords": z[name + "__coords"], "data": z[name + "__data"], "shape": tuple(int(s) for s in z[name + "__shape"]),
             "mode": int(z[name + "__mode"]), "out": z[name + "__out"], "gcxs": bool(z[name + "__gcxs"]),
             "factors": [z[f"{name}__u{d}"] if f"{name}__u{d}" in z.files else None for d in range(ndim)]}
        cases[name] = c
    return cases

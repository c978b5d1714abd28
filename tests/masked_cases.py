"""masked_matmul: the order contract restated in NumPy, the exact comparison values with their bound, and the seeded case
generators that tests/test_masked_matmul.py and tests/test_masked_matmul_gpu.py share.  TEST INFRASTRUCTURE: nothing in
sparse_amd imports this.

`masked_restated` is written from the contract in include/sparse_amd.h (A13), not from the kernel.  At a stored mask
position (i, j) with value m the terms are the k, ascending, stored in both row i of `a` and column j of `b`:
    acc = +0;  per term: acc = acc + a[i, k] * b[k, j];  out = m * acc           (a position without a term: +0)
exact form: every operation rounded on its own in the result type; fused form: a term's multiply and add are one fma, the
mask multiply stays its own operation.  The fma is restated EXACTLY for both float types: for float32 the product is exact
in float64, the sum is rounded to odd there (TwoSum gives the sign of what was lost) and then rounded to float32 - 53 bits
are more than 2 x 24 + 2, so the double rounding is harmless; for float64 it is `math.fma` where Python has it, else exact
rational arithmetic with one correctly rounded division.  Integers wrap as NumPy's do.

A matrix is a triple (coords[2, n], data[n], shape): canonical COO (C-order sorted, no duplicates)."""
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_matmul.npz")


# ---- fused multiply-add on the host -------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma(a, b, c), exactly rounded"""
    a, b, c = float(a), float(b), float(c)
    p = a * b                                       # exact: 24 + 24 bits
    s = p + c
    if not math.isfinite(s) or s == 0.0:
        return np.float32(s)
    t = s - p
    err = (p - (s - t)) + (c - t)                   # TwoSum: p + c = s + err exactly
    if err != 0.0 and (np.float64(s).view(np.int64) & 1) == 0:
        s = math.nextafter(s, math.inf if err > 0 else -math.inf)      # round to odd
    return np.float32(s)


def fma64(a, b, c):
    """float64 fma(a, b, c), exactly rounded"""
    a, b, c = float(a), float(b), float(c)
    if hasattr(math, "fma"):
        try:
            return np.float64(math.fma(a, b, c))
        except (OverflowError, ValueError):
            return np.float64(a * b + c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return np.float64(a * b + c)
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return np.float64(a * b + c)                # the sign of an exact zero: as the two-step form gives it
    try:
        return np.float64(r.numerator / r.denominator)  # int / int is correctly rounded
    except OverflowError:                           # beyond the float64 range: as the `math.fma` branch falls back
        return np.float64(a * b + c)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _rows(m):
    """row -> (columns ascending, values) of a canonical COO triple"""
    coords, data, shape = m
    r = np.asarray(coords[0], dtype=np.int64)
    bounds = np.searchsorted(r, np.arange(shape[0] + 1))
    c = np.asarray(coords[1], dtype=np.int64)
    return [(c[bounds[i]:bounds[i + 1]], data[bounds[i]:bounds[i + 1]]) for i in range(shape[0])]


def transpose(m):
    coords, data, shape = m
    order = np.lexsort((coords[0], coords[1]))
    return np.stack([coords[1][order], coords[0][order]]), np.asarray(data)[order], (shape[1], shape[0])


def terms_of(s, a, b):
    """per stored mask element: (positions in a's row, positions in b's column) of the common k, ascending"""
    arows, bcols = _rows(a), _rows(transpose(b))
    out = []
    for i, j in zip(*np.asarray(s[0], dtype=np.int64)):
        _, ia, ib = np.intersect1d(arows[i][0], bcols[j][0], assume_unique=True, return_indices=True)
        out.append((arows[i][1][ia], bcols[j][1][ib]))
    return out


def masked_restated(s, a, b, dtype, fused=False):
    """the values at the mask's stored positions, in its stored order, in `dtype` (every operand converted to it first)"""
    dtype = np.dtype(dtype)
    cast = lambda m: (m[0], np.asarray(m[1]).astype(dtype), m[2])          # noqa: E731
    s, a, b = cast(s), cast(a), cast(b)
    out = np.zeros(len(s[1]), dtype=dtype)
    fma = fma32 if dtype == np.float32 else fma64
    with np.errstate(all="ignore"):
        for e, (av, bv) in enumerate(terms_of(s, a, b)):
            if len(av) == 0:
                continue                                                  # no term: +0 whatever m is
            acc = dtype.type(0)
            for x, y in zip(av, bv):
                if fused and dtype.kind == "f":
                    acc = fma(x, y, acc)
                else:
                    acc = dtype.type(acc + dtype.type(x * y))
            out[e] = dtype.type(s[1][e] * acc)
    return out


def dense_of(m, dtype=None):
    coords, data, shape = m
    x = np.zeros(shape, dtype=np.asarray(data).dtype if dtype is None else dtype)
    x[tuple(np.asarray(coords, dtype=np.int64))] = np.asarray(data).astype(x.dtype)
    return x


def dense_result(s, vals):
    """the dense image of values given at the mask's stored positions"""
    x = np.zeros(s[2], dtype=vals.dtype)
    x[tuple(np.asarray(s[0], dtype=np.int64))] = vals
    return x


def exact_and_bound(s, a, b, dtype):
    """(want, bound) per stored mask element, from the values as `dtype` holds them: want = m * sum_k a_k b_k as an exact
    rational (a Fraction: no rounding of its own, so the bound below is asserted as it stands, for float64 results too),
    bound = (n + 2) * eps * |m| * sum|a_k b_k| with n the element's term count and eps of `dtype` - n products, n additions
    and the final multiply; the sum of absolute products is exact as well and rounded to float64 once."""
    dtype = np.dtype(dtype)
    f = lambda m: (m[0], np.asarray(m[1]).astype(dtype).astype(np.float64), m[2])      # noqa: E731
    s, a, b = f(s), f(a), f(b)
    eps = float(np.finfo(dtype).eps) if dtype.kind == "f" else 0.0
    want, bound = np.full(len(s[1]), Fraction(0), dtype=object), np.zeros(len(s[1]))
    for e, (av, bv) in enumerate(terms_of(s, a, b)):
        if len(av):
            prods = [Fraction(float(x)) * Fraction(float(y)) for x, y in zip(av, bv)]
            m = Fraction(float(s[1][e]))
            want[e] = m * sum(prods)
            bound[e] = (len(av) + 2) * eps * float(abs(m) * sum(abs(p) for p in prods))
    return want, bound


def abs_err(got, want):
    """|got - want| per element against exact rational `want`: the difference is exact, rounded to float64 once"""
    return np.array([float(abs(Fraction(float(g)) - w)) for g, w in zip(np.asarray(got).ravel(), np.asarray(want).ravel())]
                    ).reshape(np.shape(got))


def term_counts(s, a, b):
    return np.array([len(av) for av, _ in terms_of(s, a, b)], dtype=np.int64)


# ---- seeded generators -------------------------------------------------------------------------------------------------------
def values(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return np.ones(n, dtype=bool)
    if dtype.kind in "iu":
        return (rng.integers(1, 6, n) * rng.choice([-1, 1], n)).astype(dtype)
    v = rng.random(n) - 0.5
    return np.where(np.abs(v) < 1e-3, 0.25, v).astype(dtype)


def big_values(rng, n, dtype):
    """integers large enough for products and sums to wrap"""
    info = np.iinfo(dtype)
    return rng.integers(info.min // 2, info.max // 2, n).astype(dtype)


def random_matrix(seed, shape, nnz, dtype=np.float64, idx_dtype=np.int64):
    rng = np.random.default_rng(seed)
    size = int(shape[0]) * int(shape[1])
    lin = np.sort(rng.choice(size, min(nnz, size), replace=False)) if size else np.zeros(0, np.int64)
    coords = np.array(np.unravel_index(lin, shape)).astype(idx_dtype).reshape(2, -1)
    return coords, values(rng, coords.shape[1], dtype), tuple(shape)


def rows_matrix(seed, lengths, ncols, dtype=np.float64, idx_dtype=np.int64, first=None):
    """row i holds lengths[i] stored elements at random ascending columns of `ncols` (row i's columns are `first[i]` when
    given instead)"""
    rng = np.random.default_rng(seed)
    r, c = [], []
    for i, n in enumerate(lengths):
        cols = np.sort(rng.choice(ncols, n, replace=False)) if first is None or first[i] is None else np.asarray(first[i])
        r.append(np.full(len(cols), i))
        c.append(cols)
    coords = np.stack([np.concatenate(r), np.concatenate(c)]).astype(idx_dtype)
    return coords, values(rng, coords.shape[1], dtype), (len(lengths), ncols)


def cols_matrix(seed, lengths, nrows, dtype=np.float64, idx_dtype=np.int64, first=None):
    """column j holds lengths[j] stored elements: the transpose of `rows_matrix`"""
    c, d, sh = transpose(rows_matrix(seed, lengths, nrows, dtype, idx_dtype, first))
    return c.astype(idx_dtype), d, sh


def full_mask(seed, shape, dtype=np.float64, idx_dtype=np.int64):
    return random_matrix(seed, shape, shape[0] * shape[1], dtype, idx_dtype)


# ---- the fixture (tools/gen_masked_matmul_golden.py writes it by running the reference) ----------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    cases = {}
    for name in sorted({k.split("__")[0] for k in z.files}):
        c = {"out": z[name + "__out"], "formats": tuple(int(v) for v in z[name + "__formats"])}
        for op in "sab":
            c[op] = (z[f"{name}__{op}_coords"], z[f"{name}__{op}_data"], tuple(int(v) for v in z[f"{name}__{op}_shape"]))
        cases[name] = c
    return cases


FORMAT_NAMES = {0: "coo", 1: "gcxs0", 2: "gcxs1"}     # the `formats` flags of a fixture case, for s, a, b

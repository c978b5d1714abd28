"""softmax over stored elements: the order contract restated in NumPy, the exact comparison values with their bound, and the
seeded case generators that tests/test_softmax.py and tests/test_softmax_gpu.py share.  TEST INFRASTRUCTURE: nothing in
sparse_amd imports this.

`exp_det` and `group_softmax` are written from the contract in include/sparse_amd.h (A14) and the step list at the top of
csrc/exp_det.h, not from the kernels.  Every step is one exactly rounded IEEE operation; the fused multiply-adds are the
array forms `fma32v` / `fma64v` of `masked_cases.fma32` / `fma64` (tests/test_softmax.py holds them to those, element by
element): float32 through an exact float64 product and a sum rounded to odd, float64 through an exact product (Veltkamp /
Dekker), two exact sums and one sum rounded to odd (Boldo and Melquiond, "Emulation of FMA and correctly rounded sums", 2008 -
exact unless an intermediate under- or overflows, which the arguments of `exp_det` never make it do).

An array is a triple (coords[ndim, n], data[n], shape) in STORED order; a group is the stored elements that share their
coordinates on the axes that are not normalised, in stored order."""
import math

import numpy as np

# ---- measured accuracy of exp_det (tools/exp_det_ulp.py; DESIGN A14) --------------------------------------------------------
# largest error found, in ulp of the result (normal / subnormal results): float32 0.894 / 0.848 against float64 np.exp over
# 4 x 10^6 arguments; float64 0.863 / 0.876 against longdouble np.exp over 4 x 10^6 and 0.856 / 0.798 against mpmath over 2 x 10^5.
# The bound of the tolerance tests takes the measured value rounded up to the next half ulp; the condition is U <= 3.
U = {np.dtype("float32"): 1.0, np.dtype("float64"): 1.0}
U_MAX = 3.0

_CONSTS = {
    np.dtype("float32"): dict(lo=-104.0, log2e=float.fromhex("0x1.715476p+0"), ln2_hi=float.fromhex("0x1.62e400p-1"),
                              ln2_lo=float.fromhex("0x1.7f7d1cp-20"), degree=7),
    np.dtype("float64"): dict(lo=-746.0, log2e=float.fromhex("0x1.71547652b82fep+0"), ln2_hi=float.fromhex("0x1.62e42fee00000p-1"),
                              ln2_lo=float.fromhex("0x1.a39ef35793c76p-33"), degree=13),
}


# ---- fused multiply-add on arrays --------------------------------------------------------------------------------------------
def _to_odd(s, err):
    """`s`, the float64 rounding of an exact value s + err, rounded to odd instead"""
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    up = np.where(err > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, up), s)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma32v(a, b, c):
    """float32 fma(a, b, c) of arrays, exactly rounded"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                        # exact: 24 + 24 bits
        s, err = _two_sum(p, c)
        ok = np.isfinite(s) & (s != 0)
        return np.where(ok, _to_odd(s, np.where(ok, err, 0.0)), s).astype(np.float32)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64v(a, b, c):
    """float64 fma(a, b, c) of arrays, exactly rounded (no intermediate may under- or overflow)"""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        plain = a * b + c
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        zs, ze = _two_sum(tl, vl)
        z = _to_odd(zs, ze)
        out = vh + z
        return np.where(np.isfinite(plain) & np.isfinite(out), out, plain)


def _fma(dtype):
    return fma32v if dtype == np.float32 else fma64v


# ---- exp_det ---------------------------------------------------------------------------------------------------------------------
def exp_det(d, dtype):
    """csrc/exp_det.h, step by step, for an array of arguments <= 0 (or NaN)"""
    dtype = np.dtype(dtype)
    c, T, fma = _CONSTS[dtype], np.dtype(dtype).type, _fma(dtype)
    d = np.atleast_1d(np.asarray(d, dtype=dtype))
    out = np.zeros(d.shape, dtype=dtype)
    nan = np.isnan(d)
    out[nan] = d[nan]
    with np.errstate(all="ignore"):
        go = ~nan & (d >= T(c["lo"]))
        x = d[go]
        k = np.rint(x * T(c["log2e"]))
        assert k.dtype == dtype
        r = fma(-k, T(c["ln2_hi"]), x)
        r = fma(-k, T(c["ln2_lo"]), r)
        coef = [T(1.0 / math.factorial(i)) for i in range(c["degree"] + 1)]
        p = np.full(x.shape, coef[-1], dtype=dtype)
        for ci in coef[-2::-1]:
            p = fma(p, r, ci)
        out[go] = np.ldexp(p, k.astype(np.int32))
    assert out.dtype == dtype
    return out


def ulp_error(got, want):
    """|got - want| in units of the last place of `got`'s type at `want` (`want` in a wider type; subnormal results count in
    units of the smallest subnormal)"""
    dtype = np.asarray(got).dtype
    fi = np.finfo(dtype)
    want = np.asarray(want)
    w = np.abs(want).astype(np.float64)
    exp = np.floor(np.log2(np.maximum(w, float(fi.smallest_subnormal)))).astype(np.int64)
    ulp = np.ldexp(want.dtype.type(1), np.maximum(exp, fi.minexp) - fi.nmant)        # (in the wider type: no rounding of its own)
    return (np.abs(np.asarray(got).astype(want.dtype) - want) / ulp).astype(np.float64)


def exp_arguments(rng, n, dtype):
    """arguments that cover (-underflow, 0] densely, the subnormal results, and the neighbourhood of 0 down to 1e-8"""
    lo = _CONSTS[np.dtype(dtype)]["lo"]
    sub = float(np.log(np.finfo(dtype).smallest_normal))
    parts = [rng.uniform(lo - 1, 0, n // 2), rng.uniform(lo, sub, n // 8), rng.uniform(-1, 0, n // 8),
             -np.exp(rng.uniform(np.log(1e-8), 0, n // 8)), -np.arange(1, n // 8 + 1) * (math.log(2) / 2) * (1 + rng.uniform(-1e-6, 1e-6, n // 8))]
    return np.concatenate(parts).astype(dtype)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def piece_sum(e):
    """64 accumulators (accumulator l adds e[l], e[l + 64], .. in order), folded by halving"""
    dtype = e.dtype
    rows = np.zeros(-(-len(e) // 64) * 64, dtype=dtype)
    rows[:len(e)] = e
    rows = rows.reshape(-1, 64)
    a = rows[0].copy()
    for row in rows[1:]:
        a = a + row
    h = 32
    while h >= 1:
        a = a[:h] + a[h:2 * h]
        h //= 2
    assert a.dtype == dtype
    return a[0]


def group_softmax(x, chunk, scale=None):
    """one group's values in stored order -> its results, in the type of `x`"""
    dtype = x.dtype
    with np.errstate(all="ignore"):
        t = x if scale is None else dtype.type(scale) * x
        m = dtype.type(np.nan) if np.isnan(t).any() else t.max()
        e = exp_det(t - m, dtype)
        s = None
        for b in range(0, len(e), chunk):
            ps = piece_sum(e[b:b + chunk])
            s = ps if s is None else s + ps
        out = e / s
    assert out.dtype == dtype
    return out


def result_dtype(dtype):
    return np.dtype(dtype) if np.dtype(dtype) in (np.dtype("float32"), np.dtype("float64")) else np.dtype("float64")


def groups_of(coords, shape, axis):
    """lists of stored positions, one per non-empty group, each ascending (stored order)"""
    axis = tuple(a % len(shape) for a in (axis if isinstance(axis, tuple) else (axis,)))
    kept = [a for a in range(len(shape)) if a not in axis]
    n = coords.shape[1]
    if not kept:
        return [np.arange(n)] if n else []
    gid = np.ravel_multi_index(tuple(np.asarray(coords[a], dtype=np.int64) for a in kept), tuple(shape[a] for a in kept))
    order = np.argsort(gid, kind="stable")
    cuts = np.flatnonzero(np.diff(gid[order])) + 1
    return [g for g in np.split(order, cuts) if len(g)]


def softmax_restated(coords, data, shape, axis, chunk, scale=None):
    """the values at the stored positions, in stored order"""
    x = np.asarray(data).astype(result_dtype(np.asarray(data).dtype))
    out = np.zeros_like(x)
    for g in groups_of(np.asarray(coords), shape, axis):
        out[g] = group_softmax(x[g], chunk, scale)
    return out


def dense_neg_inf(coords, data, shape, scale=None):
    """float64 dense image with -inf at the unstored positions (scale applied in the values' result type first)"""
    x = np.asarray(data).astype(result_dtype(np.asarray(data).dtype))
    if scale is not None:
        x = x.dtype.type(scale) * x
    d = np.full(shape, -np.inf)
    d[tuple(np.asarray(coords, dtype=np.int64))] = x.astype(np.float64)
    return d


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload of a NaN is no result)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = f"u{a.dtype.itemsize}"
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


# ---- exact values and the bound --------------------------------------------------------------------------------------------------
def exact_and_bound(coords, data, shape, axis, scale=None, use_mpmath=False):
    """(want, bound) per stored element, both longdouble, from the ROUNDED t_i = scale * x_i (so `scale` enters exactly):
    want = exp(t_i - m) / sum_j exp(t_j - m), by mpmath at 80 digits or in longdouble;
    bound = (D + 2 U + n / 2 + 1) * eps * want + the smallest subnormal, D the largest finite |t_j - m| of the group, n its
    length, eps and U of the result type: the subtraction's rounding scales by |d|, two exponentials' errors, n - 1
    additions of positive terms and one division; + 1 for the second-order terms.  Groups with a NaN or an infinite maximum
    are left NaN (they have no tolerance: tests/test_softmax_gpu.py checks them as facts)."""
    x = np.asarray(data).astype(result_dtype(np.asarray(data).dtype))
    dtype = x.dtype
    with np.errstate(all="ignore"):
        t = x if scale is None else dtype.type(scale) * x
    fi = np.finfo(dtype)
    want = np.full(len(t), np.nan, dtype=np.longdouble)
    bound = np.full(len(t), np.nan, dtype=np.longdouble)
    for g in groups_of(np.asarray(coords), shape, axis):
        tg = t[g].astype(np.longdouble)
        m = tg.max() if not np.isnan(tg).any() else np.nan
        if not np.isfinite(m):
            continue
        d = tg - m                                              # exact in longdouble: both are values of the narrower type
        if use_mpmath:
            import mpmath

            with mpmath.workprec(270):
                e = [mpmath.exp(mpmath.mpf(float(v))) if np.isfinite(v) else mpmath.mpf(0) for v in d]
                s = mpmath.fsum(e)
                p = np.array([np.longdouble(mpmath.nstr(v / s, 25)) for v in e], dtype=np.longdouble)
        else:
            e = np.exp(d)
            p = e / e.sum()
        D = float(np.abs(d[np.isfinite(d)]).max())
        want[g] = p
        bound[g] = (D + 2 * U[dtype] + len(g) / 2 + 1) * np.longdouble(fi.eps) * p + np.longdouble(fi.smallest_subnormal)
    return want, bound


def bound_share(got, want, bound):
    """the largest |got - want| / bound over the elements that have a bound"""
    ok = ~np.isnan(bound)
    if not ok.any():
        return 0.0
    return float((np.abs(np.asarray(got)[ok].astype(np.longdouble) - want[ok]) / bound[ok]).max())


# ---- seeded generators -----------------------------------------------------------------------------------------------------------
def rows_array(seed, lengths, dtype=np.float32, idx_dtype=np.int64, spread=3.0):
    """2-D canonical COO triple whose row i holds lengths[i] stored elements at random ascending columns"""
    rng = np.random.default_rng(seed)
    ncols = max(max(lengths, default=0), 1) + 3
    r, c = [], []
    for i, n in enumerate(lengths):
        r.append(np.full(n, i))
        c.append(np.sort(rng.choice(ncols, n, replace=False)))
    coords = np.stack([np.concatenate(r), np.concatenate(c)]).astype(idx_dtype) if lengths else np.zeros((2, 0), idx_dtype)
    return coords, values(rng, coords.shape[1], dtype, spread), (len(lengths), ncols)


def values(rng, n, dtype, spread=3.0):
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return rng.random(n) < 0.5
    if dtype.kind in "iu":
        return rng.integers(-6, 7, n).astype(dtype)
    return (rng.standard_normal(n) * spread).astype(dtype)


def random_array(seed, shape, nnz, dtype=np.float32, idx_dtype=np.int64, spread=3.0):
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    lin = np.sort(rng.choice(size, min(nnz, size), replace=False)) if size else np.zeros(0, np.int64)
    coords = np.array(np.unravel_index(lin, shape)).astype(idx_dtype).reshape(len(shape), -1)
    return coords, values(rng, coords.shape[1], dtype, spread), tuple(shape)


def listed_lengths(chunk):
    """the group lengths of the bit-for-bit tests, for one chunk: every form's first and last length, pieces, runs of empty groups,
    the first and the last group empty"""
    return [0, 0, 1, 2, 7, 8, 9, 0, 15, 16, 17, 31, 32, 33, 0, 0, 0, 63, 64, 65, 127, 128, 129, chunk - 1, chunk, chunk + 1,
            2 * chunk + 3, 5 * chunk, 3, 0]

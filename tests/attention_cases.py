"""sparse_attention: the order contract of include/sparse_amd.h A15 restated in NumPy, the two derived bounds, and the seeded case
generators that tests/test_attention.py and tests/test_attention_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd
imports this.

The restatement is written from the contract, not from the kernels: the dot product by 64 accumulators in the array fmas of
tests/softmax_cases.py, `group_softmax` of that file on the restated scores, the output by piece-wise fma accumulation.  A
mask is its CSR triple (indptr, indices, values) in STORED order; q (M, D), k (N, D), v (N, Dv) are one head.

The bounds (eps = finfo.eps of the result type, twice the unit roundoff u: that factor is the margin)
  score   |t_i - s_i scale (q . k)| <= (ceil(D / 64) + 8) eps |s_i scale| sum_j |q_j k_j| + the smallest subnormal
          ceil(D / 64) fmas and 6 folds on every path to the result, 2 multiplies: ceil(D / 64) + 8 roundings of at most u each,
          every one of a partial sum or product bounded by |s_i scale| sum |q_j k_j| (first order; eps = 2 u pays the rest)
  output  with p_i the exact softmax of the ROUNDED t_i and b_i A14's bound (D_r + 2 U + n / 2 + 1) eps p_i + the smallest
          subnormal of tests/softmax_cases.py:
          |out_j - sum_i p_i v_ij| <= sum_i b_i |v_ij| + (n + 1) eps sum_i p_i |v_ij| + the smallest subnormal
          the probabilities' own errors weighted by |v|, then n fmas and at most n / chunk piece additions on sums bounded by
          sum p |v|"""
import math

import numpy as np

import softmax_cases as sc


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def dot64(qrow, krows):
    """w[i] = dot(qrow, krows[i]) by 64 accumulators: accumulator l takes fma(q[l + 64 j], k[l + 64 j], a_l) for j ascending,
    then a[l] = a[l] + a[l + h] for h = 32 .. 1"""
    dtype = qrow.dtype
    fma = sc._fma(dtype)
    n, D = krows.shape
    a = np.zeros((n, 64), dtype=dtype)
    with np.errstate(all="ignore"):
        for j0 in range(0, D, 64):
            w = min(64, D - j0)
            a[:, :w] = fma(np.broadcast_to(qrow[j0:j0 + w], (n, w)), krows[:, j0:j0 + w], a[:, :w])
        h = 32
        while h >= 1:
            a = a[:, :h] + a[:, h:2 * h]
            h //= 2
    assert a.dtype == dtype
    return a[:, 0]


def row_attention(svals, cols, qrow, k, v, chunk, scale=None):
    """one row of one head: (out[Dv], t[n], p[n]) in the type of `qrow`"""
    dtype = qrow.dtype
    fma = sc._fma(dtype)
    n, Dv = len(cols), v.shape[1]
    if n == 0:
        return np.zeros(Dv, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    with np.errstate(all="ignore"):
        t = svals.astype(dtype) * dot64(qrow, k[cols])
        if scale is not None:
            t = dtype.type(scale) * t
        p = sc.group_softmax(t, chunk)
        out = None
        for b in range(0, n, chunk):
            acc = np.zeros(Dv, dtype)
            for i in range(b, min(b + chunk, n)):
                acc = fma(np.broadcast_to(p[i], (Dv,)), v[cols[i]], acc).astype(dtype, copy=False)
            out = acc if out is None else out + acc
    assert out.dtype == dtype and t.dtype == dtype
    return out, t, p


def attention_restated(indptr, indices, svals, q, k, v, chunk, scale=None):
    """one head: (out (M, Dv), t (nnz), p (nnz)); the mask values are converted to the type of q first"""
    dtype = q.dtype
    assert dtype in (np.float32, np.float64) and k.dtype == dtype and v.dtype == dtype
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    svals = np.asarray(svals).astype(dtype)
    M = len(indptr) - 1
    out = np.zeros((M, v.shape[1]), dtype)
    t, p = np.zeros(len(indices), dtype), np.zeros(len(indices), dtype)
    for r in range(M):
        b, e = indptr[r], indptr[r + 1]
        out[r], t[b:e], p[b:e] = row_attention(svals[b:e], indices[b:e], q[r], k, v, chunk, scale)
    return out, t, p


def attention_heads(indptr, indices, svals, q, k, v, chunk, scale=None):
    """any leading head axes: the restated output of every head, stacked in the shape of the leading axes"""
    lead = q.shape[:-2]
    q3, k3, v3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v))
    outs = [attention_restated(indptr, indices, svals, q3[h], k3[h], v3[h], chunk, scale)[0] for h in range(q3.shape[0])]
    return np.stack(outs).reshape(lead + outs[0].shape) if outs else np.zeros(lead + (len(indptr) - 1, v.shape[-1]), q.dtype)


# ---- exact values and the bounds ----------------------------------------------------------------------------------------------------
LD = np.longdouble


def _rows(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def score_exact_and_bound(indptr, indices, svals, q, k, scale=None):
    """(want, bound) per stored element in longdouble: want = s_i scale (q . k) with the scale rounded to the result type"""
    dtype = q.dtype
    fi = np.finfo(dtype)
    rows, cols = _rows(indptr), np.asarray(indices, dtype=np.int64)
    prod = q.astype(LD)[rows] * k.astype(LD)[cols]
    f = np.asarray(svals).astype(dtype).astype(LD) * (LD(1) if scale is None else LD(dtype.type(scale)))
    want = f * prod.sum(axis=1)
    bound = (math.ceil(q.shape[1] / 64) + 8) * LD(fi.eps) * np.abs(f) * np.abs(prod).sum(axis=1) + LD(fi.smallest_subnormal)
    return want, bound


def output_exact_and_bound(indptr, indices, t, v):
    """(want, bound, spv), each (M, Dv) in longdouble, from the ROUNDED scores `t`: want = sum_i p_i v_ij with p the exact
    softmax of t over each row, spv = sum_i p_i |v_ij|.  Rows whose scores hold a NaN or an infinite maximum are NaN."""
    dtype = t.dtype
    fi = np.finfo(dtype)
    indptr = np.asarray(indptr, dtype=np.int64)
    rows, cols = _rows(indptr), np.asarray(indices, dtype=np.int64)
    p, b = sc.exact_and_bound(np.stack([rows, cols]), t, (len(indptr) - 1, v.shape[0]), 1)
    M, Dv = len(indptr) - 1, v.shape[1]
    want, bound, spv = (np.zeros((M, Dv), LD) for _ in range(3))
    vl = v.astype(LD)
    for r in range(M):
        s, e = indptr[r], indptr[r + 1]
        if s == e:
            continue
        vr = vl[cols[s:e]]
        want[r] = (p[s:e, None] * vr).sum(axis=0)
        spv[r] = (p[s:e, None] * np.abs(vr)).sum(axis=0)
        bound[r] = (b[s:e, None] * np.abs(vr)).sum(axis=0) + (e - s + 1) * LD(fi.eps) * spv[r] + LD(fi.smallest_subnormal)
    return want, bound, spv


def share(got, want, bound):
    """the largest |got - want| / bound over the entries that have a bound"""
    ok = ~np.isnan(bound) & (bound > 0)
    if not ok.any():
        return 0.0
    return float((np.abs(np.asarray(got)[ok].astype(LD) - want[ok]) / bound[ok]).max())


def other_form_bound(indptr, indices, svals, q, k, v, t, scale=None):
    """(want, bound) for a result computed another way from the same inputs - a dense float attention, the three-call
    expression - against the restated (or fused) output: the output bound, plus what scores that are each within the score
    bound of the exact score, so at most 2 sb apart, do to the exact result - every p_i changes by a factor within
    exp(+-2 * 2 sb_max) of itself, sb_max the row's largest score bound - so (exp(4 sb_max) - 1) sum_i p_i |v_ij|"""
    want, ob, spv = output_exact_and_bound(indptr, indices, t, v)
    _, sb = score_exact_and_bound(indptr, indices, svals, q, k, scale)
    indptr = np.asarray(indptr, dtype=np.int64)
    prop = np.zeros_like(ob)
    for r in range(len(indptr) - 1):
        s, e = indptr[r], indptr[r + 1]
        if e > s:
            prop[r] = np.expm1(4 * sb[s:e].max()) * spv[r]
    return want, ob + prop


# ---- seeded generators --------------------------------------------------------------------------------------------------------------
def csr_mask(seed, lengths, dtype=np.float32, idx_dtype=np.int64, ncols=None):
    """(indptr, indices, values, shape) of a mask whose row i holds lengths[i] elements at random ascending columns; the values
    are non-zero (floats: magnitude in [0.5, 1.5] with a random sign; integers: non-zero in -3 .. 3; booleans: True)"""
    rng = np.random.default_rng(seed)
    ncols = ncols or max(max(lengths, default=0), 1) + 3
    cols = [np.sort(rng.choice(ncols, n, replace=False)) for n in lengths]
    indices = (np.concatenate(cols) if lengths else np.zeros(0)).astype(idx_dtype)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(idx_dtype)
    nnz = len(indices)
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        vals = np.ones(nnz, dtype=bool)
    elif dtype.kind in "iu":
        vals = (rng.integers(1, 4, nnz) * rng.choice([-1, 1], nnz)).astype(dtype)
    else:
        vals = (rng.uniform(0.5, 1.5, nnz) * rng.choice([-1, 1], nnz)).astype(dtype)
    return indptr, indices, vals, (len(lengths), ncols)


def coords_of(indptr, indices):
    return np.stack([_rows(indptr), np.asarray(indices, dtype=np.int64)])


def operands(seed, shape, D, Dv, dtype=np.float32, lead=(), spread=1.0):
    """q (lead + (M, D)) of `spread` standard deviations, k (lead + (N, D)) and v (lead + (N, Dv)) of one"""
    rng = np.random.default_rng(seed)
    M, N = shape
    q = (rng.standard_normal(lead + (M, D)) * spread).astype(dtype)
    k = rng.standard_normal(lead + (N, D)).astype(dtype)
    v = rng.standard_normal(lead + (N, Dv)).astype(dtype)
    return q, k, v


SHORT_LENGTHS = [0, 1, 2, 7, 8, 9, 33, 64, 65, 100]

"""sparse_attention_grad: the order contract of include/sparse_amd.h A16 restated in NumPy, the exact gradient in longdouble, the
derived first-order bounds, and the seeded case generators that tests/test_attention_grad.py and
tests/test_attention_grad_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd imports this.

The restatement is written from the contract, not from the kernels.  It reuses `dot64` and `row_attention` of
tests/attention_cases.py (the forward's steps 1 to 3) and `piece_sum` / `_fma` of tests/softmax_cases.py (the float64 fma with
its underflow case made exact, `_fma64_exact`).  A mask is its CSR triple (indptr, indices, values) in STORED order; q (M, D),
k (N, D), v (N, Dv), g (M, Dv) are one head.

The bounds.  eps = finfo.eps of the result type = twice the unit roundoff u; every rounding is counted as eps instead of u, and
that factor of two is the only margin (it pays the second-order terms).  Exact values (longdouble, from the inputs):
    t_i = s_i c (q_r . k_ci),  p = softmax of the row's t,  e_i = g_r . v_ci,  delta = sum_i p_i e_i,
    y_i = s_i c p_i (e_i - delta),  dq_r = sum_i y_i k_ci,  dk_c = sum_{i in c} y_i q_ri,  dv_c = sum_{i in c} p_i g_ri
  pb_i  probability: A14's bound b_i of `softmax_cases.exact_and_bound` holds against the exact softmax of the ROUNDED scores;
        the rounded scores are within sb (the score bound of `attention_cases.score_exact_and_bound`) of the exact ones, which
        changes every p_i by a factor within exp(+-2 sb_max), sb_max the row's largest: pb_i = b_i + expm1(2 sb_max) p_i
  eb_i  e by the 64-accumulator dot product: ceil(Dv / 64) fmas and 6 folds on every path, each rounding a partial sum bounded
        by A_i = sum_j |g_j v_ij|: eb_i = (ceil(Dv / 64) + 6) eps A_i
  ub_i  u_i = p_i e_i, one multiply: ub_i = pb_i |e_i| + p_i eb_i + eps p_i |e_i|
  db    delta: the terms' own errors, and L roundings on the longest path of the sum - ceil(min(n, chunk) / 64) additions in
        an accumulator, 6 folds, ceil(n / chunk) piece additions -, each of a partial sum bounded by sum p_i |e_i|:
        db = sum_i ub_i + L eps sum_i p_i |e_i|
  zb_i  z_i = p_i (e_i - delta), a subtraction and a multiply: zb_i = pb_i |e_i - delta| + p_i (eb_i + db) + 2 eps p_i |e_i - delta|
  yb_i  y_i = c s_i z_i, one multiply or two: yb_i = |c s_i| zb_i + (1 | 2) eps |y_i|
  dq    n fmas and at most n / chunk piece additions on sums bounded by sum |y_i k_ij| (the forward's count, n + 1):
        dqb_j = sum_i yb_i |k_ij| + (n + 1) eps sum_i |y_i k_ij| + the smallest subnormal
  dk    the same over a column of m elements: dkb_j = sum yb_i |q_rij| + (m + 1) eps sum |y_i q_rij| + the smallest subnormal
  dv    dvb_j = sum pb_i |g_rij| + (m + 1) eps sum p_i |g_rij| + the smallest subnormal
Rows whose scores hold a NaN or an infinite maximum have no bound (NaN): the tests check them as facts.

`other_form_factor`: a result computed another way from the same inputs - a dense float attention differentiated by torch -
performs the same operations in another order (its additional terms are exact zeros: exp(-inf) = 0), so it satisfies the same
path-length bounds; two such results are at most 2 bounds apart, plus the comparison value's own final rounding."""
import math

import numpy as np

import attention_cases as ac
import softmax_cases as sc

LD = np.longdouble
OTHER_FORM_FACTOR = 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _fma64_exact(a, b, c):
    """`softmax_cases.fma64v`, which is exact unless an intermediate underflows, with the elements where one can - a product
    below 2^-900, whose low half (Dekker's error term, 53 bits further down) need not be a float64 - computed in rational
    arithmetic and rounded once.  A gradient meets such products: y_i of a row whose probabilities are 1 and 1e-300"""
    from fractions import Fraction

    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c)))
    out = np.array(sc.fma64v(a, b, c), dtype=np.float64)
    with np.errstate(all="ignore"):
        risky = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & (a != 0) & (b != 0) & (np.abs(a * b) < 2.0 ** -900)
    for i in zip(*np.nonzero(risky)):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def _fma(dtype):
    return sc.fma32v if dtype == np.float32 else _fma64_exact


def _pieces_fma(vals, rows, width, chunk, dtype):
    """sum_i vals[i] * rows[i] by the piece rule: a piece starts at +0.0 and takes acc = fma(vals[i], rows[i], acc) for i
    ascending; the piece sums are added in piece order, the first piece's sum being the start.  No element: +0.0"""
    fma = _fma(dtype)
    out = None
    with np.errstate(all="ignore"):
        for b in range(0, len(vals), chunk):
            acc = np.zeros(width, dtype)
            for i in range(b, min(b + chunk, len(vals))):
                acc = fma(np.broadcast_to(vals[i], (width,)), rows[i], acc).astype(dtype, copy=False)
            out = acc if out is None else out + acc
    return np.zeros(width, dtype) if out is None else out


def row_grad(svals, cols, qrow, grow, k, v, chunk, scale=None):
    """the row pass for one row of one head: (dq[D], p[n], y[n]) in the type of `qrow`"""
    dtype = qrow.dtype
    n, D = len(cols), k.shape[1]
    if n == 0:
        return np.zeros(D, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    with np.errstate(all="ignore"):
        _, t, p = ac.row_attention(svals, cols, qrow, k, v[:, :0], chunk, scale)            # steps 1 to 3 of A15
        e = ac.dot64(grow, v[cols])
        u = p * e
        delta = None
        for b in range(0, n, chunk):
            ps = sc.piece_sum(u[b:b + chunk])
            delta = ps if delta is None else delta + ps
        z = p * (e - delta)
        y = svals.astype(dtype) * z
        if scale is not None:
            y = dtype.type(scale) * y
    assert p.dtype == dtype and y.dtype == dtype and e.dtype == dtype
    return _pieces_fma(y, k[cols], D, chunk, dtype), p, y


def column_order(indptr, indices):
    """(colperm, colrows, columns): the stored positions grouped by column, ascending within a column, with their row and column ids"""
    indices = np.asarray(indices, dtype=np.int64)
    perm = np.argsort(indices, kind="stable")
    return perm, ac._rows(indptr)[perm], indices[perm]


def grad_restated(indptr, indices, svals, q, k, v, g, chunk, scale=None):
    """one head: (dq (M, D), dk (N, D), dv (N, Dv), p (nnz), y (nnz)); the mask values are converted to the type of q first"""
    dtype = q.dtype
    assert dtype in (np.float32, np.float64) and k.dtype == dtype and v.dtype == dtype and g.dtype == dtype
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    svals = np.asarray(svals).astype(dtype)
    M, N, D, Dv = len(indptr) - 1, k.shape[0], q.shape[1], v.shape[1]
    dq = np.zeros((M, D), dtype)
    p, y = np.zeros(len(indices), dtype), np.zeros(len(indices), dtype)
    for r in range(M):
        b, e = indptr[r], indptr[r + 1]
        dq[r], p[b:e], y[b:e] = row_grad(svals[b:e], indices[b:e], q[r], g[r], k, v, chunk, scale)
    dk, dv = np.zeros((N, D), dtype), np.zeros((N, Dv), dtype)
    perm, rows, cols = column_order(indptr, indices)
    cuts = np.searchsorted(cols, np.arange(N + 1))
    for c in range(N):
        pos, rr = perm[cuts[c]:cuts[c + 1]], rows[cuts[c]:cuts[c + 1]]
        if len(pos):
            dv[c] = _pieces_fma(p[pos], g[rr], Dv, chunk, dtype)
            dk[c] = _pieces_fma(y[pos], q[rr], D, chunk, dtype)
    return dq, dk, dv, p, y


def grad_heads(indptr, indices, svals, q, k, v, g, chunk, scale=None):
    """any leading head axes: the restated (dq, dk, dv) of every head, stacked in the shape of the leading axes"""
    lead = q.shape[:-2]
    q3, k3, v3, g3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v, g))
    outs = [grad_restated(indptr, indices, svals, q3[h], k3[h], v3[h], g3[h], chunk, scale)[:3] for h in range(q3.shape[0])]
    return tuple(np.stack([o[i] for o in outs]).reshape(lead + outs[0][i].shape) for i in range(3))


# ---- the exact gradient and the bounds ---------------------------------------------------------------------------------------------
def _sum_depth(n, chunk):
    return math.ceil(min(n, chunk) / 64) + 6 + math.ceil(n / chunk)


def exact_and_bounds(indptr, indices, svals, q, k, v, g, chunk, scale=None, t=None):
    """((dq, dk, dv), (dqb, dkb, dvb)) in longdouble: the dense formula over the stored positions and the bounds of the module
    docstring.  `t`: the restated (rounded) scores, for A14's bound; computed when not given"""
    dtype = q.dtype
    fi = np.finfo(dtype)
    eps, tiny = LD(fi.eps), LD(fi.smallest_subnormal)
    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    rows = ac._rows(indptr)
    M, N, D, Dv = len(indptr) - 1, k.shape[0], q.shape[1], v.shape[1]
    if t is None:
        t = ac.attention_restated(indptr, indices, svals, q, k, v[:, :0], chunk, scale)[1]
    ql, kl, vl, gl = (x.astype(LD) for x in (q, k, v, g))
    f = np.asarray(svals).astype(dtype).astype(LD) * (LD(1) if scale is None else LD(dtype.type(scale)))
    tx, sb = ac.score_exact_and_bound(indptr, indices, svals, q, k, scale)
    _, b14 = sc.exact_and_bound(np.stack([rows, cols]), t, (M, N), 1)
    nr = 1 if scale is None else 2
    nnz = len(cols)
    p, pb, y, yb = (np.full(nnz, np.nan, LD) for _ in range(4))
    dq, dqb = np.zeros((M, D), LD), np.zeros((M, D), LD)
    with np.errstate(all="ignore"):
        for r in range(M):
            s, e_ = indptr[r], indptr[r + 1]
            n = e_ - s
            if n == 0:
                dqb[r] = tiny
                continue
            tr = tx[s:e_]
            if not np.isfinite(tr.max()) or np.isnan(b14[s:e_]).any():
                dq[r], dqb[r] = np.nan, np.nan
                continue
            ex = np.exp(tr - tr.max())
            pr = ex / ex.sum()
            pbr = b14[s:e_] + np.expm1(2 * sb[s:e_].max()) * pr
            vr = vl[cols[s:e_]]
            e = (gl[r] * vr).sum(axis=1)
            A = np.abs(gl[r] * vr).sum(axis=1)
            eb = (math.ceil(Dv / 64) + 6) * eps * A
            ub = pbr * np.abs(e) + pr * eb + eps * pr * np.abs(e)
            delta = (pr * e).sum()
            db = ub.sum() + _sum_depth(n, chunk) * eps * (pr * np.abs(e)).sum()
            z = pr * (e - delta)
            zb = pbr * np.abs(e - delta) + pr * (eb + db) + 2 * eps * np.abs(z)
            yr = f[s:e_] * z
            ybr = np.abs(f[s:e_]) * zb + nr * eps * np.abs(yr)
            p[s:e_], pb[s:e_], y[s:e_], yb[s:e_] = pr, pbr, yr, ybr
            kr = kl[cols[s:e_]]
            dq[r] = (yr[:, None] * kr).sum(axis=0)
            dqb[r] = (ybr[:, None] * np.abs(kr)).sum(axis=0) + (n + 1) * eps * np.abs(yr[:, None] * kr).sum(axis=0) + tiny
        dk, dkb, dv, dvb = np.zeros((N, D), LD), np.full((N, D), tiny, LD), np.zeros((N, Dv), LD), np.full((N, Dv), tiny, LD)
        perm, prow, pcol = column_order(indptr, indices)
        cuts = np.searchsorted(pcol, np.arange(N + 1))
        for c in range(N):
            pos, rr = perm[cuts[c]:cuts[c + 1]], prow[cuts[c]:cuts[c + 1]]
            m = len(pos)
            if m == 0:
                continue
            dv[c] = (p[pos, None] * gl[rr]).sum(axis=0)
            dvb[c] = (pb[pos, None] * np.abs(gl[rr])).sum(axis=0) + (m + 1) * eps * (p[pos, None] * np.abs(gl[rr])).sum(axis=0) + tiny
            dk[c] = (y[pos, None] * ql[rr]).sum(axis=0)
            dkb[c] = (yb[pos, None] * np.abs(ql[rr])).sum(axis=0) + (m + 1) * eps * np.abs(y[pos, None] * ql[rr]).sum(axis=0) + tiny
    return (dq, dk, dv), (dqb, dkb, dvb)


def shares(got, want, bounds):
    """the largest |got - want| / bound of dq, dk and dv over the entries that have a bound"""
    return tuple(ac.share(a, w, b) for a, w, b in zip(got, want, bounds))


# ---- seeded generators --------------------------------------------------------------------------------------------------------------
def grad_operand(seed, shape, Dv, dtype=np.float32, lead=()):
    """g (lead + (M, Dv)) of one standard deviation"""
    return np.random.default_rng(seed).standard_normal(lead + (shape[0], Dv)).astype(dtype)


def transposed_mask(seed, lengths, dtype=np.float32):
    """(indptr, indices, values, shape) whose COLUMN c holds lengths[c] elements: the transpose of `attention_cases.csr_mask`,
    re-sorted to CSR on the host (a stable sort by row, so the columns ascend within a row)"""
    cptr, cidx, vals, (ncol, nrow) = ac.csr_mask(seed, lengths, dtype)
    cols = ac._rows(cptr)
    rows = np.asarray(cidx, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=nrow)))).astype(np.int64)
    return indptr, cols[order].astype(np.int64), vals[order], (nrow, ncol)

"""sparse_attention with an additive bias: the one step the bias adds to the order contracts of include/sparse_amd.h A15 and A16,
restated in NumPy, the exact value and bound of a biased score, and the seeded bias generators that
tests/test_attention_bias.py and tests/test_attention_bias_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd imports this.

The restatement is written from the contract, not from the kernels, on the pieces of the unbiased restatements:
`attention_cases.dot64`, `softmax_cases.group_softmax` and `_fma`, `attention_grad_cases._pieces_fma` and `column_order`.  A bias
is one value per stored element in STORED (CSR) order, `(nnz,)` for one head.

    t_i = s_i * w_i;  t_i = scale * t_i (with a scale);  t_i = t_i + b_i          one add, rounded once, after the scale
    dbias_i = z_i = p_i * (e_i - delta)                                          A16's z_i, as it stands

The bound of a biased score.  With T the exact score s_i c (q . k), t the rounded one, sb A15's score bound
(`attention_cases.score_exact_and_bound`): the add is rounded once, so |fl(t + b) - (T + b)| <= |t - T| + (eps / 2) |t + b|
<= sb + eps (|T + b| + sb); the smallest subnormal is added as there.  Where the bias is infinite the score is that infinity and
has no bound (NaN): the tests check it as a fact."""
import numpy as np

import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc

LD = np.longdouble


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def row_attention_bias(svals, cols, qrow, k, v, chunk, scale=None, bias=None):
    """one row of one head: (out[Dv], t[n], p[n]) in the type of `qrow`; `bias` None is `attention_cases.row_attention`"""
    if bias is None:
        return ac.row_attention(svals, cols, qrow, k, v, chunk, scale)
    dtype = qrow.dtype
    fma = sc._fma(dtype)
    n, Dv = len(cols), v.shape[1]
    if n == 0:
        return np.zeros(Dv, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    assert bias.dtype == dtype and bias.shape == (n,)
    with np.errstate(all="ignore"):
        t = svals.astype(dtype) * ac.dot64(qrow, k[cols])
        if scale is not None:
            t = dtype.type(scale) * t
        t = t + bias
        p = sc.group_softmax(t, chunk)
        out = None
        for b in range(0, n, chunk):
            acc = np.zeros(Dv, dtype)
            for i in range(b, min(b + chunk, n)):
                acc = fma(np.broadcast_to(p[i], (Dv,)), v[cols[i]], acc).astype(dtype, copy=False)
            out = acc if out is None else out + acc
    assert out.dtype == dtype and t.dtype == dtype
    return out, t, p


def attention_bias_restated(indptr, indices, svals, q, k, v, chunk, scale=None, bias=None):
    """one head: (out (M, Dv), t (nnz), p (nnz)); `bias` (nnz,) in stored order, of the type of q"""
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
        out[r], t[b:e], p[b:e] = row_attention_bias(svals[b:e], indices[b:e], q[r], k, v, chunk, scale, None if bias is None else bias[b:e])
    return out, t, p


def _bias3(bias, nheads, nnz):
    """the bias of every head: (nheads, nnz) from (nnz,) - shared - or lead + (nnz,)"""
    return np.broadcast_to(bias, (nheads, nnz)) if bias.ndim == 1 else bias.reshape(nheads, nnz)


def attention_bias_heads(indptr, indices, svals, q, k, v, chunk, scale=None, bias=None):
    """any leading head axes: the restated output of every head; `bias` (nnz,) or lead + (nnz,)"""
    lead = q.shape[:-2]
    q3, k3, v3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v))
    b3 = _bias3(bias, q3.shape[0], len(indices))
    outs = [attention_bias_restated(indptr, indices, svals, q3[h], k3[h], v3[h], chunk, scale, b3[h])[0] for h in range(q3.shape[0])]
    return np.stack(outs).reshape(lead + outs[0].shape)


def row_grad_bias(svals, cols, qrow, grow, k, v, chunk, scale=None, bias=None):
    """the row pass for one row of one head: (dq[D], p[n], y[n], z[n]) in the type of `qrow`"""
    dtype = qrow.dtype
    n, D = len(cols), k.shape[1]
    if n == 0:
        return np.zeros(D, dtype), np.zeros(0, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    with np.errstate(all="ignore"):
        _, t, p = row_attention_bias(svals, cols, qrow, k, v[:, :0], chunk, scale, bias)      # steps 1 to 3 of A15, with the bias
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
    assert p.dtype == dtype and y.dtype == dtype and z.dtype == dtype
    return gc._pieces_fma(y, k[cols], D, chunk, dtype), p, y, z


def grad_bias_restated(indptr, indices, svals, q, k, v, g, chunk, scale=None, bias=None):
    """one head: (dq (M, D), dk (N, D), dv (N, Dv), dbias (nnz)); `bias` (nnz,) in stored order or None (dbias is z all the same)"""
    dtype = q.dtype
    assert dtype in (np.float32, np.float64) and k.dtype == dtype and v.dtype == dtype and g.dtype == dtype
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    svals = np.asarray(svals).astype(dtype)
    M, N, D, Dv = len(indptr) - 1, k.shape[0], q.shape[1], v.shape[1]
    dq = np.zeros((M, D), dtype)
    p, y, z = (np.zeros(len(indices), dtype) for _ in range(3))
    for r in range(M):
        b, e = indptr[r], indptr[r + 1]
        dq[r], p[b:e], y[b:e], z[b:e] = row_grad_bias(svals[b:e], indices[b:e], q[r], g[r], k, v, chunk, scale,
                                                      None if bias is None else bias[b:e])
    dk, dv = np.zeros((N, D), dtype), np.zeros((N, Dv), dtype)
    perm, rows, cols = gc.column_order(indptr, indices)
    cuts = np.searchsorted(cols, np.arange(N + 1))
    for c in range(N):
        pos, rr = perm[cuts[c]:cuts[c + 1]], rows[cuts[c]:cuts[c + 1]]
        if len(pos):
            dv[c] = gc._pieces_fma(p[pos], g[rr], Dv, chunk, dtype)
            dk[c] = gc._pieces_fma(y[pos], q[rr], D, chunk, dtype)
    return dq, dk, dv, z


def grad_bias_heads(indptr, indices, svals, q, k, v, g, chunk, scale=None, bias=None):
    """any leading head axes: the restated (dq, dk, dv, dbias) of every head; dbias is lead + (nnz,), per head"""
    lead = q.shape[:-2]
    q3, k3, v3, g3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v, g))
    b3 = _bias3(bias, q3.shape[0], len(indices))
    outs = [grad_bias_restated(indptr, indices, svals, q3[h], k3[h], v3[h], g3[h], chunk, scale, b3[h]) for h in range(q3.shape[0])]
    return tuple(np.stack([o[i] for o in outs]).reshape(lead + outs[0][i].shape) for i in range(4))


# ---- exact values and the bounds ----------------------------------------------------------------------------------------------------
def biased_score_exact_and_bound(indptr, indices, svals, q, k, bias, scale=None):
    """(want, bound) per stored element in longdouble: want = s_i scale (q . k) + b_i; the bound of the module docstring, NaN
    where the bias is not finite"""
    fi = np.finfo(q.dtype)
    T, sb = ac.score_exact_and_bound(indptr, indices, svals, q, k, scale)
    with np.errstate(all="ignore"):
        want = T + bias.astype(LD)
        bound = sb + LD(fi.eps) * (np.abs(want) + sb) + LD(fi.smallest_subnormal)
    bound[~np.isfinite(bias)] = np.nan
    return want, bound


def other_form_bound(indptr, indices, svals, q, k, v, t, bias, scale=None):
    """`attention_cases.other_form_bound` with the biased score bound in the place of the score bound: (want, bound) for a
    result computed another way from the same inputs against the restated (or fused) output whose rounded scores are `t`"""
    want, ob, spv = ac.output_exact_and_bound(indptr, indices, t, v)
    _, sb = biased_score_exact_and_bound(indptr, indices, svals, q, k, bias, scale)
    sb = np.where(np.isnan(sb), 0, sb)                              # (an element masked by -inf has the probability 0 in both)
    indptr = np.asarray(indptr, dtype=np.int64)
    prop = np.zeros_like(ob)
    for r in range(len(indptr) - 1):
        s, e = indptr[r], indptr[r + 1]
        if e > s:
            prop[r] = np.expm1(4 * sb[s:e].max()) * spv[r]
    return want, ob + prop


def dense_attention64(indptr, indices, svals, q, k, v, bias, scale=None):
    """softmax(scale * s * (q @ k.T) + B, -inf at the unstored positions) @ v in float64; rows without a stored element are 0"""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows, cols = ac._rows(indptr), np.asarray(indices, dtype=np.int64)
    M, N = len(indptr) - 1, k.shape[0]
    c = 1.0 if scale is None else float(q.dtype.type(scale))          # the scale enters rounded to the result type, as in A15
    sv = np.asarray(svals).astype(q.dtype).astype(np.float64)
    q, k, v = (x.astype(np.float64) for x in (q, k, v))
    scores = np.full((M, N), -np.inf)
    with np.errstate(all="ignore"):
        scores[rows, cols] = c * (sv * (q @ k.T)[rows, cols]) + bias.astype(np.float64)
        m = scores.max(axis=1, keepdims=True)
        e = np.exp(scores - np.where(np.isfinite(m), m, 0))
        p = np.nan_to_num(e / e.sum(axis=1, keepdims=True))
    return p @ v


# ---- seeded generators --------------------------------------------------------------------------------------------------------------
def bias_of(seed, nnz, dtype=np.float32, lead=None, spread=1.5, neg_inf=0.0):
    """a bias of `spread` standard deviations: (nnz,) for lead None (shared), else lead + (nnz,); a share `neg_inf` of the entries
    is -inf"""
    rng = np.random.default_rng(seed)
    shape = (nnz,) if lead is None else tuple(lead) + (nnz,)
    b = (rng.standard_normal(shape) * spread).astype(dtype)
    if neg_inf:
        b[rng.random(shape) < neg_inf] = -np.inf
    return b

"""Attention dropout: the keep decision of csrc/attention_dropout.h and the steps dropout adds to the order contracts of
include/sparse_amd.h A15 and A16, restated in NumPy, the exact values and derived bounds, shared by
tests/test_attention_dropout.py and tests/test_attention_dropout_gpu.py.  TEST INFRASTRUCTURE: nothing in sparse_amd imports this.

The restatement is written from the contract, not from the kernels, on the pieces of the restatements without dropout:
`attention_bias_cases.row_attention_bias` (steps 1 to 3 of A15 with the bias step), `attention_cases.dot64`,
`softmax_cases.piece_sum` and `_fma`, `attention_grad_cases._pieces_fma` and `column_order`.

    keep_i = philox4x32_10(key (seed lo, seed hi), counter (pos lo, pos hi, head lo, head hi))[0] >= thr
    thr    = floor(rate * 2^32) (the multiply exact in double);  c = (T)(1.0 / (1.0 - rate))
    pd_i   = keep_i ? p_i * c : +0.0            out takes pd_i in the place of p_i
    ed_i   = keep_i ? e_i * c : +0.0            u_i = p_i * ed_i, delta over these, z_i = p_i * (ed_i - delta); dv takes pd_i

The bounds (eps = finfo.eps = twice the unit roundoff, the factor that pays the second-order terms, as in
tests/attention_cases.py and tests/attention_grad_cases.py).  c enters EXACTLY, as the rounded value the kernel multiplies by.
  pd_i  one more rounding on p_i c: with b_i the bound of the computed p_i, |pd_i - c p_i| <= c b_i + eps c p_i (kept), 0 (dropped)
  ed_i  likewise on e_i: edb_i = c eb_i + eps c |e_i| (kept), 0 (dropped)
and every later bound of the two files follows with pd_i / ed_i and these in the place of p_i / e_i and theirs."""
import math

import numpy as np

import attention_bias_cases as bc
import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc

LD = np.longdouble
M0, M1 = 0xD2511F53, 0xCD9E8D57                                            # Random123's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                                            # ... and key increments
_LOW = np.uint64(0xFFFFFFFF)


# ---- the generator --------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """the four output words (uint32 arrays) of Philox4x32-10; `counter` four and `key` two arrays (or scalars) of 32-bit
    words that broadcast.  The products are uint64"""
    c = [np.asarray(x, dtype=np.uint64) & _LOW for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _LOW for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _LOW]
        k = [(k[0] + np.uint64(W0)) & _LOW, (k[1] + np.uint64(W1)) & _LOW]
    return [x.astype(np.uint32) for x in c]


def threshold(rate):
    """thr = floor(rate * 2^32): the product of a double by a power of two is exact"""
    rate = float(rate)
    assert 0.0 <= rate < 1.0
    return int(math.floor(rate * 4294967296.0))


def keep_restated(nnz, H, rate, seed, pos0=0, head0=0):
    """bool (H, nnz): position pos0 + p of head head0 + h is kept"""
    seed, pos0, head0 = int(seed), int(pos0), int(head0)
    assert 0 <= seed < 1 << 64
    pos = (np.arange(nnz, dtype=np.uint64) + np.uint64(pos0))[None, :]
    head = (np.arange(H, dtype=np.uint64) + np.uint64(head0))[:, None]
    x = philox4x32_10((pos & _LOW, pos >> np.uint64(32), head & _LOW, head >> np.uint64(32)), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return np.broadcast_to(x, (H, nnz)) >= np.uint32(threshold(rate))


def c_of(rate, dtype):
    """c = (T)(1.0 / (1.0 - rate)): the division in double, rounded once"""
    return np.dtype(dtype).type(1.0 / (1.0 - float(rate)))


def _dropped(x, keep, c):
    """keep ? x * c : +0.0, one multiply"""
    with np.errstate(all="ignore"):
        return np.where(keep, x * c, x.dtype.type(0)).astype(x.dtype, copy=False)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def row_attention_dropout(svals, cols, qrow, k, v, chunk, scale, bias, keep, c):
    """one row of one head: (out[Dv], t[n], p[n], pd[n]) in the type of `qrow`; `keep` bool[n], `c` of that type"""
    dtype = qrow.dtype
    fma = sc._fma(dtype)
    n, Dv = len(cols), v.shape[1]
    if n == 0:
        return np.zeros(Dv, dtype), np.zeros(0, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    _, t, p = bc.row_attention_bias(svals, cols, qrow, k, v[:, :0], chunk, scale, bias)
    pd = _dropped(p, keep, c)
    out = None
    with np.errstate(all="ignore"):
        for b in range(0, n, chunk):
            acc = np.zeros(Dv, dtype)
            for i in range(b, min(b + chunk, n)):
                acc = fma(np.broadcast_to(pd[i], (Dv,)), v[cols[i]], acc).astype(dtype, copy=False)
            out = acc if out is None else out + acc
    assert out.dtype == dtype and pd.dtype == dtype
    return out, t, p, pd


def _prep(indptr, indices, svals, dtype):
    return np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(svals).astype(dtype)


def attention_dropout_restated(indptr, indices, svals, q, k, v, chunk, scale=None, bias=None, rate=0.0, seed=0, head=0):
    """one head, number `head` of the call: (out (M, Dv), t, p, pd (nnz each), keep bool (nnz))"""
    dtype = q.dtype
    assert dtype in (np.float32, np.float64) and k.dtype == dtype and v.dtype == dtype
    indptr, indices, svals = _prep(indptr, indices, svals, dtype)
    M, nnz = len(indptr) - 1, len(indices)
    keep, c = keep_restated(nnz, 1, rate, seed, 0, head)[0], c_of(rate, dtype)
    out = np.zeros((M, v.shape[1]), dtype)
    t, p, pd = (np.zeros(nnz, dtype) for _ in range(3))
    for r in range(M):
        b, e = indptr[r], indptr[r + 1]
        out[r], t[b:e], p[b:e], pd[b:e] = row_attention_dropout(svals[b:e], indices[b:e], q[r], k, v, chunk, scale,
                                                                None if bias is None else bias[b:e], keep[b:e], c)
    return out, t, p, pd, keep


def _bias3(bias, nheads, nnz):
    return [None] * nheads if bias is None else bc._bias3(bias, nheads, nnz)


def attention_dropout_heads(indptr, indices, svals, q, k, v, chunk, scale=None, bias=None, rate=0.0, seed=0, head0=0):
    """any leading head axes: the restated output of every head; the heads are numbered head0 .. in the flattened leading axes"""
    lead = q.shape[:-2]
    q3, k3, v3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v))
    b3 = _bias3(bias, q3.shape[0], len(indices))
    outs = [attention_dropout_restated(indptr, indices, svals, q3[h], k3[h], v3[h], chunk, scale, b3[h], rate, seed, head0 + h)[0]
            for h in range(q3.shape[0])]
    return np.stack(outs).reshape(lead + outs[0].shape)


def row_grad_dropout(svals, cols, qrow, grow, k, v, chunk, scale, bias, keep, c):
    """the row pass for one row of one head: (dq[D], pd[n], y[n], z[n]) in the type of `qrow`"""
    dtype = qrow.dtype
    n, D = len(cols), k.shape[1]
    if n == 0:
        return np.zeros(D, dtype), np.zeros(0, dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    with np.errstate(all="ignore"):
        _, t, p = bc.row_attention_bias(svals, cols, qrow, k, v[:, :0], chunk, scale, bias)
        pd = _dropped(p, keep, c)
        ed = _dropped(ac.dot64(grow, v[cols]), keep, c)
        u = p * ed
        delta = None
        for b in range(0, n, chunk):
            ps = sc.piece_sum(u[b:b + chunk])
            delta = ps if delta is None else delta + ps
        z = p * (ed - delta)
        y = svals.astype(dtype) * z
        if scale is not None:
            y = dtype.type(scale) * y
    assert pd.dtype == dtype and y.dtype == dtype and z.dtype == dtype
    return gc._pieces_fma(y, k[cols], D, chunk, dtype), pd, y, z


def grad_dropout_restated(indptr, indices, svals, q, k, v, g, chunk, scale=None, bias=None, rate=0.0, seed=0, head=0):
    """one head, number `head` of the call: (dq (M, D), dk (N, D), dv (N, Dv), dbias = z (nnz))"""
    dtype = q.dtype
    assert dtype in (np.float32, np.float64) and k.dtype == dtype and v.dtype == dtype and g.dtype == dtype
    indptr, indices, svals = _prep(indptr, indices, svals, dtype)
    M, N, D, Dv, nnz = len(indptr) - 1, k.shape[0], q.shape[1], v.shape[1], len(indices)
    keep, c = keep_restated(nnz, 1, rate, seed, 0, head)[0], c_of(rate, dtype)
    dq = np.zeros((M, D), dtype)
    pd, y, z = (np.zeros(nnz, dtype) for _ in range(3))
    for r in range(M):
        b, e = indptr[r], indptr[r + 1]
        dq[r], pd[b:e], y[b:e], z[b:e] = row_grad_dropout(svals[b:e], indices[b:e], q[r], g[r], k, v, chunk, scale,
                                                          None if bias is None else bias[b:e], keep[b:e], c)
    dk, dv = np.zeros((N, D), dtype), np.zeros((N, Dv), dtype)
    perm, rows, cols = gc.column_order(indptr, indices)
    cuts = np.searchsorted(cols, np.arange(N + 1))
    for col in range(N):
        pos, rr = perm[cuts[col]:cuts[col + 1]], rows[cuts[col]:cuts[col + 1]]
        if len(pos):
            dv[col] = gc._pieces_fma(pd[pos], g[rr], Dv, chunk, dtype)
            dk[col] = gc._pieces_fma(y[pos], q[rr], D, chunk, dtype)
    return dq, dk, dv, z


def grad_dropout_heads(indptr, indices, svals, q, k, v, g, chunk, scale=None, bias=None, rate=0.0, seed=0, head0=0):
    """any leading head axes: the restated (dq, dk, dv, dbias) of every head; dbias is lead + (nnz,), per head"""
    lead = q.shape[:-2]
    q3, k3, v3, g3 = (x.reshape((-1,) + x.shape[-2:]) for x in (q, k, v, g))
    b3 = _bias3(bias, q3.shape[0], len(indices))
    outs = [grad_dropout_restated(indptr, indices, svals, q3[h], k3[h], v3[h], g3[h], chunk, scale, b3[h], rate, seed, head0 + h)
            for h in range(q3.shape[0])]
    return tuple(np.stack([o[i] for o in outs]).reshape(lead + outs[0][i].shape) for i in range(4))


# ---- exact values and the bounds ----------------------------------------------------------------------------------------------------
def output_exact_and_bound(indptr, indices, t, v, keep, c):
    """`attention_cases.output_exact_and_bound` with dropout: (want, bound), each (M, Dv) in longdouble, from the ROUNDED scores
    `t`: want = sum_i keep_i c p_i v_ij with p the exact softmax of t; the bound is that function's with pd_i = keep_i c p_i in
    the place of p_i and c b_i + eps c p_i - the one extra rounding of p_i c - in the place of b_i"""
    dtype = t.dtype
    fi = np.finfo(dtype)
    indptr = np.asarray(indptr, dtype=np.int64)
    rows, cols = ac._rows(indptr), np.asarray(indices, dtype=np.int64)
    p, b = sc.exact_and_bound(np.stack([rows, cols]), t, (len(indptr) - 1, v.shape[0]), 1)
    cl = LD(c)
    pd = np.where(keep, cl * p, LD(0))
    bd = np.where(keep, cl * b + LD(fi.eps) * cl * p, LD(0))
    M, Dv = len(indptr) - 1, v.shape[1]
    want, bound = np.zeros((M, Dv), LD), np.zeros((M, Dv), LD)
    vl = v.astype(LD)
    for r in range(M):
        s, e = indptr[r], indptr[r + 1]
        if s == e:
            continue
        vr = vl[cols[s:e]]
        want[r] = (pd[s:e, None] * vr).sum(axis=0)
        spv = (pd[s:e, None] * np.abs(vr)).sum(axis=0)
        bound[r] = (bd[s:e, None] * np.abs(vr)).sum(axis=0) + (e - s + 1) * LD(fi.eps) * spv + LD(fi.smallest_subnormal)
    return want, bound


def grad_exact_and_bounds(indptr, indices, svals, q, k, v, g, chunk, keep, c, scale=None, t=None):
    """`attention_grad_cases.exact_and_bounds` with dropout (no bias): ((dq, dk, dv), (dqb, dkb, dvb)) in longdouble, with
    ed_i = keep_i c e_i and pd_i = keep_i c p_i and their bounds of the module docstring in the place of e_i and (for dv) p_i"""
    dtype = q.dtype
    fi = np.finfo(dtype)
    eps, tiny, cl = LD(fi.eps), LD(fi.smallest_subnormal), LD(c)
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
    pd, pdb, y, yb = (np.full(nnz, np.nan, LD) for _ in range(4))
    dq, dqb = np.zeros((M, D), LD), np.zeros((M, D), LD)
    with np.errstate(all="ignore"):
        for r in range(M):
            s, e_ = indptr[r], indptr[r + 1]
            n = e_ - s
            if n == 0:
                dqb[r] = tiny
                continue
            tr, kp = tx[s:e_], keep[s:e_]
            ex = np.exp(tr - tr.max())
            pr = ex / ex.sum()
            pbr = b14[s:e_] + np.expm1(2 * sb[s:e_].max()) * pr
            vr = vl[cols[s:e_]]
            e = (gl[r] * vr).sum(axis=1)
            eb = (math.ceil(Dv / 64) + 6) * eps * np.abs(gl[r] * vr).sum(axis=1)
            ed = np.where(kp, cl * e, LD(0))
            edb = np.where(kp, cl * eb + eps * cl * np.abs(e), LD(0))
            ub = pbr * np.abs(ed) + pr * edb + eps * pr * np.abs(ed)
            delta = (pr * ed).sum()
            db = ub.sum() + gc._sum_depth(n, chunk) * eps * (pr * np.abs(ed)).sum()
            z = pr * (ed - delta)
            zb = pbr * np.abs(ed - delta) + pr * (edb + db) + 2 * eps * np.abs(z)
            yr = f[s:e_] * z
            ybr = np.abs(f[s:e_]) * zb + nr * eps * np.abs(yr)
            pd[s:e_] = np.where(kp, cl * pr, LD(0))
            pdb[s:e_] = np.where(kp, cl * pbr + eps * cl * pr, LD(0))
            y[s:e_], yb[s:e_] = yr, ybr
            kr = kl[cols[s:e_]]
            dq[r] = (yr[:, None] * kr).sum(axis=0)
            dqb[r] = (ybr[:, None] * np.abs(kr)).sum(axis=0) + (n + 1) * eps * np.abs(yr[:, None] * kr).sum(axis=0) + tiny
        dk, dkb, dv, dvb = np.zeros((N, D), LD), np.full((N, D), tiny, LD), np.zeros((N, Dv), LD), np.full((N, Dv), tiny, LD)
        perm, prow, pcol = gc.column_order(indptr, indices)
        cuts = np.searchsorted(pcol, np.arange(N + 1))
        for col in range(N):
            pos, rr = perm[cuts[col]:cuts[col + 1]], prow[cuts[col]:cuts[col + 1]]
            m = len(pos)
            if m == 0:
                continue
            dv[col] = (pd[pos, None] * gl[rr]).sum(axis=0)
            dvb[col] = (pdb[pos, None] * np.abs(gl[rr])).sum(axis=0) + (m + 1) * eps * (pd[pos, None] * np.abs(gl[rr])).sum(axis=0) + tiny
            dk[col] = (y[pos, None] * ql[rr]).sum(axis=0)
            dkb[col] = (yb[pos, None] * np.abs(ql[rr])).sum(axis=0) + (m + 1) * eps * np.abs(y[pos, None] * ql[rr]).sum(axis=0) + tiny
    return (dq, dk, dv), (dqb, dkb, dvb)

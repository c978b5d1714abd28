"""semiring_matmul_grad: the order contract of include/sparse_amd.h A18 restated in NumPy, the generators and the hand-written
cases that tests/test_semiring_grad.py and tests/test_semiring_grad_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd
imports this.

The restatement is written from the contract, not from the kernels: `da` by 64 accumulators over the columns and the fold by
halving, `db` by sequential pieces over each column's stored elements in stored order, `dinit` by the comparison with -1.  The
exactly rounded fma is `attention_grad_cases._fma`; the forward is `semiring_cases.semiring_restated`."""
import numpy as np

import attention_grad_cases as agc
import semiring_cases as sr

MULS = sr.MULS
DTYPES = (np.float32, np.float64)
CHUNK = 1024          # SEMIRING_GRAD_CHUNK: the pieces of db
LENGTHS = sr.LENGTHS


def _as2(x, M):
    x = np.asarray(x)
    return x.reshape(M, -1)


def da_restated(indptr, indices, b2, arg2, g2, mul):
    """da[e]: accumulator l starts at +0.0 and takes the columns j = l, l + 64, .. in ascending order - a + g, or fma(g, b, a), on
    a hit -, then the fold by halving, h = 32 .. 1.  (The elements of a row go side by side: one row of 64 accumulators each.)"""
    dtype = g2.dtype
    fma = agc._fma(dtype)
    M, N = arg2.shape
    da = np.zeros(len(indices), dtype)
    with np.errstate(all="ignore"):
        for r in range(M):
            s, e = int(indptr[r]), int(indptr[r + 1])
            if s == e:
                continue
            ks = indices[s:e]
            acc = np.zeros((e - s, 64), dtype)
            for jb in range(0, N, 64):
                w = min(64, N - jb)
                hit = arg2[r, jb:jb + w][None, :] == ks[:, None]
                grow = np.broadcast_to(g2[r, jb:jb + w], (e - s, w))
                if mul == "plus":
                    new = acc[:, :w] + grow
                else:
                    new = fma(grow, b2[ks, jb:jb + w], acc[:, :w]).astype(dtype, copy=False)
                acc[:, :w] = np.where(hit, new, acc[:, :w])
            h = 32
            while h >= 1:
                acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
                h //= 2
            da[s:e] = acc[:, 0]
    return da


def db_restated(indptr, indices, vals, K, arg2, g2, mul, chunk=CHUNK):
    """db[k][j]: the column's stored elements in stored order, in pieces of `chunk`; a piece starts at +0.0 and takes acc + g, or
    fma(a, g, acc), on a hit; the piece sums are added in piece order, the first piece's sum being the start.  (The columns go
    side by side: step t takes the t-th element of every piece that has one.)"""
    dtype = g2.dtype
    fma = agc._fma(dtype)
    N = arg2.shape[1]
    perm, rows, cols = agc.column_order(indptr, indices)
    db = np.zeros((K, N), dtype)
    bounds = np.searchsorted(cols, np.arange(K + 1))
    lens = np.diff(bounds)
    with np.errstate(all="ignore"):
        for piece in range(-(-int(lens.max(initial=0)) // chunk)):
            start = bounds[:-1] + piece * chunk
            size = np.clip(lens - piece * chunk, 0, chunk)
            acc = np.zeros((K, N), dtype)
            for t in range(int(size.max(initial=0))):
                live = np.nonzero(size > t)[0]                      # the columns whose piece has a t-th element
                at = start[live] + t
                r, pos = rows[at], perm[at]
                hit = arg2[r] == live[:, None]
                if mul == "plus":
                    new = acc[live] + g2[r]
                else:
                    new = fma(np.broadcast_to(vals[pos][:, None], (len(live), N)), g2[r], acc[live]).astype(dtype, copy=False)
                acc[live] = np.where(hit, new, acc[live])
            has = size > 0
            db[has] = acc[has] if piece == 0 else db[has] + acc[has]
    return db


def grad_restated(indptr, indices, vals, b, arg, g, mul, chunk=CHUNK):
    """(da (nnz,), db of the shape of b, dinit of the shape of g) of the contract; `vals` are converted to the type of `b` first"""
    b = np.asarray(b)
    dtype = b.dtype
    assert dtype in [np.dtype(d) for d in DTYPES] and mul in MULS
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    vals = np.asarray(vals).astype(dtype)
    M, K = len(indptr) - 1, b.shape[0]
    b2, arg2, g2 = b.reshape(K, -1), _as2(arg, M), np.ascontiguousarray(_as2(g, M))
    assert g2.dtype == dtype and arg2.shape == g2.shape == (M, b2.shape[1])
    da = da_restated(indptr, indices, b2, arg2, g2, mul)
    db = db_restated(indptr, indices, vals, K, arg2, g2, mul, chunk)
    dinit = np.where(arg2 == -1, g2, dtype.type(0))
    return da, db.reshape(b.shape), dinit.reshape(np.asarray(g).shape)


# ---- generators -----------------------------------------------------------------------------------------------------------------------
def transposed(indptr, indices, vals, shape):
    """the CSR triple of the transposed pattern: its ROW lengths are the column lengths of the argument (elements of a row in
    ascending column order)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    perm, rows, cols = agc.column_order(indptr, indices)
    tptr = np.searchsorted(cols, np.arange(shape[1] + 1)).astype(np.asarray(indices).dtype)
    return tptr, rows.astype(np.asarray(indices).dtype), np.asarray(vals)[perm], (shape[1], shape[0])


def tie_free(seed, lengths, K, N, dtype, mul, with_init=True):
    """(indptr, indices, vals, b, init): operands whose products are pairwise distinct in every output, with gaps of at least
    1e-3 - a distinct integer multiple of 1 / 64 per stored element (plus), or distinct factors (times) against a b whose rows
    differ by more.  Row i holds lengths[i] elements"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    indptr, indices, _, shape = sr.csr_mask(seed, lengths, dtype, ncols=K, shuffle=False)
    nnz = len(indices)
    M = len(lengths)
    if mul == "plus":
        # a_e = distinct multiples of 1 / 64 below 2^-2 steps of b: t = a + b[k, j] with b[k, j] = k * 16 + j-dependent offset
        vals = (rng.permutation(max(nnz, 1))[:nnz] / 64.0).astype(dtype)
        b = (np.arange(K)[:, None] * (nnz / 64.0 + 1.0) + rng.permutation(K * N).reshape(K, N) / (64.0 * K * N)).astype(dtype)
    else:
        vals = (1.0 + rng.permutation(max(nnz, 1))[:nnz] / 64.0).astype(dtype) * np.where(rng.random(nnz) < 0.5, -1, 1).astype(dtype)
        b = ((1.0 + rng.permutation(K * N).reshape(K, N) / 8.0) * np.where(rng.random((K, N)) < 0.5, -1, 1)).astype(dtype)
    init = (rng.permutation(M * N).reshape(M, N) / 4.0 - M * N / 8.0 + 1.0 / 128).astype(dtype)
    return indptr, indices, vals, b, (init if with_init else None)


def products_distinct(indptr, indices, vals, b, mul, init=None, gap=0.0):
    """are the terms of every output - the init included - pairwise distinct (by more than `gap`) and NaN-free?"""
    M, N = len(indptr) - 1, b.shape[1]
    for r in range(M):
        s, e = int(indptr[r]), int(indptr[r + 1])
        for j in range(N):
            t = sr.products(vals[s:e], np.ascontiguousarray(b[indices[s:e], j]), mul)
            if init is not None:
                t = np.concatenate((init[r, j:j + 1], t))
            if np.isnan(t).any() or (len(t) > 1 and np.min(np.diff(np.sort(t))) <= gap):
                return False
    return True


# ---- the hand-written cases -----------------------------------------------------------------------------------------------------------
INF, NAN = np.inf, np.nan


def hand_cases(dtype=np.float64):
    """[(name, indptr, indices, vals, b (K, N), arg (M, N), g (M, N), mul, da, db, dinit)]: the rules of A18 spelled out by hand"""
    f = lambda x: np.array(x, dtype)
    i64 = lambda x: np.array(x, np.int64)
    out = []
    # one row of three elements at the inner indices 1, 3, 4 of K = 6; two columns
    ptr, idx, val = i64([0, 3]), i64([1, 3, 4]), f([2.0, -3.0, 0.5])
    b = f([[9, 9], [1, 2], [9, 9], [3, 4], [5, 6], [9, 9]])
    zb = np.zeros_like(b)
    for mul in MULS:
        g = f([[7.0, -2.0]])
        out.append((f"arg all -1, {mul}", ptr, idx, val, b, i64([[-1, -1]]), g, mul, f([0, 0, 0]), zb, g))
        gz = f([[-0.0, 1.0]])
        db = zb.copy()
        # one hit with g = -0.0 at (0, 0) through k = 3: +0.0 + -0.0 = +0.0 (plus); fma(-3, -0.0, +0.0) = +0.0 (times)
        out.append((f"one hit with g = -0.0, {mul}", ptr, idx, val, b, i64([[3, -1]]), gz, mul, f([0, 0.0, 0]), db, f([[0.0, 1.0]])))
        # an in-range arg that is not stored in its row (2, 0 and 5) credits nothing - and is never used as an address (10 ** 12)
        out.append((f"arg not stored in its row, {mul}", ptr, idx, val, b, i64([[2, 10 ** 12]]), g, mul, f([0, 0, 0]), zb, f([[0, 0]])))
    # NaN and inf in g reach only the credited elements
    g = f([[NAN, INF]])
    arg = i64([[1, 4]])
    db = zb.copy()
    db[1, 0], db[4, 1] = NAN, INF
    out.append(("nan and inf in g, plus", ptr, idx, val, b, arg, g, "plus", f([NAN, 0, INF]), db, f([[0, 0]])))
    db = zb.copy()
    db[1, 0], db[4, 1] = NAN, INF                                  # a * g: 2 * NaN, 0.5 * inf
    out.append(("nan and inf in g, times", ptr, idx, val, b, arg, g, "times", f([NAN, 0, INF]), db, f([[0, 0]])))
    # empty rows and columns: rows 0 and 2 empty, row 1 holds (1, 0) and (1, 2); K = 4: columns 1 and 3 empty
    ptr2, idx2, val2 = i64([0, 0, 2, 2]), i64([0, 2]), f([2.0, 4.0])
    b2 = f([[1.0], [2.0], [3.0], [4.0]])
    g2 = f([[5.0], [6.0], [7.0]])
    out.append(("empty rows and columns, plus", ptr2, idx2, val2, b2, i64([[-1], [2], [-1]]), g2, "plus", f([0, 6.0]),
                f([[0], [0], [6.0], [0]]), f([[5.0], [0], [7.0]])))
    out.append(("empty rows and columns, times", ptr2, idx2, val2, b2, i64([[-1], [0], [-1]]), g2, "times", f([6.0, 0]),
                f([[12.0], [0], [0], [0]]), f([[5.0], [0], [7.0]])))
    # a stored zero under times: the element takes g * b, b takes 0 * g = 0 (a NaN g gives NaN there: 0 * NaN)
    out.append(("a stored zero under times", i64([0, 2]), i64([0, 1]), f([0.0, 1.0]), f([[3.0], [-1.0]]), i64([[0]]), f([[2.0]]),
                "times", f([6.0, 0]), f([[0.0], [0]]), f([[0]])))
    # duplicates: both stored (0, 1) are credited
    out.append(("duplicates all credited, plus", i64([0, 3]), i64([1, 1, 2]), f([1.0, 2.0, 3.0]), f([[0], [1.0], [2.0]]), i64([[1]]),
                f([[4.0]]), "plus", f([4.0, 4.0, 0]), f([[0], [8.0], [0]]), f([[0]])))
    out.append(("duplicates all credited, times", i64([0, 3]), i64([1, 1, 2]), f([1.0, 2.0, 3.0]), f([[0], [5.0], [2.0]]), i64([[1]]),
                f([[4.0]]), "times", f([20.0, 20.0, 0]), f([[0], [12.0], [0]]), f([[0]])))
    return out


def n130_case(dtype, mul):
    """one element hit at all 130 columns: the accumulators 0 and 1 take three terms (j, j + 64, j + 128), the others two; the
    expected da is written out term by term"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(130)
    g = (rng.integers(-2 ** 20, 2 ** 20, (1, 130)) / 2.0 ** 12).astype(dtype) * (1 + np.arange(130) % 7)
    g = g.astype(dtype)
    b = (rng.integers(1, 2 ** 12, (2, 130)) / 2.0 ** 6).astype(dtype)
    fma = agc._fma(dtype)
    acc = [dtype.type(0)] * 64
    for j in range(130):
        acc[j % 64] = (acc[j % 64] + g[0, j]) if mul == "plus" else dtype.type(fma(g[0, j:j + 1], b[1, j:j + 1], np.array([acc[j % 64]]))[0])
    h = 32
    while h >= 1:
        for l in range(h):
            acc[l] = acc[l] + acc[l + h]
        h //= 2
    arg = np.full((1, 130), 1, np.int64)
    return np.array([0, 1]), np.array([1]), np.array([1.5], dtype), b, arg, g, np.array([acc[0]], dtype)


PLACED = ("hit", "g = -0.0", "nan and inf in g", "stored zero", "arg not stored", "arg all -1", "duplicate")


def _placed_g(rng, kind, shape, dtype):
    g = rng.standard_normal(shape).astype(dtype)
    if kind == "g = -0.0":
        g[...] = -0.0
    elif kind == "nan and inf in g":
        g[..., 0], g[..., 1:] = NAN, -INF
    return g


def place_in(n, where, dtype, mul, kind="hit", N=3):
    """a row of n elements among K = n + 2 columns with one of the hand-written situations at position `where`: (indptr, indices,
    vals, b, arg, g).  "hit": that element alone is credited, at every column; "g = -0.0" / "nan and inf in g": the same with
    such a gradient; "stored zero": its value is 0; "arg not stored": arg names a column the row does not store (nothing is
    credited); "arg all -1"; "duplicate": the next position (the previous one at the end) repeats its inner index - both are
    credited"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(n * 1000 + where)
    idx = np.sort(rng.choice(n + 2, n, replace=False)).astype(np.int64)
    vals = sr.values(rng, n, dtype)
    vals[vals == 0] = 1
    b = rng.standard_normal((n + 2, N)).astype(dtype)
    g = _placed_g(rng, kind, (1, N), dtype)
    arg = np.full((1, N), idx[where], np.int64)
    if kind == "stored zero":
        vals[where] = 0
    elif kind == "arg not stored":
        arg[...] = np.setdiff1d(np.arange(n + 2), idx)[where % 2]
    elif kind == "arg all -1":
        arg[...] = -1
    elif kind == "duplicate":
        idx[where + 1 if where + 1 < n else where - 1] = idx[where]
    return np.array([0, n], np.int64), idx, vals, b, arg, g


def place_in_column(n, where, dtype, mul, kind="hit", N=3):
    """the same situations in a COLUMN of n elements: n rows of one element each in column 1 of K = 3; row `where` alone names
    it ("arg not stored": it names column 2; "duplicate": the next row names it too)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(n * 1000 + where + 500)
    vals = sr.values(rng, n, dtype)
    vals[vals == 0] = 1
    b = rng.standard_normal((3, N)).astype(dtype)
    g = rng.standard_normal((n, N)).astype(dtype)
    g[where] = _placed_g(rng, kind, (N,), dtype)
    arg = np.full((n, N), -1, np.int64)
    arg[where] = 1
    if kind == "stored zero":
        vals[where] = 0
    elif kind == "arg not stored":
        arg[where] = 2
    elif kind == "arg all -1":
        arg[where] = -1
    elif kind == "duplicate":
        arg[where + 1 if where + 1 < n else where - 1] = 1
    return np.arange(n + 1, dtype=np.int64), np.ones(n, np.int64), vals, b, arg, g

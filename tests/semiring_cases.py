"""semiring_matmul: the contract of include/sparse_amd.h A17 restated in NumPy, a dense brute force for the inputs where one is
unambiguous, the hand-written adversarial sequences and the seeded case generators that tests/test_semiring.py and
tests/test_semiring_gpu.py share.  TEST INFRASTRUCTURE: nothing in sparse_amd imports this.

The restatement is written from the contract, not from the kernels: per output (row, column) it forms the sequence - the init
if given, then one product per stored element in stored order - and asks `np.argmin` / `np.argmax` which element is picked.
NumPy's own rule IS the contract: the first NaN if there is one, else the first element that attains the extremum, with -0.0
and +0.0 comparing equal."""
import numpy as np

ADDS = ("min", "max")
MULS = ("plus", "times")
SEMIRINGS = [(add, mul) for add in ADDS for mul in MULS]
DTYPES = (np.float32, np.float64, np.int32, np.int64)


def identity(add, dtype):
    """the identity of the add: what an output without any element holds"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(np.inf if add == "min" else -np.inf)
    lim = np.iinfo(dtype)
    return dtype.type(lim.max if add == "min" else lim.min)


def products(avals, brow, mul):
    """t_e = a_e (+ | *) b_e in the type of the operands: one operation; integers wrap in two's complement"""
    dtype = avals.dtype
    assert brow.dtype == dtype
    with np.errstate(all="ignore"):
        if dtype.kind == "f":
            return (avals + brow if mul == "plus" else avals * brow).astype(dtype, copy=False)
        u = np.dtype(f"u{dtype.itemsize}")
        au, bu = avals.view(u), brow.view(u)
        return (au + bu if mul == "plus" else au * bu).astype(u, copy=False).view(dtype)


def pick(seq, add):
    """the position `np.argmin` / `np.argmax` picks in the sequence"""
    return int(np.argmin(seq) if add == "min" else np.argmax(seq))


def semiring_restated(indptr, indices, vals, b, add, mul, init=None):
    """(out, arg) of the contract: `vals` are converted to the type of `b` first; b (K, N) or (K,), init None or of the
    result's shape.  A plain loop over (row, column)"""
    b = np.asarray(b)
    dtype = b.dtype
    assert dtype in [np.dtype(d) for d in DTYPES] and add in ADDS and mul in MULS
    one_d = b.ndim == 1
    b2 = b.reshape(b.shape[0], -1)
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    vals = np.asarray(vals).astype(dtype)
    M, N = len(indptr) - 1, b2.shape[1]
    i2 = None if init is None else np.asarray(init).reshape(M, N)
    assert i2 is None or i2.dtype == dtype
    out = np.full((M, N), identity(add, dtype), dtype=dtype)
    arg = np.full((M, N), -1, dtype=np.int64)
    for r in range(M):
        s, e = indptr[r], indptr[r + 1]
        ks = indices[s:e]
        for j in range(N):
            t = products(vals[s:e], np.ascontiguousarray(b2[ks, j]), mul)
            seq = t if i2 is None else np.concatenate((i2[r, j:j + 1], t))
            if len(seq) == 0:
                continue
            at = pick(seq, add)
            out[r, j] = seq[at]
            if i2 is None:
                arg[r, j] = ks[at]
            elif at > 0:
                arg[r, j] = ks[at - 1]
    return (out[:, 0], arg[:, 0]) if one_d else (out, arg)


def brute_force(dense_a, stored, b, add, mul):
    """(out, arg) of the dense statement `np.where(stored, a op b, identity).min(axis=1)` with its argmin: unambiguous only
    without ties, NaN and signed zeros, and with at least one stored element per row"""
    dtype = b.dtype
    a3, b3 = dense_a.astype(dtype)[:, :, None], b[None, :, :]
    with np.errstate(all="ignore"):
        t = a3 + b3 if mul == "plus" else a3 * b3
    t = np.where(stored[:, :, None], t, identity(add, dtype))
    return (t.min(axis=1), t.argmin(axis=1)) if add == "min" else (t.max(axis=1), t.argmax(axis=1))


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload of a NaN is no result)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    u = f"u{a.dtype.itemsize}"
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


# ---- generators -----------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 7, 8, 9, 33, 63, 64, 65, 100, 0, 128, 129, 200]


def csr_mask(seed, lengths, dtype=np.float32, idx_dtype=np.int64, ncols=None, shuffle=True):
    """(indptr, indices, values, shape): row i holds lengths[i] elements (the rows shuffled by the seed) at random ascending
    columns.  Float values are multiples of 1 / 8 in [-4, 4] - with zeros, so that ties and stored zeros occur -, integer values
    lie in -5 .. 5"""
    rng = np.random.default_rng(seed)
    lengths = list(lengths)
    if shuffle:
        lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    ncols = ncols or max(max(lengths, default=0), 1) + 3
    cols = [np.sort(rng.choice(ncols, n, replace=False)) for n in lengths]
    indices = (np.concatenate(cols) if lengths else np.zeros(0)).astype(idx_dtype)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(idx_dtype)
    return indptr, indices, values(rng, len(indices), dtype), (len(lengths), ncols)


def values(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return rng.integers(0, 2, n).astype(bool)
    if dtype.kind in "iu":
        return rng.integers(-5, 6, n).astype(dtype)
    return (rng.integers(-32, 33, n) / 8).astype(dtype)


def operand(seed, shape, dtype):
    """a dense operand of few distinct values (multiples of 1 / 8; small integers): products tie often"""
    rng = np.random.default_rng(seed)
    return values(rng, int(np.prod(shape)), dtype).reshape(shape)


def coords_of(indptr, indices):
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    return np.stack([rows, np.asarray(indices, dtype=np.int64)])


# ---- the hand-written adversarial sequences ---------------------------------------------------------------------------------------------
# (name, add, mul, a values, b values, init or None, the position picked in the sequence - the init counts as position 0 when
# given -, the value expected there): the rules of A17 spelled out by hand.  float64 unless a dtype is named
INF, NAN = np.inf, np.nan
ADVERSARIAL = [
    ("nan first", "min", "plus", [NAN, 1.0, -5.0], [0.0, 0.0, 0.0], None, 0, NAN),
    ("nan middle", "min", "plus", [1.0, NAN, -5.0], [0.0, 0.0, 0.0], None, 1, NAN),
    ("nan last", "max", "plus", [1.0, 9.0, NAN], [0.0, 0.0, 0.0], None, 2, NAN),
    ("two nans: the first", "max", "times", [1.0, NAN, 3.0, NAN], [1.0, 1.0, 1.0, 1.0], None, 1, NAN),
    ("tie of first and last", "min", "plus", [1.0, 2.0, 3.0, 1.0], [0.5, 0.5, 0.5, 0.5], None, 0, 1.5),
    ("tie of first and last, max", "max", "times", [3.0, 2.0, 1.0, 3.0], [2.0, 2.0, 2.0, 2.0], None, 0, 6.0),
    ("-0 then +0", "min", "plus", [-0.0, 0.0], [-0.0, 0.0], None, 0, -0.0),
    ("+0 then -0", "min", "plus", [0.0, -0.0], [0.0, -0.0], None, 0, 0.0),
    ("-0 then +0, max", "max", "times", [-1.0, 1.0], [0.0, 0.0], None, 0, -0.0),
    ("+0 then -0, max", "max", "times", [1.0, -1.0], [0.0, 0.0], None, 0, 0.0),
    ("an init that ties", "min", "plus", [1.0, 2.0], [1.0, 0.0], 2.0, 0, 2.0),
    ("an init of -0 against +0", "max", "plus", [0.0], [0.0], -0.0, 0, -0.0),
    ("an init that loses", "min", "plus", [1.0, 2.0], [0.0, 0.0], 5.0, 1, 1.0),
    ("an init that is nan", "min", "plus", [1.0], [0.0], NAN, 0, NAN),
    ("inf + -inf", "min", "plus", [1.0, INF, -7.0], [0.0, -INF, 0.0], None, 1, NAN),
    ("0 * inf", "max", "times", [1.0, 0.0, 7.0], [1.0, INF, 1.0], None, 1, NAN),
    ("an element equal to the identity", "min", "plus", [INF, INF], [0.0, 0.0], None, 0, INF),
    ("int32 overflow wraps, plus", "min", "plus", np.array([2 ** 31 - 1, 5], np.int32), np.array([1, 0], np.int32), None, 0, -2 ** 31),
    ("int32 overflow wraps, times", "max", "times", np.array([2 ** 30, 3], np.int32), np.array([2, 1], np.int32), None, 1, 3),
    ("int32 element equal to the identity", "min", "plus", np.array([2 ** 31 - 1, 2 ** 31 - 1], np.int32), np.array([0, 0], np.int32), None, 0, 2 ** 31 - 1),
]


def adversarial_case(case, dtype=None):
    """(indptr, indices, vals, b (K, 1), init (1, 1) or None, add, mul, picked position, value) of one entry as a matrix of one
    row; float entries in `dtype` (default float64)"""
    name, add, mul, av, bv, init, at, value = case
    av, bv = np.asarray(av), np.asarray(bv)
    dt = av.dtype if av.dtype.kind == "i" else np.dtype(dtype or np.float64)
    n = len(av)
    indices = np.arange(n, dtype=np.int64) * 2 + 1             # inner indices 1, 3, 5, ..: not the positions
    b = np.zeros((2 * n + 1, 1), dt)
    b[indices, 0] = bv.astype(dt)
    ini = None if init is None else np.array([[init]], dt)
    return np.array([0, n]), indices, av.astype(dt), b, ini, add, mul, at, dt.type(value)

"""Cases for sparse @ sparse (`_kernels.dot_csr_csr` / `_spgemm_rows`: csrc/spgemm_small.hip, csrc/spgemm_rows.hip, the global
expand-sort-compress of `_spgemm_keys`): a plain NumPy reference, a dense exact second formulation, a model of the bucket
kernel's `bucket_of` and of the host's route rules, and a case table in which every case puts a row, a bucket, a pass, a key
width or a size exactly where the code switches path.  No GPU, no torch, no package import.

The reference sums every output element left to right in the order of A's elements, starting from zero of the result type,
with a separately rounded multiply and add: what the library promises bit for bit on every route but the grouped reduce.
The numbers the table is aimed at are the constants below; tests/test_spgemm_cases.py reads the kernels' from the text of the
.hip sources and of _reduce.py (`source_constants`) and the host's from `sparse_amd._kernels` itself (its `SPGEMM_*` values),
so a retune that moves a boundary fails there instead of silently un-aiming the table.

A case builds its operands for a value size (4 or 8 bytes: the row classes, the capacity and the small kernel's widths depend
on it) and states the route the product must take under the switches it sets - what `SPGEMM_STATS["route"]` must then say -
and the `heavy_or_declined` count beside it (`parts` is the bitmap kernel's word: no case here takes it, and it must stay
unset).  `predict` derives the same from a restatement of the host's rules and `bucket_model`, independent of the one choice
the library makes (`_kernels._spgemm_route`); tests/test_spgemm_cases.py feeds that function every case's own numbers and
holds the steps it returns against `predict`."""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants the table is aimed at ---------------------------------------------------------------------------------
SPG_BUCKET_MAX = 16
C0, C1 = 256 * 4, 512 * 8
N_COL_LIMIT = 2 ** 31 - 1                    # n_col >= this: the bucket kernels decline
SMALL_MAX_CELLS, SMALL_MAX_NNZ = 1 << 22, 1 << 16
RUN_PROBE_MIN, RUN_DUPS_MIN, LONG_RUN_WINDOW = 1 << 13, 1023, 1024


def mid_top(key_bytes, val_bytes):
    mid = 16 if key_bytes + val_bytes <= 12 else 14
    return mid, (24 if key_bytes + val_bytes <= 8 else mid)


def row_classes(key_bytes, val_bytes):
    """[(BLOCK, ITEMS, PASSES, lo, hi)]: the class serves rows with lo < products <= hi (class 0 also the empty rows)"""
    mid, top = mid_top(key_bytes, val_bytes)
    c2, c3, c4 = 512 * mid, 512 * top, 1024 * top
    out = [(256, 4, 1, -1, C0), (512, 8, 1, C0, C1), (512, mid, 2, C1, c2)]
    out.append((512, top, 2, c2, c3) if c3 > c2 else None)
    out.append((1024, top, 8, c3, c4))
    return out


def bounds(key_bytes, val_bytes):
    """(c0, c1, c2, c3, c4)"""
    mid, top = mid_top(key_bytes, val_bytes)
    return C0, C1, 512 * mid, 512 * top, 1024 * top


def capp(block, items, passes):
    n = block * items
    return n if passes == 1 else (n // passes) * 9 // 8


def nbp(block, items, passes):
    c = capp(block, items, passes)
    x = max(c, block) if passes > 2 else max(c // 2, block)
    p = 1
    while p < x:
        p <<= 1
    return p


def stage(block, items, passes):
    """A elements of a row the kernel stages in LDS at a time"""
    return min(capp(block, items, passes), 2048)


def spg_bits(n):
    b = 1
    while (1 << b) <= n:
        b += 1
    return b


def key_bits(n_col, max_arow):
    return spg_bits(n_col) + spg_bits(max_arow - 1 if max_arow > 0 else 0)


def key_bytes_of(n_col, max_arow):
    return 4 if key_bits(n_col, max_arow) <= 32 else 8


def sm_max_cols(val_bytes, waves):
    return ((64 * 1024) // waves - 32) * 8 // (8 * val_bytes + 1)


def bucket_of(n_col, block, items, passes, cols):
    """the kernel's `bucket_of` for an array of columns: floor(col * floor(NBP * PASSES * 2^32 / n_col) / 2^32)
    (col * scale < 2^15 * 2^32: no overflow)"""
    scale = ((nbp(block, items, passes) * passes) << 32) // n_col
    return (np.asarray(cols, dtype=np.int64) * scale) >> 32


def bucket_model(n_col, key_bytes, val_bytes, columns_of_row):
    """the kernel's view of one output row whose products have the columns `columns_of_row` (one entry per product):
    (class index or None above the capacity, largest bucket count, largest per-pass count)"""
    cols = np.asarray(columns_of_row, dtype=np.int64)
    P = cols.size
    classes = row_classes(key_bytes, val_bytes)
    cls = next((i for i, c in enumerate(classes) if c is not None and c[3] < P <= c[4]), None)
    if P == 0:
        return 0, 0, 0
    if cls is None:
        return None, 0, 0
    block, items, passes = classes[cls][:3]
    b = bucket_of(n_col, block, items, passes, cols)
    assert b.max() < nbp(block, items, passes) * passes
    return cls, int(np.bincount(b).max()), int(np.bincount(b // nbp(block, items, passes)).max())


def served(n_col, key_bytes, val_bytes, columns_of_row):
    """True: the row kernel computes the row; False: it declines it (a bucket above SPG_BUCKET_MAX, a pass above CAPP);
    None: above the capacity, skipped"""
    cls, big, in_pass = bucket_model(n_col, key_bytes, val_bytes, columns_of_row)
    if cls is None:
        return None
    if len(columns_of_row) == 0:
        return True
    return big <= SPG_BUCKET_MAX and in_pass <= capp(*row_classes(key_bytes, val_bytes)[cls][:3])


def pass_start(n_col, cls, p):
    """the smallest column whose bucket lies in pass >= p of the class (block, items, passes)"""
    lo, hi = 0, n_col
    while lo < hi:
        mid = (lo + hi) // 2
        if bucket_of(n_col, *cls[:3], [mid])[0] // nbp(*cls[:3]) >= p:
            hi = mid
        else:
            lo = mid + 1
    return lo


def source_constants():
    """the same numbers as the source files state them today"""
    def src(*parts):
        return open(os.path.join(ROOT, "sparse_amd", *parts)).read()

    def grab(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: `{pattern}` is gone from the source - move the cases of tests/spgemm_cases.py with it"
        return m

    rows, small, red = src("csrc", "spgemm_rows.hip"), src("csrc", "spgemm_small.hip"), src("_reduce.py")
    out = {"SPG_BUCKET_MAX": int(grab(rows, r"constexpr int SPG_BUCKET_MAX = (\d+);", "SPG_BUCKET_MAX")[1])}
    m = grab(rows, r"static constexpr int MID = sizeof\(KEY\) \+ sizeof\(V\) <= (\d+) \? (\d+) : (\d+);", "MID")
    out["MID"] = tuple(int(x) for x in m.groups())
    m = grab(rows, r"static constexpr int64_t c0 = (\d+) \* (\d+), c1 = (\d+) \* (\d+), c2 = (\d+) \* MID;", "c0, c1, c2")
    out["c0"], out["c1"], out["c2_block"] = int(m[1]) * int(m[2]), int(m[3]) * int(m[4]), int(m[5])
    m = grab(rows, r"static constexpr int TOP = sizeof\(KEY\) \+ sizeof\(V\) <= (\d+) \? (\d+) : MID;", "TOP")
    out["TOP"] = (int(m[1]), int(m[2]))
    out["c3_block"] = int(grab(rows, r"static constexpr int64_t c3 = (\d+) \* TOP;", "c3")[1])
    out["c4_block"] = int(grab(rows, r"static constexpr int64_t c4 = (\d+) \* TOP;", "c4")[1])
    lines = re.findall(r"^\s*(?:if \((.*?)\) )?SPG_CLASS\((\d+), ([\w:]+), (\d+), ([-\w:]+), ([\w:]+)\)$", rows, re.M)
    assert len(lines) == 5, "the five SPG_CLASS lines"
    out["classes"] = [(cond, int(b), it.replace("C::", ""), int(p), lo.replace("C::", ""), hi.replace("C::", ""))
                      for cond, b, it, p, lo, hi in lines]
    grab(rows, r"static constexpr int CAPP = PASSES == 1 \? N : \(N / PASSES\) \* 9 / 8;", "CAPP")
    grab(rows, r"NBP = pow2_at_least\(PASSES > 2 \? \(CAPP > BLOCK \? CAPP : BLOCK\) : \(CAPP / 2 > BLOCK \? CAPP / 2 : BLOCK\)\);", "NBP")
    grab(rows, r"static constexpr int STAGE = CAPP < 2048 \? CAPP : 2048;", "STAGE")
    grab(rows, r"for \(int c0 = 0; c0 < nA; c0 \+= STAGE\) \{", "the staging chunks")
    grab(rows, r"scale = \(\(\(uint64_t\)\(NBP \* PASSES\)\) << 32\) / \(uint64_t\)n_col;", "the bucket scale")
    grab(rows, r"return \(int\)\(\(\(uint64_t\)\(key >> ebits\) \* scale\) >> 32\);", "bucket_of")
    grab(rows, r"if \(P64 <= lo \|\| P64 > hi\) \{", "the class range (lo, hi]")
    grab(rows, r"if \(in_pass > CAPP\) \{", "the pass capacity test")
    grab(rows, r"if \(c > SPG_BUCKET_MAX\) \{", "the bucket capacity test")
    grab(rows, r"const bool k32 = spg_bits\(n_col\) \+ spg_bits\(max_arow > 0 \? max_arow - 1 : 0\) <= 32;", "the key width rule")
    grab(rows, r"while \(\(\(int64_t\)1 << b\) <= n\) \+\+b;", "spg_bits")
    grab(rows, r"const bool by_prod = prod\[r\] > cap, by_a = alen > cap,", "the classification by the capacity")
    out["N_COL_LIMIT"] = int(grab(rows, r"n_col >= (\d+)LL", "the column limit")[1])
    m = grab(small, r"const int64_t per_wave = \((\d+) \* 1024\) / waves - (\d+);\s+return per_wave \* 8 / \(8 \* \(int64_t\)sizeof\(V\) \+ 1\);",
             "sm_max_cols")
    out["sm_lds_kb"], out["sm_reserve"] = int(m[1]), int(m[2])
    grab(small, r"if \(n_col <= sm_max_cols<V>\(4\)\) \{", "the four-wave switch")
    grab(small, r"\} else if \(n_col <= sm_max_cols<V>\(1\)\) \{", "the one-wave switch")
    out["LONG_RUN_WINDOW"] = int(grab(red, r"LONG_RUN_WINDOW = (\d+)", "LONG_RUN_WINDOW")[1])
    return out


# ---- the reference -------------------------------------------------------------------------------------------------------
def bits_of(a):
    """the unsigned bit view of a value array (complex as [n, 2] words); every NaN as ONE pattern: IEEE 754 leaves the sign
    and payload of a generated NaN to the implementation (x86 gives inf * 0 the sign bit, other hardware does not)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        return bits_of(a.view(f"f{a.dtype.itemsize // 2}")).reshape(-1, 2)
    out = a.view(f"u{a.dtype.itemsize}").copy()
    if a.dtype.kind == "f":
        out[np.isnan(a)] = np.array(np.nan, dtype=a.dtype).view(out.dtype)
    return out


def _mul(x, y):
    """one rounded multiply per real product; complex: four products, a subtraction and an addition, nothing fused"""
    with np.errstate(all="ignore"):
        if x.dtype.kind == "c":
            re = x.real * y.real - x.imag * y.imag
            im = x.real * y.imag + x.imag * y.real
            out = np.empty(x.shape, dtype=x.dtype)
            out.real, out.imag = re, im
            return out
        return x * y


class Expanded:
    """every product of A @ B, stably sorted by (row, column): A-element order survives inside an output element.
    rows / cols / vals per product, start / length per output element"""

    def __init__(self, n_row, n_col, A, B):
        (ad, ai, ap), (bd, bi, bp) = A, B
        assert ad.dtype == bd.dtype
        ai, ap, bi, bp = (np.asarray(x, dtype=np.int64) for x in (ai, ap, bi, bp))
        assert ap.size == n_row + 1
        lens = bp[ai + 1] - bp[ai]
        P = int(lens.sum())
        e = np.repeat(np.arange(ai.size, dtype=np.int64), lens)
        first = np.cumsum(lens) - lens
        q = bp[ai][e] + (np.arange(P, dtype=np.int64) - first[e])
        rows = np.repeat(np.arange(n_row, dtype=np.int64), np.diff(ap))[e]
        cols = bi[q]
        vals = _mul(ad[e], bd[q])
        order = np.lexsort((cols, rows))                   # (stable)
        self.rows, self.cols, self.vals = rows[order], cols[order], vals[order]
        head = np.ones(P, dtype=bool)
        head[1:] = (self.rows[1:] != self.rows[:-1]) | (self.cols[1:] != self.cols[:-1])
        self.start = np.flatnonzero(head)
        self.length = np.diff(np.append(self.start, P))
        self.n_row, self.n_col = n_row, n_col


def spgemm_ref(n_row, n_col, A, B, expanded=None):
    """(data, indices, indptr) of A @ B: sorted columns, explicit zeros kept, every element 0 + p1 + p2 + ... left to right
    in the result type (integers wrap)"""
    x = expanded or Expanded(n_row, n_col, A, B)
    sums = np.zeros(x.start.size, dtype=x.vals.dtype)
    with np.errstate(all="ignore"):
        for t in range(int(x.length.max()) if x.length.size else 0):
            sel = np.flatnonzero(x.length > t)
            sums[sel] = sums[sel] + x.vals[x.start[sel] + t]
    indptr = np.zeros(n_row + 1, dtype=np.int64)
    np.cumsum(np.bincount(x.rows[x.start], minlength=n_row), out=indptr[1:])
    return sums, x.cols[x.start].copy(), indptr


def prune_bits(data, indices, indptr):
    """the same without the elements whose bits are all zero (+0.0 / 0; -0.0 stays): (data, rows, cols)"""
    b = bits_of(data)
    keep = b.any(axis=1) if b.ndim == 2 else b != 0
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    return data[keep], rows[keep], indices[keep]


def dense_exact(n_row, n_col, A, B):
    """integer-valued operands: the int64 dense product over the columns that occur (a second formulation; exact while
    nothing exceeds 2^63), as (dense [n_row, distinct columns], the distinct columns)"""
    (ad, ai, ap), (bd, bi, bp) = A, B
    cols, inv = np.unique(np.asarray(bi, dtype=np.int64), return_inverse=True)
    n_inner = len(bp) - 1
    da, db = np.zeros((n_row, n_inner), dtype=np.int64), np.zeros((n_inner, max(cols.size, 1)), dtype=np.int64)
    da[np.repeat(np.arange(n_row), np.diff(ap)), np.asarray(ai, dtype=np.int64)] = np.asarray(ad).real.astype(np.int64)
    db[np.repeat(np.arange(n_inner), np.diff(bp)), inv] = np.asarray(bd).real.astype(np.int64)
    return da @ db, cols


def reassociation_bound(x):
    """per output element: (n - 1) * eps * sum |p_i| in longdouble - the bound for any two summation orders of the same
    rounded products (each of the n - 1 additions of either order rounds a partial sum of magnitude <= sum |p_i|)"""
    mag = np.abs(x.vals).astype(np.longdouble)
    tot = np.add.reduceat(mag, x.start) if x.start.size else mag[:0]
    real = np.dtype(f"f{x.vals.dtype.itemsize // 2}") if x.vals.dtype.kind == "c" else x.vals.dtype
    return (x.length - 1) * np.longdouble(np.finfo(real).eps) * tot


def exact_sums(x):
    """per output element: math.fsum of its products (real values)"""
    v = x.vals.astype(np.float64)
    return np.array([math.fsum(v[s:s + n]) for s, n in zip(x.start, x.length)], dtype=np.float64)


# ---- structures ----------------------------------------------------------------------------------------------------------
class Struct:
    """the pattern of A [n_row, n_inner] and B [n_inner, n_col] (int64 arrays) and the index types the operands are given in
    (a_indices, a_indptr, b_indices, b_indptr)"""

    def __init__(self, n_row, n_inner, n_col, ai, ap, bi, bp, idx=("int64",) * 4, values=None):
        self.n_row, self.n_inner, self.n_col = n_row, n_inner, n_col
        self.ai, self.ap, self.bi, self.bp = (np.asarray(x, dtype=np.int64) for x in (ai, ap, bi, bp))
        self.idx, self.values = idx, values
        assert self.ap.size == n_row + 1 and self.bp.size == n_inner + 1 and self.ap[-1] == self.ai.size and self.bp[-1] == self.bi.size
        assert self.bi.size == 0 or (0 <= self.bi.min() and self.bi.max() < n_col)
        assert self.ai.size == 0 or (0 <= self.ai.min() and self.ai.max() < n_inner)

    @functools.cached_property
    def blen(self):
        return np.diff(self.bp)

    @functools.cached_property
    def prod(self):
        """products per output row"""
        per_e = self.blen[self.ai]
        return np.add.reduceat(np.append(per_e, 0), self.ap[:-1]) * (np.diff(self.ap) > 0) if self.ai.size else np.zeros(self.n_row, np.int64)

    @functools.cached_property
    def alen(self):
        return np.diff(self.ap)

    def columns_of_row(self, r):
        e = self.ai[self.ap[r]:self.ap[r + 1]]
        return np.concatenate([self.bi[self.bp[k]:self.bp[k + 1]] for k in e]) if e.size else np.zeros(0, np.int64)

    @property
    def max_arow(self):
        return int(self.alen.max()) if self.n_row else 0

    @property
    def key_bytes(self):
        return key_bytes_of(self.n_col, self.max_arow)


def assemble(n_col, rows, idx=("int64",) * 4, values=None):
    """rows[r] = the B rows (column arrays, strictly ascending) that A row r's elements point to, one new B row per A
    element, in order"""
    ap, bp, bi = [0], [0], []
    for r in rows:
        ap.append(ap[-1] + len(r))
        for cols in r:
            cols = np.asarray(cols, dtype=np.int64)
            assert cols.size < 2 or (np.diff(cols) > 0).all()
            bi.append(cols)
            bp.append(bp[-1] + cols.size)
    n_inner = max(ap[-1], 1)
    bp += [bp[-1]] * (n_inner + 1 - len(bp))
    return Struct(len(rows), n_inner, n_col, np.arange(ap[-1]), ap, np.concatenate(bi) if bi else np.zeros(0, np.int64), bp, idx, values)


def spread(P, n_col, m=16, g=4, lo=0, hi=None):
    """P products of one output row from m A elements: product i belongs to A element i % m and shares its column with the
    products of the other elements of its group of g (runs of g products, summed in A's order); the columns are spread evenly
    over [lo, hi)"""
    hi = n_col if hi is None else hi
    i = np.arange(P, dtype=np.int64)
    j, t = i % m, i // m
    d = t * (-(-m // g)) + j // g
    D = int(d.max()) + 1 if P else 1
    assert hi - lo >= D
    col = lo + d * (hi - lo) // D
    return [col[j == e] for e in range(m)]


def glue(*parts):
    """B rows of several `spread`s with ascending column ranges, A element by A element"""
    return [np.concatenate([p[e] for p in parts]) for e in range(len(parts[0]))]


FEW = (2, 3, 7, 40)        # the products of "the other rows"


def _few(n_col, m=16):
    return [spread(P, n_col, m) for P in FEW]


# ---- values --------------------------------------------------------------------------------------------------------------
REAL_TYPES = ("float32", "float64", "int32", "int64")
COMPLEX_TYPES = ("complex64", "complex128")


def pools_of(dtype):
    return {"f": ("exact", "ordered"), "i": ("exact", "wrap"), "c": ("exact", "ordered")}[np.dtype(dtype).kind]


def pool_values(pool, dtype, n, rng):
    dt = np.dtype(dtype)
    if pool == "exact":
        v = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), size=n).astype(dt)
        return v + (1j * rng.choice(np.array([-2, -1, 0, 1, 2]), size=n)).astype(dt) if dt.kind == "c" else v
    if pool == "ordered":
        def draw():
            return rng.standard_normal(n) * 2.0 ** rng.integers(-8, 9, size=n)
        return (draw() + 1j * draw()).astype(dt) if dt.kind == "c" else draw().astype(dt)
    assert pool == "wrap" and dt.kind == "i"
    top = np.iinfo(dt).max // 4
    return (rng.choice(np.array([-1, 1]), size=n) * (top - rng.integers(0, 1000, size=n))).astype(dt)


def operands(st, pool, dtype, seed=0):
    """((a_data, a_indices, a_indptr), (b_data, b_indices, b_indptr)) in the structure's index types"""
    dt = np.dtype(dtype)
    if st.values is not None:
        assert pool == "zeros"
        va, vb = (np.asarray(v).astype(dt) for v in st.values(dt))
    else:
        rng = np.random.default_rng(seed)
        va, vb = pool_values(pool, dt, st.ai.size, rng), pool_values(pool, dt, st.bi.size, rng)
    t = st.idx
    return (va, st.ai.astype(t[0]), st.ap.astype(t[1])), (vb, st.bi.astype(t[2]), st.bp.astype(t[3]))


def reverse_a_rows(A):
    """the same A with the elements of every row in the opposite order"""
    ad, ai, ap = A
    ad, ai = ad.copy(), ai.copy()
    for r in range(ap.size - 1):
        ad[ap[r]:ap[r + 1]], ai[ap[r]:ap[r + 1]] = ad[ap[r]:ap[r + 1]][::-1].copy(), ai[ap[r]:ap[r + 1]][::-1].copy()
    return ad, ai, ap


def zeros_struct(n_col, filler=0):
    """the `zeros` pool: one scenario per row (column c of scenario s: spread over the columns), then `filler` plain rows"""
    def tiny(dt):
        real = np.dtype(f"f{dt.itemsize // 2}") if dt.kind == "c" else dt
        return 1e-200 if real.itemsize == 8 else 1e-30

    c = [k * (n_col - 1) // 11 for k in range(12)]
    scen = [                                                       # [(A value, [(column, B value)])] per A element
        ("a stored +0.0 times a negative value: a lone -0.0", [(0.0, [(c[1], -2.0)])]),
        ("an underflow: a lone -0.0", [("-tiny", [(c[2], "tiny")])]),
        ("a run whose products are all -0.0", [(0.0, [(c[3], -1.0)]), ("-tiny", [(c[3], "tiny")]), (-0.0, [(c[3], 5.0)])]),
        ("x + (-x)", [(1.5, [(c[4], 2.0)]), (-1.5, [(c[4], 2.0)])]),
        ("inf * 0 in one element only", [(np.inf, [(c[0], 0.0), (c[5], 1.0)]), (2.0, [(c[6], 3.0)])]),
        ("a stored -0.0 operand", [(-0.0, [(c[7], 3.0), (c[8], -3.0)])]),
        ("-0.0 first, then a value; a value, then -0.0", [(0.0, [(c[9], -1.0), (c[10], 4.0)]), (2.0, [(c[9], 1.25), (c[10], -0.0)])]),
        ("-0.0 + (+0.0)", [(0.0, [(c[11], -1.0)]), (0.0, [(c[11], 1.0)])]),
    ]
    rows = [[np.array([col for col, _ in el]) for _, el in s[1]] for s in scen] + [spread(P, n_col, 4) for P in (5, 9, 33)][:filler]

    def values(dt):
        t = tiny(dt)
        val = lambda v: {"tiny": t, "-tiny": -t}.get(v, v) if isinstance(v, str) else v
        va = [val(a) for s in scen for a, _ in s[1]]
        vb = [val(b) for s in scen for _, el in s[1] for _, b in el]
        nfa, nfb = sum(len(r) for r in rows[len(scen):]), sum(len(x) for r in rows[len(scen):] for x in r)
        return np.array(va + [1.5] * nfa), np.array(vb + [-2.0] * nfb)

    return assemble(n_col, rows, values=values)


# ---- the host's route rules ----------------------------------------------------------------------------------------------
DEFAULT_SWITCHES = {"SPGEMM_ROW_LOCAL": True, "SPGEMM_SMALL": True, "SPGEMM_SMALL_SECOND": True, "SPGEMM_BITMAP": True,
                    "SPGEMM_SMALL_MAX_CELLS": SMALL_MAX_CELLS, "SPGEMM_SMALL_MAX_NNZ": SMALL_MAX_NNZ}


def mostly_heavy(st, vb):
    """the bucket path's own decline: rows above the capacity (by their products or by their A elements) that are more than
    a quarter of the rows or hold more than three quarters of the products, or a row heavy by its A elements alone"""
    cap = bounds(st.key_bytes, vb)[4]
    by_prod, by_a = st.prod > cap, st.alen > cap
    heavy = by_prod | by_a
    return bool(heavy.any() and (heavy.sum() * 4 > st.n_row or int(st.prod[heavy].sum()) * 4 > int(st.prod.sum()) * 3 or (by_a & ~by_prod).any()))


def predict(st, dtype, switches):
    """(route, heavy_or_declined) of `_spgemm_rows` / `dot_csr_csr` by the rules of _kernels.py, the bitmap kernel switched off:
    route = small/first | small/second | buckets | global"""
    sw = dict(DEFAULT_SWITCHES, **switches)
    dt = np.dtype(dtype)
    vb = dt.itemsize
    cells, nnz_a, total = st.n_row * st.n_col, st.ai.size, int(st.prod.sum())
    if not sw["SPGEMM_ROW_LOCAL"]:
        return "global", None
    assert not sw["SPGEMM_BITMAP"], "the bitmap kernel's policy is not modelled here"
    fits = dt.kind != "c" and st.n_row > 0 and 0 < st.n_col <= sm_max_cols(vb, 1)
    if sw["SPGEMM_SMALL"] and cells <= sw["SPGEMM_SMALL_MAX_CELLS"] and nnz_a <= sw["SPGEMM_SMALL_MAX_NNZ"] and fits:
        return "small/first", 0
    if dt.kind == "c" or st.n_col >= N_COL_LIMIT or st.n_row == 0:
        return "global", None
    if sw["SPGEMM_SMALL"] and sw["SPGEMM_SMALL_SECOND"] and total and fits:
        fill = total / cells
        if fill >= 1.0 or (st.n_col <= sm_max_cols(vb, 4) and fill >= 0.25):
            return "small/second", 0
    kb = st.key_bytes
    cap = bounds(kb, vb)[4]
    by_prod, by_a = st.prod > cap, st.alen > cap
    if mostly_heavy(st, vb):
        return "global", None
    declined = [r for r in range(st.n_row) if not (by_prod[r] or by_a[r]) and not served(st.n_col, kb, vb, st.columns_of_row(r))]
    return "buckets", int((by_prod | by_a).sum()) + len(declined)


# ---- the table -----------------------------------------------------------------------------------------------------------
BUCKETS = {"SPGEMM_SMALL": False, "SPGEMM_BITMAP": False}
SMALL = {"SPGEMM_BITMAP": False}
SECOND = {"SPGEMM_BITMAP": False, "SPGEMM_SMALL_MAX_NNZ": 0}      # no first chance: the second one decides
GLOBAL = {"SPGEMM_ROW_LOCAL": False}
N32, N64 = 40009, 2 ** 28 + 9         # with A rows of at most 16 elements: 16 + 4 = 20 key bits | 29 + 4 = 33


class Case:
    """build(vb) -> Struct for values of vb bytes; `route` / `heavy` are what SPGEMM_STATS must say under `switches` (and
    `patch`, the other module values the case sets); `claims(st, vb)` yields (what, got, want) for tests/test_spgemm_cases.py;
    `group_reduce`: whether the grouped reduce must run (None: not observed)"""

    def __init__(self, build, route, switches, heavy=0, claims=None, dtypes=REAL_TYPES, pools=None, patch=None, group_reduce=None):
        self.build, self.route, self.switches, self.heavy, self.claims = build, route, switches, heavy, claims
        self.dtypes, self.pools, self.patch, self.group_reduce = dtypes, pools, patch or {}, group_reduce


CASES = {}


def _case(name, route, switches, **kw):
    def register(build):
        CASES[name] = Case(build, route, switches, **kw)
        return build
    return register


@functools.lru_cache(maxsize=None)
def case_struct(name, vb):
    return CASES[name].build(vb)


def _model(st, vb, r):
    return bucket_model(st.n_col, st.key_bytes, vb, st.columns_of_row(r))


# -- buckets: the row-class boundaries, per key width ------------------------------------------------------------------------
def boundary_products(kb, vb):
    c0, c1, c2, c3, c4 = bounds(kb, vb)
    return [0, 1, c0, c0 + 1, c1, c1 + 1, c2, c2 + 1] + ([c3, c3 + 1] if c3 > c2 else []) + [c4, c4 + 1]


def _classes(n_col, kb):
    def build(vb):
        rows = [spread(P, n_col) for P in boundary_products(kb, vb)]
        return assemble(n_col, rows[:6] + _few(n_col) + rows[6:] + [[]])

    def claims(st, vb):
        yield "key bytes", st.key_bytes, kb
        want = boundary_products(kb, vb)
        got = sorted(set(st.prod.tolist()) - set(FEW))
        yield "products of the boundary rows", got, want
        b = bounds(kb, vb)
        for r in range(st.n_row):
            P = int(st.prod[r])
            cls, big, in_pass = _model(st, vb, r)
            expect = None if P > b[4] else next(i for i, hi in enumerate(b) if P <= hi and not (i == 3 and b[3] == b[2]))
            yield f"class of the row with {P} products", cls, expect
            if cls is not None and P:
                yield f"{P} products: no bucket above 4", big <= 4, True
                yield f"{P} products: no pass above CAPP", in_pass <= capp(*row_classes(kb, vb)[cls][:3]), True
    return build, claims


for _name, _n, _kb in (("classes, u32 keys", N32, 4), ("classes, u64 keys", N64, 8)):
    _b, _c = _classes(_n, _kb)
    CASES[_name] = Case(_b, "buckets", BUCKETS, heavy=1, claims=_c)      # the row of c4 + 1 products: skipped and merged


def _max_prod_on(which, n_col, kb):
    def build(vb):
        top = bounds(kb, vb)[which]
        return assemble(n_col, [[]] + _few(n_col) + [spread(top, n_col), spread(top - 1, n_col), [], spread(1, n_col, 1)])

    def claims(st, vb):
        yield "key bytes", st.key_bytes, kb
        yield "max_prod", int(st.prod.max()), bounds(kb, vb)[which]
    return build, claims


for _which in range(5):
    for _n, _kb in ((N32, 4), (N64, 8)):
        _b, _c = _max_prod_on(_which, _n, _kb)
        CASES[f"max_prod = c{_which}, u{8 * _kb} keys"] = Case(_b, "buckets", BUCKETS, claims=_c)


# -- buckets: runs inside a bucket -------------------------------------------------------------------------------------------
RUNS_SERVED = (1, 4, 5, 8, 9, 16)


def _run_row(n_col, k, col, extra=()):
    """k products of column `col` (k A elements whose B rows hold it), every B row with one more column of its own in front"""
    return [np.array([3 + 2 * e, col] + list(extra)) for e in range(k)]


def _runs(ks, n_col):
    def build(vb):
        return assemble(n_col, [_run_row(n_col, k, n_col // 2 + 7 * i) for i, k in enumerate(ks)] + _few(n_col))

    def claims(st, vb):
        yield "key bytes", st.key_bytes, 4 if n_col == N32 else 8
        for i, k in enumerate(ks):
            cols = st.columns_of_row(i)
            yield f"row {i}: a run of {k}", int((cols == n_col // 2 + 7 * i).sum()), k
            yield f"row {i}: the largest bucket", _model(st, vb, i)[1], k
    return build, claims




def _two_columns(k1, k2, n_col):
    col = n_col // 3

    def build(vb):
        row = [np.array([col]) for _ in range(k1 - 2)] + [np.array([col, col + 1])] * 2 + [np.array([col + 1]) for _ in range(k2 - 2)]
        return assemble(n_col, [row] + _few(n_col))

    def claims(st, vb):
        cols = st.columns_of_row(0)
        yield "key bytes", st.key_bytes, 4 if n_col == N32 else 8
        yield "products of the two adjacent columns", ((cols == col).sum(), (cols == col + 1).sum()), (k1, k2)
        yield "one bucket holds both", _model(st, vb, 0)[1], k1 + k2
    return build, claims


for _n, _kb in ((N32, 4), (N64, 8)):
    _b, _c = _runs(RUNS_SERVED, _n)
    CASES[f"runs of 1, 4, 5, 8, 9, 16 in a bucket, u{8 * _kb} keys"] = Case(_b, "buckets", BUCKETS, claims=_c)
    _b, _c = _runs((17,), _n)
    CASES[f"a run of 17: declined, u{8 * _kb} keys"] = Case(_b, "buckets", BUCKETS, heavy=1, claims=_c)
    _b, _c = _two_columns(7, 9, _n)
    CASES[f"16 products of two adjacent columns in a bucket, u{8 * _kb} keys"] = Case(_b, "buckets", BUCKETS, claims=_c)
    _b, _c = _two_columns(8, 9, _n)
    CASES[f"17 products of two adjacent columns in a bucket, u{8 * _kb} keys"] = Case(_b, "buckets", BUCKETS, heavy=1, claims=_c)


# -- buckets: the pass capacity ----------------------------------------------------------------------------------------------
def _first_pass(cls_index, extra, n_col, kb):
    """a row of the class whose first pass holds CAPP + extra products"""
    def build(vb):
        cls = row_classes(kb, vb)[cls_index]
        cut, n = pass_start(n_col, cls, 1), capp(*cls[:3]) + extra
        P = (cls[3] + cls[4]) // 2
        return assemble(n_col, _few(n_col) + [glue(spread(n, n_col, hi=cut), spread(P - n, n_col, lo=cut))])

    def claims(st, vb):
        cls = row_classes(kb, vb)[cls_index]
        r = st.n_row - 1
        b = bucket_of(n_col, *cls[:3], st.columns_of_row(r))
        yield "key bytes", st.key_bytes, kb
        yield "the row's class", _model(st, vb, r)[0], cls_index
        yield "products of the first pass", int((b < nbp(*cls[:3])).sum()), capp(*cls[:3]) + extra
        yield "the first pass is the fullest", _model(st, vb, r)[2], capp(*cls[:3]) + extra
        yield "no bucket above 4", _model(st, vb, r)[1] <= 4, True
    return build, claims


for _ci, _n, _kb in ((2, N32, 4), (3, N32, 4), (4, N32, 4), (2, N64, 8), (4, N64, 8)):
    for _extra in (0, 1):
        _b, _c = _first_pass(_ci, _extra, _n, _kb)
        # (class 3 exists for 32-bit keys with 4-byte values only)
        CASES[f"class {_ci}, u{8 * _kb} keys: first pass of CAPP{' + 1' if _extra else ''}"] = Case(
            _b, "buckets", BUCKETS, heavy=_extra, claims=_c, dtypes=("float32", "int32") if _ci == 3 else REAL_TYPES)


@_case("every product in the last pass", "buckets", BUCKETS,
       claims=lambda st, vb: [("class", _model(st, vb, 0)[0], 2), ("per-pass count = the row", _model(st, vb, 0)[2], 4500),
                              ("the first column's pass", int(bucket_of(N32, 512, 16, 2, st.columns_of_row(0)).min()) // nbp(512, 16, 2), 1)])
def _(vb):
    cls = row_classes(4, vb)[2]
    assert cls[:3] == (512, 16, 2) and capp(*cls[:3]) >= 4500 > C1
    return assemble(N32, [spread(4500, N32, lo=pass_start(N32, cls, 1))] + _few(N32))


# -- buckets: key width, column limits -----------------------------------------------------------------------------------------
def _key_width(arow):
    n_col = 2 ** 27 - 1

    def build(vb):
        return assemble(n_col, [spread(3 * arow, n_col, arow)] + _few(n_col))
    return build, lambda st, vb: [("key bits", key_bits(st.n_col, st.max_arow), 32 if arow == 32 else 33), ("longest A row", st.max_arow, arow)]


for _arow in (32, 33):
    _b, _c = _key_width(_arow)
    CASES[f"key bits: n_col = 2^27 - 1, A row of {_arow}"] = Case(_b, "buckets", BUCKETS, claims=_c)


@_case("n_col = 2^31 - 2, the last column set", "buckets", BUCKETS,
       claims=lambda st, vb: [("last column", int(st.bi.max()), 2 ** 31 - 3), ("key bits", key_bits(st.n_col, st.max_arow), 32)])
def _(vb):
    n = 2 ** 31 - 2
    return assemble(n, [[np.array([0, 5, n - 1]), np.array([5, n - 2, n - 1])], [np.array([n - 1])], [], [np.array([0]), np.array([0, 1])]])


@_case("n_col = 2^31 - 1: declined, the global form answers", "global", BUCKETS,
       claims=lambda st, vb: [("n_col", st.n_col, N_COL_LIMIT)])
def _(vb):
    n = 2 ** 31 - 1
    return assemble(n, [[np.array([0, 5, n - 1]), np.array([5, n - 2, n - 1])], [np.array([n - 1])], [], [np.array([0]), np.array([0, 1])]])


# -- buckets: A rows at the capacity, the fall-back rule -------------------------------------------------------------------------
def _long_a_row(extra):
    def build(vb):
        n = bounds(4, vb)[4] + extra
        lens = (np.arange(n) % 7 == 0).astype(np.int64)                  # every seventh B row holds one element
        bi = np.arange(int(lens.sum()), dtype=np.int64) * (N32 // int(lens.sum()))          # (columns spread out: no full bucket)
        ap = [0, 2, 2 + n, 4 + n]
        ai = np.concatenate([[0, 7], np.arange(n), [14, 21]])
        return Struct(3, n, N32, ai, ap, bi, np.concatenate([[0], np.cumsum(lens)]))

    def claims(st, vb):
        yield "key bytes", st.key_bytes, 4
        yield "longest A row", st.max_arow, bounds(4, vb)[4] + extra
        yield "its products stay below the capacity", int(st.prod.max()) <= bounds(4, vb)[4], True
    return build, claims


def _staged(vb):
    """A rows of exactly STAGE and STAGE + 1 elements of classes 0 and 1, every element with products: full staging chunks
    whose LAST element has products, and a second chunk of one element"""
    rows = [spread(C0, N32, 1024, 1), spread(1025, N32, 1025, 1), spread(C1, N32, 2048, 1), spread(2049 + 1000, N32, 2049, 1)]
    return assemble(N32, _few(N32) + rows + [[]])


def _staged_claims(st, vb):
    rows = range(len(FEW), len(FEW) + 4)
    yield "A rows", [int(st.alen[r]) for r in rows], [stage(256, 4, 1), stage(256, 4, 1) + 1, stage(512, 8, 1), stage(512, 8, 1) + 1]
    yield "classes", [_model(st, vb, r)[0] for r in rows], [0, 1, 1, 1]
    yield "every element has products", all(int(st.blen[st.ai[st.ap[r]:st.ap[r + 1]]].min()) >= 1 for r in rows), True


CASES["A rows of STAGE and STAGE + 1 elements, all with products"] = Case(_staged, "buckets", BUCKETS, claims=_staged_claims)
_b, _c = _long_a_row(0)
CASES["an A row of cap elements"] = Case(_b, "buckets", BUCKETS, claims=_c)
_b, _c = _long_a_row(1)
CASES["an A row of cap + 1 elements: the whole product falls back"] = Case(_b, "global", BUCKETS, claims=_c)


def _heavy_rows(n_heavy, others, empty=0):
    """n_heavy rows of c4 + 1 products among rows with `others(H)` products, then `empty` empty rows"""
    def build(vb):
        H = bounds(4, vb)[4] + 1
        rows = [spread(P, N32) for P in others(H)]
        rows[1:1] = [spread(H, N32) for _ in range(n_heavy)]
        return assemble(N32, rows + [[]] * empty)
    return build


CASES["n_heavy * 4 == n_row: row-local"] = Case(_heavy_rows(1, lambda H: (C1, C1 + 5, C1)), "buckets", BUCKETS, heavy=1,
                                              claims=lambda st, vb: [("n_heavy * 4, n_row", (int((st.prod > bounds(4, vb)[4]).sum()) * 4, st.n_row), (4, 4))])
CASES["n_heavy * 4 > n_row: falls back"] = Case(_heavy_rows(2, lambda H: (2 * C1, 2 * C1, 2 * C1, 9, 9)), "global", BUCKETS,
                                                claims=lambda st, vb: [("n_heavy * 4, n_row", (int((st.prod > bounds(4, vb)[4]).sum()) * 4, st.n_row), (8, 7))])


def _heavy_share(minus):
    """one heavy row of H products (H the smallest multiple of 3 above c4) among 8 rows: heavy * 4 == total * 3 when the others
    hold H / 3 products together"""
    def heavy_of(vb):
        c4 = bounds(4, vb)[4]
        return c4 + 3 - c4 % 3

    def build(vb):
        H = heavy_of(vb)
        rest = H // 3 - minus
        parts = [rest // 4, rest // 4, rest // 4, rest - 3 * (rest // 4)]
        return assemble(N32, [spread(parts[0], N32), [], spread(H, N32)] + [spread(P, N32) for P in parts[1:]] + [[], []])

    def claims(st, vb):
        H = heavy_of(vb)
        yield "rows", st.n_row, 8
        yield "the heavy row", int(st.prod.max()), H
        yield "heavy * 4 - total * 3", H * 4 - int(st.prod.sum()) * 3, 3 * minus
    return build, claims


_b, _c = _heavy_share(0)
CASES["heavy products * 4 == total * 3: row-local"] = Case(_b, "buckets", BUCKETS, heavy=1, claims=_c)
_b, _c = _heavy_share(1)
CASES["heavy products * 4 > total * 3: falls back"] = Case(_b, "global", BUCKETS, claims=_c)

CASES["empty A rows around a heavy row"] = Case(
    lambda vb: assemble(N32, [spread(C1, N32), [], [], spread(bounds(4, vb)[4] + 1, N32), [], []] + [spread(C1, N32)] * 2 + [[]] * 4),
    "buckets", BUCKETS, heavy=1, claims=lambda st, vb: [("the rows around the heavy one are empty", st.alen[[1, 2, 4, 5]].tolist(), [0] * 4)])
CASES["an empty B"] = Case(lambda vb: Struct(5, 7, N32, [0, 3, 6, 2], [0, 2, 2, 3, 4, 4], [], [0] * 8), "buckets", BUCKETS,
                           claims=lambda st, vb: [("products", int(st.prod.sum()), 0), ("elements of A", st.ai.size, 4)])
CASES["an A whose every row is empty"] = Case(lambda vb: Struct(5, 3, N32, [], [0] * 6, [1, 4, 9, 4], [0, 2, 3, 4]), "buckets", BUCKETS,
                                              claims=lambda st, vb: [("elements of A", st.ai.size, 0)])
CASES["n_row = 1"] = Case(lambda vb: assemble(N32, [spread(C0 + 1, N32)]), "buckets", BUCKETS,
                          claims=lambda st, vb: [("rows", st.n_row, 1), ("class", _model(st, vb, 0)[0], 1)])
for _i, _idx in enumerate((("int32", "int64", "int32", "int64"), ("int64", "int32", "int32", "int32"), ("int32",) * 4)):
    CASES[f"index types {'/'.join(t[3:] for t in _idx)}"] = Case(
        functools.partial(lambda idx, vb: assemble(N32, _few(N32) + [spread(C0 + 1, N32), [], spread(C1 + 1, N32)], idx=idx), _idx),
        "buckets", BUCKETS, claims=lambda st, vb: [("classes", sorted({_model(st, vb, r)[0] for r in range(st.n_row)}), [0, 1, 2])])


# -- the small kernel ------------------------------------------------------------------------------------------------------------
def _random_struct(n_row, n_inner, n_col, a_len, b_len, seed, ends=True, idx=("int64",) * 4):
    """A rows of a_len(r) distinct B rows, B rows of b_len(k) distinct columns; `ends`: B row 0 holds columns 0 and n_col - 1
    and every A row begins with it"""
    rng = np.random.default_rng(seed)
    bi, bp = [], [0]
    for k in range(n_inner):
        n = min(b_len(k) if callable(b_len) else b_len, n_col)
        cols = np.sort(rng.choice(n_col, size=n, replace=False)) if n < n_col else np.arange(n_col)
        if ends and k == 0:
            cols = np.unique(np.concatenate([[0, n_col - 1], cols]))
        bi.append(cols)
        bp.append(bp[-1] + cols.size)
    ai, ap = [], [0]
    for r in range(n_row):
        n = min(a_len(r) if callable(a_len) else a_len, n_inner)
        e = np.sort(rng.choice(n_inner, size=n, replace=False))
        if ends and n:
            e = np.unique(np.concatenate([[0], e]))[:n]
        ai.append(e)
        ap.append(ap[-1] + e.size)
    return Struct(n_row, n_inner, n_col, np.concatenate(ai) if ai else [], ap, np.concatenate(bi), bp, idx)


def _ends_claims(st, vb):
    r = next(r for r in range(st.n_row) if st.alen[r])
    cols = st.columns_of_row(r)
    yield "result columns 0 and n_col - 1 of a row", (int(cols.min()), int(cols.max())), (0, st.n_col - 1)


def _small_cols(waves, extra):
    def build(vb):
        return _random_struct(6, 40, sm_max_cols(vb, waves) + extra, lambda r: (0, 5, 9, 1, 7, 3)[r], lambda k: 10 + 20 * (k % 4), 11)

    def claims(st, vb):
        yield "n_col", st.n_col, {(4, 4): 3964, (8, 4): 2012, (4, 1): 15879, (8, 1): 8062}[(vb, waves)] + extra
        yield from _ends_claims(st, vb)
    return build, claims


for _waves in (4, 1):
    for _extra in (0, 1):
        _b, _c = _small_cols(_waves, _extra)
        _leaves = _waves == 1 and _extra == 1
        CASES[f"small: n_col = sm_max_cols({_waves}){' + 1' if _extra else ''}"] = Case(
            _b, "buckets" if _leaves else "small/first", SMALL, claims=_c)

for _n in (1, 31, 32, 33, 2048, 2049):
    CASES[f"small: n_col = {_n}"] = Case(
        functools.partial(lambda n, vb: _random_struct(7, 30, n, lambda r: 2 + 3 * (r % 3), lambda k: 1 + k % 5 + (n // 3) * (k % 2), 20 + n), _n),
        "small/first", SMALL, claims=_ends_claims)
for _n in (1, 3, 4, 5):
    CASES[f"small: n_row = {_n}"] = Case(functools.partial(lambda n, vb: _random_struct(n, 20, 300, 6, 25, 40 + n), _n), "small/first", SMALL,
                                         claims=lambda st, vb: [("rows", st.n_row in (1, 3, 4, 5), True)])
for _n in (63, 64, 65):
    CASES[f"small: A rows of {_n}"] = Case(functools.partial(lambda n, vb: _random_struct(5, 90, 500, n, 12, 50 + n), _n), "small/first", SMALL,
                                           claims=functools.partial(lambda n, st, vb: [("A rows", set(st.alen.tolist()), {n})], _n))
    CASES[f"small: B rows of {_n}"] = Case(functools.partial(lambda n, vb: _random_struct(5, 30, 700, 7, n, 60 + n, ends=False), _n), "small/first", SMALL,
                                           claims=functools.partial(lambda n, st, vb: [("B rows", set(st.blen.tolist()), {n})], _n))
CASES["small: a fully dense result row"] = Case(
    lambda vb: _random_struct(5, 12, 333, lambda r: 12 if r == 2 else 3, lambda k: 333 if k in (4, 9) else 20, 70), "small/first", SMALL,
    claims=lambda st, vb: [("distinct columns of row 2", np.unique(st.columns_of_row(2)).size, st.n_col)])


def _cells(extra):
    def build(vb):
        st = _random_struct(8, 16, 4096, 3, 30, 80)
        n_row = 1024 + extra
        return Struct(n_row, 16, 4096, st.ai, np.concatenate([st.ap, np.full(n_row - 8, st.ap[-1])]), st.bi, st.bp)
    return build, lambda st, vb: [("cells - SPGEMM_SMALL_MAX_CELLS", st.n_row * st.n_col - SMALL_MAX_CELLS, extra * 4096)]


def _nnz(extra):
    def build(vb):
        n = 256                                                   # 256 rows of 256 elements (+ one), every B row one element
        ai = np.concatenate([np.tile(np.arange(n), n), np.arange(extra)])
        return Struct(n + 1, n + 1, 64, ai, np.concatenate([np.arange(n + 1) * n, [n * n + extra]]), np.arange(n + 1) % 64, np.arange(n + 2))
    return build, lambda st, vb: [("elements of A - SPGEMM_SMALL_MAX_NNZ", st.ai.size - SMALL_MAX_NNZ, extra)]


for _extra in (0, 1):
    _b, _c = _cells(_extra)
    CASES[f"small: first chance, cells = 2^22{' + 4096' if _extra else ''}"] = Case(_b, "buckets" if _extra else "small/first", SMALL, claims=_c)
    _b, _c = _nnz(_extra)
    CASES[f"small: first chance, nnz = 2^16{' + 1' if _extra else ''}"] = Case(
        _b, "buckets" if _extra else "small/first", dict(SMALL, SPGEMM_SMALL_SECOND=False), claims=_c)


def _fill_one(minus):
    def build(vb):
        rows = [[np.arange(100 * e, 100 * e + 100) for e in range(60)] for _ in range(4)]
        rows[2] = rows[2][:59] + [np.arange(5900, 6000 - minus)]
        return assemble(6000, rows)
    return build, lambda st, vb: [("n_row * n_col - products", st.n_row * st.n_col - int(st.prod.sum()), minus),
                                  ("more columns than four waves take", st.n_col > sm_max_cols(vb, 4), True)]


def _fill_quarter(minus):
    def build(vb):
        n = sm_max_cols(vb, 4)
        return assemble(n, [[], [np.arange(e, n, 4)[:None if e != 1 or not minus else -1] for e in range(4)], [], []])
    return build, lambda st, vb: [("n_row * n_col - 4 * products", st.n_row * st.n_col - 4 * int(st.prod.sum()), 4 * minus),
                                  ("n_col == four_waves", st.n_col, sm_max_cols(vb, 4))]


for _minus in (0, 1):
    _b, _c = _fill_one(_minus)
    CASES[f"small: second chance, fill {'< 1' if _minus else '== 1'}"] = Case(_b, "buckets" if _minus else "small/second", SECOND, claims=_c)
    _b, _c = _fill_quarter(_minus)
    CASES[f"small: second chance, fill {'< 1/4' if _minus else '== 1/4'} at n_col = four_waves"] = Case(
        _b, "buckets" if _minus else "small/second", SECOND, claims=_c)


# -- the global form ---------------------------------------------------------------------------------------------------------
CHUNK = 64
ALL_TYPES = REAL_TYPES + COMPLEX_TYPES


def _chunks(products):
    def build(vb):
        return assemble(N32, [spread(P, N32, 8) if P else [] for P in products])
    return build, lambda st, vb: [("products per row", st.prod.tolist(), list(products))]


for _name, _products in (("rows of 63, 64, 65 around empty rows", (63, 0, 64, 0, 0, 65, 1, 63, 1, 0, 64)),
                         ("a first and a last row above the chunk", (200, 3, 0, 61, 3, 0, 65, 200)),
                         ("empty rows at the ends", (0, 0, 64, 64, 0, 63, 2, 0))):
    _b, _c = _chunks(_products)
    CASES[f"global, chunks of 64: {_name}"] = Case(_b, "global", GLOBAL, claims=_c, dtypes=ALL_TYPES, patch={"SPGEMM_CHUNK_PRODUCTS": CHUNK})


def _long_run(n):
    """sorted products: 1025 single ones (row 0), then ONE element of n products (row 1), then 6000 more"""
    def build(vb):
        run = [np.array([77]) for _ in range(n)]
        return assemble(N32, [spread(LONG_RUN_WINDOW + 1, N32, 16, 1), run] + [spread(2000, N32, 16, 1) for _ in range(3)])

    def claims(st, vb):
        x = Expanded(st.n_row, st.n_col, (np.ones(st.ai.size), st.ai, st.ap), (np.ones(st.bi.size), st.bi, st.bp))
        i = int(np.argmax(x.length))
        yield "products", x.rows.size >= RUN_PROBE_MIN, True
        yield "products that share their element with an earlier one", x.rows.size - x.start.size >= RUN_DUPS_MIN, True
        yield "the longest element", int(x.length[i]), n
        yield "it begins one past an aligned window start", int(x.start[i]) % LONG_RUN_WINDOW, 1
        head = np.zeros(x.rows.size, dtype=bool)
        head[x.start] = True
        nw = x.rows.size // LONG_RUN_WINDOW
        without = int((~head[:nw * LONG_RUN_WINDOW].reshape(nw, LONG_RUN_WINDOW).any(axis=1)).sum())
        yield "aligned windows without a head", without, 1 if n == 2 * LONG_RUN_WINDOW - 1 else 0
    return build, claims


for _n in (2 * LONG_RUN_WINDOW - 1, 2 * LONG_RUN_WINDOW - 2):
    _b, _c = _long_run(_n)
    CASES[f"global: an element of {_n} products"] = Case(_b, "global", GLOBAL, claims=_c, group_reduce=_n == 2 * LONG_RUN_WINDOW - 1)


# -- the zeros pool, on every route ------------------------------------------------------------------------------------------------
FLOATS = ("float32", "float64")
CASES["zeros: small"] = Case(lambda vb: zeros_struct(97, 3), "small/first", SMALL, dtypes=FLOATS, pools=("zeros",))
CASES["zeros: buckets"] = Case(lambda vb: zeros_struct(N32, 3), "buckets", BUCKETS, dtypes=FLOATS, pools=("zeros",))
CASES["zeros: buckets, a heavy row merged from the global form"] = Case(
    lambda vb: assemble(N32, [r for r in _zeros_rows(N32)] + [_run_row(N32, 17, 501)], values=_zeros_values(N32, 17)),
    "buckets", BUCKETS, heavy=1, dtypes=FLOATS, pools=("zeros",))
CASES["zeros: global"] = Case(lambda vb: zeros_struct(N32, 3), "global", GLOBAL, dtypes=FLOATS + COMPLEX_TYPES, pools=("zeros",))
CASES["zeros: global, chunks of 64"] = Case(lambda vb: zeros_struct(N32, 3), "global", GLOBAL, dtypes=FLOATS + COMPLEX_TYPES, pools=("zeros",),
                                            patch={"SPGEMM_CHUNK_PRODUCTS": CHUNK})


def _zeros_rows(n_col):
    st = zeros_struct(n_col)
    return [[st.bi[st.bp[k]:st.bp[k + 1]] for k in st.ai[st.ap[r]:st.ap[r + 1]]] for r in range(st.n_row)]


def _zeros_values(n_col, k):
    """the zeros scenarios' values, then a declined row: k products -0.0 of one column behind k positive ones of others"""
    inner = zeros_struct(n_col).values

    def values(dt):
        va, vb = inner(dt)
        return np.concatenate([va, np.zeros(k)]), np.concatenate([vb, np.tile([1.0, -1.0], k)])
    return values


def slug(name):
    """a case's name as a test id: letters, digits and underscores only"""
    for sign, word in (("==", " eq "), ("<", " lt "), (">", " gt "), ("+", " plus "), ("^", "pow"), ("/", " by "), ("=", " is ")):
        name = name.replace(sign, word)
    return re.sub(r"[^A-Za-z0-9]+", "_", name).strip("_")


assert len({slug(n) for n in CASES}) == len(CASES)

# the smallest case of every route with float32 values, by the stored elements of A and B (the first of the table on a tie;
# `buckets` with no row and with a row left to the global form): what the C-ABI calls of one product are counted on
SMALLEST = {"small/first": "small: n_col = 1", "small/second": "small: second chance, fill == 1/4 at n_col = four_waves",
            "buckets": "an empty B", "buckets/heavy": "zeros: buckets, a heavy row merged from the global form",
            "global": "n_col = 2^31 - 1: declined, the global form answers"}


def smallest_cases():
    """the same, worked out from the table"""
    best = {}
    for name, c in CASES.items():
        if "float32" in c.dtypes:
            st = case_struct(name, 4)
            key = "buckets/heavy" if c.route == "buckets" and c.heavy else c.route
            if key not in best or st.ai.size + st.bi.size < best[key][0]:
                best[key] = (st.ai.size + st.bi.size, name)
    return {key: name for key, (_, name) in best.items()}


def runs():
    """every (case, dtype) of the table: one GPU test each, over the pools of `calls`"""
    return [(name, dt) for name, c in CASES.items() for dt in c.dtypes]


def calls(names=None):
    """every (case, dtype, pool) of the table"""
    return [(name, dt, pool) for name, c in CASES.items() if names is None or name in names
            for dt in c.dtypes for pool in (c.pools or pools_of(dt))]


@functools.lru_cache(maxsize=4)
def case_operands(name, dtype, pool):
    A, B = operands(case_struct(name, value_bytes(dtype)), pool, dtype, seed=len(name))
    for a in A + B:
        a.setflags(write=False)
    return A, B


def value_bytes(dtype):
    """the value size the case is built for: the real types' own; complex values take the global form, where it decides nothing"""
    dt = np.dtype(dtype)
    return dt.itemsize // 2 if dt.kind == "c" else dt.itemsize


@functools.lru_cache(maxsize=4)
def case_reference(name, dtype, pool):
    """(data, indices, indptr, Expanded), read-only"""
    st = case_struct(name, value_bytes(dtype))
    A, B = case_operands(name, dtype, pool)
    x = Expanded(st.n_row, st.n_col, A, B)
    out = spgemm_ref(st.n_row, st.n_col, A, B, x)
    for a in out:
        a.setflags(write=False)
    return (*out, x)

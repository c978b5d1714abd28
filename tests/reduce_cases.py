"""Cases for the grouped reduce (csrc/group_reduce.hip, `spamd_segment_reduce`): run layouts aimed at the kernel's
units, keys, data whose expected result is exact in ANY association, and host references.  No GPU, no package import.

A layout is `(heads, n)`: the sorted positions where a run starts (always containing 0) and the number of elements.
The kernel's units are 4 elements per thread, 256 per wave, TILE = 2048 per workgroup, and WALK = 32 head-less tiles:
the longest stretch the fast fix-up walks back over before the chained fix-up takes everything.
"""
import math

import numpy as np

ITEMS, WAVE, TILE, WALK = 4, 256, 2048, 32
EDGE_POSITIONS = (255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)

INT_DTYPES = (np.int32, np.int64)
FLOAT_DTYPES = (np.float32, np.float64)
REAL_DTYPES = INT_DTYPES + FLOAT_DTYPES
# the table: every (op, value dtype) whose expected result is compared exactly
TABLE = ([("add", dt) for dt in REAL_DTYPES] + [("multiply", dt) for dt in REAL_DTYPES]
         + [(op, dt) for op in ("maximum", "minimum", "fmax", "fmin") for dt in REAL_DTYPES]
         + [("logical_or", np.uint8), ("logical_and", np.uint8)])
UFUNC = {"add": np.add, "multiply": np.multiply, "maximum": np.maximum, "minimum": np.minimum, "fmax": np.fmax,
         "fmin": np.fmin, "logical_or": np.logical_or, "logical_and": np.logical_and}


# ---- layouts -------------------------------------------------------------------------------------------------------
def _from_lengths(lengths, n):
    """heads of consecutive runs of the given lengths, cut (or the last run extended) to end at n"""
    heads = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    return np.unique(heads[heads < n]), int(n)


def _short_runs(lo, hi, rng):
    """heads of runs of 1..9 elements that fill [lo, hi), the first at lo"""
    if hi <= lo:
        return np.zeros(0, dtype=np.int64)
    h = lo + np.concatenate([[0], np.cumsum(rng.integers(1, 10, size=hi - lo))])
    return h[h < hi].astype(np.int64)


def _thread():
    n = 3 * TILE + 3
    heads, n = _from_lengths(np.resize(np.arange(1, 10), n), n)
    assert set((heads % ITEMS).tolist()) == {0, 1, 2, 3}
    return heads, n


def _edges(rng):
    n = EDGE_POSITIONS[-1] + 40
    parts, lo = [], 0
    for p in EDGE_POSITIONS + (n,):
        parts.append(_short_runs(lo, p, rng))       # a run ends at p - 1 ...
        lo = p                                      # ... and the next starts at p
    heads = np.unique(np.concatenate(parts))
    assert all(p in heads for p in EDGE_POSITIONS)
    return heads, n


def _singles_at_edge():
    heads = np.unique(np.concatenate([np.arange(0, 2047, 300), [2047, 2048, 2049, 2050], np.arange(2400, 3000, 300)]))
    return heads.astype(np.int64), 3000


def _tile_exact(n):
    return np.arange(0, n, TILE, dtype=np.int64), int(n)


def _walk(w, rng, tail=TILE + 3):
    """short runs, a head at the LAST element of tile 0, exactly `w` head-less tiles, a head at the FIRST element of tile
    w + 1, short runs to the end"""
    after = (w + 1) * TILE
    heads = np.concatenate([_short_runs(0, TILE - 1, rng), [TILE - 1], _short_runs(after, after + tail, rng)])
    return heads.astype(np.int64), after + tail


def _walk_mixed(rng):
    h1, n1 = _walk(33, rng, tail=TILE)           # ends on a tile boundary: the edge positions keep their place in a tile
    h2, n2 = _edges(rng)
    return np.concatenate([h1, h2 + n1]), n1 + n2


def _open_end(n, rng):
    last = n - 3 * TILE - 5                      # the last run covers the final 3 tiles (and 5 elements more)
    return np.concatenate([_short_runs(0, last, rng), [last]]).astype(np.int64), int(n)


def layouts():
    """name -> (heads, n), the same arrays on every call"""
    rng = np.random.default_rng(20240607)
    out = {"thread": _thread(), "edges": _edges(rng), "singles_at_edge": _singles_at_edge()}
    for n in (5 * TILE - 1, 5 * TILE, 5 * TILE + 1):
        out[f"tile_exact_{n}"] = _tile_exact(n)
    out["all_heads"] = (np.arange(3 * TILE + 3, dtype=np.int64), 3 * TILE + 3)
    for w in (WALK - 1, WALK, WALK + 1):
        out[f"walk_{w}"] = _walk(w, rng)
    out["walk_mixed"] = _walk_mixed(rng)
    for n in (4 * TILE, 4 * TILE + 1, 4 * TILE + 2, 4 * TILE - 1):      # n % 2048 in {0, 1, 2, 2047}, n % 4 in {0, 1, 2, 3}
        out[f"open_end_{n}"] = _open_end(n, rng)
    for n in range(1, 6):
        out[f"tiny_one_run_{n}"] = (np.zeros(1, dtype=np.int64), n)
        out[f"tiny_all_heads_{n}"] = (np.arange(n, dtype=np.int64), n)
    for name, (heads, n) in out.items():
        check_layout(heads, n)
        out[name] = (heads.astype(np.int64), int(n))
    return out


def check_layout(heads, n):
    assert n >= 1 and heads[0] == 0 and heads[-1] < n and np.all(np.diff(heads) > 0)


def run_lengths(heads, n):
    return np.diff(np.concatenate([heads, [n]])).astype(np.int64)


def run_of(heads, n):
    """index of the run each element belongs to"""
    return np.repeat(np.arange(len(heads), dtype=np.int64), run_lengths(heads, n))


def pad_to_quotient(heads, n, q):
    """(heads, n) with one-element runs appended until n // runs == q exactly (the quotient `spamd_segment_reduce`
    chooses its kernel by); the layout must start above q"""
    assert n // len(heads) >= q
    add = 0
    while (n + add) // (len(heads) + add) > q:
        add += 1
    heads, n = np.concatenate([heads, n + np.arange(add, dtype=np.int64)]), n + add
    assert n // len(heads) == q, (n, len(heads), q)
    check_layout(heads, n)
    return heads, int(n)


# ---- keys ----------------------------------------------------------------------------------------------------------
def make_keys(heads, n, divisor, rng, first_gid=0):
    """key = gid * divisor + j: gids increase from run to run with random gaps, j increases strictly inside a run and
    stays below the divisor (divisor 1: every key of a run is the same).  Returns (keys, gids of the runs)."""
    lens = run_lengths(heads, n)
    gids = first_gid + np.cumsum(rng.integers(1, 4, size=len(heads))) - 1
    pos = np.arange(n, dtype=np.int64) - np.repeat(heads, lens)
    if divisor == 1:
        j = np.zeros(n, dtype=np.int64)
    else:
        assert lens.max() <= divisor, "a run longer than the divisor has no strictly increasing j"
        j = pos + np.repeat((rng.random(len(heads)) * (divisor - lens + 1)).astype(np.int64), lens)
    assert int(gids[-1]) * divisor + divisor - 1 < 2 ** 62
    keys = np.repeat(gids, lens) * np.int64(divisor) + j
    assert np.all(np.diff(keys) >= 0) and np.all(j < divisor)
    return keys.astype(np.int64), gids.astype(np.int64)


RANGE_DIVISORS = (1, 3, 141, 2 ** 31 - 1, 2 ** 31, 10 ** 12 + 39)


def d_estimate(k, divisor):
    """the double-precision id path's first guess: floor((double)k * (1 / d)), before its one correction"""
    return np.floor(k.astype(np.float64) * (1.0 / float(divisor))).astype(np.int64)


def range_keys(heads, n, divisor, top, rng):
    """Sorted keys below `top` (at most 2^62) for the id arithmetic at range: consecutive group ids q - 1, q, q + 1 whose
    runs begin with j = 0 and end with j = divisor - 1, so that the keys q d - 1, q d and q d + 1 meet at run boundaries;
    ids at the bottom of the range, at its very top, and at quotients where the double-precision guess for q d is one too
    small or the one for q d - 1 one too large (found by evaluating `d_estimate`).  Runs longer than the divisor repeat
    keys.  Returns (keys, number of keys whose guess is too small, too large) - the counts for keys below 2^53 only."""
    assert top <= 2 ** 62
    lens = run_lengths(heads, n)
    R = len(heads)
    qmax = top // divisor - 1                     # every key of group qmax is below top
    assert qmax >= R
    q = np.unique(np.concatenate([rng.integers(qmax // 2, qmax + 1, size=200_000), qmax - np.arange(0, 4096)]))
    q = q[q >= 1]
    low = q[d_estimate(q * divisor, divisor) < q][-60:]
    high = q[d_estimate(q * divisor - 1, divisor) > q - 1][-60:]
    special = np.concatenate([low, high])
    must = np.concatenate([[0, 1, 2], qmax - np.arange(300), special - 1, special, special + 1])
    must = np.unique(must[(must >= 0) & (must <= qmax)])
    pool = np.concatenate([rng.integers(0, qmax + 1, size=4 * R), rng.integers(max(0, qmax - 4 * R), qmax + 1, size=4 * R)])
    pool = np.setdiff1d(pool, must)
    assert 0 <= R - len(must) <= len(pool)
    gids = np.sort(np.concatenate([must, rng.choice(pool, R - len(must), replace=False)])).astype(np.int64)
    pos = np.arange(n, dtype=np.int64) - np.repeat(heads, lens)
    len_of = np.repeat(lens, lens)
    j = np.where(pos == len_of - 1, divisor - 1, np.minimum(pos, divisor - 1))       # 0, 1, 2, ..., divisor - 1
    j = np.where(len_of == 1, np.repeat(np.arange(R) % 2, lens) * (divisor - 1), j)   # one element: 0 or divisor - 1 in turn
    keys = np.repeat(gids, lens) * np.int64(divisor) + j
    assert int(keys.max()) < top and int(gids[-1]) == qmax and np.all(np.diff(keys) >= 0) and np.all((0 <= j) & (j < divisor))
    est = d_estimate(keys, divisor)
    true = keys // divisor
    return keys.astype(np.int64), int(np.sum(est < true)), int(np.sum(est > true))


# ---- data ----------------------------------------------------------------------------------------------------------
def exact_limit(dtype):
    """integers up to this magnitude are exact in `dtype`: 2^24 / 2^53"""
    return 2 ** (np.finfo(dtype).nmant + 1)


def make_data(op, dtype, heads, n, rng):
    """values for which `op` over every run has ONE result whatever the association (see the module docstring)"""
    dtype = np.dtype(dtype)
    lens = run_lengths(heads, n)
    runs = run_of(heads, n)
    if op in ("add", "multiply") and dtype.kind == "i":
        info = np.iinfo(dtype)
        v = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=dtype)        # the ring is associative
        # (factors are odd: units of the ring.  64 even factors wrap to 0, and a long run would then hide a lost element)
        return v | dtype.type(1) if op == "multiply" else v
    if op == "add":
        v = rng.integers(-8, 9, size=n).astype(dtype)
        assert_exact_sums(v, heads, n)
        return v
    if op == "multiply":
        # +-1 everywhere, about 30 twos and 30 halves in a run at the most
        p = np.repeat(np.minimum(0.2, 30.0 / lens), lens)
        pick = rng.random(n)
        v = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        v = np.where(pick < p, 2.0, np.where(pick > 1.0 - p, 0.5, v)).astype(dtype)
        assert_exact_products(v, heads, n)
        return v
    if op in ("maximum", "minimum", "fmax", "fmin"):
        v = (rng.permutation(n) - n // 2).astype(dtype)              # distinct: no ties, no +-0
        if dtype.kind == "f":
            v += dtype.type(0.5)
            nan_at = [heads[1::7], (heads[2::5] + lens[2::5] - 1), [p for p in (TILE - 1, TILE) if p < n]]
            if len(heads) > 3:
                r = len(heads) // 2                                    # one run of nothing but NaNs
                nan_at.append(np.arange(heads[r], heads[r] + lens[r]))
            v[np.concatenate(nan_at).astype(np.int64)] = np.nan
        return v
    if op in ("logical_or", "logical_and"):
        # a run holds an odd one out with probability 1/2; one run of only zeros and one of only ones
        p = np.repeat(1.0 - 0.5 ** (1.0 / lens), lens)
        odd = rng.random(n) < p
        if len(heads) > 2:
            odd[runs == len(heads) // 3] = False
            odd[runs == 2 * len(heads) // 3] = True
        return (odd if op == "logical_or" else ~odd).astype(np.uint8)
    raise ValueError(op)


def assert_exact_sums(v, heads, n):
    """every partial sum of a run is an integer below 2^24 / 2^53: exact in any association"""
    assert np.all(v == np.rint(v))
    assert np.add.reduceat(np.abs(v.astype(np.float64)), heads).max() < exact_limit(v.dtype), "a run's sum |v| is not exact"


def assert_exact_products(v, heads, n):
    """powers of two only, at most 100 twos and 100 halves in a run: every partial product is exact and in range"""
    a = np.abs(v)
    assert np.all((a == 1) | (a == 2) | (a == 0.5))
    assert np.add.reduceat((a == 2).astype(np.int64), heads).max() <= 100, "more than 100 twos in a run"
    assert np.add.reduceat((a == 0.5).astype(np.int64), heads).max() <= 100, "more than 100 halves in a run"


def rounding_data(dtype, n, rng):
    """real values of mixed sign for the rounding case of float add"""
    return (rng.random(n) * 2.0 - 1.0).astype(dtype)


# ---- references ----------------------------------------------------------------------------------------------------
def reference(op, data, heads, n):
    """np.<ufunc>.reduceat over the runs, in the value type (integers wrap)"""
    with np.errstate(all="ignore"):
        out = UFUNC[op].reduceat(data, heads)
    return out.astype(data.dtype)


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2.0


def gamma(k, dtype):
    """Higham's gamma_k = k u / (1 - k u)"""
    ku = k * unit_roundoff(dtype)
    assert ku < 1.0, "gamma_k is defined for k u < 1"
    return ku / (1.0 - ku)


def sum_bound(m, sum_abs, exact, dtype):
    """|computed - exact| for m terms added in ANY order in `dtype`: gamma_(m-1) * sum|v|, plus the rounding of the exact
    sum itself to the nearest `dtype` value (u |exact|) when anything was added at all"""
    if m <= 1:
        return 0.0
    return gamma(m - 1, dtype) * sum_abs + unit_roundoff(dtype) * abs(exact)


def accurate_sum(v):
    """the sum of a long array, correct to well below one rounding of a double: math.fsum (exact, rounded once) up to a few
    million elements; beyond, NumPy's pairwise sum in an extended type whose 64-bit mantissa leaves an error of about
    log2(n) * 2^-64 * sum|v| (fsum again where long double is no wider than double)"""
    if len(v) <= 5_000_000 or np.finfo(np.longdouble).nmant < 63:
        return math.fsum(v.tolist())
    return float(np.sum(v, dtype=np.longdouble))


def fsum_reference(data, heads, n):
    """per run: (the exact sum rounded once to double by math.fsum, the any-order bound of `sum_bound`)"""
    ends = np.concatenate([heads[1:], [n]])
    exact, bound = np.empty(len(heads)), np.empty(len(heads))
    for r, (a, b) in enumerate(zip(heads.tolist(), ends.tolist())):
        v = data[a:b].astype(np.float64).tolist()
        exact[r] = math.fsum(v)
        bound[r] = sum_bound(b - a, math.fsum(map(abs, v)), exact[r], data.dtype)
    return exact, bound


def sequential_reference(data, heads, n):
    """per run: the values added strictly left to right in the value type"""
    ends = np.concatenate([heads[1:], [n]])
    out = np.empty(len(heads), dtype=data.dtype)
    for r, (a, b) in enumerate(zip(heads.tolist(), ends.tolist())):
        acc = data[a]
        for x in data[a + 1:b]:
            acc = data.dtype.type(acc + x)
        out[r] = acc
    return out


def same_values(got, want):
    """equal element for element, NaNs in the same places"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if want.dtype.kind == "f":
        return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]))
    return bool(np.array_equal(got, want))

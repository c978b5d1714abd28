"""Cases for the merge-path union (csrc/merge.hip, csrc/merge_complex.hip behind `_umath.merge_union`) and the older
three-kernel union (csrc/ewise.hip behind `_umath.union_merge`): a plain NumPy reference, a second formulation of it, the
tile structure a correct merge path has, and a case table in which every case is built around one place where the tile logic
can be off by one.  No GPU, no torch, no package import.  Everything is integers and single IEEE operations on values that
are small integers (exact in every type): every comparison against these references is exact, bit for bit.

A merged sequence is written as TOKENS, one per distinct key:
    a   a key only in A (1 merged rank)        m   a key in both (2 ranks: the A item, then the B item - ties go A first)
    b   a key only in B (1 rank)               m0  a matched pair of stored zeros: its result is the fill value of `add` and
                                                   `multiply` with zero fills, so it is dropped there
so a case can put a token at an exact merged rank (`Seq`).  The boundaries the table is aimed at come from the constants
below; tests/test_merge_cases.py reads every one of them from the source text (`source_constants`), so a retune that moves
a boundary fails there instead of silently un-aiming the table:

  MP_THREADS x MP_VT = TILE   a tile of 4096 merged ranks, 1024 threads x 4 ranks, 16 waves of 256 ranks
  STORE_FACTOR                tiles with `tot * 4 >= TILE` outputs stage them in LDS, sparser tiles store from registers
  LOOKBACK_WINDOW             the look-back reads 64 predecessors per round trip
  MERGE_FUSED_MAX_ITEMS       up to 2^22 items the fused single launch, above it partition + single pass
  GRID_CAP x 256 = N1         ewise.hip's grid-stride loops take a second trip from element 1,048,576 on
"""
import functools
import os
import re

import numpy as np

MP_THREADS, MP_VT = 1024, 4
TILE = MP_THREADS * MP_VT
WAVE = 64
WAVE_RANKS = WAVE * MP_VT
STORE_FACTOR = 4                       # LDS route when tot * 4 >= TILE
LOOKBACK_WINDOW = 64
MERGE_FUSED_MAX_ITEMS = 1 << 22
GRID_CAP = 4096
N1 = GRID_CAP * 256
MAX_KEY = 2 ** 63 - 2                  # the largest linear location: the look-ahead sentinel is INT64_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_constants():
    """the same constants as the source files state them today"""
    def src(*parts):
        return open(os.path.join(ROOT, "sparse_amd", *parts)).read()

    def grab(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: `{pattern}` is gone from the source - move the cases of tests/merge_cases.py with it"
        return m

    merge, cmerge, common = src("csrc", "merge.hip"), src("csrc", "merge_complex.hip"), src("csrc", "common.h")
    ewise, umath = src("csrc", "ewise.hip"), src("_umath.py")
    out = {"MP_THREADS": int(grab(merge, r"#define SPAMD_MP_THREADS (\d+)", "MP_THREADS")[1]),
           "MP_VT": int(grab(merge, r"#define SPAMD_MP_VT (\d+)", "MP_VT")[1])}
    grab(merge, r"constexpr int MP_TILE = MP_THREADS \* MP_VT;", "MP_TILE")
    grab(merge, r"constexpr int TILE = MP_THREADS \* VT;", "TILE")
    m = grab(merge, r"if \(tot \* (\d+) (>=|>) TILE\) \{", "the store route switch")
    out["STORE_FACTOR"], out["STORE_COMPARE"] = int(m[1]), m[2]
    m = grab(cmerge, r"constexpr int CM_THREADS = (\d+), CM_VT = (\d+), CM_TILE = CM_THREADS \* CM_VT;", "CM_TILE")
    out["CM_THREADS"], out["CM_VT"] = int(m[1]), int(m[2])
    out["LOOKBACK_WINDOW"] = int(grab(common, r"hi -= (\d+);", "the look-back window")[1])
    grab(common, r"const int64_t j = hi - lane;", "the look-back window (one predecessor per lane)")
    m = grab(umath, r"MERGE_FUSED_MAX_ITEMS = 1 << (\d+)", "MERGE_FUSED_MAX_ITEMS")
    out["MERGE_FUSED_MAX_ITEMS"] = 1 << int(m[1])
    grab(umath, r"na \+ nb <= MERGE_FUSED_MAX_ITEMS", "the recipe switch (fused up to and including the bound)")
    m = grab(ewise, r"int64_t b = ceil_div\(n, (\d+)\);\s+if \(b > (\d+) \* (\d+)\) b = (\d+) \* (\d+);", "ewise.hip grid_for")
    assert (m[2], m[3]) == (m[4], m[5])
    out["GRID_CAP"], out["GRID_THREADS"] = int(m[2]) * int(m[3]), int(m[1])
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------
def bits_of(a):
    """the unsigned bit view of a value array (bool and complex included: complex as [n, 2] words)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        return a.view(f"u{a.dtype.itemsize // 2}").reshape(-1, 2)
    return a.view(f"u{a.dtype.itemsize}")


def differs_from(values, fill):
    """elementwise: the bits of values[i] are not the bits of `fill` (-0.0 differs from +0.0)"""
    ne = bits_of(values) != bits_of(np.array([fill], dtype=values.dtype))
    return ne.any(axis=1) if ne.ndim == 2 else ne


def _apply(name, x, y):
    with np.errstate(all="ignore"):
        return getattr(np, name)(x, y)


def fill_result(name, dtype, fill_a, fill_b):
    return _apply(name, np.array([fill_a], dtype=dtype), np.array([fill_b], dtype=dtype))[0]


def union_ref(name, ka, va, kb, vb, fill_a, fill_b):
    """(keys, vals, fill_out) of np.<name>(a or fill_a, b or fill_b) over the union of the keys, results whose bits are
    those of np.<name>(fill_a, fill_b) dropped"""
    assert va.dtype == vb.dtype
    keys = np.union1d(ka, kb)

    def fetch(k, v, fill):
        out = np.full(keys.size, fill, dtype=v.dtype)
        if k.size:
            pos = np.minimum(np.searchsorted(k, keys), k.size - 1)
            hit = k[pos] == keys
            out[hit] = v[pos[hit]]
        return out

    r = _apply(name, fetch(ka, va, fill_a), fetch(kb, vb, fill_b))
    fo = fill_result(name, va.dtype, fill_a, fill_b)
    keep = differs_from(r, fo)
    return keys[keep], r[keep], fo


def union_dense(name, ka, va, kb, vb, fill_a, fill_b, size):
    """the second formulation, over a small key space [0, size): scatter, apply, take what differs from the fill"""
    A, B = np.full(size, fill_a, dtype=va.dtype), np.full(size, fill_b, dtype=vb.dtype)
    A[ka], B[kb] = va, vb
    r = _apply(name, A, B)
    fo = fill_result(name, va.dtype, fill_a, fill_b)
    keys = np.flatnonzero(differs_from(r, fo)).astype(np.int64)
    return keys, r[keys], fo


def num_tiles(n, tile=TILE):
    return (n + tile - 1) // tile


class Structure:
    """what a correct merge path does with (ka, kb) and the surviving keys `kept`, from a stable sort of concatenate(ka, kb)
    (A first on ties): part[p] = A items among the first min(p * tile, na + nb) merged ranks; per tile la, lb, tot (surviving
    outputs); per thread its surviving outputs (threads[p, t]).  An output belongs to the rank of its A item, or of its B
    item when the key is in B only."""

    def __init__(self, ka, kb, kept, tile=TILE, vt=MP_VT):
        na, nb = ka.size, kb.size
        n = na + nb
        allk = np.concatenate([ka, kb])
        order = np.argsort(allk, kind="stable")
        from_a = order < na
        mk = allk[order]
        count_a = np.concatenate([[0], np.cumsum(from_a)]).astype(np.int64)
        self.nblocks = num_tiles(n, tile)
        edges = np.minimum(np.arange(self.nblocks + 1, dtype=np.int64) * tile, n)
        self.part = count_a[edges]
        self.la = np.diff(self.part)
        self.lb = np.diff(edges) - self.la
        second = np.zeros(n, dtype=bool)               # the B item of a matched pair: its A item sits one rank earlier
        second[1:] = mk[1:] == mk[:-1]
        assert not (second & from_a).any()
        self.from_a, self.second, self.keys = from_a, second, mk
        emits = ~second & np.isin(mk, kept)
        padded = np.zeros(self.nblocks * tile, dtype=np.int64)
        padded[:n] = emits
        self.threads = padded.reshape(self.nblocks, tile // vt, vt).sum(axis=2).astype(np.int8)
        self.tot = self.threads.sum(axis=1, dtype=np.int64)
        self.total = int(self.tot.sum())
        assert self.total == kept.size

    def straddles(self, every):
        """merged ranks r = every * p - 1 (p >= 1) at which the A item of a matched pair is the last rank before a boundary
        and its B item the first one behind it"""
        r = np.flatnonzero(self.second) - 1
        return r[(r + 1) % every == 0]


# ---- the token builder -------------------------------------------------------------------------------------------------
A_, B_, M_, M0 = 0, 1, 2, 3
_CODE = {"a": A_, "b": B_, "m": M_, "m0": M0}
_RANKS = np.array([1, 1, 2, 2])


class Seq:
    """a merged sequence, token by token; `rank` = merged ranks used so far (the next token's first item gets that rank)"""

    def __init__(self):
        self.parts, self.rank = [], 0

    def add(self, tok, count=1):
        if count > 0:
            self.parts.append(np.full(count, _CODE[tok], dtype=np.uint8))
            self.rank += count * int(_RANKS[_CODE[tok]])
        return self

    def singles(self, upto):
        """`a a b a a b ...` up to merged rank `upto`"""
        n = upto - self.rank
        assert n >= 0, (self.rank, upto)
        self.parts.append((np.arange(n) % 3 == 2).astype(np.uint8))
        self.rank = upto
        return self

    def m_at(self, rank, tok="m"):
        """singles, then a matched pair whose A item has merged rank `rank` (its B item `rank + 1`)"""
        return self.singles(rank).add(tok)

    def tile(self, n_matched, tok="m", tile=TILE):
        """one whole tile (from a tile edge): n_matched pairs spread evenly among single items"""
        assert self.rank % tile == 0 and 2 * n_matched <= tile
        n_single = tile - 2 * n_matched
        codes = np.concatenate([np.full(n_matched, _CODE[tok], dtype=np.uint8), (np.arange(n_single) % 3 == 2).astype(np.uint8)])
        if n_matched and n_single:       # interleave: a stable sort by the fractional position
            pos = np.concatenate([(np.arange(n_matched) + 0.5) / n_matched, (np.arange(n_single) + 0.25) / n_single])
            codes = codes[np.argsort(pos, kind="stable")]
        self.parts.append(codes)
        self.rank += tile
        return self

    def codes(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.uint8)


def rank_of(codes):
    """merged rank of every token's first item"""
    r = np.zeros(codes.size + 1, dtype=np.int64)
    np.cumsum(_RANKS[codes], out=r[1:])
    return r


TYPES = ("float32", "float64", "int32", "int64", "uint8", "bool", "complex64", "complex128")


def operands(codes, dtype, first_key=0, stride=3, last_key=None, values=None):
    """token codes -> (ka, va, kb, vb): strictly increasing keys first_key + stride * (token index) (the last one `last_key`
    when given); A values 1 + i % 7, B values 1 + i % 5 (complex: + (1 + i % 3) j / + 2 j), m0 pairs 0 and 0; `values`:
    {token index: (x, y)} placed by hand"""
    dt = np.dtype(dtype)
    n = codes.size
    idx = np.arange(n, dtype=np.int64)
    keys = first_key + stride * idx
    if last_key is not None and n:
        assert n == 1 or keys[-2] < last_key
        keys[-1] = last_key
    x, y = (1 + idx % 7).astype(np.float64), (1 + idx % 5).astype(np.float64)
    if dt.kind == "c":
        x, y = x + 1j * (1 + idx % 3), y + 2j
    zero = codes == M0
    x[zero], y[zero] = 0, 0
    for i, (xv, yv) in (values or {}).items():
        x[i], y[i] = xv, yv
    in_a, in_b = codes != B_, codes != A_
    return keys[in_a], x[in_a].astype(dt), keys[in_b], y[in_b].astype(dt)


# ---- the table ---------------------------------------------------------------------------------------------------------
ZERO_OPS = (("add", 0, 0), ("multiply", 0, 0))
TYPED_OPS = {"real": (("multiply", 0, 0), ("greater", 0, 0), ("add", 2, 0)),
             "bool": (("logical_and", False, False), ("logical_or", False, False), ("not_equal", True, False)),
             "complex": (("multiply", 0, 0), ("not_equal", 0, 0), ("add", 1 + 1j, 0))}


def ops_of_type(dtype):
    kind = np.dtype(dtype).kind
    return TYPED_OPS["complex" if kind == "c" else ("bool" if kind == "b" else "real")]


class Case:
    def __init__(self, build, ops=ZERO_OPS, dtypes=("float64",), big=False, **kw):
        self.build, self.ops, self.dtypes, self.big, self.kw = build, ops, dtypes, big, kw


CASES = {}
LOOKBACK_TILES = (2, 63, 64, 65, 66, 129, 130)
MANY_TILES = 1024
STORE_TOTS = (TILE // 4 - 1, TILE // 4, TILE // 4 + 1, 0, 1, TILE // 2, TILE // 4, TILE // 4 - 1)   # adjacent tiles, other routes
LOOKBACK_TOTS = (0, 5, TILE // 2, 0, TILE // 4, 77)        # per-tile outputs of `multiply`, cyclically
LAST_TILE_TOTALS = (TILE - 1, TILE, TILE + 1, TILE + 2, 2 * TILE + 1)
RECIPE_TOTALS = (MERGE_FUSED_MAX_ITEMS - 1, MERGE_FUSED_MAX_ITEMS, MERGE_FUSED_MAX_ITEMS + 1)
EDGE_LATER = 3                                             # "a later p" of the tile-edge cases
DIAG_THREADS = (5, WAVE - 1, 14 * WAVE + WAVE - 1, 15 * WAVE + 10)   # inside a wave | last lane of wave 0 | of wave 14 | in the last wave


def _case(name, **kw):
    def register(build):
        CASES[name] = Case(build, **kw)
        return build
    return register


@_case("thread diagonals")
def _():
    s = Seq()
    for t in DIAG_THREADS:                    # the A item is the thread's last rank, the B item the next thread's first
        s.m_at(MP_VT * t + MP_VT - 1)
    return s.singles(TILE + 100).codes()


def _edge(kind, p):
    """a matched pair at tile edge p: `straddle` (A item the last rank of tile p - 1), `before` (both items in front of
    the edge), `after` (both behind it); two more tiles' worth of items around it"""
    first = {"straddle": TILE * p - 1, "before": TILE * p - 2, "after": TILE * p}[kind]
    return Seq().m_at(first).singles(TILE * p + 700).add("m").singles(TILE * (p + 1) + 9).codes()


for _kind in ("straddle", "before", "after"):
    for _p in (1, EDGE_LATER):
        _case(f"tile edge {_p}: {_kind}", dtypes=TYPES if (_kind, _p) == ("straddle", 1) else ("float64",),
              ops=None if (_kind, _p) == ("straddle", 1) else ZERO_OPS)(functools.partial(_edge, _kind, _p))


@_case("every edge straddled")
def _():
    s = Seq()
    for p in range(1, 6):
        s.m_at(TILE * p - 1)
    return s.add("m0").singles(TILE * 5 + 3).codes()


@_case("A-only tile, then its partner")
def _():
    # tile 1 takes 4096 A items (lb = 0); the last one's partner is the first B item of tile 2
    return Seq().singles(TILE).add("a", TILE - 1).add("m").singles(2 * TILE + 50).add("b", 30).codes()


@_case("B-only tiles")
def _():
    # A ends inside tile 0: tile 1 and tile 2 are B only (la = 0, a0 == na)
    return Seq().singles(TILE - 10).add("m").add("b", 2 * TILE + 5).codes()


_case("A below B")(lambda: Seq().add("a", 5000).add("b", 6000).codes())
_case("B below A")(lambda: Seq().add("b", 6000).add("a", 5000).codes())


@_case("skew 10 + 40000")
def _():
    s = Seq()
    for i in range(10):
        s.add("b", 3990 + i).add("m" if i % 2 else "a")
    return s.add("b", 40_000 + 10 - s.rank).codes()


@_case("skew 40000 + 10")
def _():
    s = Seq()
    for i in range(10):
        s.add("a", 3990 + i).add("m" if i % 2 else "b")
    return s.add("a", 40_000 + 10 - s.rank).codes()


_case("na = 0")(lambda: Seq().add("b", 5).codes())
_case("nb = 0")(lambda: Seq().add("a", 5).codes())
_case("nothing")(lambda: Seq().codes())
_case("(1, 0)")(lambda: Seq().add("a").codes())
_case("(0, 1)")(lambda: Seq().add("b").codes())
_case("(1, 1) equal keys")(lambda: Seq().add("m").codes())
_case("(1, 1) other keys")(lambda: Seq().add("b").add("a").codes())
EMPTY_CASES = ("na = 0", "nb = 0", "nothing", "(1, 0)", "(0, 1)", "(1, 1) equal keys", "(1, 1) other keys")

for _total in LAST_TILE_TOTALS:      # the sequence ends in a matched pair: the last tile holds its B item, or both items
    _case(f"total {_total}")(functools.partial(lambda total: Seq().add("b").m_at(total - 2).codes(), _total))

_case("last key in A", last_key=MAX_KEY)(lambda: Seq().add("b").singles(300).add("m").add("b").add("a").codes())
_case("last key in B", last_key=MAX_KEY)(lambda: Seq().add("b").singles(300).add("m").add("a").add("b").codes())
_case("last key in both", last_key=MAX_KEY)(lambda: Seq().add("b").singles(TILE - 1).add("m").codes())   # ... across a tile edge


@_case("store switch", dtypes=TYPES, ops=None)
def _():
    s = Seq()
    for k in STORE_TOTS:
        s.tile(k)
    return s.singles(s.rank + 7).codes()


@_case("full tiles", ops=(("add", 0, 0),))
def _():
    return Seq().singles(2 * TILE + 40).codes()          # disjoint operands: every rank is an output


@_case("scan mix", ops=(("add", 0, 0), ("multiply", 0, 0), ("add", 2, 0)))
def _():
    rng = np.random.default_rng(7)                        # every token at random: every thread pattern, at every alignment
    return rng.choice(np.array([A_, B_, M_, M0], dtype=np.uint8), size=3 * TILE, p=(0.3, 0.3, 0.2, 0.2))


def _lookback(tiles):
    s = Seq()
    for p in range(tiles - 1):
        s.tile(LOOKBACK_TOTS[p % len(LOOKBACK_TOTS)])
    return s.m_at(s.rank + 8).singles(s.rank + 3).codes()      # a short last tile


for _tiles in LOOKBACK_TILES:
    _case(f"look-back {_tiles} tiles")(functools.partial(_lookback, _tiles))
_case(f"look-back {MANY_TILES} tiles", big=True)(functools.partial(_lookback, MANY_TILES))


def _recipe(total):
    reps = total // 7 + 1                                  # a a b m a b: 4 items of A and 3 of B per 7 ranks (na != nb)
    codes = np.tile(np.array([A_, A_, B_, M_, A_, B_], dtype=np.uint8), reps)
    codes = codes[:int(np.searchsorted(rank_of(codes), total, "right")) - 1]
    s = Seq()
    s.parts, s.rank = [codes], int(rank_of(codes)[-1])
    return s.singles(total).codes()


for _total in RECIPE_TOTALS:
    _case(f"recipe {_total}", big=True, ops=(("add", 0, 0),))(functools.partial(_recipe, _total))


@_case("specials: add", ops=(("add", 0, 0),),
       values={0: (-0.0, 0), 1: (0, -0.0), 2: (1.5, -1.5), 3: (-0.0, -0.0), 4: (np.inf, 0), 5: (0, -np.inf), 6: (np.inf, 1),
               7: (0.0, 0), 8: (2.0 ** -1074, -2.0 ** -1074), 9: (-3, 0)})
def _():   # -0 + 0 = +0 (dropped) | 0 + -0 | exact cancellation | -0 + -0 = -0 (kept) | infinities | a stored +0 | denormals
    return Seq().add("a").add("b").add("m").add("m").add("a").add("b").add("m").add("a").add("m").add("a").singles(40).codes()


@_case("specials: multiply", ops=(("multiply", 0, 0),),
       values={0: (-2, 0), 1: (0, -3), 2: (-0.0, 5), 3: (-1, -0.0), 4: (0.0, 7), 5: (-0.0, 0), 6: (2.0 ** -600, 2.0 ** -600)})
def _():   # -2 * 0 = -0 (kept) | 0 * -3 | -0 * 5 = -0 | -1 * -0 = +0 (dropped) | 0 * 7 | -0 * 0 | an underflow to +0
    return Seq().add("a").add("b").add("m").add("m").add("m").add("a").add("m").singles(40).codes()


# cases the older union (`union_merge`: csrc/ewise.hip) takes as well; the last one is the second trip of its grid-stride loops
def _second_trip():
    codes = np.random.default_rng(3).choice(np.array([A_, B_, M_], dtype=np.uint8), size=750_000, p=(0.3, 0.2, 0.5))
    codes = codes[:int(np.searchsorted(rank_of(codes), N1 + 257, "right")) - 1]
    s = Seq()
    s.parts, s.rank = [codes], int(rank_of(codes)[-1])
    return s.singles(N1 + 257).codes()


CASES["grid second trip"] = Case(_second_trip, big=True, ops=(("add", 0, 0),))
UNION_MERGE_CASES = tuple(n for n in CASES if n.startswith("tile edge")) + EMPTY_CASES + (
    "A-only tile, then its partner", "B-only tiles", "A below B", "B below A", "last key in both", "grid second trip")


@functools.lru_cache(maxsize=None)
def case_codes(name):
    codes = CASES[name].build()
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=8)
def case_operands(name, dtype="float64"):
    """(ka, va, kb, vb) of a case, read-only"""
    out = operands(case_codes(name), dtype, **CASES[name].kw)
    for a in out:
        a.setflags(write=False)
    return out


def case_ops(name, dtype):
    return CASES[name].ops or ops_of_type(dtype)


def calls():
    """every (case, dtype, ufunc name, fill_a, fill_b) of the table"""
    return [(name, dt, *op) for name, c in CASES.items() for dt in c.dtypes for op in case_ops(name, dt)]


@functools.lru_cache(maxsize=None)
def case_reference(name, dtype, op, fill_a, fill_b):
    """(keys, vals, fill_out, Structure) of one call, read-only"""
    ka, va, kb, vb = case_operands(name, dtype)
    keys, vals, fo = union_ref(op, ka, va, kb, vb, fill_a, fill_b)
    for a in (keys, vals):
        a.setflags(write=False)
    return keys, vals, fo, Structure(ka, kb, keys)

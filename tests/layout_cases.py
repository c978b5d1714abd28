"""Cases for the kernels and host code that MOVE data between layouts: the slab merge (csrc/lead_rotate.hip), the one-pass
broadcast (csrc/broadcast.hip), the strided transpose (csrc/transpose.hip), the hub-row combine and its plan (csrc/hot_rows.hip,
`_dot.hot_piece_plan`), indexing (`_indexing.py`) and the joins (`_batched.py`).  Plain NumPy references written from the
contracts in include/sparse_amd.h and the docstrings, and seeded case generators in which every case is built around one
place where the code takes another path.  No GPU, no torch, no package import.  Everything here moves bits, so every
comparison against these references is exact; tests/test_layout_cases.py proves from the inputs alone that each case sits
where its name says and that each reference agrees with a brute-force evaluation on the dense array.

The boundaries the tables are aimed at (tests/test_layout_cases.py reads them from the source text, `source_constants`):
  RL_MAX_SLABS, RL_MAX_CELLS, RL_CAP   limits 0-2 of `spamd_keys_lead_last_limits`: slabs, cells per range, elements per range
  RL_MAX_PER_CELL = 64                 elements of one output cell (no getter: csrc/lead_rotate.hip `constexpr int RL_MAX_PER_CELL`)
  RL_GAP = 8                           table words an element fills itself; longer gaps are the binary search's
  broadcast / transpose / combine      workgroups of 256 threads, 64 x 64 tiles, 256-column slabs
"""
import functools
import itertools
import os
import re
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RL_MAX_SLABS = 2048
RL_MAX_CELLS = 2048
RL_CAP = 4096
RL_MAX_PER_CELL = 64      # csrc/lead_rotate.hip: `constexpr int RL_MAX_PER_CELL = 64;` (the C ABI has no getter for it)
RL_GAP = 8
BLOCK = 256               # threads of a workgroup of the broadcast and combine kernels
TILE = 64                 # the transpose's tile edge

EINVAL, ETYPE = -1, -2    # include/sparse_amd.h


def source_constants():
    """the same constants as the source files state them today"""
    def src(*parts):
        return open(os.path.join(ROOT, "sparse_amd", *parts)).read()

    def grab(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: `{pattern}` is gone from the source - move the cases of tests/layout_cases.py with it"
        return m

    lead, bc, tr, hot = src("csrc", "lead_rotate.hip"), src("csrc", "broadcast.hip"), src("csrc", "transpose.hip"), src("csrc", "hot_rows.hip")
    out = {name: int(grab(lead, rf"constexpr int {name} = (\d+);", name)[1])
           for name in ("RL_MAX_SLABS", "RL_MAX_CELLS", "RL_CAP", "RL_MAX_PER_CELL", "RL_GAP")}
    grab(lead, r"if \(cnt <= 0 \|\| cnt > RL_GAP\) return;", "the hand-over between the two table passes")
    grab(lead, r"if \(T > RL_CAP\)", "the range limit (a range of exactly RL_CAP elements is merged)")
    grab(lead, r"if \(mx > RL_MAX_PER_CELL\) bad = 1;", "the cell limit (a cell of exactly RL_MAX_PER_CELL elements is merged)")
    out["BC_BLOCK"] = int(grab(bc, r"blockIdx\.x \* (\d+) \+ threadIdx\.x", "the broadcast's workgroup")[1])
    out["TILE"] = int(grab(tr, r"__shared__ E tile\[(\d+)\]\[\d+\];", "the transpose's tile")[1])
    out["HOT_BLOCK"] = int(grab(hot, r"% slabs\) \* (\d+) \+ threadIdx\.x", "the combine's column slab")[1])
    return out


def payload_bits(n, nbytes, seed=0):
    """n values of `nbytes` bytes as unsigned words: random bits with the patterns a value-aware copy would change among them
    (-0.0, quiet and signalling NaNs with payloads, the all-ones word)"""
    rng = np.random.default_rng(1000 + 17 * nbytes + seed)
    dt = np.dtype(f"u{nbytes}")
    bits = rng.integers(0, 2 ** (8 * nbytes), size=n, dtype=np.uint64, endpoint=False).astype(dt) if nbytes < 8 else \
        rng.integers(0, 2 ** 64, size=n, dtype=np.uint64, endpoint=False)
    special = {1: [0x80, 0xff, 0x00], 2: [0x8000, 0x7e01, 0xfc00, 0xffff],
               4: [0x80000000, 0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff],
               8: [0x8000000000000000, 0x7ff8000000000001, 0xfff8000012345678, 0x7ff0000000000001, 0xffffffffffffffff]}[nbytes]
    for k, s in enumerate(special):
        if k < n:
            bits[(k * 7919) % n] = s
    return bits.astype(dt)


def bits_of(a):
    """the unsigned bit view of an array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == bool else f"u{a.dtype.itemsize}")


# ---- A. the slab merge ------------------------------------------------------------------------------------------------------
class LeadCase(NamedTuple):
    name: str
    S: int
    P: int
    cells: int
    keys: np.ndarray     # sorted, duplicate-free, key = s * P + c


def ref_lead_last(keys, vals, S, P):
    """(out_keys, out_vals) of `spamd_keys_lead_last`: new key c * S + s, in ascending order"""
    s, c = np.divmod(np.asarray(keys, dtype=np.int64), P)
    new = c * S + s
    order = np.argsort(new, kind="stable")
    return new[order], np.asarray(vals)[order]


def lead_counts(keys, S, P, cells):
    """(elements per range [ranges], the largest element count of one output cell)"""
    c = np.asarray(keys, dtype=np.int64) % P
    ranges = -(-P // cells)
    per_range = np.bincount(c // cells, minlength=ranges)
    per_cell = np.unique(c, return_counts=True)[1]
    return per_range, int(per_cell.max()) if per_cell.size else 0


def lead_predicts_failed(keys, S, P, cells, cap=RL_CAP, per_cell=RL_MAX_PER_CELL):
    """the documented refusal: a range holds more than limit 2 elements, or an output cell more than 64"""
    per_range, most = lead_counts(keys, S, P, cells)
    return bool(per_range.max(initial=0) > cap or most > per_cell)


def lead_failed_ranges(keys, S, P, cells, cap=RL_CAP, per_cell=RL_MAX_PER_CELL):
    """boolean [ranges]: which ranges refuse (nothing is written for them)"""
    c = np.asarray(keys, dtype=np.int64) % P
    ranges = -(-P // cells)
    per_range = np.bincount(c // cells, minlength=ranges)
    cu, cn = np.unique(c, return_counts=True)
    bad = per_range > cap
    bad[np.unique(cu[cn > per_cell] // cells)] = True
    return bad


def lead_table(keys, S, P, cells):
    """the boundary table (csrc/lead_rotate.hip): bnd[b * S + s] = first element of run s whose cell is >= b * cells, for
    b = 0 .. ranges (the last row: the runs' ends)"""
    keys = np.asarray(keys, dtype=np.int64)
    ranges = -(-P // cells)
    b = np.arange(ranges + 1, dtype=np.int64)[:, None]
    s = np.arange(S, dtype=np.int64)[None, :]
    return np.searchsorted(keys, s * P + np.minimum(b * cells, P), side="left").astype(np.int32).reshape(-1)


def lead_word_gaps(keys, S, P, cells):
    """for every element, the number of table words between its predecessor's word (exclusive) and its own (inclusive), in
    (run, range) order; the first element counts from the table's first word.  An element fills 1 .. RL_GAP words itself."""
    keys = np.asarray(keys, dtype=np.int64)
    nb1 = -(-P // cells) + 1
    s, c = np.divmod(keys, P)
    flat = s * nb1 + c // cells
    return np.diff(flat, prepend=-1)


def _lead(name, S, P, cells, s, c):
    keys = np.unique(np.asarray(s, dtype=np.int64) * P + np.asarray(c, dtype=np.int64))
    assert keys.size == np.asarray(s).size, name
    return LeadCase(name, S, P, cells, keys)


def _lead_random(name, S, P, cells, n, seed, slabs=None):
    rng = np.random.default_rng(seed)
    if slabs is None:
        keys = np.sort(rng.choice(S * P, size=n, replace=False)) if S * P < 2 ** 24 else \
            np.unique(rng.integers(0, S * P, size=n + n // 8))[:n]
    else:     # only these slabs hold elements
        slabs = np.asarray(slabs, dtype=np.int64)
        pick = np.sort(rng.choice(slabs.size * P, size=n, replace=False))
        keys = np.sort(slabs[pick // P] * P + pick % P)
    return LeadCase(name, S, P, cells, keys.astype(np.int64))


LEAD_GRID_S = (1, 63, 64, 65, 2047, 2048)
LEAD_GRID_CELLS = (1, 2, 64, 2048)


def _lead_grid_P(cells):
    return sorted({p for p in (1, cells - 1, cells, cells + 1, 7 * cells + 3) if p >= 1})


def _lead_grid():
    out = {}
    for S in LEAD_GRID_S:
        for cells in LEAD_GRID_CELLS:
            for P in _lead_grid_P(cells):
                total = S * P
                n = total if total <= 256 else min(total // 2, 3000)
                name = f"grid S={S} cells={cells} P={P}"
                out[name] = functools.partial(_lead_random, name, S, P, cells, n, seed=S * 7 + cells * 3 + P)
    return out


def _lead_full(name, S, P, cells):
    s, c = np.divmod(np.arange(S * P, dtype=np.int64), P)
    return _lead(name, S, P, cells, s, c)


def _lead_one_range(name, S, P, cells, n, extra_cell=None):
    """n elements in range 0 (cells 0 .. cells - 1), dealt to the cells round robin so that no cell holds more than
    ceil(n / cells); `extra_cell` (a, b): one element moved from cell b to cell a.  A few elements in range 1 follow."""
    q = np.arange(n, dtype=np.int64)
    c, s = q % cells, q // cells
    if extra_cell is not None:
        a, b = extra_cell
        last = np.flatnonzero(c == b)[-1]
        c[last], s[last] = a, s[c == a].max() + 1
    tail_s = np.arange(0, S, 97, dtype=np.int64)
    return _lead(name, S, P, cells, np.concatenate([s, tail_s]), np.concatenate([c, np.full(tail_s.size, cells + 1)]))


def _lead_gap(name, first_flat, gap, cross_slab):
    """S = 4 runs, 21 table words per run (20 ranges of 64 cells): element 0 at table word `first_flat`, element 1 exactly
    `gap` words behind it - in the same run, or (cross_slab) in the next run - and a dense stretch at the end"""
    S, cells, ranges = 4, 64, 20
    P, nb1 = cells * ranges, ranges + 1
    flat0 = first_flat
    flat1 = flat0 + gap
    assert (flat1 // nb1 != flat0 // nb1) == cross_slab and flat0 % nb1 < ranges and flat1 % nb1 < ranges, name
    s = [flat0 // nb1, flat1 // nb1] + [3] * 40
    c = [(flat0 % nb1) * cells + 5, (flat1 % nb1) * cells] + list(range(19 * cells, 19 * cells + 40))
    return _lead(name, S, P, cells, s, c)


@functools.lru_cache(maxsize=None)
def lead_case(name):
    return LEAD_CASES[name]()


LEAD_CASES = _lead_grid()
LEAD_CASES.update({
    "empty slabs at the head": functools.partial(_lead_random, "empty slabs at the head", 100, 1000, 64, 2500, 1, slabs=range(30, 100)),
    "empty slabs in the middle": functools.partial(_lead_random, "empty slabs in the middle", 100, 1000, 64, 2500, 2,
                                                   slabs=list(range(0, 20)) + list(range(75, 100))),
    "90 empty trailing slabs": functools.partial(_lead_random, "90 empty trailing slabs", 200, 1000, 64, 2500, 3, slabs=range(0, 110)),
    "gap of 8 words inside a run": functools.partial(_lead_gap, "gap of 8 words inside a run", 2, 8, False),
    "gap of 9 words inside a run": functools.partial(_lead_gap, "gap of 9 words inside a run", 2, 9, False),
    "gap of 8 words across a run end": functools.partial(_lead_gap, "gap of 8 words across a run end", 18, 8, True),
    "gap of 9 words across a run end": functools.partial(_lead_gap, "gap of 9 words across a run end", 18, 9, True),
    "first element 8 words into the table": functools.partial(_lead_gap, "first element 8 words into the table", 7, 3, False),
    "first element 9 words into the table": functools.partial(_lead_gap, "first element 9 words into the table", 8, 3, False),
    "n=1 no word written by an element": lambda: _lead("n=1 no word written by an element", 8, 64 * 20, 64, [5], [64 * 13 + 7]),
    "n=1 every word before it written by the element": lambda: _lead("n=1 every word before it written by the element", 8, 64 * 20, 64, [0], [64 * 7]),
    "S=P=cells=64 full: 4096 in the range, 64 in every cell": functools.partial(
        _lead_full, "S=P=cells=64 full: 4096 in the range, 64 in every cell", 64, 64, 64),
    "S=65 P=cells=64 full: 4160 in the range": functools.partial(_lead_full, "S=65 P=cells=64 full: 4160 in the range", 65, 64, 64),
    "S=2048 cells=4: 4096 in one range": functools.partial(_lead_one_range, "S=2048 cells=4: 4096 in one range", 2048, 8, 4, 4096),
    "S=2048 cells=4: 4097 in one range": functools.partial(_lead_one_range, "S=2048 cells=4: 4097 in one range", 2048, 8, 4, 4097),
    "S=2048 cells=64: 4096 in one range, 64 in every cell": functools.partial(
        _lead_one_range, "S=2048 cells=64: 4096 in one range, 64 in every cell", 2048, 130, 64, 4096),
    "S=2048 cells=64: 4097 in one range": functools.partial(_lead_one_range, "S=2048 cells=64: 4097 in one range", 2048, 130, 64, 4097),
    "S=2048 cells=64: 4096 in one range, one cell of 65": functools.partial(
        _lead_one_range, "S=2048 cells=64: 4096 in one range, one cell of 65", 2048, 130, 64, 4096, extra_cell=(3, 9)),
    "two full ranges then a partial one": functools.partial(_lead_full, "two full ranges then a partial one", 64, 64 * 2 + 10, 64),
    "S=2048 P=2048*1000+5: a large, mostly untouched table": functools.partial(
        _lead_random, "S=2048 P=2048*1000+5: a large, mostly untouched table", 2048, 2048 * 1000 + 5, 2048, 5000, 4),
})

# (what, val_bytes, n, S, P, cells, code): arguments the entry point declines, with the documented code
LEAD_ERRORS = (
    ("S=2049", 4, 10, 2049, 16, 4, EINVAL),
    ("cells=3", 4, 10, 8, 16, 3, EINVAL),
    ("cells=4096", 4, 10, 8, 16, 4096, EINVAL),
    ("val_bytes=2", 2, 10, 8, 16, 4, ETYPE),
    ("P=2**42", 8, 10, 8, 2 ** 42, 4, EINVAL),
)

# the at-limit and over-limit inputs as (S, P) arrays for `x.sum(axis=0)`, `max`, `prod`
LEAD_PRODUCT_CASES = ("S=P=cells=64 full: 4096 in the range, 64 in every cell", "S=65 P=cells=64 full: 4160 in the range",
                      "S=2048 cells=4: 4096 in one range", "S=2048 cells=4: 4097 in one range",
                      "S=2048 cells=64: 4096 in one range, 64 in every cell", "S=2048 cells=64: 4097 in one range",
                      "two full ranges then a partial one")


# ---- B. the broadcast -------------------------------------------------------------------------------------------------------
class BcastCase(NamedTuple):
    name: str
    b0: int
    k1: int
    b1: int
    k2: int
    b2: int
    keys: np.ndarray     # sorted, duplicate-free, key = p1 * k2 + p2


def ref_broadcast(keys, vals, b0, k1, b1, k2, b2):
    """(out_keys, out_vals) of `spamd_coo_broadcast`: every (p1, p2, value) replicated over all (beta0, beta1, beta2), the
    keys by the header's formula, sorted"""
    keys = np.asarray(keys, dtype=np.int64)
    p1, p2 = np.divmod(keys, k2)
    p1, p2 = p1[None, :, None, None], p2[None, :, None, None]
    beta0 = np.arange(b0, dtype=np.int64)[:, None, None, None]
    beta1 = np.arange(b1, dtype=np.int64)[None, None, :, None]
    beta2 = np.arange(b2, dtype=np.int64)[None, None, None, :]
    out = ((((beta0 * k1 + p1) * b1 + beta1) * k2 + p2) * b2 + beta2).reshape(-1)
    src = np.broadcast_to(np.arange(keys.size)[None, :, None, None], (b0, keys.size, b1, b2)).reshape(-1)
    order = np.argsort(out, kind="stable")
    return out[order], np.asarray(vals)[src[order]]


def run_lengths(keys, k2):
    """lengths of the runs (the elements of one p1), in order"""
    return np.unique(np.asarray(keys, dtype=np.int64) // k2, return_counts=True)[1]


def _bc_rows(name, b, k1, k2, lens, seed=0):
    """row p1 holds lens[p1] elements at random p2"""
    rng = np.random.default_rng(seed + 5)
    keys = np.concatenate([p1 * k2 + np.sort(rng.choice(k2, size=n, replace=False)) for p1, n in enumerate(lens)] + [np.zeros(0, np.int64)])
    return BcastCase(name, b[0], k1, b[1], k2, b[2], keys.astype(np.int64))


def _bc_combo(bits):
    """each of b0, k1, b1, k2, b2 equal to 1 or larger than 1 (sizes 2-5)"""
    big = (3, 5, 2, 4, 3)
    b0, k1, b1, k2, b2 = (g if on else 1 for g, on in zip(big, bits))
    name = "groups " + " ".join(f"{n}{'>1' if on else '=1'}" for n, on in zip(("b0", "k1", "b1", "k2", "b2"), bits))
    rng = np.random.default_rng(sum(bit << i for i, bit in enumerate(bits)))
    total = k1 * k2
    keys = np.sort(rng.choice(total, size=max(1, (total + 1) // 2), replace=False)).astype(np.int64)
    return BcastCase(name, b0, k1, b1, k2, b2, keys)


@functools.lru_cache(maxsize=None)
def bcast_case(name):
    return BCAST_CASES[name]()


BCAST_CASES = {}
for _bits in itertools.product((0, 1), repeat=5):
    _c = _bc_combo(_bits)
    BCAST_CASES[_c.name] = functools.partial(_bc_combo, _bits)
BCAST_CASES.update({
    "one run, its p1 first": lambda: _bc_rows("one run, its p1 first", (2, 3, 2), 5, 300, [200, 0, 0, 0, 0]),
    "one run, its p1 in the middle": lambda: _bc_rows("one run, its p1 in the middle", (2, 3, 2), 5, 300, [0, 0, 200, 0, 0]),
    "one run, its p1 last": lambda: _bc_rows("one run, its p1 last", (2, 3, 2), 5, 300, [0, 0, 0, 0, 200]),
    "every run of length 1": lambda: _bc_rows("every run of length 1", (2, 3, 2), 50, 7, [1] * 50),
    "runs of 2, 3, 257 and 1000 beside runs of 1": lambda: _bc_rows(
        "runs of 2, 3, 257 and 1000 beside runs of 1", (2, 3, 2), 12, 1200, [1, 2, 1, 3, 1, 257, 1, 1000, 1, 0, 1, 1]),
    "long first and last runs": lambda: _bc_rows("long first and last runs", (1, 2, 3), 6, 1200, [1000, 1, 0, 1, 1, 257]),
    "n=1": lambda: BcastCase("n=1", 3, 4, 2, 5, 3, np.array([2 * 5 + 3], dtype=np.int64)),
    "n_out=255": lambda: _bc_rows("n_out=255", (3, 1, 1), 17, 9, [5] * 17),
    "n_out=256": lambda: _bc_rows("n_out=256", (1, 4, 1), 16, 9, [4] * 16),
    "n_out=257": lambda: BcastCase("n_out=257", 1, 3, 1, 4, 257, np.array([6], dtype=np.int64)),
    "b2=1 with b1>1, long runs": lambda: _bc_rows("b2=1 with b1>1, long runs", (2, 5, 1), 4, 500, [300, 1, 40, 257], 1),
    "b1=1 with b2>1, long runs": lambda: _bc_rows("b1=1 with b2>1, long runs", (2, 1, 5), 4, 500, [300, 1, 40, 257], 2),
    "k1=1 with every other group non-trivial": lambda: _bc_rows("k1=1 with every other group non-trivial", (3, 2, 4), 1, 700, [600], 3),
})
BCAST_VAL_BYTES = (1, 2, 4, 8)


# ---- C. the transpose -------------------------------------------------------------------------------------------------------
TRANSPOSE_EXTENTS = (1, 63, 64, 65, 129)
TRANSPOSE_ELEM_BYTES = (1, 2, 4, 8)
TRANSPOSE_LD_IN_EXTRA, TRANSPOSE_LD_OUT_EXTRA = 3, 5


def transpose_case(rows, cols, nbytes):
    """(the wider input matrix [rows, cols + 3] as unsigned words, the sentinel) - the block is its leading `cols` columns"""
    wide = payload_bits(rows * (cols + TRANSPOSE_LD_IN_EXTRA), nbytes, seed=rows * 131 + cols).reshape(rows, cols + TRANSPOSE_LD_IN_EXTRA)
    return wide, np.array(0xa5a5a5a5a5a5a5a5 >> (64 - 8 * nbytes), dtype=f"u{nbytes}")


def ref_transpose_into(wide, cols, sentinel):
    """the output buffer [cols, rows + 5] after the call: the block's transpose, sentinels everywhere else"""
    rows = wide.shape[0]
    out = np.full((cols, rows + TRANSPOSE_LD_OUT_EXTRA), sentinel, dtype=wide.dtype)
    out[:, :rows] = wide[:, :cols].T
    return out


# ---- D. hub rows ------------------------------------------------------------------------------------------------------------
COMBINE_N_COLS = (1, 255, 256, 257, 513)
COMBINE_PIECES = (1, 7, 8, 9, 128, 129)      # pieces per hot row: around the loop's unroll of 8 and the fan of 128
COMBINE_DTYPES = ("float32", "float64", "int32", "int64")
COMBINE_LD_EXTRA = (7, 3)                    # ld_part - n_cols, ld_out - n_cols


def combine_parts(n_pieces, n_cols, dtype, seed=0):
    """[n_pieces, n_cols] values whose sum depends on the order of the additions (floats of very different magnitudes) or
    wraps around (integers near the type's range)"""
    rng = np.random.default_rng(77 + seed + n_cols)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = rng.standard_normal((n_pieces, n_cols)) * np.exp2(rng.integers(-20, 20, size=(n_pieces, n_cols)))
        v[rng.random((n_pieces, n_cols)) < 0.05] = -0.0
        return v.astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min // 3, info.max // 3, size=(n_pieces, n_cols), dtype=dt)


def ref_combine(part, vfirst, rows, out):
    """`spamd_hot_rows_combine`: acc = T(0); for v in vfirst[h] .. vfirst[h + 1]: acc = acc + part[v, :], in the result type, into
    row rows[h] of `out` (a copy is returned); rows not named keep their contents"""
    out = out.copy()
    with np.errstate(over="ignore"):
        for h, r in enumerate(rows):
            acc = np.zeros(part.shape[1], dtype=out.dtype)
            for v in range(int(vfirst[h]), int(vfirst[h + 1])):
                acc = acc + part[v]
            out[r] = acc
    return out


def ref_piece_plan(lens, groups, fan):
    """`hot_piece_plan` restated from its docstring: (piece size, pieces per row, vptr, first piece of every group of at most
    `fan` pieces of one row or None)"""
    lens = [int(n) for n in lens]
    total = sum(lens)
    piece = min(4096, max(32, total // (groups * 35) // 32 * 32))
    counts = [-(-n // piece) for n in lens]
    vptr, base = [0], 0
    for n in lens:
        vptr += [base + min(k * piece, n) for k in range(1, -(-n // piece) + 1)]
        base += n
    g1 = None
    if max(counts) > fan:
        g1, first = [0], 0
        for cnt in counts:
            g1 += [first + min(k * fan, cnt) for k in range(1, -(-cnt // fan) + 1)]
            first += cnt
    return piece, counts, np.asarray(vptr, dtype=np.int64), None if g1 is None else np.asarray(g1, dtype=np.int64)


PLAN_ROW_LENGTHS = (4096, 4097, 4128, 4129, 40_000)
# filler rows (hot rows of their own) that bring the total to where the piece size is 32, a larger multiple of 32, and 4096
PLAN_FILLERS = {"piece 32": (), "piece 96": (35 * 1024 * 96,), "piece 4096": (35 * 1024 * 4096, 5000)}


def hub_matrix(M=600, K=6000, hot_min=4096, min_nnz=1 << 14, seed=3):
    """(indptr, indices) of a CSR pattern with one row of exactly `hot_min` elements, one of hot_min - 1, one of 4129 and short
    rows that bring the stored elements to at least `min_nnz`: (indptr, indices, {row: length} of the three long rows)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, size=M)
    long_rows = {17: hot_min, 300: hot_min - 1, M - 1: 4129}
    for r, n in long_rows.items():
        lens[r] = n
    short = [r for r in range(M) if r not in long_rows]
    while lens.sum() < min_nnz + 200:
        lens[rng.choice(short)] += 5
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(K, size=int(n), replace=False)) for n in lens]).astype(np.int64)
    return indptr, indices, long_rows


def hub_values(nnz, dtype, seed=4):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.random(nnz) + 0.5).astype(dtype) * rng.choice([-1, 1], size=nnz).astype(dtype)
    return (rng.integers(1, 10, size=nnz) * rng.choice([-1, 1], size=nnz)).astype(dtype)      # (no zero: a COO would drop it)


def hub_bound(indptr, indices, data, b, dtype):
    """(want in float64, bound): |got - want| <= (n_r + 2) eps sum_k |a_rk| |b_kj| with eps = 2u of `dtype`"""
    M, N = len(indptr) - 1, b.shape[1]
    a64, b64 = np.zeros((M, b.shape[0])), np.asarray(b, dtype=np.float64)
    a64[np.repeat(np.arange(M), np.diff(indptr)), indices] = np.asarray(data, dtype=np.float64)
    want, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
    n_r = np.diff(indptr).astype(np.float64)[:, None]
    return want, (n_r + 2) * np.finfo(dtype).eps * mag


# ---- E. indexing ------------------------------------------------------------------------------------------------------------
INDEX_SHAPE = (5, 6, 7)


class Arr(NamedTuple):
    """an array index to be: kind "list" | "int32" (ndarray) | "bool" (ndarray) | "tensor" (torch, made by the GPU test)"""
    kind: str
    values: tuple


def index_dense(dtype=np.float64, seed=11):
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 100, size=INDEX_SHAPE).astype(dtype)
    d[rng.random(INDEX_SHAPE) >= 0.4] = 0
    return d


def array_indices(n):
    """name -> `Arr` for an axis of n >= 5 elements"""
    some = tuple(bool((i * 5 + 1) % 3 == 0) for i in range(n))
    return {"empty": Arr("list", ()), "one": Arr("list", (3,)), "duplicates out of order": Arr("list", (2, 2, 0, 2)),
            "descending": Arr("list", tuple(range(n - 1, -1, -1))), "negative": Arr("list", (-1, -5)),
            "full range": Arr("list", tuple(range(n))), "mask none": Arr("bool", (False,) * n), "mask some": Arr("bool", some),
            "mask all": Arr("bool", (True,) * n), "tensor": Arr("tensor", (1, 0, 3)), "int32 ndarray": Arr("int32", (4, 1, 1))}


def as_numpy_index(index):
    """the index expression with every `Arr` as NumPy takes it"""
    def one(i):
        if isinstance(i, Arr):
            return np.asarray(i.values, dtype=bool if i.kind == "bool" else np.int32 if i.kind == "int32" else np.int64)
        return i
    return tuple(one(i) for i in index)


def numpy_moves_the_array_axis_first(index):
    """NumPy counts an integer as an advanced index too: when the integer and the array are not neighbours in the index, the
    array's axis goes to the FRONT of the result.  -> (does that change anything, the array's place among the result's axes).
    The library (like the reference it is modelled on, and as tests/golden pins it) leaves the axis in the array's place."""
    adv = [k for k, i in enumerate(index) if isinstance(i, (int, Arr))]
    place = sum(1 for i in index[:next(k for k, i in enumerate(index) if isinstance(i, Arr))] if not isinstance(i, int) and i is not Ellipsis)
    return (adv[-1] - adv[0] + 1 != len(adv)) and place != 0, place


def index_expected(dense, index):
    """what `x[index]` holds: NumPy's result, with the array's axis where the array stands (see above)"""
    want = dense[as_numpy_index(index)]
    moved, place = numpy_moves_the_array_axis_first(index)
    return np.moveaxis(want, 0, place) if moved else want


def index_by_axis(dense, index):
    """the same, evaluated one axis after the other (integers drop their axis, slices and the array act on theirs alone, `None`
    adds one): the brute force `index_expected` is checked against"""
    index = list(index)
    if Ellipsis in index:
        at = index.index(Ellipsis)
        real = sum(1 for i in index if i is not None and i is not Ellipsis)
        index[at:at + 1] = [slice(None)] * (dense.ndim - real)
    index += [slice(None)] * (dense.ndim - sum(1 for i in index if i is not None))
    out, axis = dense, 0
    for i in index:
        if i is None:
            out = np.expand_dims(out, axis)
            axis += 1
        elif isinstance(i, int):
            out = np.take(out, i, axis=axis)
        elif isinstance(i, slice):
            out = out[(slice(None),) * axis + (i,)]
            axis += 1
        else:
            sel = np.flatnonzero(np.asarray(i.values, dtype=bool)) if i.kind == "bool" else np.asarray(i.values, dtype=np.int64)
            out = np.take(out, sel, axis=axis)
            axis += 1
    return out


def index_cases():
    """name -> index tuple: one array index on each axis, alone and combined with an integer / a slice of step -2 on every
    other axis, `None` before and after, and an Ellipsis"""
    out = {}
    full = slice(None)
    for axis in range(3):
        for aname, arr in array_indices(INDEX_SHAPE[axis]).items():
            base = [full, full, full]
            base[axis] = arr
            out[f"axis {axis} {aname}"] = tuple(base[:axis + 1])
            for other in range(3):
                if other == axis:
                    continue
                for what, it in (("integer", 2), ("negative integer", -1), ("step -2", slice(None, None, -2)), ("step -2 from 4", slice(4, 0, -2))):
                    idx = list(base)
                    idx[other] = it
                    out[f"axis {axis} {aname}, {what} on axis {other}"] = tuple(idx)
            out[f"axis {axis} {aname}, None before"] = tuple(base[:axis] + [None, arr])
            out[f"axis {axis} {aname}, None after"] = tuple(base[:axis] + [arr, None])
            out[f"axis {axis} {aname}, Ellipsis"] = (Ellipsis, arr) + (full,) * (2 - axis)
    return out


SLICE_POINTS = (None,) + tuple(range(-6, 7))
SLICE_STEPS = (-3, -2, -1, 1, 2, 3)
SLICE_DENSE_1D = np.array([1.0, 2.0, 0.0, 4.0, 5.0])
SLICE_DENSE_2D = np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [4.0, 5.0, 6.0], [0.0, 7.0, 0.0]])


# ---- F. joins ---------------------------------------------------------------------------------------------------------------
CONCAT_MERGE_MAX_OPERANDS = 8
CONCAT_MERGE_ELEMENT_SIZES = (1, 4, 8)


class Operand(NamedTuple):
    shape: tuple
    dtype: str
    idx: str              # "int32" | "int64": the width of its coordinates (COO) or indices / pointers (GCXS)
    density: float
    seed: int


# value types `_kernels.convert` moves between on the device; a join that would have to promote another one (int8 with float32)
# raises TypeError, so the promoted cases keep to these
CONVERTIBLE = ("bool", "int32", "int64", "float32", "float64")


class JoinCase(NamedTuple):
    name: str
    operands: tuple
    axis: int
    route: str            # "append" (joined axis 0: the operands one after the other), "merge" (k-way union_merge), "sort"


def operand_dense(op, fill=0):
    rng = np.random.default_rng(op.seed)
    dt = np.dtype(op.dtype)
    d = np.full(op.shape, fill, dtype=dt)
    mask = rng.random(op.shape) < op.density
    vals = rng.integers(1, 100, size=op.shape)
    d[mask] = True if dt.kind == "b" else vals[mask].astype(dt)
    return d


def concat_keys_unsorted(operands, axis):
    """do the operands' stored elements, one operand after the other, come out of C order in the result?  (then the cat + sort
    route really sorts)"""
    dense = [operand_dense(o) for o in operands]
    offs = np.cumsum([0] + [d.shape[axis] for d in dense])
    shape = np.concatenate(dense, axis=axis).shape
    keys = []
    for d, off in zip(dense, offs):
        c = list(np.nonzero(d))
        c[axis] = c[axis] + off
        keys.append(np.ravel_multi_index(c, shape))
    keys = np.concatenate(keys)
    return bool((np.diff(keys) < 0).any())


def predicted_route(operands, axis):
    """the route `_batched.concatenate` documents for COO operands (and GCXS operands on its general path)"""
    nd = len(operands[0].shape)
    axis = axis % nd
    dt = np.result_type(*[np.dtype(o.dtype) for o in operands])
    if axis == 0:
        return "append"
    if len(operands) <= CONCAT_MERGE_MAX_OPERANDS and dt.itemsize in CONCAT_MERGE_ELEMENT_SIZES \
            and any(np.count_nonzero(operand_dense(o)) for o in operands):
        return "merge"
    return "sort"


def _ops(count, shape, dtype, axis, idx="int64", extents=None, density=0.4, dtypes=None, idxs=None, empty=()):
    out = []
    for k in range(count):
        s = list(shape)
        if extents is not None:
            s[axis % len(shape)] = extents[k % len(extents)]
        out.append(Operand(tuple(s), (dtypes[k % len(dtypes)] if dtypes else dtype), (idxs[k % len(idxs)] if idxs else idx),
                           0.0 if k in empty else density, 100 + k))
    return tuple(out)


def join_cases():
    out = []

    def add(name, operands, axis):
        out.append(JoinCase(name, operands, axis, predicted_route(operands, axis)))

    shape = (3, 4, 5)
    for count in (1, 2, 8, 9):
        for axis in (0, 1, 2, -1):
            add(f"{count} operands axis {axis}", _ops(count, shape, "float32", axis), axis)
    for dtype in ("bool", "int8", "int16", "float32", "float64", "int64"):
        for axis in (0, 1, 2):
            add(f"{dtype} axis {axis}", _ops(3, shape, dtype, axis), axis)
    for axis in (0, 2):
        add(f"bool + int32 + float32 promoted axis {axis}", _ops(3, shape, None, axis, dtypes=("bool", "int32", "float32")), axis)
        add(f"bool + float32 promoted axis {axis}", _ops(3, shape, None, axis, dtypes=("bool", "float32")), axis)
        add(f"int32 + int64 + float64 promoted axis {axis}", _ops(3, shape, None, axis, dtypes=("int32", "int64", "float64")), axis)
        for where, k in (("first", 0), ("middle", 1), ("last", 2)):
            add(f"empty operand {where} axis {axis}", _ops(3, shape, "float64", axis, empty=(k,)), axis)
        add(f"all operands empty axis {axis}", _ops(3, shape, "float64", axis, empty=(0, 1, 2)), axis)
        add(f"all but one operand empty axis {axis}", _ops(3, shape, "float64", axis, empty=(0, 2)), axis)
        add(f"int32 and int64 coordinates axis {axis}", _ops(4, shape, "float32", axis, idxs=("int32", "int64")), axis)
        add(f"different extents axis {axis}", _ops(4, shape, "int64", axis, extents=(1, 5, 2, 9)), axis)
    add("different extents axis 1, 9 operands", _ops(9, shape, "float64", 1, extents=(1, 5, 2)), 1)
    return out


def gcxs_join_cases():
    """(name, operands, compressed axis of the operands, axis, compressed_axes argument, takes the pointer route)"""
    out = []
    shape = (6, 5)
    for ca, axis in ((0, 0), (1, 1), (0, -2), (1, -1)):
        ops = _ops(3, shape, "float64", axis, extents=(6, 1, 4))
        out.append((f"compressed {ca} joined on axis {axis}", ops, ca, axis, None, True))
        out.append((f"compressed {ca} joined on axis {axis}, empty rows", _ops(3, shape, "float32", axis, density=0.12, extents=(6, 3, 4)),
                    ca, axis, None, True))
        out.append((f"compressed {ca} joined on axis {axis}, an empty operand", _ops(3, shape, "int64", axis, empty=(1,)), ca, axis, None, True))
        out.append((f"compressed {ca} joined on axis {axis}, mixed pointer widths",
                    _ops(4, shape, "float64", axis, idxs=("int32", "int64")), ca, axis, None, True))
        out.append((f"compressed {ca} joined on axis {axis}, promoted", _ops(3, shape, None, axis, dtypes=("bool", "float32", "int64")),
                    ca, axis, None, True))
    for ca, axis in ((0, 1), (1, 0)):
        out.append((f"compressed {ca} joined on axis {axis} (not the pointer route)", _ops(3, shape, "float64", axis), ca, axis, None, False))
    out.append(("compressed 0 joined on axis 0, compressed_axes=(1,) asked", _ops(3, shape, "float64", 0), 0, 0, (1,), False))
    out.append(("compressed 0 joined on axis 0, compressed_axes=(0,) asked", _ops(3, shape, "float64", 0), 0, 0, (0,), True))
    return out


STACK_SHAPES = ((4,), (3, 4), (2, 3, 4))

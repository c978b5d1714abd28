"""tests/merge_cases.py on its own, without a GPU: the reference against its second formulation, the tile structure against a
plain two-pointer merge, the constants the table was built for against the source text of the kernels, and the table against
every boundary it claims to hold - a boundary that is missing is a failure here, not a weaker GPU test."""
import numpy as np
import pytest

import merge_cases as mc

TILE, VT = mc.TILE, mc.MP_VT


# ---- the constants, from the source ------------------------------------------------------------------------------------
def test_constants_in_the_source_are_the_ones_the_table_was_built_for():
    src = mc.source_constants()
    assert (src["MP_THREADS"], src["MP_VT"]) == (mc.MP_THREADS, mc.MP_VT) == (1024, 4) and mc.TILE == 4096
    assert (src["CM_THREADS"], src["CM_VT"]) == (mc.MP_THREADS, mc.MP_VT), "CM_TILE != MP_TILE: the complex cases aim at the wrong ranks"
    assert (src["STORE_FACTOR"], src["STORE_COMPARE"]) == (mc.STORE_FACTOR, ">=") and TILE % mc.STORE_FACTOR == 0
    assert src["LOOKBACK_WINDOW"] == mc.LOOKBACK_WINDOW == mc.WAVE == 64
    assert src["MERGE_FUSED_MAX_ITEMS"] == mc.MERGE_FUSED_MAX_ITEMS == 2 ** 22
    assert (src["GRID_CAP"], src["GRID_THREADS"]) == (mc.GRID_CAP, 256) and mc.N1 == 2 ** 20
    assert mc.WAVE_RANKS == 256 and mc.MAX_KEY == np.iinfo(np.int64).max - 1


# ---- the reference, a second way -----------------------------------------------------------------------------------------
_REAL_OPS = ("add", "subtract", "multiply", "maximum", "minimum", "fmax", "fmin", "greater", "greater_equal", "less", "less_equal",
             "equal", "not_equal", "logical_and", "logical_or", "logical_xor")
_OPS = {"f": _REAL_OPS + ("divide",), "i": _REAL_OPS + ("bitwise_and", "bitwise_or", "bitwise_xor"),
        "u": _REAL_OPS + ("bitwise_and", "bitwise_or", "bitwise_xor"),
        "b": ("logical_and", "logical_or", "logical_xor", "equal", "not_equal", "greater", "less"),
        "c": ("add", "subtract", "multiply", "divide", "equal", "not_equal")}


@pytest.mark.parametrize("dtype", mc.TYPES)
def test_both_formulations_of_the_reference_agree(dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(len(dtype))
    size = 300
    for op in _OPS[dt.kind]:
        for fill_a, fill_b in ((0, 0), (2, 1), (0, 3)):
            if op == "divide" and fill_b == 0:
                continue                                     # (0 / 0: NaN semantics stay with the conformance tests)
            ka = np.sort(rng.choice(size, size=rng.integers(0, 120), replace=False)).astype(np.int64)
            kb = np.sort(rng.choice(size, size=rng.integers(0, 120), replace=False)).astype(np.int64)
            pool = np.array([0, 1, 2, 3, 5, -1, -2, -0.0] if dt.kind in "fc" else ([0, 1, 2, 3, 5, -1, -2] if dt.kind == "i" else [0, 1, 2, 3, 5]))
            va, vb = rng.choice(pool, size=ka.size).astype(dt), rng.choice(pool[:5] if op == "divide" else pool, size=kb.size).astype(dt)
            if op == "divide":
                vb[vb == 0] = 4
            if dt.kind == "c":
                va = (va + 1j * rng.choice(pool, size=ka.size)).astype(dt)
            got = mc.union_ref(op, ka, va, kb, vb, fill_a, fill_b)
            want = mc.union_dense(op, ka, va, kb, vb, fill_a, fill_b, size)
            assert np.array_equal(got[0], want[0]), (dtype, op, fill_a, fill_b)
            assert got[1].dtype == want[1].dtype and np.array_equal(mc.bits_of(got[1]), mc.bits_of(want[1])), (dtype, op)
            assert np.array_equal(mc.bits_of(np.array([got[2]])), mc.bits_of(np.array([want[2]])))
            assert got[0].size <= np.union1d(ka, kb).size


def test_the_prune_compares_bits():
    ka, kb = np.array([1, 2, 3, 4], dtype=np.int64), np.array([2, 3, 9], dtype=np.int64)
    va, vb = np.array([-0.0, -0.0, 1.5, 0.0]), np.array([-0.0, -1.5, -0.0])
    keys, vals, fo = mc.union_ref("add", ka, va, kb, vb, 0.0, 0.0)
    # -0 + 0 = +0 (fill) | -0 + -0 = -0 (kept) | 1.5 - 1.5 = +0 | a stored +0 | 0 + -0 = +0
    assert keys.tolist() == [2] and np.signbit(vals[0]) and vals[0] == 0 and not np.signbit(fo)


def _merge_loop(ka, kb, kept, tile, vt):
    """part, tot, threads by a two-pointer merge (ties: A first)"""
    ka, kb, kept = ka.tolist(), kb.tolist(), set(kept.tolist())
    i = j = 0
    ranks = []                                           # (from A, emits)
    while i < len(ka) or j < len(kb):
        if i < len(ka) and (j >= len(kb) or ka[i] <= kb[j]):
            ranks.append((True, ka[i] in kept))
            i += 1
        else:
            ranks.append((False, kb[j] in kept and not (i > 0 and ka[i - 1] == kb[j])))
            j += 1
    n = len(ranks)
    nblocks = (n + tile - 1) // tile
    part = [sum(1 for r in ranks[:min(p * tile, n)] if r[0]) for p in range(nblocks + 1)]
    threads = [[sum(1 for r in ranks[p * tile + t * vt:min(p * tile + (t + 1) * vt, (p + 1) * tile)] if r[1]) for t in range(tile // vt)]
               for p in range(nblocks)]
    return part, [sum(t) for t in threads], threads


def test_the_structure_reference_against_a_two_pointer_merge():
    rng = np.random.default_rng(11)
    for trial in range(30):
        codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=rng.integers(0, 90), p=(0.25, 0.25, 0.3, 0.2))
        ka, va, kb, vb = mc.operands(codes, "float64")
        for op in ("add", "multiply"):
            kept = mc.union_ref(op, ka, va, kb, vb, 0, 0)[0]
            st = mc.Structure(ka, kb, kept, tile=8, vt=2)
            part, tot, threads = _merge_loop(ka, kb, kept, 8, 2)
            assert st.part.tolist() == part and st.tot.tolist() == tot and st.threads.tolist() == threads, (trial, op)
            assert (st.la + st.lb).sum() == ka.size + kb.size and st.nblocks == mc.num_tiles(ka.size + kb.size, 8)


def test_the_token_builder():
    s = mc.Seq().add("b").m_at(9).add("m0").singles(20).add("a", 2)
    codes = s.codes()
    assert s.rank == 22 and mc.rank_of(codes)[-1] == 22
    ka, va, kb, vb = mc.operands(codes, "float64", last_key=mc.MAX_KEY)
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0) and kb[0] == 0 and ka[-1] == mc.MAX_KEY
    both = np.intersect1d(ka, kb)
    assert both.size == 2
    st = mc.Structure(ka, kb, np.union1d(ka, kb))
    assert np.flatnonzero(st.second).tolist() == [10, 12]            # the pair's B item one rank behind its A item
    z = both[1]
    assert va[ka == z] == 0 and vb[kb == z] == 0                     # m0: stored zeros
    assert va[ka != z].min() >= 1 and vb[kb != z].min() >= 1         # everything else positive: x * 0 = +0, the fill
    for dtype in mc.TYPES:
        a = mc.operands(codes, dtype)
        assert a[1].dtype == a[3].dtype == np.dtype(dtype) and a[0].dtype == np.int64
    t = mc.Seq().tile(1000).tile(0).tile(TILE // 2)
    assert t.rank == 3 * TILE and (t.codes() == mc.M_).sum() == 1000 + TILE // 2


# ---- the table holds what it is for ------------------------------------------------------------------------------------
def _st(name, op="multiply", dtype="float64", fills=(0, 0)):
    return mc.case_reference(name, dtype, op, *fills)[3]


def test_every_case_is_canonical_and_every_call_is_listed():
    assert len(mc.CASES) >= 45
    for name, c in mc.CASES.items():
        for dtype in c.dtypes:
            if c.big and dtype != "float64":
                pytest.fail("big cases take one dtype")
            ka, va, kb, vb = mc.case_operands(name, dtype)
            assert ka.dtype == kb.dtype == np.int64 and va.dtype == vb.dtype == np.dtype(dtype)
            assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0), name
            for k in (ka, kb):
                assert k.size == 0 or (k[0] >= 0 and k[-1] <= mc.MAX_KEY)
            assert np.isfinite(va.astype(np.complex128)).all() or name.startswith("specials")
    assert sum(1 for c in mc.CASES.values() if c.big) == 5          # 1024 tiles, three around 2^22, the second grid trip: no more
    calls = mc.calls()
    assert len(set(calls)) == len(calls) and {c[0] for c in calls} == set(mc.CASES)


def test_matched_pairs_across_thread_and_wave_diagonals():
    st = _st("thread diagonals")
    ranks = st.straddles(VT).tolist()
    assert ranks == [VT * t + VT - 1 for t in mc.DIAG_THREADS]
    assert [r for r in ranks if (r + 1) % mc.WAVE_RANKS == 0] == [mc.WAVE_RANKS - 1, 15 * mc.WAVE_RANKS - 1] == [255, 3839]
    assert st.straddles(mc.WAVE_RANKS).tolist() == [255, 3839] and st.straddles(TILE).size == 0
    lanes = {(r // VT) % mc.WAVE for r in ranks}
    assert mc.WAVE - 1 in lanes and any(0 < lane < mc.WAVE - 1 for lane in lanes)          # the last lane of a wave, and one inside
    assert max(r // mc.WAVE_RANKS for r in ranks) == mc.MP_THREADS // mc.WAVE - 1           # the last wave of the tile


@pytest.mark.parametrize("p", (1, mc.EDGE_LATER))
def test_matched_pairs_at_a_tile_edge_and_their_neighbours(p):
    assert p == 1 or p > 1
    st = _st(f"tile edge {p}: straddle")
    assert st.straddles(TILE).tolist() == [TILE * p - 1]
    assert st.from_a[TILE * p - 1] and st.second[TILE * p] and st.part[p] > 0          # tile p looks behind at a real key
    for kind, first in (("before", TILE * p - 2), ("after", TILE * p)):
        st = _st(f"tile edge {p}: {kind}")
        assert st.straddles(TILE).size == 0
        assert st.from_a[first] and st.second[first + 1] and not st.second[TILE * p]
    st = _st("every edge straddled")
    assert st.straddles(TILE).tolist() == [TILE * q - 1 for q in range(1, 6)] and st.nblocks == 6
    assert mc.CASES["tile edge 1: straddle"].dtypes == mc.TYPES


def test_one_sided_tiles_and_empty_operands():
    st = _st("A-only tile, then its partner")
    assert st.lb[1] == 0 and st.la[1] == TILE and st.straddles(TILE).tolist() == [2 * TILE - 1]
    assert st.lb[2] > 0 and st.second[2 * TILE]                       # ... whose partner opens the next tile
    st = _st("B-only tiles")
    na = mc.case_operands("B-only tiles")[0].size
    assert st.la[1] == 0 and st.la[2] == 0 and st.lb[1] == TILE and st.part[1] == st.part[2] == st.part[3] == na
    assert any((_st(n).lb == 0).any() for n in mc.CASES) and any((_st(n).la == 0).any() for n in mc.CASES)
    sizes = {n: (mc.case_operands(n)[0].size, mc.case_operands(n)[2].size) for n in mc.EMPTY_CASES}
    assert sizes == {"na = 0": (0, 5), "nb = 0": (5, 0), "nothing": (0, 0), "(1, 0)": (1, 0), "(0, 1)": (0, 1),
                     "(1, 1) equal keys": (1, 1), "(1, 1) other keys": (1, 1)}
    ka, _, kb, _ = mc.case_operands("(1, 1) equal keys")
    assert ka[0] == kb[0]
    ka, _, kb, _ = mc.case_operands("(1, 1) other keys")
    assert kb[0] < ka[0]


def test_last_tiles():
    assert mc.LAST_TILE_TOTALS == (TILE - 1, TILE, TILE + 1, TILE + 2, 2 * TILE + 1)
    for total in mc.LAST_TILE_TOTALS:
        st = _st(f"total {total}")
        ka, _, kb, _ = mc.case_operands(f"total {total}")
        assert ka.size + kb.size == total and st.second[total - 1]                      # the sequence ends in a pair's B item
        assert int(st.la[-1] + st.lb[-1]) == (total - 1) % TILE + 1
    assert _st(f"total {TILE + 1}").straddles(TILE).tolist() == [TILE - 1] and _st(f"total {TILE + 1}").la[-1] == 0
    assert _st(f"total {TILE + 2}").straddles(TILE).size == 0 and _st(f"total {TILE + 2}").la[-1] == 1
    assert _st(f"total {2 * TILE + 1}").straddles(TILE).tolist() == [2 * TILE - 1]


def test_key_range():
    for name, in_a, in_b in (("last key in A", True, False), ("last key in B", False, True), ("last key in both", True, True)):
        ka, _, kb, _ = mc.case_operands(name)
        assert (ka[-1] == mc.MAX_KEY) == in_a and (kb[-1] == mc.MAX_KEY) == in_b
        assert kb[0] == 0 and ka[0] > 0                                              # key 0, in B only: the look-behind sentinel is -1
    assert _st("last key in both").straddles(TILE).tolist() == [TILE - 1]
    assert sum(1 for n in mc.CASES if mc.case_operands(n)[0].size and mc.case_operands(n)[0][0] == 0) > 10     # key 0 in A


def test_store_route_switch():
    q = TILE // mc.STORE_FACTOR
    st = _st("store switch")
    assert tuple(st.tot[:len(mc.STORE_TOTS)].tolist()) == mc.STORE_TOTS
    assert {0, 1, q - 1, q, q + 1, TILE // 2} <= set(st.tot.tolist())
    lds = st.tot * mc.STORE_FACTOR >= TILE
    assert (lds[:-1] != lds[1:]).sum() >= 4                                       # adjacent tiles on different routes
    assert mc.CASES["store switch"].dtypes == mc.TYPES
    full = _st("full tiles", op="add")
    assert full.tot[0] == full.tot[1] == TILE and (full.threads[:2] == VT).all()    # every thread emits 4: the staging area is full
    everything = set()
    for name, dtype, op, fa, fb in mc.calls():
        if not mc.CASES[name].big:
            everything |= set(mc.case_reference(name, dtype, op, fa, fb)[3].tot.tolist())
    assert {0, 1, q - 1, q, q + 1, TILE} <= everything


def test_block_scan_mix():
    for op, fills in (("add", (0, 0)), ("multiply", (0, 0)), ("add", (2, 0))):
        st = _st("scan mix", op=op, fills=fills)
        waves = st.threads.reshape(st.nblocks, -1, mc.WAVE)
        if op == "add":
            assert any(set(w.tolist()) == {0, 1, 2, 3, 4} for w in waves[0]), "no wave holds threads of every count"
            assert {0, 1, 2, 3, 4} == set(st.threads.ravel().tolist())
        assert len(set(waves[0].sum(axis=1).tolist())) > 4                             # the waves' totals differ
    assert _st("scan mix").straddles(VT).size > 100 and _st("scan mix").straddles(TILE).size + _st("scan mix").straddles(mc.WAVE_RANKS).size > 0


def test_look_back_tile_counts():
    assert mc.LOOKBACK_TILES == (2, 63, 64, 65, 66, 129, 130) and mc.MANY_TILES == 1024
    W = mc.LOOKBACK_WINDOW
    assert {(t - 2) // W + 1 for t in mc.LOOKBACK_TILES} == {1, 2, 3}                 # windows the last tile may have to read
    assert {W - 1, W, W + 1, W + 2, 2 * W + 1, 2 * W + 2} <= set(mc.LOOKBACK_TILES)
    for tiles in mc.LOOKBACK_TILES + (mc.MANY_TILES,):
        st = _st(f"look-back {tiles} tiles")
        assert st.nblocks == tiles
        tots = st.tot.tolist()
        assert (tiles == 2 or (0 in tots[:-1] and len(set(tots)) >= 4)) and 0 < st.la[-1] + st.lb[-1] < TILE
        assert _st(f"look-back {tiles} tiles", op="add").total > st.total > 0


def test_recipe_switch_and_skew():
    B = mc.MERGE_FUSED_MAX_ITEMS
    assert mc.RECIPE_TOTALS == (B - 1, B, B + 1)
    for total in mc.RECIPE_TOTALS:
        ka, _, kb, _ = mc.case_operands(f"recipe {total}")
        assert ka.size + kb.size == total and ka.size != kb.size and np.intersect1d(ka, kb).size > total // 8
    sizes = {n: (mc.case_operands(n)[0].size, mc.case_operands(n)[2].size) for n in ("skew 10 + 40000", "skew 40000 + 10")}
    assert sizes == {"skew 10 + 40000": (10, 40_000), "skew 40000 + 10": (40_000, 10)}
    for n in sizes:
        ka, _, kb, _ = mc.case_operands(n)
        assert np.intersect1d(ka, kb).size == 5
    ka, _, kb, _ = mc.case_operands("A below B")
    assert ka[-1] < kb[0] and ka.size > TILE and kb.size > TILE
    ka, _, kb, _ = mc.case_operands("B below A")
    assert kb[-1] < ka[0] and ka.size > TILE and kb.size > TILE


def test_value_types_and_fills():
    assert set(mc.TYPES) == {"float32", "float64", "int32", "int64", "uint8", "bool", "complex64", "complex128"}
    for name in ("tile edge 1: straddle", "store switch"):
        for dtype in mc.TYPES:
            ops = mc.case_ops(name, dtype)
            out_types = {mc.fill_result(op, np.dtype(dtype), fa, fb).dtype for op, fa, fb in ops}
            assert np.dtype(bool) in out_types and (np.dtype(dtype) in out_types)         # one to-bool op, one same-type op
            assert any(fa != 0 for _, fa, _ in ops)                                       # a non-zero fill on one side
            for op, fa, fb in ops:
                keys, vals, fo, st = mc.case_reference(name, dtype, op, fa, fb)
                assert 0 < keys.size < st.keys.size
    st = mc.case_reference("tile edge 1: straddle", "complex128", "multiply", 0, 0)[3]
    assert st.total == np.count_nonzero(st.second)             # with zero fills only the matched pairs survive a product


def test_cases_of_the_older_union():
    names = set(mc.UNION_MERGE_CASES)
    assert names >= set(mc.EMPTY_CASES) and {n for n in mc.CASES if n.startswith("tile edge")} <= names
    assert {"A-only tile, then its partner", "B-only tiles", "grid second trip"} <= names
    ka, _, kb, _ = mc.case_operands("grid second trip")
    assert ka.size + kb.size == mc.N1 + 257 and np.intersect1d(ka, kb).size > 100_000

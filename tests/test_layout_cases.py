"""The cases of tests/layout_cases.py hold what their names promise, and its references agree with a brute-force evaluation
on the dense array - shown from the inputs alone, without a GPU.  `hot_piece_plan` is pure host arithmetic: its properties
are tested here as well."""
import numpy as np

import layout_cases as lc


def test_the_constants_are_the_sources():
    c = lc.source_constants()
    assert (c["RL_MAX_SLABS"], c["RL_MAX_CELLS"], c["RL_CAP"], c["RL_MAX_PER_CELL"], c["RL_GAP"]) == \
        (lc.RL_MAX_SLABS, lc.RL_MAX_CELLS, lc.RL_CAP, lc.RL_MAX_PER_CELL, lc.RL_GAP)
    assert c["BC_BLOCK"] == c["HOT_BLOCK"] == lc.BLOCK and c["TILE"] == lc.TILE
    from sparse_amd import _batched, _dot

    src = open(_batched.__file__).read()
    assert "len(coos) <= %d" % lc.CONCAT_MERGE_MAX_OPERANDS in src
    assert "element_size() in (%s)" % ", ".join(map(str, lc.CONCAT_MERGE_ELEMENT_SIZES)) in src
    assert _dot.HOT_COMBINE_FAN == 128 and max(lc.COMBINE_PIECES) == _dot.HOT_COMBINE_FAN + 1 and _dot.HOT_COMBINE_FAN in lc.COMBINE_PIECES


# ---- A ----------------------------------------------------------------------------------------------------------------------
def _lead_brute(case):
    """the dense [S, P] array of element numbers, transposed and read in C order"""
    d = np.zeros((case.S, case.P), dtype=np.int64)
    s, c = np.divmod(case.keys, case.P)
    d[s, c] = np.arange(1, case.keys.size + 1)
    t = d.T.reshape(-1)
    at = np.flatnonzero(t)
    return at, t[at] - 1


def test_lead_last_cases_hold_what_their_names_promise():
    seen_failed, seen_ok = 0, 0
    for name in lc.LEAD_CASES:
        case = lc.lead_case(name)
        S, P, cells, keys = case.S, case.P, case.cells, case.keys
        assert case.name == name
        assert 1 <= S <= lc.RL_MAX_SLABS and 1 <= cells <= lc.RL_MAX_CELLS and cells & (cells - 1) == 0 and 1 <= P < 2 ** 42
        assert keys.dtype == np.int64 and keys.size >= 1 and (np.diff(keys) > 0).all() and 0 <= keys[0] and keys[-1] < S * P, name
        failed = lc.lead_predicts_failed(keys, S, P, cells)
        assert failed == bool(lc.lead_failed_ranges(keys, S, P, cells).any())
        seen_failed += failed
        seen_ok += not failed
        # the reference against the dense array (where that array is small)
        vals = lc.payload_bits(keys.size, 8, seed=3)
        rk, rv = lc.ref_lead_last(keys, vals, S, P)
        assert (np.diff(rk) > 0).all()
        if S * P <= 1 << 22:
            bk, bsrc = _lead_brute(case)
            assert np.array_equal(rk, bk) and np.array_equal(rv, vals[bsrc]), name
        # the table against its definition, word by word, on a sample of words
        table = lc.lead_table(keys, S, P, cells)
        ranges = -(-P // cells)
        assert table.size == S * (ranges + 1)
        s_of, c_of = np.divmod(keys, P)
        rng = np.random.default_rng(1)
        for t in rng.integers(0, table.size, size=20):
            b, s = divmod(int(t), S)
            assert table[t] == np.count_nonzero((s_of < s) | ((s_of == s) & (c_of < min(b * cells, P)))), name
    assert seen_failed >= 10 and seen_ok >= 50

    def counts(name):
        c = lc.lead_case(name)
        return lc.lead_counts(c.keys, c.S, c.P, c.cells)

    def gaps(name):
        c = lc.lead_case(name)
        return lc.lead_word_gaps(c.keys, c.S, c.P, c.cells)

    def failed(name):
        c = lc.lead_case(name)
        return lc.lead_predicts_failed(c.keys, c.S, c.P, c.cells)

    # the grid: every S x cells x P of the issue, the last range partial where P is no multiple of the cells
    for S in lc.LEAD_GRID_S:
        for cells in lc.LEAD_GRID_CELLS:
            for P in (1, cells - 1, cells, cells + 1, 7 * cells + 3):
                if P >= 1:
                    c = lc.lead_case(f"grid S={S} cells={cells} P={P}")
                    assert (c.S, c.P, c.cells) == (S, P, cells)
    assert (7 * 64 + 3) % 64 != 0
    # a cell of exactly 64 and of 65 elements from the grid alone: one cell, every slab stored
    assert counts("grid S=64 cells=1 P=1")[1] == 64 and not failed("grid S=64 cells=1 P=1")
    assert counts("grid S=65 cells=1 P=1")[1] == 65 and failed("grid S=65 cells=1 P=1")
    # empty slabs
    for name, empty in (("empty slabs at the head", range(0, 30)), ("empty slabs in the middle", range(20, 75)),
                        ("90 empty trailing slabs", range(110, 200))):
        c = lc.lead_case(name)
        stored = np.unique(c.keys // c.P)
        assert not np.isin(np.asarray(empty), stored).any() and stored.size == c.S - len(empty), name
        assert not failed(name)
    assert len(range(110, 200)) == 90
    # gaps in table words
    assert gaps("gap of 8 words inside a run")[1] == 8 and gaps("gap of 9 words inside a run")[1] == 9
    assert gaps("gap of 8 words across a run end")[1] == 8 and gaps("gap of 9 words across a run end")[1] == 9
    for name in ("gap of 8 words across a run end", "gap of 9 words across a run end"):
        c = lc.lead_case(name)
        assert c.keys[0] // c.P != c.keys[1] // c.P
    for name in ("gap of 8 words inside a run", "gap of 9 words inside a run"):
        c = lc.lead_case(name)
        assert c.keys[0] // c.P == c.keys[1] // c.P
    assert gaps("first element 8 words into the table")[0] == 8 and gaps("first element 9 words into the table")[0] == 9
    g = gaps("n=1 no word written by an element")
    assert g.size == 1 and g[0] > lc.RL_GAP
    g = gaps("n=1 every word before it written by the element")
    assert g.size == 1 and g[0] == lc.RL_GAP
    # the limits
    per_range, most = counts("S=P=cells=64 full: 4096 in the range, 64 in every cell")
    c = lc.lead_case("S=P=cells=64 full: 4096 in the range, 64 in every cell")
    assert per_range.tolist() == [lc.RL_CAP] and most == lc.RL_MAX_PER_CELL and not failed(c.name)
    assert (np.unique(c.keys % c.P, return_counts=True)[1] == 64).all()
    per_range, most = counts("S=65 P=cells=64 full: 4160 in the range")
    assert per_range.tolist() == [4160] and most == 65 and failed("S=65 P=cells=64 full: 4160 in the range")
    per_range, most = counts("S=2048 cells=4: 4096 in one range")
    assert per_range[0] == 4096 and most == 1024 and failed("S=2048 cells=4: 4096 in one range")     # (the cells are over their limit)
    per_range, most = counts("S=2048 cells=4: 4097 in one range")
    assert per_range[0] == 4097 and failed("S=2048 cells=4: 4097 in one range")
    per_range, most = counts("S=2048 cells=64: 4096 in one range, 64 in every cell")
    assert per_range[0] == 4096 and most == 64 and not failed("S=2048 cells=64: 4096 in one range, 64 in every cell")
    per_range, most = counts("S=2048 cells=64: 4097 in one range")
    assert per_range[0] == 4097 and most == 65 and failed("S=2048 cells=64: 4097 in one range")
    per_range, most = counts("S=2048 cells=64: 4096 in one range, one cell of 65")
    assert per_range[0] == 4096 and most == 65 and failed("S=2048 cells=64: 4096 in one range, one cell of 65")
    per_range, most = counts("two full ranges then a partial one")
    assert per_range.tolist() == [4096, 4096, 640] and most == 64 and not failed("two full ranges then a partial one")
    c = lc.lead_case("S=2048 P=2048*1000+5: a large, mostly untouched table")
    assert (c.S, c.P, c.cells) == (2048, 2048 * 1000 + 5, 2048) and 2000 <= c.keys.size <= 9000 and not failed(c.name)
    assert c.S * (-(-c.P // c.cells) + 1) > 100 * c.keys.size
    # the product-level inputs: with the cells per range the library's own plan picks for them, some are merged and some are
    # refused (`failed`), so `x.sum(axis=0)` on them exercises the fall-back to the sort
    from sparse_amd import _kernels

    outcomes = set()
    for name in lc.LEAD_PRODUCT_CASES:
        c = lc.lead_case(name)
        plan = _kernels.lead_last_plan(c.keys.size, c.S, c.P, lc.RL_MAX_SLABS, lc.RL_MAX_CELLS)
        outcomes.add("sort" if plan is None else "refused" if lc.lead_predicts_failed(c.keys, c.S, c.P, plan[0]) else "merged")
    assert {"refused", "merged"} <= outcomes
    lim = {"S=2049": lambda S, P, cells, vb: S == lc.RL_MAX_SLABS + 1, "cells=3": lambda S, P, cells, vb: cells == 3,
           "cells=4096": lambda S, P, cells, vb: cells == 2 * lc.RL_MAX_CELLS, "val_bytes=2": lambda S, P, cells, vb: vb == 2,
           "P=2**42": lambda S, P, cells, vb: P == 2 ** 42}
    for what, vb, n, S, P, cells, code in lc.LEAD_ERRORS:
        assert lim[what](S, P, cells, vb) and code in (lc.EINVAL, lc.ETYPE)


# ---- B ----------------------------------------------------------------------------------------------------------------------
def test_broadcast_cases_hold_what_their_names_promise():
    combos = set()
    for name in lc.BCAST_CASES:
        c = lc.bcast_case(name)
        assert c.name == name
        k = c.keys
        assert k.dtype == np.int64 and k.size >= 1 and (np.diff(k) > 0).all() and 0 <= k[0] and k[-1] < c.k1 * c.k2, name
        if name.startswith("groups "):
            combos.add(tuple(v > 1 for v in (c.b0, c.k1, c.b1, c.k2, c.b2)))
            assert all(v == 1 or 2 <= v <= 5 for v in (c.b0, c.k1, c.b1, c.k2, c.b2))
        # the reference against np.broadcast_to of the dense operand holding element numbers
        vals = lc.payload_bits(k.size, 4, seed=1)
        rk, rv = lc.ref_broadcast(k, vals, c.b0, c.k1, c.b1, c.k2, c.b2)
        d = np.zeros(c.k1 * c.k2, dtype=np.int64)
        d[k] = np.arange(1, k.size + 1)
        big = np.broadcast_to(d.reshape(1, c.k1, 1, c.k2, 1), (c.b0, c.k1, c.b1, c.k2, c.b2)).reshape(-1)
        at = np.flatnonzero(big)
        assert np.array_equal(rk, at) and np.array_equal(rv, vals[big[at] - 1]), name
    assert len(combos) == 32

    def runs(name):
        c = lc.bcast_case(name)
        return lc.run_lengths(c.keys, c.k2), c

    for name, p1 in (("one run, its p1 first", 0), ("one run, its p1 in the middle", 2), ("one run, its p1 last", 4)):
        r, c = runs(name)
        assert r.tolist() == [200] and c.keys[0] // c.k2 == p1 and c.k1 == 5
    r, c = runs("every run of length 1")
    assert (r == 1).all() and r.size == c.k1 == 50
    r, c = runs("runs of 2, 3, 257 and 1000 beside runs of 1")
    assert r.tolist() == [1, 2, 1, 3, 1, 257, 1, 1000, 1, 1, 1]
    r, c = runs("long first and last runs")
    assert r[0] == 1000 and r[-1] == 257 and c.keys[0] // c.k2 == 0 and c.keys[-1] // c.k2 == c.k1 - 1    # element 0 and n - 1
    assert lc.bcast_case("n=1").keys.size == 1
    for n_out in (255, 256, 257):
        c = lc.bcast_case(f"n_out={n_out}")
        assert c.keys.size * c.b0 * c.b1 * c.b2 == n_out
    assert (255, 256, 257) == (lc.BLOCK - 1, lc.BLOCK, lc.BLOCK + 1)
    r, c = runs("b2=1 with b1>1, long runs")
    assert c.b2 == 1 and c.b1 > 1 and r.max() > 256
    r, c = runs("b1=1 with b2>1, long runs")
    assert c.b1 == 1 and c.b2 > 1 and r.max() > 256
    r, c = runs("k1=1 with every other group non-trivial")
    assert c.k1 == 1 and min(c.b0, c.b1, c.k2, c.b2) > 1 and r.tolist() == [600]


# ---- C ----------------------------------------------------------------------------------------------------------------------
def test_transpose_cases_hold_what_their_names_promise():
    assert set(lc.TRANSPOSE_EXTENTS) >= {1, lc.TILE - 1, lc.TILE, lc.TILE + 1, 2 * lc.TILE + 1}
    for nbytes in lc.TRANSPOSE_ELEM_BYTES:
        for rows, cols in ((1, 1), (63, 129), (65, 64)):
            wide, sentinel = lc.transpose_case(rows, cols, nbytes)
            assert wide.shape == (rows, cols + 3) and wide.dtype.itemsize == nbytes and sentinel.dtype == wide.dtype
            want = lc.ref_transpose_into(wide, cols, sentinel)
            assert want.shape == (cols, rows + 5)
            for r in range(rows):
                for c in range(0, cols, 7):
                    assert want[c, r] == wide[r, c]
            assert (want[:, rows:] == sentinel).all()
            # the sentinel is no value of the block's (an unwritten element cannot pass for a written one by chance everywhere)
            assert np.count_nonzero(wide == sentinel) <= wide.size // 64 + 1


# ---- D ----------------------------------------------------------------------------------------------------------------------
def test_combine_reference_is_the_sequential_sum():
    for dtype in lc.COMBINE_DTYPES:
        part = lc.combine_parts(20, 5, dtype)
        vfirst, rows = np.array([0, 3, 3, 20]), np.array([4, 0, 2])
        out0 = np.full((6, 5), 9, dtype=dtype)
        got = lc.ref_combine(part, vfirst, rows, out0)
        for h, r in enumerate(rows):
            for c in range(5):
                acc = np.dtype(dtype).type(0)
                with np.errstate(over="ignore"):
                    for v in range(vfirst[h], vfirst[h + 1]):
                        acc = acc + part[v, c]
                assert got[r, c].tobytes() == np.asarray(acc, dtype=dtype).tobytes()
        assert (got[[1, 3, 5]] == 9).all() and (got[0] == 0).all()      # rows not named are kept; a hot row without pieces is zero
    # the float cases are sensitive to the order of the additions, the integer cases wrap around
    p = lc.combine_parts(129, 257, "float32")
    zero = np.zeros((1, 257), np.float32)
    assert (lc.ref_combine(p[::-1], [0, 129], [0], zero)[0] != lc.ref_combine(p, [0, 129], [0], zero)[0]).any()
    p = lc.combine_parts(129, 257, "int32").astype(np.int64)
    assert (np.abs(p.sum(axis=0)) > 2 ** 31).any()


def _plan_lens(which):
    return list(lc.PLAN_ROW_LENGTHS) + list(lc.PLAN_FILLERS[which])


def test_hot_piece_plan_cuts_every_row_into_pieces_of_one_size():
    for which in lc.PLAN_FILLERS:
        _check_piece_plan(which)
    _check_piece_plan_groups_from_129_pieces_on()


def _check_piece_plan(which):
    from sparse_amd import _dot

    groups, fan = _dot.HOT_PIECE_GROUPS, _dot.HOT_COMBINE_FAN
    lens = _plan_lens(which)
    gap = 11                               # the hot rows do not touch in the operand: the plan sees their lengths only
    p0 = np.cumsum([5] + [n + gap for n in lens[:-1]])
    p1 = p0 + np.asarray(lens)
    vptr, vfirst, g1 = _dot.hot_piece_plan(p0, p1)
    total = sum(lens)
    piece, counts, want_vptr, want_g1 = lc.ref_piece_plan(lens, groups, fan)
    assert piece == {"piece 32": 32, "piece 96": 96, "piece 4096": 4096}[which]
    assert piece % 32 == 0 and 32 <= piece <= 4096
    assert vptr[0] == 0 and vptr[-1] == total and (np.diff(vptr) > 0).all()
    assert np.array_equal(vptr, want_vptr)
    sizes = np.diff(vptr)
    firsts = np.concatenate([[0], np.cumsum(counts)])
    for h, n in enumerate(lens):           # row h's pieces: all of the common size but the last, together its elements
        mine = sizes[firsts[h]:firsts[h + 1]]
        assert (mine[:-1] == piece).all() and 1 <= mine[-1] <= piece and mine.sum() == n
    if max(counts) <= fan:
        assert g1 is None and want_g1 is None
        assert np.array_equal(vfirst, firsts)                       # vfirst[h] .. vfirst[h + 1] are exactly row h's pieces
    else:
        assert g1 is not None and np.array_equal(g1, want_g1)
        assert g1[0] == 0 and g1[-1] == len(vptr) - 1 and (np.diff(g1) >= 1).all() and (np.diff(g1) <= fan).all()
        assert vfirst[0] == 0 and vfirst[-1] == len(g1) - 1
        for h in range(len(lens)):         # row h's groups cover exactly its pieces, in order, and no group spans two rows
            assert g1[vfirst[h]] == firsts[h] and g1[vfirst[h + 1]] == firsts[h + 1]
            assert vfirst[h + 1] - vfirst[h] == -(-counts[h] // fan)


def _check_piece_plan_groups_from_129_pieces_on():
    from sparse_amd import _dot

    fan = _dot.HOT_COMBINE_FAN
    for n, pieces, grouped in ((4096, 128, False), (4097, 129, True), (4128, 129, True), (4129, 130, True)):
        vptr, vfirst, g1 = _dot.hot_piece_plan([0], [n])
        assert len(vptr) - 1 == pieces and (pieces > fan) == grouped and (g1 is not None) == grouped
        if grouped:
            assert g1.tolist() == [0, fan, pieces] and vfirst.tolist() == [0, 2]
    # an explicit fan: the same rule at a small size
    vptr, vfirst, g1 = _dot.hot_piece_plan([0, 100], [100, 200], groups=1, fan=3)
    assert np.diff(vptr).tolist() == [32, 32, 32, 4] * 2 and g1.tolist() == [0, 3, 4, 7, 8] and vfirst.tolist() == [0, 2, 4]


def test_hub_matrix_has_the_rows_its_test_needs():
    from sparse_amd import _dot

    indptr, indices, long_rows = lc.hub_matrix(hot_min=_dot.HOT_ROW_MIN, min_nnz=_dot.HOT_ROW_MIN_NNZ)
    lens = np.diff(indptr)
    assert sorted(long_rows.values()) == [_dot.HOT_ROW_MIN - 1, _dot.HOT_ROW_MIN, 4129]
    assert all(lens[r] == n for r, n in long_rows.items())
    assert np.flatnonzero(lens >= _dot.HOT_ROW_MIN).tolist() == sorted(r for r, n in long_rows.items() if n >= _dot.HOT_ROW_MIN)
    short = np.delete(lens, list(long_rows))
    assert short.max() < 200 and indptr[-1] >= _dot.HOT_ROW_MIN_NNZ and indices.size == indptr[-1]
    for r in range(len(lens)):
        assert (np.diff(indices[indptr[r]:indptr[r + 1]]) > 0).all()
    hot = [n for n in long_rows.values() if n >= _dot.HOT_ROW_MIN]
    piece, counts, _, g1 = lc.ref_piece_plan(hot, _dot.HOT_PIECE_GROUPS, _dot.HOT_COMBINE_FAN)
    assert piece == 32 and sorted(counts) == [128, 130] and g1 is not None          # more than the fan: a two-level combine
    # the bound's reference against a plain loop
    data = lc.hub_values(int(indptr[-1]), np.float32)
    b = np.random.default_rng(0).standard_normal((6000, 3)).astype(np.float32)
    want, bound = lc.hub_bound(indptr, indices, data, b, np.float32)
    for r in (17, 0, len(lens) - 1):
        sl = slice(indptr[r], indptr[r + 1])
        assert np.allclose(want[r], data[sl].astype(np.float64) @ b[indices[sl]].astype(np.float64), rtol=1e-12, atol=1e-12)
    assert (bound[17] > 0).all() and bound.shape == want.shape


# ---- E ----------------------------------------------------------------------------------------------------------------------
def test_index_cases_hold_what_their_names_promise():
    d = lc.index_dense()
    assert d.shape == lc.INDEX_SHAPE and 0.25 < np.count_nonzero(d) / d.size < 0.55
    cases = lc.index_cases()
    kinds, n_moved = set(), 0
    for name, index in cases.items():
        arrs = [i for i in index if isinstance(i, lc.Arr)]
        assert len(arrs) == 1, name
        kinds.add(arrs[0].kind)
        numpys = d[lc.as_numpy_index(index)]                # NumPy accepts every case
        want = lc.index_expected(d, index)
        assert np.array_equal(want, lc.index_by_axis(d, index)) and want.shape == lc.index_by_axis(d, index).shape, name
        moved, place = lc.numpy_moves_the_array_axis_first(index)
        # NumPy's own result is the expectation - except with an integer before the array and a slice between them, where NumPy
        # moves the array's axis to the front and the library, like its reference, leaves it in place (tests/golden pins that)
        assert moved == (isinstance(index[0], int) and isinstance(index[-1], lc.Arr) and len(index) == 3), name
        if moved:
            n_moved += 1
            assert want.shape == numpys.shape[1:] + numpys.shape[:1] and np.array_equal(np.moveaxis(want, -1, 0), numpys)
        else:
            assert want.shape == numpys.shape and np.array_equal(want, numpys)
        axis = int(name.split()[1])
        real = [i for i in index if i is not None]
        if Ellipsis not in index:
            assert isinstance(real[axis], lc.Arr), name
        if "None before" in name:
            assert index[index.index(arrs[0]) - 1] is None
        if "None after" in name:
            assert index[index.index(arrs[0]) + 1] is None
        if "integer on axis" in name:
            other = int(name.rsplit(" ", 1)[1])
            assert isinstance(index[other], int) and want.ndim == 2
        if "step -2" in name:
            other = int(name.rsplit(" ", 1)[1])
            assert index[other].step == -2
    assert kinds == {"list", "bool", "int32", "tensor"}
    assert n_moved == 11 * 2                                 # "axis 2 <array>, (negative) integer on axis 0" alone
    for axis, n in enumerate(lc.INDEX_SHAPE):
        a = lc.array_indices(n)
        assert a["empty"].values == () and len(set(a["duplicates out of order"].values)) < len(a["duplicates out of order"].values)
        assert list(a["duplicates out of order"].values) != sorted(a["duplicates out of order"].values)
        assert list(a["descending"].values) == sorted(a["descending"].values, reverse=True) and len(a["descending"].values) == n
        assert all(v < 0 for v in a["negative"].values) and min(a["negative"].values) >= -n
        assert list(a["full range"].values) == list(range(n))
        assert not any(a["mask none"].values) and all(a["mask all"].values) and 0 < sum(a["mask some"].values) < n
        assert all(len(a[k].values) == n for k in ("mask none", "mask some", "mask all"))
    # every (start, stop, step) of the slice sweep is a slice NumPy takes
    assert len(lc.SLICE_POINTS) == 14 and set(lc.SLICE_STEPS) == {-3, -2, -1, 1, 2, 3}
    assert lc.SLICE_DENSE_1D.shape == (5,) and lc.SLICE_DENSE_2D.shape[0] == 5


# ---- F ----------------------------------------------------------------------------------------------------------------------
def test_join_cases_hold_what_their_names_promise():
    cases = lc.join_cases()
    assert len({c.name for c in cases}) == len(cases)
    routes = {}
    for c in cases:
        nd = len(c.operands[0].shape)
        axis = c.axis % nd
        dense = [lc.operand_dense(o) for o in c.operands]
        want = np.concatenate(dense, axis=c.axis)
        dt = np.result_type(*[d.dtype for d in dense])
        assert want.dtype == dt
        nonempty = sum(1 for d in dense if np.count_nonzero(d))
        merge = axis != 0 and len(c.operands) <= 8 and dt.itemsize in (1, 4, 8) and nonempty >= 1
        assert c.route == ("append" if axis == 0 else "merge" if merge else "sort"), c.name
        routes.setdefault(c.route, []).append(c.name)
        if "empty operand" in c.name:
            k = {"first": 0, "middle": 1, "last": 2}[c.name.split()[2]]
            assert [np.count_nonzero(d) == 0 for d in dense] == [i == k for i in range(3)]
        if c.name.startswith("all operands empty"):
            assert nonempty == 0
        if "different extents" in c.name:
            assert len({d.shape[axis] for d in dense}) > 1
        if "coordinates" in c.name:
            assert {o.idx for o in c.operands} == {"int32", "int64"}
        if "promoted" in c.name:
            assert len({o.dtype for o in c.operands}) > 1 and all(o.dtype in lc.CONVERTIBLE for o in c.operands)
        if c.name.startswith("int16"):
            assert dt.itemsize == 2 and c.route != "merge"
        if c.route == "sort" and nonempty >= 2:
            assert lc.concat_keys_unsorted(c.operands, axis), c.name       # the sort has something to do
    by = {c.name: c for c in cases}
    assert by["8 operands axis 1"].route == "merge" and by["9 operands axis 1"].route == "sort"
    assert by["8 operands axis -1"].route == "merge" and by["9 operands axis -1"].route == "sort"
    assert by["1 operands axis 2"].route == "merge" and by["int16 axis 1"].route == "sort" and by["int8 axis 1"].route == "merge"
    assert all(len(v) >= 5 for v in routes.values()) and set(routes) == {"append", "merge", "sort"}
    g = lc.gcxs_join_cases()
    assert len({c[0] for c in g}) == len(g)
    for name, ops, ca, axis, asked, fast in g:
        want_fast = (axis % 2 == ca) and (asked is None or tuple(asked) == (axis % 2,))
        assert fast == want_fast, name
        if "empty rows" in name:
            d = [lc.operand_dense(o) for o in ops]
            assert any((np.count_nonzero(x, axis=1 - ca) == 0).any() for x in d)
        if "an empty operand" in name:
            assert any(np.count_nonzero(lc.operand_dense(o)) == 0 for o in ops)
        if "mixed pointer widths" in name:
            assert {o.idx for o in ops} == {"int32", "int64"}

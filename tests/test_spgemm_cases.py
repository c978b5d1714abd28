"""tests/spgemm_cases.py on its own, without a GPU: the constants the table was built for against the source text, the
reference against the CPU oracle and against a dense exact product, its signed zeros, its sensitivity to the order of A's
elements, and the table against every boundary it claims - product counts, classes, buckets, passes, key bits, fill, cells,
window alignment, and the route and `heavy_or_declined` count that follow from them by the host's rules.  A boundary that a
case claims and does not meet is a failure here, not a weaker GPU test."""
import numpy as np
import pytest

import spgemm_cases as sc


# ---- the constants, from the source ------------------------------------------------------------------------------------
def test_constants_in_the_source_are_the_ones_the_table_was_built_for():
    src = sc.source_constants()
    assert src["SPG_BUCKET_MAX"] == sc.SPG_BUCKET_MAX == 16
    assert (src["c0"], src["c1"]) == (sc.C0, sc.C1) == (1024, 4096)
    assert src["MID"] == (12, 16, 14) and src["TOP"] == (8, 24)
    assert (src["c2_block"], src["c3_block"], src["c4_block"]) == (512, 512, 1024)
    for kb, vb in ((4, 4), (4, 8), (8, 4), (8, 8)):
        mid = src["MID"][1] if kb + vb <= src["MID"][0] else src["MID"][2]
        top = src["TOP"][1] if kb + vb <= src["TOP"][0] else mid
        assert sc.mid_top(kb, vb) == (mid, top)
        assert sc.bounds(kb, vb) == (1024, 4096, 512 * mid, 512 * top, 1024 * top)
    assert [sc.bounds(kb, vb)[2:] for kb, vb in ((4, 4), (4, 8), (8, 4), (8, 8))] == [
        (8192, 12288, 24576), (8192, 8192, 16384), (8192, 8192, 16384), (7168, 7168, 14336)]
    assert src["classes"] == [("", 256, "4", 1, "-1", "c0"), ("max_prod > C::c0", 512, "8", 1, "c0", "c1"),
                              ("max_prod > C::c1", 512, "MID", 2, "c1", "c2"),
                              ("max_prod > C::c2 && C::c3 > C::c2", 512, "TOP", 2, "c2", "c3"),
                              ("max_prod > C::c3", 1024, "TOP", 8, "c3", "c4")]
    names = {"4": 4, "8": 8}
    for kb, vb in ((4, 4), (8, 8)):
        mid, top = sc.mid_top(kb, vb)
        b = dict(zip(("c0", "c1", "c2", "c3", "c4"), sc.bounds(kb, vb)), **{"-1": -1})
        want = [(blk, {**names, "MID": mid, "TOP": top}[it], p, b[lo], b[hi]) for _, blk, it, p, lo, hi in src["classes"]]
        got = sc.row_classes(kb, vb)
        assert [g for g in got if g is not None] == [w for w, g in zip(want, got) if g is not None]
        assert (got[3] is None) == (b["c3"] == b["c2"])
    assert [(sc.capp(*c), sc.nbp(*c)) for c in ((256, 4, 1), (512, 8, 1), (512, 16, 2), (512, 14, 2), (512, 24, 2), (1024, 24, 8),
                                                 (1024, 16, 8), (1024, 14, 8))] == [
        (1024, 512), (4096, 2048), (4608, 4096), (4032, 2048), (6912, 4096), (3456, 4096), (2304, 4096), (2016, 2048)]
    assert [sc.stage(*c) for c in ((256, 4, 1), (512, 8, 1), (512, 14, 2), (1024, 14, 8), (1024, 24, 8))] == [1024, 2048, 2048, 2016, 2048]
    assert src["N_COL_LIMIT"] == sc.N_COL_LIMIT == 2147483647
    assert (src["sm_lds_kb"], src["sm_reserve"]) == (64, 32)
    assert [sc.sm_max_cols(vb, w) for vb in (4, 8) for w in (4, 1)] == [3964, 15879, 2012, 8062]
    assert (src["SMALL_MAX_CELLS"], src["SMALL_MAX_NNZ"]) == (sc.SMALL_MAX_CELLS, sc.SMALL_MAX_NNZ) == (1 << 22, 1 << 16)
    assert (src["RUN_PROBE_MIN"], src["RUN_DUPS_MIN"], src["LONG_RUN_WINDOW"]) == (sc.RUN_PROBE_MIN, sc.RUN_DUPS_MIN, sc.LONG_RUN_WINDOW)
    assert sc.RUN_DUPS_MIN == sc.LONG_RUN_WINDOW - 1 == 1023 and sc.RUN_PROBE_MIN == 8192
    assert [sc.spg_bits(n) for n in (0, 1, 2, 3, 4, 2 ** 27 - 1, 2 ** 27, 2 ** 31 - 2)] == [1, 1, 2, 2, 3, 27, 28, 31]
    assert sc.key_bits(2 ** 27 - 1, 32) == 32 and sc.key_bits(2 ** 27 - 1, 33) == 33


# ---- the reference --------------------------------------------------------------------------------------------------------
def _sample(dtype, pool, seed, n_row=40, n_inner=50, n_col=60):
    st = sc._random_struct(n_row, n_inner, n_col, lambda r: (r * 7) % 23, lambda k: (k * 5) % 17, seed, ends=False)
    return st, sc.operands(st, pool, dtype, seed)


def _oracle_sorted(orc, st, A, B):
    wd, wi, wp = orc.dot_csr_csr((st.n_row, st.n_col), A[0], B[0], A[1], B[1], A[2], B[2])
    wd, wi = wd.copy(), wi.copy()
    for r in range(st.n_row):                          # (the reference emits rows in reverse discovery order)
        o = np.argsort(wi[wp[r]:wp[r + 1]], kind="stable")
        wd[wp[r]:wp[r + 1]], wi[wp[r]:wp[r + 1]] = wd[wp[r]:wp[r + 1]][o], wi[wp[r]:wp[r + 1]][o]
    return wd, wi, wp


def _same(got, want):
    gd, gi, gp = got
    wd, wi, wp = want
    assert np.array_equal(gp, wp) and np.array_equal(gi, wi)
    assert gd.dtype == wd.dtype and np.array_equal(sc.bits_of(gd), sc.bits_of(wd))


@pytest.mark.parametrize("dtype", sc.REAL_TYPES)
def test_the_reference_is_the_oracle_bit_for_bit(orc, dtype):
    for pool in sc.pools_of(dtype):
        for seed in (1, 2):
            st, (A, B) = _sample(dtype, pool, seed)
            _same(sc.spgemm_ref(st.n_row, st.n_col, A, B), _oracle_sorted(orc, st, A, B))
    if np.dtype(dtype).kind == "f":
        for n_col, filler in ((97, 3), (sc.N32, 0)):
            st = sc.zeros_struct(n_col, filler)
            A, B = sc.operands(st, "zeros", dtype)
            _same(sc.spgemm_ref(st.n_row, st.n_col, A, B), _oracle_sorted(orc, st, A, B))


@pytest.mark.parametrize("dtype", sc.REAL_TYPES + sc.COMPLEX_TYPES)
def test_on_exact_values_the_reference_is_the_dense_integer_product(dtype):
    st, (A, B) = _sample(dtype, "exact", 3)
    if np.dtype(dtype).kind == "c":                    # the dense product of the real parts: take real operands
        A, B = (A[0].real.astype(dtype), *A[1:]), (B[0].real.astype(dtype), *B[1:])
    data, indices, indptr = sc.spgemm_ref(st.n_row, st.n_col, A, B)
    dense, cols = sc.dense_exact(st.n_row, st.n_col, A, B)
    rows = np.repeat(np.arange(st.n_row), np.diff(indptr))
    assert np.array_equal(data.real.astype(np.int64), dense[rows, np.searchsorted(cols, indices)])
    assert not np.iscomplexobj(data) or not data.imag.any()
    stored = np.zeros(dense.shape, dtype=bool)
    stored[rows, np.searchsorted(cols, indices)] = True
    assert not dense[~stored].any()                    # what the reference does not store is zero
    assert data.dtype == np.dtype(dtype) and data.size > 200


@pytest.mark.parametrize("dtype", ("int32", "int64"))
def test_the_wrap_pool_wraps(dtype):
    st, (A, B) = _sample(dtype, "wrap", 4)
    x = sc.Expanded(st.n_row, st.n_col, A, B)
    exact = A[0].astype(object)[0] * B[0].astype(object)[0]
    assert abs(exact) > np.iinfo(dtype).max                       # a single product is beyond the type
    data = sc.spgemm_ref(st.n_row, st.n_col, A, B, x)[0]
    big = [sum(int(v) for v in x.vals[s:s + n].astype(object)) for s, n in zip(x.start, x.length)]
    bits = 8 * np.dtype(dtype).itemsize
    wrapped = np.array([((v + 2 ** (bits - 1)) % 2 ** bits) - 2 ** (bits - 1) for v in big], dtype=dtype)
    assert np.array_equal(data, wrapped) and any(abs(v) > np.iinfo(dtype).max for v in big)


@pytest.mark.parametrize("dtype", ("float32", "float64", "complex64", "complex128"))
def test_the_reference_never_returns_a_negative_zero(dtype):
    st = sc.zeros_struct(97, 3)
    A, B = sc.operands(st, "zeros", dtype)
    x = sc.Expanded(st.n_row, st.n_col, A, B)
    prods = x.vals.view(f"f{x.vals.dtype.itemsize // 2}") if x.vals.dtype.kind == "c" else x.vals
    assert ((prods == 0) & np.signbit(prods)).sum() >= 8                   # the pool does hold -0.0 products
    lone = x.length == 1
    assert ((x.vals[x.start[lone]].real == 0) & np.signbit(x.vals[x.start[lone]].real)).sum() >= 3   # ... lone ones among them
    data, indices, indptr = sc.spgemm_ref(st.n_row, st.n_col, A, B, x)
    parts = data.view(prods.dtype)
    assert not ((parts == 0) & np.signbit(parts)).any()
    # inf * 0 touches one element (complex: both its parts, and inf * 0j the imaginary part of inf's other product)
    assert np.isnan(parts).sum() == (1 if data.dtype.kind == "f" else 3) and (parts == 0).sum() >= 6
    kept = sc.prune_bits(data, indices, indptr)[0]
    assert kept.size < data.size and not (kept == 0).any()


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_the_order_of_a_rows_elements_decides_the_bits(dtype):
    """without this, a bit-exact pass would prove nothing about the order of summation"""
    st, (A, B) = _sample(dtype, "ordered", 5, n_row=60, n_inner=40, n_col=30)
    x = sc.Expanded(st.n_row, st.n_col, A, B)
    fwd = sc.spgemm_ref(st.n_row, st.n_col, A, B, x)
    rev = sc.spgemm_ref(st.n_row, st.n_col, sc.reverse_a_rows(A), B)
    assert np.array_equal(fwd[1], rev[1]) and np.array_equal(fwd[2], rev[2])
    many = x.length >= 3
    changed = sc.bits_of(fwd[0])[many] != sc.bits_of(rev[0])[many]
    assert many.sum() >= 300 and changed.sum() * 3 >= many.sum(), (changed.sum(), many.sum())
    # both orders are sums of the same products: within the re-association bound of each other, and of the exact sum
    bound = sc.reassociation_bound(x)
    assert (np.abs(fwd[0].astype(np.longdouble) - rev[0].astype(np.longdouble)) <= bound).all()
    assert (np.abs(fwd[0].astype(np.longdouble) - sc.exact_sums(x)) <= bound + np.abs(sc.exact_sums(x)) * np.finfo(dtype).eps).all()


def test_the_ordered_pool_decides_the_bits_in_the_table_too():
    """the same on a case of the table: the groups of four products of `spread`"""
    name = "classes, u32 keys"
    A, B = sc.case_operands(name, "float32", "ordered")
    st = sc.case_struct(name, 4)
    data, _, _, x = sc.case_reference(name, "float32", "ordered")
    rev = sc.spgemm_ref(st.n_row, st.n_col, sc.reverse_a_rows(A), B)[0]
    many = x.length >= 3
    assert many.sum() > 10_000 and (sc.bits_of(data)[many] != sc.bits_of(rev)[many]).sum() * 3 >= many.sum()


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_bucket_model_on_hand_made_rows():
    # class 0: 512 buckets over n_col columns; 40009 / 512 = 78.1 columns per bucket
    assert sc.bucket_model(sc.N32, 4, 4, []) == (0, 0, 0)
    assert sc.bucket_model(sc.N32, 4, 4, [5] * 16 + [40008]) == (0, 16, 17)
    assert sc.bucket_model(sc.N32, 4, 4, [0, 78, 79, 156, 157]) == (0, 2, 5)          # 78 * 512 / 40009 < 1 <= 79 * 512 / 40009
    assert sc.bucket_of(sc.N32, 256, 4, 1, [0, 78, 79, 40008]).tolist() == [0, 0, 1, 511]
    # two passes: the first pass ends where the bucket reaches NBP = 4096 of 8192
    cut = sc.pass_start(sc.N32, (512, 16, 2), 1)
    assert sc.bucket_of(sc.N32, 512, 16, 2, [cut - 1, cut]).tolist() == [4095, 4096] and abs(cut - sc.N32 / 2) <= 1
    cols = np.concatenate([np.arange(4609), np.arange(cut, cut + 100)])
    cls, big, in_pass = sc.bucket_model(sc.N32, 4, 4, cols)
    assert (cls, in_pass) == (2, 4609) and sc.served(sc.N32, 4, 4, cols) is False
    assert sc.served(sc.N32, 4, 4, cols[1:]) is True and sc.served(sc.N32, 4, 4, np.arange(24577)) is None
    assert sc.bucket_model(sc.N32, 8, 8, np.arange(7168))[0] == 2 and sc.bucket_model(sc.N32, 8, 8, np.arange(7169))[0] == 4
    # the last column of the widest matrix stays below the bucket count
    assert sc.bucket_of(2 ** 31 - 2, 256, 4, 1, [2 ** 31 - 3])[0] == 511


# ---- the table --------------------------------------------------------------------------------------------------------------
def _built(name):
    c = sc.CASES[name]
    return [(vb, sc.case_struct(name, vb)) for vb in sorted({sc.value_bytes(d) for d in c.dtypes})]


@pytest.mark.parametrize("name", list(sc.CASES), ids=sc.slug)
def test_every_case_meets_the_boundary_it_claims(name):
    c = sc.CASES[name]
    for vb, st in _built(name):
        for what, got, want in (c.claims(st, vb) if c.claims else ()):
            assert got == want, (name, vb, what, got, want)


@pytest.mark.parametrize("name", list(sc.CASES), ids=sc.slug)
def test_every_case_takes_the_route_it_states_by_the_hosts_rules(name):
    c = sc.CASES[name]
    assert c.switches.get("SPGEMM_BITMAP") is False or c.switches.get("SPGEMM_ROW_LOCAL") is False
    for dtype in c.dtypes:
        st = sc.case_struct(name, sc.value_bytes(dtype))
        route, heavy = sc.predict(st, dtype, c.switches)
        assert route == c.route, (name, dtype, route)
        assert heavy is None or heavy == c.heavy, (name, dtype, heavy)


@pytest.mark.parametrize("name", [n for n, c in sc.CASES.items() if c.route == "buckets" and "zeros" not in n], ids=sc.slug)
def test_rows_the_bucket_kernels_serve_stay_within_their_buckets(name):
    """every row a case means to be SERVED is served with room (the declined ones are counted by `predict` above); rows are
    otherwise no larger than the issue's bound of c4 + 3 products, operands of a few hundred rows but for the capacity cases"""
    for vb, st in _built(name):
        kb = st.key_bytes
        assert int(st.prod.max(initial=0)) <= sc.bounds(kb, vb)[4] + 3
        declined = sum(1 for r in range(st.n_row) if sc.served(st.n_col, kb, vb, st.columns_of_row(r)) is False)
        skipped = int((st.prod > sc.bounds(kb, vb)[4]).sum())
        assert declined + skipped == sc.CASES[name].heavy


def test_the_table_covers_what_it_set_out_to():
    names = list(sc.CASES)
    routes = {c.route for c in sc.CASES.values()}
    assert routes == {"small/first", "small/second", "buckets", "global"}
    for needle in ("u32 keys", "u64 keys", "max_prod = c0", "max_prod = c3", "a run of 17", "16 products of two", "17 products of two",
                   "class 2, u32 keys: first pass of CAPP", "class 4, u64 keys: first pass of CAPP + 1", "last pass", "A row of 32", "A row of 33", "2^31 - 2",
                   "2^31 - 1", "cap elements", "cap + 1 elements", "STAGE + 1 elements", "n_heavy * 4 == n_row", "n_heavy * 4 > n_row", "== total * 3",
                   "> total * 3", "empty A rows", "an empty B", "every row is empty", "n_row = 1", "index types", "sm_max_cols(4)",
                   "sm_max_cols(1) + 1", "n_col = 2049", "n_row = 5", "A rows of 65", "B rows of 63", "dense result row", "cells = 2^22",
                   "nnz = 2^16 + 1", "fill == 1", "fill < 1/4", "chunks of 64", "2047 products", "2046 products", "zeros: small",
                   "zeros: buckets", "zeros: global"):
        assert any(needle in n for n in names), needle
    assert len(sc.calls()) == len(set(sc.calls())) and 400 < len(sc.calls()) < 1000

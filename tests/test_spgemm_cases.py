"""tests/spgemm_cases.py on its own, without a GPU: the constants the table was built for against the kernels' source text
and the host module's values, the reference against the CPU oracle and against a dense exact product, its signed zeros, its
sensitivity to the order of A's elements, and the table against every boundary it claims - product counts, classes, buckets,
passes, key bits, fill, cells, window alignment, and the route and `heavy_or_declined` count that follow from them by the
host's rules.  A boundary that a case claims and does not meet is a failure here, not a weaker GPU test.  Then the library's
one choice of route, `_kernels._spgemm_route` (pure: the built library answers its limit queries without a device), on
every case's own numbers against that model, and on a table with a case on each side of every threshold."""
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
    from sparse_amd import _kernels as K          # the host's constants: the module's own values

    assert (K.SPGEMM_SMALL_MAX_CELLS, K.SPGEMM_SMALL_MAX_NNZ) == (sc.SMALL_MAX_CELLS, sc.SMALL_MAX_NNZ) == (1 << 22, 1 << 16)
    assert (K.SPGEMM_RUN_PROBE_MIN, K.SPGEMM_RUN_DUPS_MIN, src["LONG_RUN_WINDOW"]) == (sc.RUN_PROBE_MIN, sc.RUN_DUPS_MIN, sc.LONG_RUN_WINDOW)
    assert sc.RUN_DUPS_MIN == sc.LONG_RUN_WINDOW - 1 == 1023 and sc.RUN_PROBE_MIN == 8192
    for name, value in sc.DEFAULT_SWITCHES.items():
        assert getattr(K, name) == value, name
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


def test_the_smallest_case_of_every_route_is_the_one_named():
    assert sc.smallest_cases() == sc.SMALLEST


# ---- the library's one choice of route --------------------------------------------------------------------------------------
P, G = ("probe",), ("global",)
F = ("small", None)           # the first chance
B = (("buckets",), G)


def _steps(K, n_row, n_col, nnz_a, dtype, products):
    """every step `_kernels._spgemm` would walk if each one declined: the route before the probe, then - where it ends in the
    probe and the probe's findings are given - the route after it"""
    import torch

    dtr = getattr(torch, dtype)
    steps = K._spgemm_route(n_row, n_col, nnz_a, dtr)
    if steps[-1] == P and products is not None:
        steps += K._spgemm_route(n_row, n_col, nnz_a, dtr, products)
    return steps


def _route_names(steps):
    return ["small/first" if s == F else "small/second" if s[0] == "small" else s[0] for s in steps if s != P]


@pytest.mark.parametrize("name", list(sc.CASES), ids=sc.slug)
def test_the_librarys_route_on_every_case_is_the_models(hiplib, monkeypatch, name):
    """`_spgemm_route` on the case's own numbers, under the case's switches: the route `predict` states is among the steps and
    nothing stands before it - but the bucket kernels before a global product, where the model's mostly-heavy rule holds (the
    device's counts decide that: a decline of the executor, not a rule of the route)"""
    from sparse_amd import _kernels as K

    c = sc.CASES[name]
    for switch, value in {**c.switches, **c.patch}.items():
        monkeypatch.setattr(K, switch, value)
    for dtype in c.dtypes:
        vb = sc.value_bytes(dtype)
        st = sc.case_struct(name, vb)
        route, _ = sc.predict(st, dtype, c.switches)
        products = (int(st.prod.sum()), int(st.prod.max(initial=0)), st.max_arow)
        steps = _steps(K, st.n_row, st.n_col, st.ai.size, dtype, products)
        names = _route_names(steps)
        assert route in names, (dtype, route, steps)
        before = names[:names.index(route)]
        if route == "global":
            assert steps == (G,) or (steps == (P, *B) and sc.mostly_heavy(st, vb)), (dtype, steps)
        else:
            assert before == [], (dtype, route, steps)                 # (`buckets`: the first step after the probe)
            assert steps[0] == (F if route == "small/first" else P), (dtype, steps)   # (the first chance: before any device read)


@pytest.mark.parametrize("dtype", sc.REAL_TYPES)
def test_the_second_chance_takes_a_quarter_fill_up_to_four_waves_columns(hiplib, dtype):
    """the route's own copy of `sm_max_cols(4)` is the kernel's: at that many columns a quarter product per cell goes to the
    small kernel, just below a quarter and one column further it does not"""
    from sparse_amd import _kernels as K

    n = sc.sm_max_cols(np.dtype(dtype).itemsize, 4)
    nnz_a = K.SPGEMM_SMALL_MAX_NNZ + 1                  # (no first chance)
    for n_col, total, takes in ((n, n, True), (n, n - 1, False), (n + 1, n + 1, False), (n + 1, n, False)):
        steps = _steps(K, 4, n_col, nnz_a, dtype, (total, total, 4))
        assert steps == ((P, ("small", total), *B) if takes else (P, *B)), (n_col, total, steps)


_M9 = {"SPGEMM_BITMAP_MAX_DUPS": 10 ** 9}
_M9W = {"SPGEMM_BITMAP_MAX_DUPS": 10 ** 9, "SPGEMM_BITMAP_SPLIT": False}
_W = {"SPGEMM_BITMAP_SPLIT": False}
_MEAN0 = {"SPGEMM_BITMAP_MIN_MEAN": 0}

# (id, n_row, n_col, stored elements of A, value type, what the probe finds (total, max_prod, max_arow) or None, switches, steps).
# The steps were evaluated with the predicates of the commit before `_spgemm_route` - the branch conditions of its `_spgemm_rows`,
# `dot_csr_csr` and `_spgemm_small`, its `_spgemm_small_second` and `_spgemm_bitmap_forms`, with the built library's limits -
# on these numbers: a case on each side of every threshold, for 4-byte and 8-byte values.  70000 elements of A: no first
# chance.  `bool`: that commit's `_spgemm_rows` raised `code_of`'s TypeError; the route now hands the type to the global form,
# whose `product_code` raises it (checked below).
_SPGEMM_ROUTES = [
    ("float32-cells-2^22", 1024, 4096, 100, "float32", (1000, 10, 3), {}, (F, P, *B)),
    ("float32-cells-2^22+4096", 1025, 4096, 100, "float32", (1000, 10, 3), {}, (P, *B)),
    ("float32-nnz-2^16", 257, 64, 65536, "float32", (1000, 10, 3), {}, (F, P, *B)),
    ("float32-nnz-2^16+1", 257, 64, 65537, "float32", (1000, 10, 3), {}, (P, *B)),
    ("float32-ncol-max_cols", 4, 15879, 100, "float32", (1000, 10, 3), {}, (F, P, *B)),
    ("float32-ncol-max_cols+1", 4, 15880, 100, "float32", (1000, 10, 3), {}, (P, *B)),
    ("float32-ncol-0", 4, 0, 100, "float32", (0, 0, 2), {}, (P, *B)),
    ("float32-ncol-1", 4, 1, 100, "float32", (3, 1, 2), {}, (F, P, ("small", 3), *B)),
    ("float32-nrow-0", 0, 50, 0, "float32", None, {}, (G,)),
    ("float32-nrow-1", 1, 50, 3, "float32", (9, 9, 3), {}, (F, P, *B)),
    ("float32-ncol-2^31-2", 4, 2147483646, 15, "float32", (10, 6, 2), {}, (P, *B)),
    ("float32-ncol-2^31-1", 4, 2147483647, 15, "float32", None, {}, (G,)),
    ("float32-total-0-bitmap-mean-0", 5, 100000, 70000, "float32", (0, 0, 2), _MEAN0, (P, *B)),
    ("float32-total-1-bitmap-mean-0", 5, 100000, 70000, "float32", (1, 1, 2), _MEAN0, (P, ("bitmap", 1), *B)),
    ("float32-fill-1", 4, 6000, 70000, "float32", (24000, 6000, 60), {}, (P, ("small", 24000), *B)),
    ("float32-fill-below-1", 4, 6000, 70000, "float32", (23999, 6000, 60), {}, (P, *B)),
    ("float32-fill-1/4-four_waves", 4, 3964, 70000, "float32", (3964, 3964, 4), {}, (P, ("small", 3964), *B)),
    ("float32-fill-below-1/4-four_waves", 4, 3964, 70000, "float32", (3963, 3963, 4), {}, (P, *B)),
    ("float32-fill-1/4-four_waves+1", 4, 3965, 70000, "float32", (3965, 3965, 4), {}, (P, *B)),
    ("float32-fill-1-four_waves+1", 4, 3965, 70000, "float32", (15860, 3965, 4), {}, (P, ("small", 15860), *B)),
    ("float32-buffer-2^30", 1048576, 2000, 4194304, "float32", (1073741824, 2000, 4), {}, (P, ("small", 1073741824), *B)),
    ("float32-buffer-2^30+1", 1048576, 2000, 4194304, "float32", (1073741825, 2000, 4), {}, (P, *B)),
    ("float32-second-ncol-max_cols", 4, 15879, 70000, "float32", (63516, 15879, 4), {}, (P, ("small", 63516), *B)),
    ("float32-second-ncol-max_cols+1", 4, 15880, 70000, "float32", (63520, 15880, 4), {}, (P, *B)),
    ("float32-mean-1300", 100, 1000000, 70000, "float32", (130000, 2000, 50), {}, (P, ("bitmap", 1), *B)),
    ("float32-mean-below-1300", 100, 1000000, 70000, "float32", (129999, 2000, 50), {}, (P, *B)),
    ("float32-arow-limit", 100, 1000000, 70000, "float32", (200000, 2000, 256), {}, (P, ("bitmap", 1), *B)),
    ("float32-arow-limit+1", 100, 1000000, 70000, "float32", (200000, 2000, 257), {}, (P, *B)),
    ("float32-maxprod-limit", 100, 1000000, 70000, "float32", (2000000, 16384, 50), _M9W, (P, ("bitmap", 1), *B)),
    ("float32-maxprod-limit+1", 100, 1000000, 70000, "float32", (2000000, 16385, 50), _M9W, (P, *B)),
    ("float32-maxprod-limit+1-split", 100, 1000000, 70000, "float32", (2000000, 16385, 50), _M9, (P, ("bitmap", 3), *B)),
    ("float32-ncol-limit", 100, 1048576, 70000, "float32", (200000, 2000, 50), _W, (P, ("bitmap", 1), *B)),
    ("float32-ncol-limit+1", 100, 1048577, 70000, "float32", (200000, 2000, 50), _W, (P, *B)),
    ("float32-ncol-limit+1-split", 100, 1048577, 70000, "float32", (200000, 2000, 50), {}, (P, ("bitmap", 3), *B)),
    ("float32-dups-7745", 100, 250000, 70000, "float32", (400000, 7745, 50), _W, (P, ("bitmap", 1), *B)),
    ("float32-dups-7746", 100, 250000, 70000, "float32", (400000, 7746, 50), _W, (P, *B)),
    ("float32-split-parts-64", 100, 1000000, 70000, "float32", (100000000, 497618, 50), _M9, (P, ("bitmap", 64), *B)),
    ("float32-split-parts-65", 100, 1000000, 70000, "float32", (100000000, 497619, 50), _M9, (P, *B)),
    ("float32-split-dups-18973", 100, 1000000, 70000, "float32", (10000000, 18973, 50), {}, (P, ("bitmap", 3), *B)),
    ("float32-split-dups-18974", 100, 1000000, 70000, "float32", (10000000, 18974, 50), {}, (P, *B)),
    ("float32-both-forms-split-True", 100, 1000000, 70000, "float32", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": True}, (P, ("bitmap", 1), *B)),
    ("float32-split-only-split-True", 100, 3000000, 70000, "float32", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": True}, (P, ("bitmap", 7), *B)),
    ("float32-both-forms-split-False", 100, 1000000, 70000, "float32", (200000, 2000, 50), _W, (P, ("bitmap", 1), *B)),
    ("float32-split-only-split-False", 100, 3000000, 70000, "float32", (200000, 2000, 50), _W, (P, *B)),
    ("float32-both-forms-split-first", 100, 1000000, 70000, "float32", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": "first"}, (P, ("bitmap", 3), ("bitmap", 1), *B)),
    ("float32-split-only-split-first", 100, 3000000, 70000, "float32", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": "first"}, (P, ("bitmap", 7), *B)),
    ("float32-row-local-off", 7, 30, 40, "float32", (100, 20, 3), {"SPGEMM_ROW_LOCAL": False}, (G,)),
    ("float32-small-off", 7, 30, 40, "float32", (210, 30, 6), {"SPGEMM_SMALL": False}, (P, *B)),
    ("float32-small-on", 7, 30, 40, "float32", (210, 30, 6), {}, (F, P, ("small", 210), *B)),
    ("float32-second-off", 4, 6000, 70000, "float32", (24000, 6000, 60), {"SPGEMM_SMALL_SECOND": False}, (P, *B)),
    ("float32-bitmap-off", 100, 1000000, 70000, "float32", (200000, 2000, 50), {"SPGEMM_BITMAP": False}, (P, *B)),
    ("float64-cells-2^22", 1024, 4096, 100, "float64", (1000, 10, 3), {}, (F, P, *B)),
    ("float64-cells-2^22+4096", 1025, 4096, 100, "float64", (1000, 10, 3), {}, (P, *B)),
    ("float64-nnz-2^16", 257, 64, 65536, "float64", (1000, 10, 3), {}, (F, P, *B)),
    ("float64-nnz-2^16+1", 257, 64, 65537, "float64", (1000, 10, 3), {}, (P, *B)),
    ("float64-ncol-max_cols", 4, 8062, 100, "float64", (1000, 10, 3), {}, (F, P, *B)),
    ("float64-ncol-max_cols+1", 4, 8063, 100, "float64", (1000, 10, 3), {}, (P, *B)),
    ("float64-ncol-0", 4, 0, 100, "float64", (0, 0, 2), {}, (P, *B)),
    ("float64-ncol-1", 4, 1, 100, "float64", (3, 1, 2), {}, (F, P, ("small", 3), *B)),
    ("float64-nrow-0", 0, 50, 0, "float64", None, {}, (G,)),
    ("float64-nrow-1", 1, 50, 3, "float64", (9, 9, 3), {}, (F, P, *B)),
    ("float64-ncol-2^31-2", 4, 2147483646, 15, "float64", (10, 6, 2), {}, (P, *B)),
    ("float64-ncol-2^31-1", 4, 2147483647, 15, "float64", None, {}, (G,)),
    ("float64-total-0-bitmap-mean-0", 5, 100000, 70000, "float64", (0, 0, 2), _MEAN0, (P, *B)),
    ("float64-total-1-bitmap-mean-0", 5, 100000, 70000, "float64", (1, 1, 2), _MEAN0, (P, ("bitmap", 1), *B)),
    ("float64-fill-1", 4, 6000, 70000, "float64", (24000, 6000, 60), {}, (P, ("small", 24000), *B)),
    ("float64-fill-below-1", 4, 6000, 70000, "float64", (23999, 6000, 60), {}, (P, *B)),
    ("float64-fill-1/4-four_waves", 4, 2012, 70000, "float64", (2012, 2012, 4), {}, (P, ("small", 2012), *B)),
    ("float64-fill-below-1/4-four_waves", 4, 2012, 70000, "float64", (2011, 2011, 4), {}, (P, *B)),
    ("float64-fill-1/4-four_waves+1", 4, 2013, 70000, "float64", (2013, 2013, 4), {}, (P, *B)),
    ("float64-fill-1-four_waves+1", 4, 2013, 70000, "float64", (8052, 2013, 4), {}, (P, ("small", 8052), *B)),
    ("float64-buffer-2^30", 1048576, 2000, 4194304, "float64", (1073741824, 2000, 4), {}, (P, ("small", 1073741824), *B)),
    ("float64-buffer-2^30+1", 1048576, 2000, 4194304, "float64", (1073741825, 2000, 4), {}, (P, *B)),
    ("float64-second-ncol-max_cols", 4, 8062, 70000, "float64", (32248, 8062, 4), {}, (P, ("small", 32248), *B)),
    ("float64-second-ncol-max_cols+1", 4, 8063, 70000, "float64", (32252, 8063, 4), {}, (P, *B)),
    ("float64-mean-1300", 100, 1000000, 70000, "float64", (130000, 2000, 50), {}, (P, ("bitmap", 1), *B)),
    ("float64-mean-below-1300", 100, 1000000, 70000, "float64", (129999, 2000, 50), {}, (P, *B)),
    ("float64-arow-limit", 100, 1000000, 70000, "float64", (200000, 2000, 256), {}, (P, ("bitmap", 1), *B)),
    ("float64-arow-limit+1", 100, 1000000, 70000, "float64", (200000, 2000, 257), {}, (P, *B)),
    ("float64-maxprod-limit", 100, 1000000, 70000, "float64", (2000000, 8192, 50), _M9W, (P, ("bitmap", 1), *B)),
    ("float64-maxprod-limit+1", 100, 1000000, 70000, "float64", (2000000, 8193, 50), _M9W, (P, *B)),
    ("float64-maxprod-limit+1-split", 100, 1000000, 70000, "float64", (2000000, 8193, 50), _M9, (P, ("bitmap", 3), *B)),
    ("float64-ncol-limit", 100, 1020672, 70000, "float64", (200000, 2000, 50), _W, (P, ("bitmap", 1), *B)),
    ("float64-ncol-limit+1", 100, 1020673, 70000, "float64", (200000, 2000, 50), _W, (P, *B)),
    ("float64-ncol-limit+1-split", 100, 1020673, 70000, "float64", (200000, 2000, 50), {}, (P, ("bitmap", 3), *B)),
    ("float64-dups-7745", 100, 250000, 70000, "float64", (400000, 7745, 50), _W, (P, ("bitmap", 1), *B)),
    ("float64-dups-7746", 100, 250000, 70000, "float64", (400000, 7746, 50), _W, (P, *B)),
    ("float64-split-parts-64", 100, 1000000, 70000, "float64", (100000000, 242296, 50), _M9, (P, ("bitmap", 64), *B)),
    ("float64-split-parts-65", 100, 1000000, 70000, "float64", (100000000, 242297, 50), _M9, (P, *B)),
    ("float64-split-dups-9486", 100, 250000, 70000, "float64", (10000000, 9486, 50), {}, (P, ("bitmap", 3), *B)),
    ("float64-split-dups-9487", 100, 250000, 70000, "float64", (10000000, 9487, 50), {}, (P, *B)),
    ("float64-both-forms-split-True", 100, 1000000, 70000, "float64", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": True}, (P, ("bitmap", 1), *B)),
    ("float64-split-only-split-True", 100, 3000000, 70000, "float64", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": True}, (P, ("bitmap", 7), *B)),
    ("float64-both-forms-split-False", 100, 1000000, 70000, "float64", (200000, 2000, 50), _W, (P, ("bitmap", 1), *B)),
    ("float64-split-only-split-False", 100, 3000000, 70000, "float64", (200000, 2000, 50), _W, (P, *B)),
    ("float64-both-forms-split-first", 100, 1000000, 70000, "float64", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": "first"}, (P, ("bitmap", 3), ("bitmap", 1), *B)),
    ("float64-split-only-split-first", 100, 3000000, 70000, "float64", (200000, 2000, 50), {"SPGEMM_BITMAP_SPLIT": "first"}, (P, ("bitmap", 7), *B)),
    ("float64-row-local-off", 7, 30, 40, "float64", (100, 20, 3), {"SPGEMM_ROW_LOCAL": False}, (G,)),
    ("float64-small-off", 7, 30, 40, "float64", (210, 30, 6), {"SPGEMM_SMALL": False}, (P, *B)),
    ("float64-small-on", 7, 30, 40, "float64", (210, 30, 6), {}, (F, P, ("small", 210), *B)),
    ("float64-second-off", 4, 6000, 70000, "float64", (24000, 6000, 60), {"SPGEMM_SMALL_SECOND": False}, (P, *B)),
    ("float64-bitmap-off", 100, 1000000, 70000, "float64", (200000, 2000, 50), {"SPGEMM_BITMAP": False}, (P, *B)),
    ("complex64", 7, 30, 40, "complex64", (100, 20, 3), {}, (G,)),
    ("complex128", 7, 30, 40, "complex128", (100, 20, 3), {}, (G,)),
    ("bool", 7, 30, 40, "bool", (100, 20, 3), {}, (G,)),
    ("int32", 7, 30, 40, "int32", (100, 20, 3), {}, (F, P, ("small", 100), *B)),
    ("int64", 7, 30, 40, "int64", (100, 20, 3), {}, (F, P, ("small", 100), *B)),
]


@pytest.mark.parametrize("case", _SPGEMM_ROUTES, ids=[c[0] for c in _SPGEMM_ROUTES])
def test_spgemm_route_table(hiplib, monkeypatch, case):
    """`_kernels._spgemm_route`, the one choice of kernel for `sparse @ sparse`: the first chance of the small kernel, whether
    the row-product probe is worth a launch, then the second chance, the forms of the bitmap kernel, the bucket kernels and
    the global form"""
    import torch

    from sparse_amd import _kernels as K

    _, n_row, n_col, nnz_a, dtype, products, switches, want = case
    for switch, value in switches.items():
        monkeypatch.setattr(K, switch, value)
    assert _steps(K, n_row, n_col, nnz_a, dtype, products) == want
    if dtype == "bool":
        with pytest.raises(TypeError):
            K.product_code(getattr(torch, dtype))

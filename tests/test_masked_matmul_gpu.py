"""sparse_amd.masked_matmul on the device (csrc/masked_spgemm.hip).

Yardsticks, all from tests/masked_cases.py:
  * exact mode (SPARSE_AMD_EXACT: every multiply and add rounded on its own) against `masked_restated` - the order contract of
    include/sparse_amd.h A13 written as a NumPy loop - in the result type, BIT FOR BIT, for every forced group / cap / window;
  * default mode (a term's multiply and add are one fma) against the evaluation m * sum_k a_k b_k, computed exactly
    (rational arithmetic, so the comparison value adds no error of its own and float64 results meet the same bound):
        |got - want| <= (n + 2) * eps * |m| * sum|a_k b_k|,   n = that element's term count, eps of the result type
    (n products, n additions, one final multiply), and bit for bit against the restatement's fused form, whose host fma is
    exactly rounded for both float types;
  * the fixture (tests/golden/masked_matmul.npz: the reference's own `s * (a @ b)`, run by
    tools/gen_masked_matmul_golden.py) in both modes as dense images: equal values in exact mode, the same bound against the exact
    evaluation and against the reference's result otherwise.
Every comparison against a bound prints the largest |got - want| / bound it saw."""
import functools
import itertools

import numpy as np
import pytest
import torch

import invariants
import masked_cases as mk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (np.float32, np.float64, np.int32, np.int64)
GROUPS = (8, 16, 32, 64)
FORMATS = ("coo", "gcxs0", "gcxs1")


def _mat(m, fmt="coo", idx=None):
    import sparse_amd

    coords, data, shape = m
    x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device=DEV)
    if fmt == "coo":
        return x
    return x.asformat("gcxs", compressed_axes=(0,) if fmt == "gcxs0" else (1,))


def _dense(x):
    d = x.todense()
    return d.cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)


def _kernel(s, a, b, dt, idx=None, *, group=None, cap=None, window=None, exact=False):
    """the values at the mask's stored positions through the `_kernels` wrapper, with forced parameters"""
    from sparse_amd import _dot, _kernels as K, _masked

    sc, ac, bc = _mat(s, idx=idx), _mat(a, idx=idx), _mat(b, idx=idx)
    if idx is not None:
        assert sc.coords.dtype == (torch.int32 if np.dtype(idx) == np.int32 else torch.int64)
    conv = lambda t: (K.convert(t[0], dt), t[1], t[2])          # noqa: E731
    M, N, Kd = s[2][0], s[2][1], a[2][1]
    out = K.masked_spgemm((M, N, Kd), conv(_dot._csr_triplet(sc)), conv(_dot._csr_triplet(ac)), conv(_masked._csc_triplet(bc)),
                          group=group, cap=cap, window=window, exact=exact)
    note = out._zero_bits_count
    vals = out.cpu().numpy()
    assert int(note[0]) == int(invariants.eq_bits(vals, 0).sum())      # the count the prune will trust
    return vals


def _public(s, a, b, exact, monkeypatch, fmts=("coo", "coo", "coo"), idx=None):
    import sparse_amd
    from sparse_amd import _settings

    monkeypatch.setattr(_settings, "EXACT_MULADD", exact)
    return sparse_amd.masked_matmul(_mat(s, fmts[0], idx), _mat(a, fmts[1], idx), _mat(b, fmts[2], idx))


# ---- the case table: name -> (s, a, b, result dtype, index dtype, forced (group, cap, window) or None) ----------------------------
def _case_names():
    names = [f"bcols_g{g}" for g in GROUPS]
    names += [f"arows_cap64_{np.dtype(dt).name}_{idx}" for dt in DTYPES for idx in ("int32", "int64")]
    names += [f"lanes_g{g}" for g in GROUPS]
    names += ["no_match", "mask_rows", "ones", "hub_default", "windows", "wrap_int32", "wrap_int64", "dense_operands"]
    return names


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("bcols_g"):
        # columns of b of 0, 1, g - 1, g, g + 1 and 3 g + 2 elements; rows of a: empty, one element, sparse, full
        g = int(name[7:])
        dt, idx = DTYPES[GROUPS.index(g)], (np.int32, np.int64)[GROUPS.index(g) % 2]
        Kd = 4 * g
        b = mk.cols_matrix(10 + g, [0, 1, g - 1, g, g + 1, 3 * g + 2], Kd, dt, idx)
        a = mk.rows_matrix(20 + g, [0, 1, Kd // 3, Kd, 5], Kd, dt, idx)
        return mk.full_mask(30 + g, (5, 6), dt, idx), a, b, dt, idx, (g, 64, 8)
    if name.startswith("arows_cap64"):
        # rows of a of 0, 1, cap - 1, cap, cap + 1 and 200 elements with cap = 64: the LDS search and the global one
        _, _, dname, iname = name.split("_")
        dt, idx = np.dtype(dname).type, np.dtype(iname).type
        seed = 100 + DTYPES.index(dt) * 2 + (iname == "int64")
        a = mk.rows_matrix(seed, [0, 1, 63, 64, 65, 200], 256, dt, idx)
        b = mk.cols_matrix(seed + 50, [256, 40, 0, 3, 100, 17, 64], 256, dt, idx)
        return mk.full_mask(seed + 90, (6, 7), dt, idx), a, b, dt, idx, (16, 64, 8)
    if name.startswith("lanes_g"):
        # column 0 of b = one step of g entries, k = 0 .. g - 1; rows of a that match its first lane only, its last lane only,
        # every lane, none; column 1 = two steps, matched in the second only
        g = int(name[7:])
        dt = DTYPES[(GROUPS.index(g) + 1) % 2]
        a = mk.rows_matrix(40 + g, [1, 1, g, g, 1], 2 * g, dt,
                           first=[[0], [g - 1], np.arange(g), np.arange(g, 2 * g), [2 * g - 1]])
        b = mk.cols_matrix(41 + g, [g, 2 * g], 2 * g, dt, first=[np.arange(g), np.arange(2 * g)])
        return mk.full_mask(42 + g, (5, 2), dt), a, b, dt, np.int64, (g, 64, 8)
    if name == "no_match":
        a = mk.rows_matrix(50, [8] * 6, 40, np.float32, first=[np.arange(0, 16, 2) + 2 * i for i in range(6)])
        b = mk.cols_matrix(51, [8] * 5, 40, np.float32, first=[np.arange(1, 17, 2) + 2 * i for i in range(5)])
        return mk.full_mask(52, (6, 5), np.float32), a, b, np.float32, np.int64, (8, 64, 8)
    if name == "mask_rows":                                     # mask rows that are empty, single or full
        N = 19
        s = mk.rows_matrix(60, [0, 1, N, 0, N, 1, 0], N, np.float64)
        return s, mk.random_matrix(61, (7, 23), 80, np.float64), mk.random_matrix(62, (23, N), 200, np.float64), np.float64, np.int64, (8, 64, 8)
    if name == "ones":                                          # M = N = K = 1
        one = lambda v: (np.zeros((2, 1), np.int64), np.array([v], np.float32), (1, 1))      # noqa: E731
        return one(-3.0), one(0.5), one(7.0), np.float32, np.int64, None
    if name == "hub_default":                                   # a row of a and a column of b of 5000 elements, default parameters
        a = mk.rows_matrix(70, [5000, 3, 0, 10], 6000, np.float32, np.int32)
        b = mk.cols_matrix(71, [5000, 5, 2000, 0], 6000, np.float32, np.int32)
        return mk.full_mask(72, (4, 4), np.float32, np.int32), a, b, np.float32, np.int32, None
    if name == "windows":                                       # 600 mask elements: more than one default window, 75 of 8
        return (mk.random_matrix(80, (40, 30), 600, np.float64), mk.random_matrix(81, (40, 50), 500, np.float64),
                mk.random_matrix(82, (50, 30), 400, np.float64), np.float64, np.int64, (16, 64, 8))
    if name.startswith("wrap_"):                                # products and sums that wrap
        dt = np.dtype(name[5:]).type
        rng = np.random.default_rng(90)
        s, a, b = mk.random_matrix(91, (9, 8), 50, dt), mk.random_matrix(92, (9, 12), 60, dt), mk.random_matrix(93, (12, 8), 60, dt)
        big = lambda m: (m[0], mk.big_values(rng, len(m[1]), dt), m[2])      # noqa: E731
        return big(s), big(a), big(b), dt, np.int64, (8, 64, 8)
    if name == "dense_operands":                                # a match in every lane of every step
        return (mk.full_mask(95, (5, 4), np.float64), mk.full_mask(96, (5, 70), np.float64), mk.full_mask(97, (70, 4), np.float64),
                np.float64, np.int32, (32, 64, 8))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _restated(name, fused):
    s, a, b, dt = _case(name)[:4]
    want = mk.masked_restated(s, a, b, dt, fused=fused)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _exact(name):
    s, a, b, dt = _case(name)[:4]
    want, bound = mk.exact_and_bound(s, a, b, dt)
    want.setflags(write=False)
    bound.setflags(write=False)
    return want, bound


def _forced(case):
    f = case[5]
    return {} if f is None else {"group": f[0], "cap": f[1], "window": f[2]}


def test_the_cases_hold_what_their_names_promise():
    from sparse_amd import _kernels as K

    _, a, b = _case("hub_default")[:3]
    assert np.bincount(a[0][0]).max() == 5000 > K.MASKED_CAP and np.bincount(b[0][1]).max() == 5000
    for g in GROUPS:
        _, a, b = _case(f"bcols_g{g}")[:3]
        assert np.bincount(b[0][1], minlength=6).tolist() == [0, 1, g - 1, g, g + 1, 3 * g + 2]
        s, a, b = _case(f"lanes_g{g}")[:3]
        assert mk.term_counts(s, a, b).reshape(5, 2).tolist() == [[1, 1], [1, 1], [g, g], [0, g], [0, 1]]
    _, a, _ = _case("arows_cap64_float32_int32")[:3]
    assert np.bincount(a[0][0], minlength=6).tolist() == [0, 1, 63, 64, 65, 200]
    s, a, b = _case("no_match")[:3]
    assert not mk.term_counts(s, a, b).any()
    assert len(_case("windows")[0][1]) == 600 > K.MASKED_WINDOW
    s, a, b, dt = _case("wrap_int64")[:4]
    exact = [sum(int(x) * int(y) for x, y in zip(av, bv)) for av, bv in mk.terms_of(s, a, b)]
    assert max(abs(v) for v in exact) > 2 ** 63                      # the sums really wrap


@pytest.mark.parametrize("name", _case_names())
def test_exact_mode_is_the_restated_contract_bit_for_bit(name, monkeypatch):
    case = _case(name)
    s, a, b, dt, idx, _ = case
    want = _restated(name, False)
    got = _kernel(s, a, b, dt, idx, exact=True, **_forced(case))
    assert got.dtype == want.dtype == np.dtype(dt)
    assert invariants.same_bits(got, want), f"{np.count_nonzero(got != want)} of {got.size} values differ"
    none = mk.term_counts(s, a, b) == 0
    assert invariants.eq_bits(got[none], 0).all()                    # no term: +0
    out = _public(s, a, b, True, monkeypatch, idx=idx)
    assert out.dtype == np.dtype(dt) and (_dense(out) == mk.dense_result(s, want)).all()
    assert invariants.assert_canonical(out, pruned=True)


@pytest.mark.parametrize("name", _case_names())
def test_every_forced_variant_gives_the_bits_of_the_default(name):
    s, a, b, dt, idx, _ = _case(name)
    base = _kernel(s, a, b, dt, idx)
    variants = [(g, 64, 8) for g in GROUPS] + [(16, 1, 1), (64, 2048, 3), (8, 63, 10 ** 9), (32, 5, 64)]
    for group, cap, window in variants:
        got = _kernel(s, a, b, dt, idx, group=group, cap=cap, window=window)
        assert invariants.same_bits(got, base), (group, cap, window)


@pytest.mark.parametrize("name", _case_names())
def test_default_mode_within_the_bound_the_fused_restatement_and_the_same_bits_twice(name, monkeypatch):
    case = _case(name)
    s, a, b, dt, idx, _ = case
    got = _kernel(s, a, b, dt, idx, **_forced(case))
    if np.dtype(dt).kind == "i":
        ds, da, db = (mk.dense_of(m, dt) for m in (s, a, b))
        with np.errstate(all="ignore"):
            want = (ds * (da @ db))[tuple(s[0])]
        assert invariants.same_bits(got, want.astype(dt))             # integers: NumPy's, exactly (wrap-around included)
    else:
        want, bound = _exact(name)
        err = mk.abs_err(got, want)
        print(f"{name}: max |got - want| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
        assert invariants.same_bits(got, _restated(name, True))
    again = _kernel(s, a, b, dt, idx, **_forced(case))
    assert invariants.same_bits(got, again)
    out = _public(s, a, b, False, monkeypatch, idx=idx)
    assert (_dense(out) == mk.dense_result(s, got)).all()


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return mk.load_golden()


@pytest.mark.parametrize("exact", [False, True], ids=["fma", "exact"])
@pytest.mark.parametrize("name", sorted(mk.load_golden()))
def test_fixture_cases_against_the_reference(name, exact, monkeypatch):
    c = _golden()[name]
    fmts = tuple(mk.FORMAT_NAMES[f] for f in c["formats"])
    out = _public(c["s"], c["a"], c["b"], exact, monkeypatch, fmts)
    dt = c["out"].dtype
    assert out.dtype == dt and tuple(out.shape) == c["out"].shape
    assert type(out).__name__ == ("COO" if fmts[0] == "coo" else "GCXS")
    got = _dense(out)
    if exact or dt.kind == "i":
        assert (got == c["out"]).all()                               # value equality: signed zeros equal, all else in bits
    else:
        want, bound = mk.exact_and_bound(c["s"], c["a"], c["b"], dt)
        at = tuple(np.asarray(c["s"][0], dtype=np.int64))
        err = mk.abs_err(got[at], want)                                # against the exact evaluation ...
        ref = np.abs(got.astype(np.float64) - c["out"].astype(np.float64))      # ... and against the reference's own result
        lim = mk.dense_result(c["s"], bound)
        print(f"{name}: max |got - exact| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"max |got - reference| / bound = {np.max(ref / np.maximum(lim, 1e-300)):.3f}")
        assert (err <= bound).all() and (ref <= lim).all()
    stored = out.tocoo().coords.cpu().numpy() if hasattr(out, "tocoo") else out.coords.cpu().numpy()
    mask = {tuple(p) for p in c["s"][0].T.tolist()}
    assert all(tuple(p) in mask for p in stored.T.tolist())         # nothing outside the mask's pattern
    assert invariants.assert_canonical(out, pruned=True)


@pytest.mark.parametrize("name", ["f32_coo", "f64_gcxs0", "f64_gcxs1", "f32_coo_g0_g1", "i64_coo", "negmask_f64_coo", "emptyrows_f32_coo"])
def test_exact_mode_equals_the_librarys_own_expression(name, monkeypatch):
    from sparse_amd import _settings

    c = _golden()[name]
    fmts = tuple(mk.FORMAT_NAMES[f] for f in c["formats"])
    monkeypatch.setattr(_settings, "EXACT_MULADD", True)
    s, a, b = (_mat(c[op], f) for op, f in zip("sab", fmts))
    import sparse_amd

    fused, expr = sparse_amd.masked_matmul(s, a, b), s * (a @ b)
    assert fused.dtype == expr.dtype
    assert (_dense(fused) == _dense(expr)).all()


# ---- NaN / inf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nan_and_inf_reach_exactly_the_positions_that_own_them(bad, monkeypatch):
    s = mk.full_mask(200, (9, 8), np.float32)
    a, b = mk.random_matrix(201, (9, 30), 90, np.float32), mk.random_matrix(202, (30, 8), 80, np.float32)
    e = 41
    i, k = int(a[0][0][e]), int(a[0][1][e])
    a2 = (a[0], a[1].copy(), a[2])
    a2[1][e] = bad
    got = _dense(_public(s, a2, b, False, monkeypatch))
    want = np.zeros((9, 8), bool)
    want[i, b[0][1][b[0][0] == k]] = True                            # the columns j whose column of b stores row k
    assert want.any() and np.array_equal(~np.isfinite(got), want)
    # a NaN / inf mask value: over an empty intersection nothing is stored, over a non-empty one it shows
    counts = mk.term_counts(s, a, b)
    none, some = int(np.flatnonzero(counts == 0)[0]), int(np.flatnonzero(counts > 0)[0])
    s2 = (s[0], s[1].copy(), s[2])
    s2[1][[none, some]] = bad
    out = _public(s2, a, b, False, monkeypatch)
    stored = {tuple(p) for p in out.coords.cpu().numpy().T.tolist()}
    assert tuple(s[0][:, none]) not in stored and tuple(s[0][:, some]) in stored
    got = _dense(out)
    want = np.zeros((9, 8), bool)
    want[tuple(s[0][:, some])] = True
    assert np.array_equal(~np.isfinite(got), want)
    assert len(stored) == int((counts > 0).sum())


# ---- containers -----------------------------------------------------------------------------------------------------------------
def test_every_container_combination_gives_the_same_values_in_the_masks_format(monkeypatch):
    import sparse_amd

    s, a, b = mk.random_matrix(300, (12, 10), 70, np.float64), mk.random_matrix(301, (12, 15), 60, np.float64), mk.random_matrix(302, (15, 10), 60, np.int64)
    base = _dense(_public(s, a, b, False, monkeypatch))
    assert np.count_nonzero(base) > 10
    for fmts in itertools.product(FORMATS, repeat=3):
        sx, ax, bx = (_mat(m, f) for m, f in zip((s, a, b), fmts))
        out = sparse_amd.masked_matmul(sx, ax, bx)
        assert invariants.same_bits(_dense(out), base), fmts
        assert type(out) is type(sx) and out.dtype == np.float64 and out.device == sx.device
        if fmts[0] != "coo":
            assert out.compressed_axes == sx.compressed_axes
        assert invariants.assert_canonical(out, pruned=True)
        for x in (sx, ax, bx):                                       # the derived forms the call left on the operands
            assert invariants.assert_canonical(x)


def test_result_type_follows_the_operands(monkeypatch):
    s, a, b = mk.random_matrix(310, (6, 5), 20, np.int32), mk.random_matrix(311, (6, 7), 25, np.int32), mk.random_matrix(312, (7, 5), 25, np.int32)
    cast = lambda m, dt: (m[0], m[1].astype(dt), m[2])              # noqa: E731
    want = mk.dense_of(s, np.float64) * (mk.dense_of(a, np.float64) @ mk.dense_of(b, np.float64))
    for ds, da, db, dr in ((np.int32, np.int32, np.int32, np.int32), (np.bool_, np.int32, np.int64, np.int64),
                           (np.int64, np.float32, np.float32, np.float64), (np.float32, np.int32, np.float32, np.float64),
                           (np.float32, np.bool_, np.float32, np.float32), (np.uint8, np.float32, np.float32, np.float32)):
        out = _public(cast(s, ds), cast(a, da), cast(b, db), False, monkeypatch)
        assert out.dtype == np.dtype(dr), (ds, da, db)
        exp = mk.dense_of(cast(s, ds), np.float64) * (mk.dense_of(cast(a, da), np.float64) @ mk.dense_of(cast(b, db), np.float64))
        assert np.array_equal(_dense(out).astype(np.float64), exp), (ds, da, db)      # small integers: exact in every type
    assert np.count_nonzero(want) > 3


# ---- the derived forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmts", [("coo", "coo", "coo"), ("gcxs1", "gcxs1", "gcxs0"), ("gcxs0", "gcxs0", "gcxs1")])
def test_a_second_call_converts_nothing_and_an_in_place_write_rebuilds(fmts, monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi

    s, a, b = mk.random_matrix(400, (12, 10), 70, np.float32), mk.random_matrix(401, (12, 15), 60, np.float32), mk.random_matrix(402, (15, 10), 60, np.float32)
    sx, ax, bx = (_mat(m, f) for m, f in zip((s, a, b), fmts))
    names = []
    real = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *args: names.append(name) or real(name, *args))
    first = sparse_amd.masked_matmul(sx, ax, bx)
    n_first = names.index("spamd_masked_spgemm")
    if fmts != ("gcxs0", "gcxs0", "gcxs1"):
        assert n_first > 0                                           # forms were built: row pointers, a transposed CSR, a twin
    del names[:]
    second = sparse_amd.masked_matmul(sx, ax, bx)
    k = names.index("spamd_masked_spgemm")
    assert k == 0, names                                             # nothing before the product: no conversion kernel
    assert invariants.same_bits(_dense(first), _dense(second))
    if fmts[2] == "gcxs1":                                           # a column-compressed b is CSC already: its own arrays
        from sparse_amd import _masked

        assert _masked._csc_triplet(bx)[0] is bx.data and _masked._csc_triplet(bx)[1] is bx.indices
    # in-place writes to the stored values: the derived forms are rebuilt, the result follows
    for x, scale in ((bx, 2), (ax, 4), (sx, 8)):
        x.data *= 2
        del names[:]
        out = sparse_amd.masked_matmul(sx, ax, bx)
        assert np.array_equal(_dense(out), scale * _dense(first)), scale
    for x in (sx, ax, bx):
        assert invariants.assert_canonical(x)


# ---- triangles ------------------------------------------------------------------------------------------------------------------
def test_triangles_of_a_60_node_graph(monkeypatch):
    import sparse_amd

    rng = np.random.default_rng(500)
    up = np.triu(rng.random((60, 60)) < 0.2, 1)
    A = (up | up.T).astype(np.int64)
    a = sparse_amd.COO.from_numpy(A, device=DEV)
    want = int(np.trace(np.linalg.matrix_power(A, 3)))
    assert want > 0 and want % 6 == 0
    for x in (a, a.asformat("gcxs")):
        assert int(sparse_amd.masked_matmul(x, x, x).sum()) == want
    assert int(sparse_amd.sum(a @ a * a)) == want                     # the example's expression through this library


# ---- argument errors, trivial sizes --------------------------------------------------------------------------------------------
def test_argument_errors():
    import sparse_amd
    from sparse_amd import _kernels as K

    s, a, b = mk.random_matrix(600, (6, 5), 20, np.float32), mk.random_matrix(601, (6, 7), 25, np.float32), mk.random_matrix(602, (7, 5), 25, np.float32)
    sx, ax, bx = _mat(s), _mat(a), _mat(b)
    assert sparse_amd.masked_matmul(sx, ax, bx).shape == (6, 5)
    with pytest.raises(TypeError, match="sddmm"):
        sparse_amd.masked_matmul(sx, _dense(ax), bx)
    with pytest.raises(TypeError, match="sddmm"):
        sparse_amd.masked_matmul(sx, ax, torch.zeros((7, 5), device=DEV))
    for bad in ((sx, bx, ax), (sx, ax, ax), (ax, ax, bx), (sx, _mat(mk.random_matrix(603, (6, 8), 9, np.float32)), bx)):
        with pytest.raises(ValueError, match="shape-mismatch"):
            sparse_amd.masked_matmul(*bad)
    with pytest.raises(ValueError, match="zero fill"):
        sparse_amd.masked_matmul(sparse_amd.full((6, 5), 1.0, dtype=np.float32, device=DEV), ax, bx)
    with pytest.raises(ValueError, match="zero fill"):
        sparse_amd.masked_matmul(sx, sparse_amd.full((6, 7), 1.0, dtype=np.float32, device=DEV), bx)
    with pytest.raises(ValueError, match="2-D"):
        sparse_amd.masked_matmul(sparse_amd.zeros((6, 5, 2), dtype=np.float32, device=DEV), ax, bx)
    cast = lambda m, dt: _mat((m[0], m[1].astype(dt), m[2]))        # noqa: E731
    for ds, da, db in ((np.complex64, np.float32, np.float32), (np.float32, np.complex128, np.complex128),
                       (np.float16, np.float16, np.float16), (np.float32, np.float16, np.float32),
                       (np.bool_, np.bool_, np.bool_), (np.uint8, np.uint8, np.uint8), (np.int8, np.int8, np.int8),
                       (np.int16, np.int32, np.int32), (np.int32, np.int16, np.int32)):
        ops = cast(s, ds), cast(a, da), cast(b, db)
        assert [x.dtype for x in ops] == [np.dtype(ds), np.dtype(da), np.dtype(db)]
        with pytest.raises(TypeError, match="float32, float64, int32"):
            sparse_amd.masked_matmul(*ops)
    # (uint8 is the one unsigned type a container holds: wider unsigned values are stored as signed integers of the next width)
    trip = lambda x: (x.data, x.coords[1].contiguous(), K.rows_to_indptr(x.coords[0], x.shape[0]))      # noqa: E731
    for kw in ({"group": 24}, {"cap": 0}, {"cap": K.MASKED_MAX_CAP + 1}, {"window": 0}):
        with pytest.raises(ValueError):
            K.masked_spgemm((6, 5, 7), trip(sx), trip(ax), trip(bx.T), **kw)


def test_trivial_sizes_launch_nothing(monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi

    s, a, b = mk.random_matrix(700, (6, 5), 20, np.float32), mk.random_matrix(701, (6, 7), 25, np.float64), mk.random_matrix(702, (7, 5), 25, np.float32)
    empty = lambda shape, dt: sparse_amd.zeros(shape, dtype=dt, device=DEV)      # noqa: E731
    cases = [(empty((6, 5), np.float32), _mat(a), _mat(b), (6, 5)), (_mat(s), empty((6, 7), np.float64), _mat(b), (6, 5)),
             (_mat(s), _mat(a), empty((7, 5), np.float32), (6, 5)),
             (empty((0, 5), np.float32), empty((0, 7), np.float64), _mat(b), (0, 5)),
             (empty((6, 0), np.float32), _mat(a), empty((7, 0), np.float32), (6, 0)),
             (_mat(s), empty((6, 0), np.float64), empty((0, 5), np.float32), (6, 5)),
             (_mat(s, "gcxs1"), empty((6, 7), np.float64), _mat(b, "gcxs0"), (6, 5))]
    names = []
    real = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *args: names.append(name) or real(name, *args))
    for sx, ax, bx, shape in cases:
        del names[:]
        out = sparse_amd.masked_matmul(sx, ax, bx)
        assert names == [], names
        assert tuple(out.shape) == shape and out.nnz == 0 and out.dtype == np.float64 and type(out) is type(sx)
        assert out.device == sx.device
        if hasattr(sx, "compressed_axes") and type(sx).__name__ == "GCXS":
            assert out.compressed_axes == sx.compressed_axes

"""sparse_amd.mttkrp on the device (csrc/mttkrp.hip).

Three yardsticks, all from tests/mttkrp_cases.py:
  * exact mode (SPARSE_AMD_EXACT: every multiply and add rounded on its own) against `mttkrp_restated` - the order contract
    of include/sparse_amd.h A12 written as a NumPy loop - in the result type, BIT FOR BIT;
  * default mode (the last multiply of a term and the accumulate are one fma) against float64 np.einsum:
        |got - want| <= (n + ndim) * eps * sum|terms|      (twice that for float64 results: the comparison value is a
    float64 sum too), n = the longest row, eps = the result type's machine epsilon, sum|terms| per output element - the
    gamma_k bound of a chain of ndim - 1 products and a sum of n terms;
  * the fixture (tests/golden/mttkrp.npz: the reference's own expression, run by tools/gen_mttkrp_golden.py) in both modes,
    within the same bound with the eps of the result type plus the eps of the type the reference computed in.
Every comparison against a bound prints the largest |got - want| / bound it saw."""
import functools

import numpy as np
import pytest
import torch

import mttkrp_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tensor(coords, data, shape, idx=None, gcxs=False):
    import sparse_amd

    x = sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device=DEV)
    return x.asformat("gcxs") if gcxs else x


def _run(case, exact, monkeypatch):
    """the case through the public function (default chunk) or, with a chunk, through the `_kernels` wrapper"""
    import sparse_amd
    from sparse_amd import _kernels as K, _settings

    coords, data, shape, factors, mode, chunk, dtype, idx = case
    monkeypatch.setattr(_settings, "EXACT_MULADD", exact)
    x = _tensor(coords, data, shape, idx)
    assert x.coords.dtype == (torch.int32 if np.dtype(idx) == np.int32 else torch.int64)
    if chunk is None:
        return sparse_amd.mttkrp(x, factors, mode)
    d = torch.device(DEV)
    fac = [None if f is None else torch.from_numpy(f).to(d) for f in factors]
    plan = K.mttkrp_plan(x.coords, x.shape, mode)
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    return K.mttkrp_coo(x.coords, K.convert(x.data, tdt), x.shape, fac, mode, plan, chunk=chunk, exact=exact).cpu().numpy()


# ---- the case table: name -> (coords, data, shape, factors, mode, chunk, result dtype, index dtype) --------------------------------
WIDTHS = (1, 3, 16, 17, 25, 64, 65, 130)
ROW_LENGTHS = [0, 1, 7, 8, 9, 26]      # 0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 2 with chunk = 8


def _case_names():
    names = [f"width{R}_{idx}" for R in WIDTHS for idx in ("int32", "int64")]
    names += [f"unit_dim_mode{m}" for m in range(4)]
    names += [f"rows_mode{m}_r{R}" for m in (0, 2) for R in (5, 17)]
    names += ["one_row_chunk8", "one_row_default", "long_row_default_chunk", "two_starts_chunk64", "bool_values_2d", "int_values_5d"]
    return names


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("width"):
        R, idx = int(name[5:].split("_")[0]), np.dtype(name.split("_")[1])
        dt = np.float32 if WIDTHS.index(R) % 2 == 0 else np.float64
        shape = (9, 8, 7)
        coords, data = mc.random_tensor(100 + R, shape, 150, dt, idx)
        return coords, data, shape, tuple(mc.factors_for(R, shape, R, dt, mode=1)), 1, 8, dt, idx
    if name.startswith("unit_dim"):
        m, shape = int(name[-1]), (7, 1, 6, 5)
        coords, data = mc.random_tensor(200 + m, shape, 100, np.float32)
        return coords, data, shape, tuple(mc.factors_for(200 + m, shape, 5, np.float32, mode=m)), m, 8, np.float32, np.int64
    if name.startswith("rows_mode"):
        m, R = int(name[9]), int(name.split("_r")[1])
        dt = np.float32 if R == 5 else np.float64
        coords, data, shape = mc.rows_tensor(300 + m + R, ROW_LENGTHS, (6, 5), m, dt)
        return coords, data, shape, tuple(mc.factors_for(300 + R, shape, R, dt, mode=m)), m, 8, dt, np.int64
    if name.startswith("one_row"):
        coords, data, shape = mc.rows_tensor(400, [0, 40, 0], (8, 7), 1, np.float64)
        chunk = 8 if name.endswith("chunk8") else None
        return coords, data, shape, tuple(mc.factors_for(400, shape, 3, np.float64, mode=1)), 1, chunk, np.float64, np.int32
    if name == "long_row_default_chunk":      # 5000 elements in one row: the default chunk's multi-piece path
        coords, data, shape = mc.rows_tensor(500, [3, 5000, 0, 10], (80, 70), 1, np.float32)
        return coords, data, shape, tuple(mc.factors_for(500, shape, 3, np.float32, mode=1)), 1, None, np.float32, np.int32
    if name == "two_starts_chunk64":      # windows 2 and 3 hold two piece starts each: a long row starts mid-window after another's piece
        coords, data, shape = mc.rows_tensor(550, [3, 130, 70, 1, 200], (16, 13), 1, np.float64)
        return coords, data, shape, tuple(mc.factors_for(550, shape, 17, np.float64, mode=1)), 1, 64, np.float64, np.int64
    if name == "bool_values_2d":
        shape = (11, 13)
        coords, data = mc.random_tensor(600, shape, 60, np.bool_)
        return coords, data, shape, tuple(mc.factors_for(600, shape, 17, np.float32, mode=0)), 0, None, np.float32, np.int64
    if name == "int_values_5d":
        shape = (4, 3, 5, 2, 3)
        coords, data = mc.random_tensor(700, shape, 120, np.int64)
        return coords, data, shape, tuple(mc.factors_for(700, shape, 25, np.float64, mode=3)), 3, 8, np.float64, np.int64
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _einsum(name):
    coords, data, shape, factors, mode, _, dt, _ = _case(name)
    vals = np.asarray(data).astype(dt)         # the values the kernel sees
    fac = list(factors)
    want = mc.mttkrp_einsum(coords, vals, shape, fac, mode)
    b = mc.bound(coords, vals, shape, fac, mode, dt)
    want.setflags(write=False)
    b.setflags(write=False)
    return want, b * (2 if np.dtype(dt) == np.float64 else 1)


def _empty_rows(case):
    coords, _, shape, _, mode = case[:5]
    return np.bincount(coords[mode], minlength=shape[mode]) == 0


@pytest.mark.parametrize("name", _case_names())
def test_exact_mode_is_the_restated_contract_bit_for_bit(name, monkeypatch):
    case = _case(name)
    coords, data, shape, factors, mode, chunk, dt, _ = case
    from sparse_amd import _kernels as K

    got = _run(case, True, monkeypatch)
    want = mc.mttkrp_restated(coords, data, shape, list(factors), mode, K.MTTKRP_CHUNK if chunk is None else chunk, dt)
    assert got.dtype == want.dtype == np.dtype(dt) and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{np.count_nonzero(got != want)} of {got.size} elements differ"
    empty = _empty_rows(case)
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any()      # rows without a stored element: +0.0


@pytest.mark.parametrize("name", _case_names())
def test_default_mode_within_the_derived_bound_and_the_same_bits_twice(name, monkeypatch):
    case = _case(name)
    got = _run(case, False, monkeypatch)
    want, bound = _einsum(name)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: max |got - want| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    again = _run(case, False, monkeypatch)
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8))
    empty = _empty_rows(case)
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any()


def test_long_row_case_really_has_several_default_pieces():
    from sparse_amd import _kernels as K

    coords, _, shape, _, mode = _case("long_row_default_chunk")[:5]
    assert mc.longest_row(coords, shape, mode) == 5000 > K.MTTKRP_CHUNK >= 1


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return mc.load_golden()


def _golden_names():
    return sorted(mc.load_golden())


@pytest.mark.parametrize("exact", [False, True], ids=["fma", "exact"])
@pytest.mark.parametrize("name", _golden_names())
def test_fixture_cases_against_the_reference(name, exact, monkeypatch):
    import sparse_amd
    from sparse_amd import _settings

    c = _golden()[name]
    monkeypatch.setattr(_settings, "EXACT_MULADD", exact)
    x = _tensor(c["coords"], c["data"], c["shape"], gcxs=c["gcxs"])
    assert type(x).__name__ == ("GCXS" if c["gcxs"] else "COO")
    got = sparse_amd.mttkrp(x, c["factors"], c["mode"])
    fdt = next(f for f in c["factors"] if f is not None).dtype
    assert isinstance(got, np.ndarray) and got.dtype == fdt and got.shape == c["out"].shape
    args = (c["coords"], c["data"], c["shape"], c["factors"], c["mode"])
    bound = mc.bound(*args, fdt, c["out"].dtype)
    err = np.abs(got.astype(np.float64) - c["out"].astype(np.float64))
    print(f"{name}: max |got - reference| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    if exact:
        want = mc.mttkrp_restated(*args, 10 ** 9, fdt)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- NaN / inf -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("mode", [0, 1])
def test_nan_and_inf_reach_exactly_the_outputs_that_own_them(bad, mode):
    import sparse_amd

    shape, R = (6, 5, 4), 17
    coords, data = mc.random_tensor(800, shape, 50, np.float32)
    fac = mc.factors_for(800, shape, R, np.float32, mode=mode)
    # one stored element
    k = 23
    d2 = data.copy()
    d2[k] = bad
    out = sparse_amd.mttkrp(_tensor(coords, d2, shape), fac, mode)
    want = np.zeros((shape[mode], R), bool)
    want[coords[mode][k]] = True
    assert np.array_equal(~np.isfinite(out), want)
    if np.isnan(bad):
        assert np.isnan(out[want]).all()
    # one entry of one factor row
    d_other = 2 if mode == 1 else 1
    f2 = [None if f is None else f.copy() for f in fac]
    row = int(coords[d_other][7])
    f2[d_other][row, 5] = bad
    out = sparse_amd.mttkrp(_tensor(coords, data, shape), f2, mode)
    want = np.zeros((shape[mode], R), bool)
    want[coords[mode][coords[d_other] == row], 5] = True
    assert want.any() and np.array_equal(~np.isfinite(out), want)
    # the ignored factor may hold anything
    f3 = list(fac)
    f3[mode] = np.full((shape[mode], R), np.nan, np.float32)
    assert np.array_equal(sparse_amd.mttkrp(_tensor(coords, data, shape), f3, mode), sparse_amd.mttkrp(_tensor(coords, data, shape), fac, mode))


# ---- containers and factor types ---------------------------------------------------------------------------------------------------
def test_gcxs_gives_the_bits_of_its_coo_and_factor_types_choose_the_result_type():
    import sparse_amd

    shape, R, mode = (9, 8, 7), 25, 2
    coords, data = mc.random_tensor(900, shape, 200, np.float64)
    fac = mc.factors_for(900, shape, R, np.float64, mode=mode)
    x = _tensor(coords, data, shape)
    base = sparse_amd.mttkrp(x, fac, mode)
    assert isinstance(base, np.ndarray)
    for ca in (None, (0,), (1, 2)):
        g = x.asformat("gcxs", compressed_axes=ca) if ca else x.asformat("gcxs")
        assert np.array_equal(sparse_amd.mttkrp(g, fac, mode).view(np.uint8), base.view(np.uint8))
        assert g.__dict__["_coo_view"]._mttkrp_plan[mode] is not None      # kept on the view
    assert np.array_equal(sparse_amd.mttkrp(x, fac, -1), base)             # negative mode
    # torch factors (host or device) give a device tensor
    tf = [None if f is None else torch.from_numpy(f) for f in fac]
    out = sparse_amd.mttkrp(x, tf, mode)
    assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), base)
    tf[0] = tf[0].to(DEV)
    mixed = [tf[0], fac[1], None]
    out = sparse_amd.mttkrp(x, mixed, mode)
    assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), base)
    # a Fortran-ordered factor, a strided torch view (every second column of a wider matrix, rows of a taller one)
    fo = [np.asfortranarray(fac[0]), fac[1], None]
    assert not fo[0].flags.c_contiguous
    assert np.array_equal(sparse_amd.mttkrp(x, fo, mode), base)
    wide = torch.zeros((shape[0], 2 * R), dtype=torch.float64, device=DEV)
    wide[:, ::2] = torch.from_numpy(fac[0]).to(DEV)
    tall = torch.zeros((2 * shape[1], R + 3), dtype=torch.float64, device=DEV)
    tall[::2, :R] = torch.from_numpy(fac[1]).to(DEV)
    views = [wide[:, ::2], tall[::2, :R], None]
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    assert np.array_equal(sparse_amd.mttkrp(x, views, mode).cpu().numpy(), base)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_is_built_once_per_mode_and_rebuilt_after_an_in_place_write(monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    shape, R = (9, 8, 7), 5
    coords, data = mc.random_tensor(1000, shape, 200, np.float32)
    x = _tensor(coords, data, shape)
    built = []
    for fn in ("mttkrp_plan", "sort_keys", "rows_to_indptr"):
        real = getattr(K, fn)
        monkeypatch.setattr(K, fn, (lambda real, fn: lambda *a, **k: built.append(fn) or real(*a, **k))(real, fn))
    for mode in (0, 1):
        fac = mc.factors_for(1000, shape, R, np.float32, mode=mode)
        tf = [None if f is None else torch.from_numpy(f).to(DEV) for f in fac]
        del built[:]
        c0 = _ffi.CALLS
        first = sparse_amd.mttkrp(x, tf, mode)
        c1 = _ffi.CALLS
        assert built == (["mttkrp_plan", "rows_to_indptr"] if mode == 0 else ["mttkrp_plan", "sort_keys", "rows_to_indptr"])
        plan = x._mttkrp_plan[mode]
        assert (plan.perm is None) == (mode == 0) and plan.rowptr.dtype == torch.int64 and plan.rowptr.numel() == shape[mode] + 1
        del built[:]
        second = sparse_amd.mttkrp(x, tf, mode)
        c2 = _ffi.CALLS
        assert built == [] and x._mttkrp_plan[mode] is plan
        assert c2 - c1 == 1 < c1 - c0            # float32 values: the product's one call, nothing for the plan
        assert torch.equal(first, second)
    assert set(x._mttkrp_plan) == {0, 1}
    # stable within a row: the permutation ascends inside every row
    p1 = x._mttkrp_plan[1]
    perm, ptr = p1.perm.cpu().numpy(), p1.rowptr.cpu().numpy()
    assert sorted(perm.tolist()) == list(range(x.nnz))
    assert all((np.diff(perm[ptr[i]:ptr[i + 1]]) > 0).all() for i in range(shape[1]))
    assert np.array_equal(coords[1][perm], np.sort(coords[1]))
    # an in-place write to the values: the plans are dropped and built again, the result follows the values
    old = x._mttkrp_plan[1]
    x.data *= 2
    doubled = sparse_amd.mttkrp(x, tf, 1)
    assert x._mttkrp_plan[1] is not old and set(x._mttkrp_plan) == {1}
    assert torch.equal(doubled, 2 * second)
    # ... and to the coordinates: element k moves to another row of mode 1 (a free cell; mode 1's plan does not need the
    # C order of the stored elements, only their positions)
    k = 17
    taken = {tuple(c) for c in coords.T.tolist()}
    j = next(j for j in range(shape[1]) if (coords[0][k], j, coords[2][k]) not in taken)
    old = x._mttkrp_plan[1]
    x.coords[1, k] = j
    moved = sparse_amd.mttkrp(x, tf, 1)
    assert x._mttkrp_plan[1] is not old
    c2_ = coords.copy()
    c2_[1, k] = j
    args = (c2_, 2 * data, shape, fac, 1)
    assert (np.abs(moved.cpu().numpy() - mc.mttkrp_einsum(*args)) <= mc.bound(*args, np.float32)).all()
    assert not torch.equal(moved, doubled)


# ---- argument errors, trivial sizes --------------------------------------------------------------------------------------------
def test_argument_errors():
    import sparse_amd

    shape, R = (6, 5, 4), 3
    coords, data = mc.random_tensor(1100, shape, 30, np.float32)
    x = _tensor(coords, data, shape)
    fac = mc.factors_for(1100, shape, R, np.float32)
    assert sparse_amd.mttkrp(x, fac, 0).shape == (6, R)
    with pytest.raises(ValueError, match="zero fill"):
        sparse_amd.mttkrp(sparse_amd.full(shape, 1.0, device=DEV), fac, 0)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.mttkrp(x, fac[:2], 0)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.mttkrp(x, [None, fac[1][:4], fac[2]], 0)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.mttkrp(x, [None, fac[1], fac[2][:, :2]], 0)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.mttkrp(x, [None, fac[1][:, 0], fac[2]], 0)
    with pytest.raises(TypeError):
        sparse_amd.mttkrp(x, [None, fac[1], fac[2].astype(np.float64)], 0)
    with pytest.raises(TypeError):
        sparse_amd.mttkrp(x, [None, fac[1].astype(np.complex64), fac[2].astype(np.complex64)], 0)
    with pytest.raises(TypeError):
        sparse_amd.mttkrp(x, [None, fac[1].astype(np.float16), fac[2].astype(np.float16)], 0)
    with pytest.raises(TypeError):
        sparse_amd.mttkrp(x, [None, torch.from_numpy(fac[1]).to(torch.bfloat16), torch.from_numpy(fac[2]).to(torch.bfloat16)], 0)
    for mode in (3, -4):
        with pytest.raises(ValueError, match="out of range"):
            sparse_amd.mttkrp(x, fac, mode)
    with pytest.raises(ValueError, match="at least 2"):
        sparse_amd.mttkrp(_tensor(np.array([[0, 2]]), np.ones(2, np.float32), (4,)), [None], 0)
    nine = sparse_amd.zeros((2,) * 9, dtype=np.float32, device=DEV)
    with pytest.raises(ValueError, match="at most 8"):
        sparse_amd.mttkrp(nine, [np.ones((2, R), np.float32)] * 9, 0)
    eight = sparse_amd.COO(np.array([[0], [1], [0], [1], [1], [0], [1], [0]]), np.array([2.0], np.float32), shape=(2,) * 8, device=DEV)
    out = sparse_amd.mttkrp(eight, [np.full((2, R), 3.0, np.float32)] * 8, 7)
    assert np.array_equal(out, np.array([[2.0 * 3 ** 7] * R, [0.0] * R], np.float32))


def test_trivial_sizes():
    import sparse_amd

    shape = (6, 5, 4)
    empty = sparse_amd.zeros(shape, dtype=np.float32, device=DEV)
    fac = mc.factors_for(1200, shape, 3, np.float64)
    out = sparse_amd.mttkrp(empty, fac, 1)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (5, 3)
    assert (out == 0).all() and not np.signbit(out).any()
    coords, data = mc.random_tensor(1200, shape, 30, np.float32)
    x = _tensor(coords, data, shape)
    zero_r = [torch.zeros((s, 0), dtype=torch.float32, device=DEV) for s in shape]
    out = sparse_amd.mttkrp(x, zero_r, 2)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (4, 0) and out.dtype == torch.float32
    assert "_mttkrp_plan" not in x.__dict__                         # nothing was built, nothing launched

"""sparse_amd.softmax on the device (csrc/softmax.hip, csrc/exp_det.h).

Yardsticks, all from tests/softmax_cases.py:
  * `softmax_restated` - the order contract of include/sparse_amd.h A14 and the step list of csrc/exp_det.h written in NumPy -
    in the result type, BIT FOR BIT (any NaN equals any NaN: a payload is no result);
  * every kernel form, sub-group width and chunk against every other, bit for bit, for the lengths it accepts;
  * facts that need no restatement (a group of one element is 1.0, 2^k equal values are 2^-k, ...);
  * the exact value (mpmath, or longdouble for the larger cases) of the rounded inputs:
        |got - want| <= (D + 2 U + n / 2 + 1) * eps * want + the smallest subnormal
    with D the largest finite |t_j - max| of the group, n its length, U the measured accuracy of exp_det in ulp.
Every comparison against the bound prints the largest share of it that it saw."""
import numpy as np
import pytest
import torch

import softmax_cases as sc
from invariants import assert_canonical

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNKS = (64, 128, None)          # None: the default, `_kernels.SOFTMAX_CHUNK`


def _coo(coords, data, shape, idx=None):
    import sparse_amd

    return sparse_amd.COO(coords, data, shape=shape, has_duplicates=False, sorted=True, idx_dtype=idx, device=DEV)


def _vals(x):
    return x.data.cpu().numpy()


def _chunk(monkeypatch, chunk):
    from sparse_amd import _kernels as K

    if chunk is not None:
        monkeypatch.setattr(K, "SOFTMAX_CHUNK", chunk)
    return K.SOFTMAX_CHUNK


def _same_structure(out, x):
    import sparse_amd

    assert type(out) is type(x) and out.shape == x.shape and out.fill_value == 0 and out.nnz == x.nnz
    if isinstance(x, sparse_amd.COO):
        assert out.coords.dtype == x.coords.dtype and torch.equal(out.coords, x.coords)
    else:
        assert out.compressed_axes == x.compressed_axes and out.indices.dtype == x.indices.dtype
        assert torch.equal(out.indices, x.indices) and torch.equal(out.indptr, x.indptr)


# ---- bit for bit against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_listed_lengths_bit_for_bit(dtype, idx, chunk, monkeypatch):
    """the listed group lengths mixed in one array (runs of empty groups, the first and the last group empty), then one group
    that holds everything, then nnz = 0"""
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    coords, data, shape = sc.rows_array(40 + chunk, sc.listed_lengths(chunk), dtype, idx)
    x = _coo(coords, data, shape, idx)
    out = sparse_amd.softmax(x, 1)
    assert out.dtype == np.dtype(dtype)
    _same_structure(out, x)
    assert sc.same_bits(_vals(out), sc.softmax_restated(coords, data, shape, 1, chunk))
    plan = x._softmax_plan[(1,)]
    assert plan.segptr.numel() - 1 == sum(1 for n in sc.listed_lengths(chunk) if n)   # non-empty groups only
    tidx = torch.int32 if np.dtype(idx) == np.int32 else torch.int64
    assert plan.segptr.dtype == tidx                 # the kernels run at the array's own index width
    # the same elements as a CSR whose pointers - empty rows included - are the segment pointers as they are
    ptr = np.concatenate(([0], np.cumsum(sc.listed_lengths(chunk)))).astype(idx)
    g = sparse_amd.GCXS((data, coords[1].astype(idx), ptr), shape=shape, compressed_axes=(0,), device=DEV)
    res = sparse_amd.softmax(g, 1)
    assert g._softmax_plan[(1,)].segptr is g.indptr and g.indptr.dtype == tidx
    _same_structure(res, g)
    assert sc.same_bits(_vals(res), _vals(out))
    everything = sparse_amd.softmax(x, (0, 1))
    assert sc.same_bits(_vals(everything), sc.softmax_restated(coords, data, shape, (0, 1), chunk))
    empty = _coo(np.zeros((2, 0), idx), np.zeros(0, dtype), shape, idx)
    res = sparse_amd.softmax(empty)
    assert res.nnz == 0 and res.shape == shape and res.dtype == np.dtype(dtype) and "_softmax_plan" not in empty.__dict__


# ---- every form against every other ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_groups_and_chunks_change_no_bit(dtype, idx):
    """`idx`: the width of the segment pointers the kernels read"""
    from sparse_amd import _kernels as K, _softmax

    def runs(lengths, seed, variants):
        coords, data, shape = sc.rows_array(seed, lengths, dtype)
        x = _coo(coords, data, shape)
        plan = _softmax._build_plan(x, (1,))
        assert plan.perm is None and plan.max_len == max(lengths)
        seg = plan.segptr.to(idx)
        outs = {str(kw): K.softmax_segments(seg, None, x.data, plan.max_len, **kw).cpu().numpy() for kw in variants}
        first = next(iter(outs.values()))
        assert all(sc.same_bits(first, o) for o in outs.values()), [k for k, o in outs.items() if not sc.same_bits(first, o)]
        return coords, data, shape, first

    # lengths every form accepts: sub-groups of every width, a wave per group at two chunks, the piece form's wave per group
    short = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 5]
    variants = [dict(form="short", group=g) for g in K.SOFTMAX_GROUPS] + [dict(form="wide", chunk=c) for c in (64, 1024)]
    variants += [dict(form="long"), dict(), dict(group=8), dict(group=64, chunk=128)]
    coords, data, shape, got = runs(short, 71, variants)
    assert sc.same_bits(got, sc.softmax_restated(coords, data, shape, 1, 64))
    # up to 128: a wave per group at chunks 128 and 1024, the default split at 64 with every width, the piece form at 128
    mid = short + [65, 100, 127, 128]
    variants = [dict(form="wide", chunk=c) for c in (128, 1024)] + [dict(group=g, chunk=c) for g in K.SOFTMAX_GROUPS for c in (128, 256)]
    variants += [dict(form="long", chunk=128)]
    runs(mid, 72, variants)
    # pieces of 64 (chunk is part of the order here, so one chunk): the piece form against the default split, every width
    long_ = mid + [129, 191, 192, 193, 64 * 5, 700]
    for chunk in (64, 128):
        variants = [dict(form="long", chunk=chunk)] + [dict(group=g, chunk=chunk) for g in K.SOFTMAX_GROUPS]
        coords, data, shape, got = runs(long_, 73, variants)
        assert sc.same_bits(got, sc.softmax_restated(coords, data, shape, 1, chunk))
    with pytest.raises(ValueError, match="short"):
        K.softmax_segments(torch.tensor([0, 65], device=DEV), None, torch.zeros(65, device=DEV), 65, form="short")
    with pytest.raises(ValueError, match="wide"):
        K.softmax_segments(torch.tensor([0, 65], device=DEV), None, torch.zeros(65, device=DEV), 65, form="wide", chunk=64)


# ---- exact facts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_facts(dtype, chunk, monkeypatch):
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    rng = np.random.default_rng(3)
    # groups of one element are exactly 1.0, whatever the value
    n = 300
    coords = np.stack([np.arange(n), rng.integers(0, 50, n)])
    data = (rng.standard_normal(n) * 1e3).astype(dtype)
    data[:4] = [0.0, -0.0, np.finfo(dtype).max, -np.finfo(dtype).max]
    assert (_vals(sparse_amd.softmax(_coo(coords, data, (n, 50)), 1)) == 1.0).all()
    # a group of 2^k equal values is exactly 2^-k (k = 0 .. 11: every form, and pieces whose sums are exact integers)
    lengths = [2 ** k for k in range(12)]
    coords, data, shape = sc.rows_array(4, lengths, dtype)
    data = np.repeat((rng.standard_normal(len(lengths)) * 50).astype(dtype), lengths)
    out = _vals(sparse_amd.softmax(_coo(coords, data, shape), 1))
    assert np.array_equal(out, np.repeat(np.ldexp(1.0, -np.arange(12)).astype(dtype), lengths))
    # the element at the maximum has e = 1: beside elements whose e is +0 it is exactly 1.0
    lengths = [3, 40, 70, 2 * chunk + 5]
    coords, data, shape = sc.rows_array(5, lengths, dtype)
    data[:] = -np.inf
    firsts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    data[firsts + np.array([1, 17, 69, chunk + 3])] = [2.5, -1e30, 0.0, 7.0]
    data[firsts[1] + 3] = -1e30 - 3e3 * abs(np.spacing(dtype(-1e30)))       # finite, far below: e underflows to +0
    out = _vals(sparse_amd.softmax(_coo(coords, data, shape), 1))
    want = np.zeros(len(data), dtype)
    want[firsts + np.array([1, 17, 69, chunk + 3])] = 1
    assert np.array_equal(out, want) and not np.signbit(out).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_groups_bits_do_not_depend_on_the_other_groups_and_calls_repeat(dtype, monkeypatch):
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    lengths = sc.listed_lengths(chunk)
    coords, data, shape = sc.rows_array(9, lengths, dtype)
    x = _coo(coords, data, shape)
    full = _vals(sparse_amd.softmax(x, 1))
    assert sc.same_bits(full, _vals(sparse_amd.softmax(x, 1))) and sc.same_bits(full, _vals(sparse_amd.softmax(_coo(coords, data, shape), 1)))
    for row in (4, 11, 19, 25, 27):            # 7, 31, 65, chunk + 1, 5 * chunk: alone, and as the last of three other groups
        sel = coords[0] == row
        alone = _vals(sparse_amd.softmax(_coo(np.stack([np.zeros(sel.sum(), np.int64), coords[1][sel]]), data[sel], (1, shape[1])), 1))
        assert sc.same_bits(alone, full[sel])
        c2, d2, _ = sc.rows_array(row, [5, 200, 0], dtype)
        c3 = np.concatenate([c2, np.stack([np.full(sel.sum(), 3), coords[1][sel]])], axis=1)
        among = _vals(sparse_amd.softmax(_coo(c3, np.concatenate([d2, data[sel]]), (4, max(shape[1], 203))), 1))
        assert sc.same_bits(among[len(d2):], full[sel])


# ---- tolerance against the exact value ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,spread,scale", [(np.float32, 3.0, None), (np.float32, 30.0, 0.37), (np.float32, 80.0, -1.0),
                                                (np.float64, 3.0, None), (np.float64, 600.0, 0.37)])
def test_within_the_bound_of_the_exact_value(dtype, spread, scale):
    """lengths 1 to 5000 in one array (short, wide and piece forms at the default chunk), values of `spread` standard
    deviations, so that e runs through the subnormal range to 0 at the larger spreads; exact values in longdouble, and by
    mpmath for a second, small array"""
    import sparse_amd

    lengths = [1, 2, 5, 17, 40, 64, 65, 200, 777, 1024, 1025, 3000, 5000]
    coords, data, shape = sc.rows_array(21, lengths, dtype, spread=spread)
    got = _vals(sparse_amd.softmax(_coo(coords, data, shape), 1, scale=scale))
    want, bound = sc.exact_and_bound(coords, data, shape, 1, scale)
    share = sc.bound_share(got, want, bound)
    small = sc.rows_array(22, [1, 3, 30, 70, 150], dtype, spread=spread)
    got_s = _vals(sparse_amd.softmax(_coo(*small), 1, scale=scale))
    share_s = sc.bound_share(got_s, *sc.exact_and_bound(*small, 1, scale, use_mpmath=True))
    print(f"softmax {np.dtype(dtype)} spread {spread} scale {scale}: largest share of the bound {share:.3f} (longdouble), "
          f"{share_s:.3f} (mpmath); zeros among the results: {(got == 0).sum()}")
    assert not np.isnan(bound).any() and share <= 1 and share_s <= 1
    if spread >= 80:
        assert (got == 0).any() and ((got > 0) & (got < np.finfo(dtype).smallest_normal)).any()


# ---- values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype, chunk, monkeypatch):
    """-0.0, stored zeros, +-inf, a NaN in one group among clean ones, an all -inf group, spreads through the subnormal range,
    at lengths of every form; with and without a negative scale"""
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    inf, nan = np.inf, np.nan
    lengths = [6, 40, 130, 2 * chunk + 9] * 6
    coords, data, shape = sc.rows_array(31, lengths, dtype, spread=2.0)
    firsts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    lo = sc._CONSTS[np.dtype(dtype)]["lo"]
    for j in range(4):
        n = lengths[j]
        data[firsts[j] + n // 2] = nan                                  # groups 0-3: one NaN
        data[firsts[4 + j] + n - 1] = inf                               # groups 4-7: one +inf
        data[firsts[8 + j]:firsts[8 + j] + n] = -inf                    # groups 8-11: nothing but -inf
        data[firsts[12 + j] + 1:firsts[12 + j] + n:3] = -inf            # groups 12-15: -inf beside finite values
        data[firsts[16 + j]:firsts[16 + j] + n:2] = [0.0, -0.0][j % 2]  # groups 16-19: stored zeros of either sign
        data[firsts[20 + j]:firsts[20 + j] + n] = np.linspace(1.3 * lo, 0, n)   # groups 20-23: e through the subnormals to 0
    x = _coo(coords, data, shape)
    for scale in (None, -0.75):
        got = _vals(sparse_amd.softmax(x, 1, scale=scale))
        assert sc.same_bits(got, sc.softmax_restated(coords, data, shape, 1, chunk, scale))
        g = np.split(got, firsts[1:])
        neg = scale is not None
        assert all(np.isnan(v).all() for v in g[:4])
        if not neg:
            assert all(np.isnan(v).all() for v in g[4:12])
            for v, n in zip(g[12:16], lengths):
                assert (v[1::3] == 0).all() and not np.signbit(v).any() and np.isfinite(v).all() and abs(v.sum() - 1) < (n + 32) * np.finfo(dtype).eps
            sub = np.concatenate(g[20:24])
            assert (sub == 0).any() and ((sub > 0) & (sub < np.finfo(dtype).smallest_normal)).any()
        else:           # scale < 0: +inf becomes -inf (+0.0 beside finite values), -inf becomes +inf (NaN throughout)
            assert all(v[-1] == 0 and np.isfinite(v).all() for v in g[4:8]) and all(np.isnan(v).all() for v in g[8:16])
        assert all(np.isfinite(v).all() and (v > 0).all() for v in g[16:20])


def test_integer_and_boolean_values_give_float64(monkeypatch):
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    for dtype in (np.int32, np.int64, np.bool_):
        coords, data, shape = sc.rows_array(41, [0, 3, 70, 200, 9], dtype)
        out = sparse_amd.softmax(_coo(coords, data, shape), -1, scale=0.5)
        assert out.dtype == np.float64 and out.fill_value.dtype == np.float64
        assert sc.same_bits(_vals(out), sc.softmax_restated(coords, data, shape, 1, chunk, 0.5))


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def _gcxs_stored_coords(g):
    """[ndim, nnz] coordinates of a GCXS's stored elements in stored order, from its own arrays on the host"""
    ind, shape = g.indices.cpu().numpy().astype(np.int64), g.shape
    if len(shape) == 1:
        return ind[None, :]
    ptr, ca = g.indptr.cpu().numpy().astype(np.int64), list(g.compressed_axes)
    order = ca + [a for a in range(len(shape)) if a not in ca]
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    parts = np.unravel_index(rows, [shape[a] for a in ca]) + np.unravel_index(ind, [shape[a] for a in order[len(ca):]])
    coords = np.empty((len(shape), len(ind)), dtype=np.int64)
    for pos, a in enumerate(order):
        coords[a] = parts[pos]
    return coords


@pytest.mark.parametrize("shape,axes", [((300,), [0, -1]), ((9, 150), [0, 1, (0, 1)]), ((5, 40, 7), [0, 1, 2, (0, 2), (1, 2), (-3, 1)]),
                                        ((3, 4, 30, 5), [0, 2, 3, (1, 2), (0, 3), (1, 2, 3)])])
def test_coo_layouts(shape, axes, monkeypatch):
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    for idx in (np.int32, np.int64):
        coords, data, shape = sc.random_array(len(shape), shape, int(np.prod(shape)) // 2, np.float32, idx)
        x = _coo(coords, data, shape, idx)
        for axis in axes:
            out = sparse_amd.softmax(x, axis)
            _same_structure(out, x)
            assert sc.same_bits(_vals(out), sc.softmax_restated(coords, data, shape, axis, chunk)), axis
            assert_canonical(out)
        assert len(x._softmax_plan) - 1 == len({tuple(sorted(a % len(shape) for a in (ax if isinstance(ax, tuple) else (ax,)))) for ax in axes})


@pytest.mark.parametrize("shape,ca,axes", [((40, 150), (0,), [0, 1]), ((40, 150), (1,), [0, 1]), ((5, 40, 7), (0,), [0, 1, 2, (1, 2)]),
                                           ((5, 40, 7), (1, 2), [0, 1, (0, 2), -3]), ((300,), None, [0])])
def test_gcxs_layouts(shape, ca, axes, monkeypatch):
    """a group's elements are taken in the GCXS's own stored order (for compressed axes (1, 2) over axes (0, 2) that is not the
    order of the COO of the same elements), and the values come back at the stored positions"""
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    coords, data, shape = sc.random_array(7 + len(shape), shape, int(np.prod(shape)) // 2, np.float64)
    coo = _coo(coords, data, shape)
    g = coo.asformat("gcxs", compressed_axes=ca) if ca else coo.asformat("gcxs")
    stored, sdata = _gcxs_stored_coords(g), _vals(g)
    dense = np.zeros(shape)
    dense[tuple(coords)] = data
    assert np.array_equal(dense[tuple(stored)], sdata)
    for axis in axes:
        out = sparse_amd.softmax(g, axis)
        _same_structure(out, g)
        assert_canonical(out)
        assert sc.same_bits(_vals(out), sc.softmax_restated(stored, sdata, shape, axis, chunk)), axis
    if ca:      # over exactly the uncompressed axes a compressed row is a group as it is stored: the pointers themselves, no sort
        own = tuple(a for a in range(len(shape)) if a not in ca)
        assert own in [ax if isinstance(ax, tuple) else (ax,) for ax in axes]
        assert g._softmax_plan[own].segptr is g.indptr and g._softmax_plan[own].perm is None
    if len(shape) == 2:
        assert g._softmax_plan[(ca[0],)].perm is not None


def test_non_canonical_gcxs(monkeypatch):
    """column indices that descend inside every row: the stored order is kept - in the result and inside every group"""
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    coords, data, shape = sc.rows_array(51, [0, 3, 70, 0, 150, 9], np.float32, np.int32)
    ptr = np.concatenate(([0], np.cumsum(np.bincount(coords[0], minlength=shape[0])))).astype(np.int32)
    rev = np.concatenate([np.arange(ptr[i], ptr[i + 1])[::-1] for i in range(shape[0])])
    stored = np.stack([coords[0][rev], coords[1][rev]])
    g = sparse_amd.GCXS((data, stored[1].astype(np.int32), ptr), shape=shape, compressed_axes=(0,), device=DEV)
    for axis in (1, 0, (0, 1)):
        out = sparse_amd.softmax(g, axis)
        _same_structure(out, g)
        assert sc.same_bits(_vals(out), sc.softmax_restated(stored, data, shape, axis, chunk)), axis


# ---- structure and caches ---------------------------------------------------------------------------------------------------------------
def test_plan_is_built_once_kept_over_value_writes_and_dropped_with_the_coordinates(monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi, _softmax

    built = []
    real = _softmax._build_plan
    monkeypatch.setattr(_softmax, "_build_plan", lambda x, axis: built.append(axis) or real(x, axis))
    coords, data, shape = sc.random_array(61, (30, 40, 5), 2000, np.float32)
    x = _coo(coords, data, shape)
    c0 = _ffi.CALLS
    first = sparse_amd.softmax(x, (0, 2))
    c1 = _ffi.CALLS
    second = sparse_amd.softmax(x, (2, 0))
    c2 = _ffi.CALLS
    assert built == [(0, 2)] and c2 - c1 == 1 < c1 - c0            # float32 values: the kernel's one call, nothing for the plan
    assert sc.same_bits(_vals(first), _vals(second))
    assert_canonical(first)
    plan = x._softmax_plan[(0, 2)]
    assert plan.perm is not None and sorted(plan.perm.tolist()) == list(range(x.nnz))
    seg, perm = plan.segptr.cpu().numpy(), plan.perm.cpu().numpy()
    assert all((np.diff(perm[seg[i]:seg[i + 1]]) > 0).all() for i in range(len(seg) - 1))       # stored order within a group
    # an in-place write to the values keeps the plan, and the result follows the values
    x.data *= 2
    doubled = sparse_amd.softmax(x, (0, 2))
    assert built == [(0, 2)] and x._softmax_plan[(0, 2)] is plan
    assert sc.same_bits(_vals(doubled), sc.softmax_restated(coords, 2 * data, shape, (0, 2), 1024))
    sparse_amd.softmax(x, 1)
    assert built == [(0, 2), (1,)]
    # a replaced coordinate buffer drops every plan: two elements trade places along axis 1 (free cells, C order kept)
    c2_ = coords.copy()
    a = next(k for k in range(x.nnz - 1) if coords[0][k] == coords[0][k + 1] and coords[1][k] + 1 < coords[1][k + 1])
    c2_[1, a] += 1
    c2_[2, a] = 0
    x.coords = torch.from_numpy(c2_).to(DEV)
    x._keys = None
    moved = sparse_amd.softmax(x, (0, 2))
    assert built == [(0, 2), (1,), (0, 2)] and x._softmax_plan[(0, 2)] is not plan and set(x._softmax_plan) == {"stamp", (0, 2)}
    assert sc.same_bits(_vals(moved), sc.softmax_restated(c2_, 2 * data, shape, (0, 2), 1024))
    # drop_derived (what a replaced buffer of any kind calls) forgets them as it forgets the MTTKRP plans
    from sparse_amd import _dot

    _dot.drop_derived(x)
    assert "_softmax_plan" not in x.__dict__


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_attention_end_to_end():
    """matmul(softmax(sddmm(mask, q, bt=k)), v) on a 64 x 64 mask against the dense computation in float64: within
    (K + n + 8) * eps32 * the row's largest |v| per output - K products and sums for a score (|score| < 4 here: D <= 8), the
    softmax bound, n products and sums for the output"""
    import sparse_amd

    rng = np.random.default_rng(77)
    n, K, dv = 64, 16, 8
    mask = rng.random((n, n)) < 0.3
    mask[5] = False                                   # a row without a stored element: its output row is 0
    mask[np.arange(n) != 5, rng.integers(0, n, n)[np.arange(n) != 5]] = True
    q, k = (rng.standard_normal((n, K)) * 0.5).astype(np.float32), (rng.standard_normal((n, K)) * 0.5).astype(np.float32)
    v = rng.standard_normal((n, dv)).astype(np.float32)
    m = sparse_amd.COO.from_numpy(mask.astype(np.float32), device=DEV)
    scores = sparse_amd.sddmm(m, q, bt=k)
    assert scores.nnz == m.nnz
    p = sparse_amd.softmax(scores, -1, scale=K ** -0.5)
    assert torch.equal(p.coords, scores.coords)
    out = sparse_amd.matmul(p, v)
    out = out if isinstance(out, np.ndarray) else out.todense()
    s64 = np.where(mask, (q.astype(np.float64) @ k.astype(np.float64).T) * np.float64(np.float32(K ** -0.5)), -np.inf)
    with np.errstate(all="ignore"):
        e = np.exp(s64 - s64.max(axis=1, keepdims=True))
        p64 = np.nan_to_num(e / e.sum(axis=1, keepdims=True))
    want = p64 @ v.astype(np.float64)
    err = np.abs(out - want).max(axis=1)
    bound = (K + mask.sum(axis=1) + 8) * np.finfo(np.float32).eps * np.abs(v).max()
    print(f"attention 64 x 64: largest share of the bound {np.max(err / bound):.3f}")
    assert (err <= bound).all() and (out[5] == 0).all()
    assert abs(_vals(p).sum() - (n - 1)) < 1e-4

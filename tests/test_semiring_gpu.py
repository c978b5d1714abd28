"""sparse_amd.semiring_matmul on the device (csrc/semiring_spmm.hip).

The yardstick is `semiring_restated` of tests/semiring_cases.py - the contract of include/sparse_amd.h A17 as a plain NumPy loop
over `np.argmin` / `np.argmax` - BIT FOR BIT for the values (any NaN equals any NaN: a payload is no result; the sign of a zero
counts) and exactly for the args; and every kernel form and sub-group width against every other.  The operands hold few distinct
values (multiples of 1 / 8, small integers, stored zeros), so products tie in nearly every output and the leftmost-wins rule is
what is tested."""
import functools

import numpy as np
import pytest
import torch

import semiring_cases as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (1, 2, 3, 4, 5, 16, 17, 64, 65, 130)
GROUPS = (8, 16, 32, 64)


def _coo(indptr, indices, vals, shape, idx=None):
    import sparse_amd

    return sparse_amd.COO(sr.coords_of(indptr, indices), vals, shape=shape, idx_dtype=idx, device=DEV, has_duplicates=False, sorted=True)


def _csr(indptr, indices, vals, shape):
    import sparse_amd

    return sparse_amd.GCXS((vals, indices, indptr), shape=shape, compressed_axes=(0,), device=DEV)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)


def _same(got, want):
    return sr.same_bits(_np(got[0]), want[0]) and np.array_equal(_np(got[1]), want[1])


@pytest.fixture
def spy(monkeypatch):
    """records the CSR triple every `semiring_spmm` call was given"""
    from sparse_amd import _kernels as K

    seen = []
    real = K.semiring_spmm

    def wrapped(indptr, indices, vals, *a, **kw):
        seen.append((indptr, indices, vals))
        return real(indptr, indices, vals, *a, **kw)

    monkeypatch.setattr(K, "semiring_spmm", wrapped)
    return seen


@functools.lru_cache(maxsize=None)
def _lengths_case(dtype, hub=False):
    """the listed lengths shuffled into one mask - or one row of 3 * 64 + 5 among empty rows -, b of 130 columns and an init; the
    restated results of every semiring for every width are computed once per type (`_want`) and shared"""
    dtype = np.dtype(dtype)
    lengths = [0, 0, 3 * 64 + 5, 0] if hub else sr.LENGTHS
    indptr, indices, vals, shape = sr.csr_mask(50 + hub, lengths, dtype, shuffle=not hub)
    b = sr.operand(51, (shape[1], 130), dtype)
    init = sr.operand(52, (shape[0], 130), dtype)
    for a in (indptr, indices, vals, b, init):
        a.setflags(write=False)
    return indptr, indices, vals, shape, b, init


@functools.lru_cache(maxsize=None)
def _want(dtype, hub, add, mul, N, with_init=False):
    """the restated (out, arg) for the first N columns of the case's b (N = 0: the 1-D b, column 0)"""
    indptr, indices, vals, shape, b, init = _lengths_case(dtype, hub)
    bb = np.ascontiguousarray(b[:, 0] if N == 0 else b[:, :N])
    ii = None if not with_init else np.ascontiguousarray(init[:, 0] if N == 0 else init[:, :N])
    out, arg = sr.semiring_restated(indptr, indices, vals, bb, add, mul, init=ii)
    out.setflags(write=False)
    arg.setflags(write=False)
    return out, arg


# ---- row lengths, widths, types, index widths -------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", sr.DTYPES)
def test_listed_lengths_and_widths_bit_for_bit(dtype, idx, monkeypatch):
    """chunk 64, so the rows of 65 to 200 elements and the row of 3 * 64 + 5 take the long form; every semiring, every width and
    the 1-D b, through the public function on a canonical COO: NumPy in, NumPy out"""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "SEMIRING_CHUNK", 64)
    for hub in (False, True):
        indptr, indices, vals, shape, b, init = _lengths_case(dtype, hub)
        a = _coo(indptr.astype(idx), indices.astype(idx), vals, shape, idx)
        for add, mul in sr.SEMIRINGS:
            for N in (0,) + WIDTHS:
                bb = np.ascontiguousarray(b[:, 0] if N == 0 else b[:, :N])
                got = sparse_amd.semiring_matmul(a, bb, add=add, mul=mul, return_arg=True)
                assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
                assert got[0].dtype == np.dtype(dtype) and got[1].dtype == np.int64
                assert got[0].shape == got[1].shape == ((shape[0],) if N == 0 else (shape[0], N))
                assert _same(got, _want(dtype, hub, add, mul, N)), (hub, add, mul, N)
            # without the arg (other kernels: no arg registers) and with an init
            for N in (1, 5, 65):
                out = sparse_amd.semiring_matmul(a, np.ascontiguousarray(b[:, :N]), add=add, mul=mul)
                assert isinstance(out, np.ndarray) and sr.same_bits(out, _want(dtype, hub, add, mul, N)[0]), (hub, add, mul, N)
                ii = np.ascontiguousarray(init[:, :N])
                got = sparse_amd.semiring_matmul(a, np.ascontiguousarray(b[:, :N]), add=add, mul=mul, init=ii, return_arg=True)
                assert _same(got, _want(dtype, hub, add, mul, N, True)), (hub, add, mul, N)
                out = sparse_amd.semiring_matmul(a, np.ascontiguousarray(b[:, :N]), add=add, mul=mul, init=ii)
                assert sr.same_bits(out, _want(dtype, hub, add, mul, N, True)[0]) and np.array_equal(ii, init[:, :N])


# ---- every form and sub-group width -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sr.DTYPES)
def test_every_form_and_group_width_gives_the_same_bits(dtype):
    """the kernel layer with `form`, `group` and `chunk` forced: "rows" and "lanes" without pieces and with pieces of 64 (which
    folds the pieces in the rows and in the lanes shape at every width), "long" - all equal to the restatement, so to each other"""
    from sparse_amd import _kernels as K

    for hub in (False, True):
        indptr, indices, vals, shape, b, init = _lengths_case(dtype, hub)
        tp, ti, tv = _dev(indptr), _dev(indices), _dev(vals)
        max_len = int(np.diff(indptr).max())
        for add, mul in sr.SEMIRINGS:
            for N in (1, 3, 5, 17, 64):
                tb, tinit = _dev(b[:, :N]), _dev(init[:, :N])
                want, want_i = _want(dtype, hub, add, mul, N), _want(dtype, hub, add, mul, N, True)
                for form, chunk in (("rows", None), ("lanes", None), ("long", None), ("rows", 64), ("lanes", 64), ("long", 128)):
                    for group in GROUPS:
                        kw = dict(add=add, mul=mul, form=form, group=group, chunk=chunk)
                        got = K.semiring_spmm(tp, ti, tv, tb, max_len, return_arg=True, **kw)
                        assert _same(got, want), (hub, add, mul, N, form, chunk, group)
                        got = K.semiring_spmm(tp, ti, tv, tb, max_len, init=tinit, return_arg=True, **kw)
                        assert _same(got, want_i), (hub, add, mul, N, form, chunk, group, "init")
                    out = K.semiring_spmm(tp, ti, tv, tb, max_len, add=add, mul=mul, form=form, chunk=chunk)      # no arg, default group
                    assert sr.same_bits(_np(out), want[0]), (hub, add, mul, N, form, chunk)


# ---- formats, strides, kinds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_coo_csr_and_csc_of_one_pattern_give_the_same_bits(dtype, spy, monkeypatch):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    monkeypatch.setattr(K, "SEMIRING_CHUNK", 64)
    indptr, indices, vals, shape, b, init = _lengths_case(dtype)
    bb = np.ascontiguousarray(b[:, :17])
    want = _want(dtype, False, "max", "times", 17)
    coo = _coo(indptr, indices, vals, shape)
    assert _same(sparse_amd.semiring_matmul(coo, bb, add="max", mul="times", return_arg=True), want)
    assert np.array_equal(_np(spy[-1][0]), indptr) and np.array_equal(_np(spy[-1][1]), indices)
    g = _csr(indptr, indices, vals, shape)                                   # a row-compressed GCXS: its own arrays, untouched
    assert _same(sparse_amd.semiring_matmul(g, bb, add="max", mul="times", return_arg=True), want)
    assert spy[-1][0] is g.indptr and spy[-1][1] is g.indices and spy[-1][2] is g.data
    gc = coo.asformat("gcxs", compressed_axes=(1,))                          # a column-compressed GCXS: the memoised CSR twin
    assert gc.compressed_axes == (1,)
    assert _same(sparse_amd.semiring_matmul(gc, bb, add="max", mul="times", return_arg=True), want)
    first = spy[-1]
    c0 = _ffi.CALLS
    assert _same(sparse_amd.semiring_matmul(gc, bb, add="max", mul="times", return_arg=True), want)
    assert all(x is y for x, y in zip(spy[-1], first)) and _ffi.CALLS == c0 + 1        # a second call converts nothing: one launch


@pytest.mark.parametrize("vdtype", [np.bool_, np.int32, np.float32, np.float64])
def test_values_are_converted_to_the_type_of_b(vdtype):
    import sparse_amd

    indptr, indices, vals, shape = sr.csr_mask(60, [0, 3, 70, 9, 1], vdtype)
    a = _coo(indptr, indices, vals, shape)
    for bdt in (np.float32, np.float64, np.int32, np.int64):
        b = sr.operand(61, (shape[1], 6), bdt)
        if not (np.dtype(vdtype).kind == "b" or np.can_cast(vdtype, bdt, "same_kind")):
            with pytest.raises(TypeError, match="cannot be converted"):
                sparse_amd.semiring_matmul(a, b)
            continue
        got = sparse_amd.semiring_matmul(a, b, add="max", mul="plus", return_arg=True)
        assert got[0].dtype == np.dtype(bdt) and _same(got, sr.semiring_restated(indptr, indices, vals, b, "max", "plus"))


def test_strided_operands_and_the_kind_of_the_result():
    """b and init as a transposed view and as a column slice with a pitch; NumPy in gives NumPy out, any tensor a device tensor"""
    import sparse_amd

    indptr, indices, vals, shape, b, init = _lengths_case(np.float64)
    a = _coo(indptr, indices, vals, shape)
    for N in (1, 4, 6, 64):
        want = _want(np.float64, False, "min", "times", N, True)
        views = {"transposed": (_dev(b[:, :N].T).T, _dev(init[:, :N].T).T), "sliced": (_dev(b)[:, :N], _dev(init)[:, :N]),
                 "offset": (_dev(b[:, :N + 3])[:, 3:], _dev(init[:, :N + 3])[:, 3:])}
        for name, (tb, ti) in views.items():
            assert N == 1 or not tb.is_contiguous()
            w = want if name != "offset" else sr.semiring_restated(indptr, indices, vals, b[:, 3:N + 3], "min", "times", init=init[:, 3:N + 3])
            keep = ti.clone()
            got = sparse_amd.semiring_matmul(a, tb, add="min", mul="times", init=ti, return_arg=True)
            assert isinstance(got[0], torch.Tensor) and isinstance(got[1], torch.Tensor) and got[0].is_cuda and got[1].dtype == torch.int64
            assert _same(got, w), (N, name)
            assert torch.equal(ti, keep)                                                 # the init is not modified
        nb, ni = np.asfortranarray(b[:, :N]), np.asfortranarray(init[:, :N])            # strided ndarrays
        got = sparse_amd.semiring_matmul(a, nb, add="min", mul="times", init=ni, return_arg=True)
        assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray) and _same(got, want)
        mixed = sparse_amd.semiring_matmul(a, nb, add="min", mul="times", init=_dev(ni))
        assert isinstance(mixed, torch.Tensor) and sr.same_bits(_np(mixed), want[0])
    t1 = sparse_amd.semiring_matmul(a, _dev(b)[:, 7], add="min", mul="times", return_arg=True)      # a 1-D b with a stride
    assert t1[0].shape == (shape[0],) and _same(t1, sr.semiring_restated(indptr, indices, vals, b[:, 7], "min", "times"))


# ---- adversarial values ---------------------------------------------------------------------------------------------------------------
def _adversarial_matrix(dtype, with_init):
    """every hand-written sequence of tests/semiring_cases.py (those with / without an init) of one semiring placed into rows of 65 and
    129 elements, its elements at every ascending choice of the positions 0, G - 1, G, n - 1 for G = 8, 16, 32, 64; the other
    elements of such a row are fillers that never win.  Returns {(add, mul): (indptr, indices, vals, b, init)}; b has 5 equal columns"""
    dtype = np.dtype(dtype)
    import itertools

    big = 1e30 if dtype.kind == "f" else 1000
    mats = {}
    for case in sr.ADVERSARIAL:
        name, add, mul, av, bv, ini, at, value = case
        av, bv = np.asarray(av), np.asarray(bv)
        if (av.dtype.kind == "i") != (dtype.kind == "i") or (ini is not None) != with_init:
            continue
        rows = mats.setdefault((add, mul), [])
        fill_a = big if add == "min" else -big
        fill_b = 0 if mul == "plus" else 1
        for n in (65, 129):
            for G in GROUPS:
                for places in itertools.combinations(sorted({0, G - 1, G, n - 1}), len(av)):
                    ra, rb = np.full(n, fill_a, dtype), np.full(n, fill_b, dtype)
                    ra[list(places)], rb[list(places)] = av.astype(dtype), bv.astype(dtype)
                    rows.append((ra, rb, fill_a if ini is None else ini))
    out = {}
    for key, rows in mats.items():
        # row r's element e sits at inner index e of its own block of b: K = the sum of the lengths
        lens = [len(r[0]) for r in rows]
        indptr = np.concatenate(([0], np.cumsum(lens)))
        vals = np.concatenate([r[0] for r in rows])
        b = np.repeat(np.concatenate([r[1] for r in rows])[:, None], 5, axis=1)
        init = np.repeat(np.array([r[2] for r in rows], dtype)[:, None], 5, axis=1) if with_init else None
        out[key] = (indptr, np.arange(len(vals), dtype=np.int64), vals, b, init)
    return out


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_adversarial_values_across_lane_register_and_piece_boundaries(dtype, with_init):
    """NaN first / middle / last, ties, signed zeros, inf - inf, 0 * inf, integer wrap-around, an init that ties: value bits (the
    sign of a zero included) and arg, in the default form (rows: N = 5), in the lanes form (N = 1) and in every forced form with
    pieces of 64, so that the special elements sit at the first and last lane of a sub-group, the first element of the next
    fetch, and the first and last element of a piece"""
    from sparse_amd import _kernels as K

    mats = _adversarial_matrix(dtype, with_init)
    assert mats or (np.dtype(dtype).kind == "i" and with_init)
    for (add, mul), (indptr, indices, vals, b, init) in mats.items():
        want5 = sr.semiring_restated(indptr, indices, vals, b, add, mul, init=init)
        want1 = (want5[0][:, :1], want5[1][:, :1])
        tp, ti, tv, tb = _dev(indptr), _dev(indices), _dev(vals), _dev(b)
        tinit = None if init is None else _dev(init)
        for N, want in ((5, want5), (1, want1)):
            bN, iN = tb[:, :N], (None if tinit is None else tinit[:, :N])
            assert _same(K.semiring_spmm(tp, ti, tv, bN, 129, add=add, mul=mul, init=iN, return_arg=True), want), (add, mul, N)
            for form, chunk in (("rows", None), ("lanes", None), ("rows", 64), ("lanes", 64)):
                for group in GROUPS:
                    got = K.semiring_spmm(tp, ti, tv, bN, 129, add=add, mul=mul, init=iN, return_arg=True, form=form, group=group, chunk=chunk)
                    assert _same(got, want), (add, mul, N, form, chunk, group)
                out = K.semiring_spmm(tp, ti, tv, bN, 129, add=add, mul=mul, init=iN, form=form, chunk=chunk)
                assert sr.same_bits(_np(out), want[0]), (add, mul, N, form, chunk)


# ---- init and degenerate shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_init_of_identities_and_a_bellman_ford_step(dtype, monkeypatch):
    """`init=None` against an init of identities: the same `out`.  The args differ exactly where the result IS the identity and
    the row is not empty - every product of the row equals the identity -: without an init the first element is picked (arg =
    its k), with one the init ties and comes first (arg = -1).  Empty rows give -1 either way."""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "SEMIRING_CHUNK", 64)
    dtype = np.dtype(dtype)
    indptr, indices, vals, shape = sr.csr_mask(70, [0, 5, 70, 3, 130, 0, 2], dtype)
    b = sr.operand(71, (shape[1], 6), dtype)
    a = _coo(indptr, indices, vals, shape)
    for add in sr.ADDS:
        ident = sr.identity(add, dtype)
        vals2 = vals.copy()
        r = int(np.nonzero(np.diff(indptr) == 3)[0][0])                      # the row of 3 elements: all of them the identity
        vals2[indptr[r]:indptr[r + 1]] = ident
        b2 = b.copy()
        b2[indices[indptr[r]:indptr[r + 1]]] = 0
        a2 = _coo(indptr, indices, vals2, shape)
        plain = sparse_amd.semiring_matmul(a2, b2, add=add, mul="plus", return_arg=True)
        full = sparse_amd.semiring_matmul(a2, b2, add=add, mul="plus", init=np.full((shape[0], 6), ident), return_arg=True)
        assert _same(plain, sr.semiring_restated(indptr, indices, vals2, b2, add, "plus"))
        assert sr.same_bits(plain[0], full[0])
        empty = np.diff(indptr) == 0
        differ = plain[1] != full[1]
        assert differ.any(axis=1).tolist() == [i == r for i in range(shape[0])] and differ[r].all()
        assert (plain[1][r] == indices[indptr[r]]).all() and (full[1][r] == -1).all() and (plain[0][r] == ident).all()
        assert (plain[1][empty] == -1).all() and (full[1][empty] == -1).all() and (plain[0][empty] == ident).all()
    # one Bellman-Ford step d' = min(d, A min.+ d): init = d, a finite vector; d is not modified
    sq = sr.csr_mask(73, [0, 5, 70, 3, 130, 0, 2] + [1] * (shape[1] - 7), dtype, ncols=shape[1])
    dd = sr.operand(74, (shape[1],), dtype)
    keep = dd.copy()
    got = sparse_amd.semiring_matmul(_coo(*sq[:3], sq[3]), dd, add="min", mul="plus", init=dd, return_arg=True)
    assert _same(got, sr.semiring_restated(*sq[:3], dd, "min", "plus", init=dd)) and np.array_equal(dd, keep)
    with np.errstate(over="ignore"):
        assert (got[0] <= dd).all() and ((got[1] == -1) == (got[0] == dd)).all()


def test_degenerate_shapes_make_no_launch():
    import sparse_amd
    from sparse_amd import _ffi

    def coo(shape, dtype=np.float32):
        return sparse_amd.COO(np.zeros((2, 0), np.int64), np.zeros(0, dtype), shape=shape, device=DEV)

    e69, e09, e60 = coo((6, 9)), coo((0, 9)), coo((6, 0))
    ints = {dt: coo((6, 9), dt) for dt in (np.int32, np.int64)}
    init = np.arange(24, dtype=np.float32).reshape(6, 4)
    tinit = _dev(init)
    c0 = _ffi.CALLS
    for add, ident in (("min", np.inf), ("max", -np.inf)):
        out, arg = sparse_amd.semiring_matmul(e69, np.ones((9, 4), np.float32), add=add, return_arg=True)                # nnz = 0
        assert out.shape == arg.shape == (6, 4) and out.dtype == np.float32 and (out == ident).all() and (arg == -1).all()
        out = sparse_amd.semiring_matmul(e69, np.ones(9, np.float64), add=add)
        assert out.shape == (6,) and out.dtype == np.float64 and (out == ident).all()
    for add, pick in (("min", "max"), ("max", "min")):
        for dt in (np.int32, np.int64):
            out = sparse_amd.semiring_matmul(ints[dt], np.ones((9, 2), dt), add=add)
            assert out.dtype == np.dtype(dt) and (out == getattr(np.iinfo(dt), pick)).all()
    out, arg = sparse_amd.semiring_matmul(e69, np.ones((9, 4), np.float32), init=init, return_arg=True)
    assert np.array_equal(out, init) and (arg == -1).all() and not np.shares_memory(out, init)
    tout = sparse_amd.semiring_matmul(e69, np.ones((9, 4), np.float32), init=tinit)
    assert isinstance(tout, torch.Tensor) and torch.equal(tout, tinit) and tout.data_ptr() != tinit.data_ptr()
    out, arg = sparse_amd.semiring_matmul(e09, np.ones((9, 4), np.float32), return_arg=True)                             # M = 0
    assert out.shape == arg.shape == (0, 4) and arg.dtype == np.int64
    out, arg = sparse_amd.semiring_matmul(e60, np.ones((0, 4), np.float32), add="max", return_arg=True)                  # K = 0
    assert out.shape == (6, 4) and (out == -np.inf).all() and (arg == -1).all()
    assert _ffi.CALLS == c0
    one = _coo(np.array([0, 1, 1]), np.array([2]), np.ones(1, np.float32), (2, 9))                                       # N = 0
    out, arg = sparse_amd.semiring_matmul(one, np.ones((9, 0), np.float32), return_arg=True)
    assert out.shape == arg.shape == (2, 0)


def test_two_calls_return_the_same_bits():
    import sparse_amd

    indptr, indices, vals, shape, b, init = _lengths_case(np.float32)
    a = _coo(indptr, indices, vals, shape)
    for N in (1, 64):
        tb = _dev(b[:, :N])
        one = sparse_amd.semiring_matmul(a, tb, add="max", mul="plus", return_arg=True)
        two = sparse_amd.semiring_matmul(a, tb, add="max", mul="plus", return_arg=True)
        assert torch.equal(one[0].view(torch.int32), two[0].view(torch.int32)) and torch.equal(one[1], two[1])
        assert one[0].data_ptr() != two[0].data_ptr()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_single_source_shortest_paths_equal_a_numpy_bellman_ford():
    """200 nodes, about 4 edges in per node, integer-valued float32 weights 1 .. 9 (every sum is exact): d = min(d, A min.+ d)
    until nothing changes, against Bellman-Ford over the edge list in NumPy - exactly.  A[i, k] is the weight of the edge
    k -> i, so row i relaxes node i over its incoming edges"""
    import sparse_amd

    rng = np.random.default_rng(80)
    n = 200
    dense = rng.random((n, n)) < 4 / n
    np.fill_diagonal(dense, False)
    dense[150:, :] = False
    dense[150:, 150:] = rng.random((50, 50)) < 0.1                         # an island the source does not reach: +inf stays
    np.fill_diagonal(dense, False)
    dst, src = np.nonzero(dense)
    w = rng.integers(1, 10, len(dst)).astype(np.float32)
    indptr = np.concatenate(([0], np.cumsum(dense.sum(axis=1))))
    a = _coo(indptr, src, w, (n, n))
    d0 = np.full(n, np.inf, np.float32)
    d0[0] = 0
    want = d0.copy()
    for _ in range(n):
        relaxed = want.copy()
        np.minimum.at(relaxed, dst, want[src] + w)
        if np.array_equal(relaxed, want):
            break
        want = relaxed
    d = _dev(d0)
    for steps in range(1, n + 1):
        new, arg = sparse_amd.semiring_matmul(a, d, add="min", mul="plus", init=d, return_arg=True)
        if torch.equal(new, d):
            break
        d = new
    got = _np(d)
    assert steps < n and np.array_equal(got, want) and np.isinf(got[150:]).all() and np.isfinite(got[:150]).sum() > 100
    assert (_np(arg) == -1).all()                                           # the fixed point: the init wins every tie

"""sparse_amd.semiring_matmul_grad and semiring_matmul_autograd on the device (csrc/semiring_grad.hip).

The yardstick is `grad_restated` of tests/semiring_grad_cases.py - the contract of include/sparse_amd.h A18 as plain NumPy loops -
BIT FOR BIT (any NaN equals any NaN; the sign of a zero counts) for da, db and dinit, with the arg taken from the fused forward
of each of the four semirings; and every column form and sub-group width against that same restatement."""
import functools

import numpy as np
import pytest
import torch

import semiring_cases as sr
import semiring_grad_cases as sg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (1, 2, 3, 4, 5, 16, 17, 64, 65, 130)
GROUPS = (8, 16, 32, 64)
HUB = 3 * 64 + 5


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
    return len(got) == len(want) and all(sr.same_bits(_np(a), b) for a, b in zip(got, want))


def _grad_operand(seed, shape, dtype):
    """full mantissas, so that every sum rounds; a few exact zeros and one -0.0"""
    g = np.random.default_rng(seed).standard_normal(shape).astype(dtype)
    g.reshape(-1)[::7] = 0
    g.reshape(-1)[3:4] = -0.0
    return g


@functools.lru_cache(maxsize=None)
def _mask(kind, dtype):
    """"rows": the listed lengths as row lengths; "cols": its transpose - the listed lengths as column lengths; "hub_row" /
    "hub_col": one row / column of 3 * 64 + 5 elements among empty ones.  With b and g of 130 columns and an init"""
    dtype = np.dtype(dtype)
    if kind in ("rows", "cols"):
        m = sr.csr_mask(50, sr.LENGTHS, dtype)
    else:
        m = sr.csr_mask(51, [0, 0, HUB, 0], dtype, shuffle=False)
    indptr, indices, vals, shape = m if kind in ("rows", "hub_row") else sg.transposed(*m)
    indptr, indices = indptr.astype(np.int64), indices.astype(np.int64)
    b = sr.operand(52, (shape[1], 130), dtype)
    init = sr.operand(53, (shape[0], 130), dtype)
    g = _grad_operand(54, (shape[0], 130), dtype)
    for a in (indptr, indices, vals, b, init, g):
        a.setflags(write=False)
    return indptr, indices, vals, shape, b, init, g


def _cut(x, N):
    return np.ascontiguousarray(x[:, 0] if N == 0 else x[:, :N])


@functools.lru_cache(maxsize=None)
def _arg(kind, dtype, add, mul, N, with_init):
    """the arg of the fused forward (the restated one: tests/test_semiring_gpu.py pins the device's to it bit for bit)"""
    indptr, indices, vals, shape, b, init, g = _mask(kind, dtype)
    arg = sr.semiring_restated(indptr, indices, vals, _cut(b, N), add, mul, init=_cut(init, N) if with_init else None)[1]
    arg.setflags(write=False)
    return arg


@functools.lru_cache(maxsize=None)
def _want(kind, dtype, add, mul, N, with_init, chunk=sg.CHUNK):
    indptr, indices, vals, shape, b, init, g = _mask(kind, dtype)
    arg = _arg(kind, dtype, add, mul, N, with_init)
    out = sg.grad_restated(indptr, indices, vals, _cut(b, N), arg, _cut(g, N), mul, chunk)
    for a in out:
        a.setflags(write=False)
    return out


# ---- row and column lengths, widths, types, index widths ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", sg.DTYPES)
def test_listed_lengths_and_widths_bit_for_bit(dtype, idx):
    """the public function on a canonical COO, NumPy in, NumPy out; the arg comes from the fused forward of the semiring on the
    device.  The widths take turns between the semirings and between with and without an init, so that every width meets both
    muls, and both adds, with and without an init"""
    import sparse_amd

    n = 0
    for kind in ("rows", "cols"):
        indptr, indices, vals, shape, b, init, g = _mask(kind, dtype)
        a = _coo(indptr.astype(idx), indices.astype(idx), vals, shape, idx)
        for wi, N in enumerate((0,) + WIDTHS):
            for si, (add, mul) in enumerate(sr.SEMIRINGS):
                if (wi + si) % 2 != (kind == "cols"):
                    continue
                with_init = (wi + si // 2) % 2 == 1
                bb, gg, ii = _cut(b, N), _cut(g, N), (_cut(init, N) if with_init else None)
                out, arg = sparse_amd.semiring_matmul(a, bb, add=add, mul=mul, init=ii, return_arg=True)
                assert np.array_equal(arg, _arg(kind, dtype, add, mul, N, with_init))
                got = sparse_amd.semiring_matmul_grad(a, bb, arg, gg, mul=mul, with_init=True)
                assert all(isinstance(t, np.ndarray) and t.dtype == np.dtype(dtype) for t in got)
                assert got[0].shape == vals.shape and got[1].shape == bb.shape and got[2].shape == gg.shape
                assert _same(got, _want(kind, dtype, add, mul, N, with_init)), (kind, add, mul, N, with_init)
                assert _same(sparse_amd.semiring_matmul_grad(a, bb, arg, gg, mul=mul), _want(kind, dtype, add, mul, N, with_init)[:2])
                n += 1
    assert n == 44


# ---- the column forms at every width ------------------------------------------------------------------------------------------------
def _kernel_args(kind, dtype, N):
    from sparse_amd import _attention as A

    indptr, indices, vals, shape, b, init, g = _mask(kind, dtype)
    a = _csr(indptr, indices, vals, shape)
    plan = A._column_grouping(a, a.indices, a.indptr)
    return a, plan, _dev(_cut(b, N)), _dev(_cut(g, N))


@pytest.mark.parametrize("dtype", sg.DTYPES)
def test_every_column_form_at_every_width(dtype):
    """sub-groups (short_max 64: the columns of at most 64 elements; the longer ones a wave each), a wave each (short_max 0),
    pieces (chunk 64: the columns of 65 to 200 elements and the column of 3 * 64 + 5) - at every width, and a lane per column for
    the results of at most 4 columns.  short_max and the widths change no bit; `chunk` is part of the order"""
    from sparse_amd import _kernels as K

    for kind in ("cols", "hub_col"):
        for N, (add, mul) in zip((3, 17, 130, 4), sr.SEMIRINGS):
            a, plan, tb, tg = _kernel_args(kind, dtype, N)
            targ = _dev(_arg(kind, dtype, add, mul, N, False))
            assert plan["max_col"] == (200 if kind == "cols" else HUB)
            for kw, chunk in ((dict(short_max=64), sg.CHUNK), (dict(short_max=0), sg.CHUNK), (dict(col_form="wide"), sg.CHUNK),
                              (dict(col_form="long"), 64), (dict(chunk=64, short_max=64), 64), (dict(chunk=128, short_max=7), 128)):
                want = _want(kind, dtype, add, mul, N, False, chunk)
                for cg in GROUPS + ((1,) if N <= 4 else ()):
                    got = K.semiring_grad(a.indptr, a.indices, a.data, plan["colptr"], plan["colperm"], plan["colrows"], tb, targ, tg,
                                          plan["max_col"], mul=mul, want=(True, True, True), col_group=cg, **kw)
                    assert _same(got, want), (kind, N, mul, kw, cg)


@pytest.mark.parametrize("dtype", sg.DTYPES)
def test_element_pass_at_every_width(dtype):
    """every sub-group width on one row of 3 * 64 + 5 elements and on the listed lengths: no bit changes"""
    from sparse_amd import _kernels as K

    for kind in ("hub_row", "rows"):
        for N, (add, mul) in zip((1, 5, 64, 130), sr.SEMIRINGS):
            a, plan, tb, tg = _kernel_args(kind, dtype, N)
            targ = _dev(_arg(kind, dtype, add, mul, N, False))
            want = _want(kind, dtype, add, mul, N, False)
            for group in GROUPS:
                got = K.semiring_grad(a.indptr, a.indices, a.data, None, None, None, tb, targ, tg, 0, mul=mul, want=(True, False, False),
                                      group=group)
                assert got[1] is None and got[2] is None and sr.same_bits(_np(got[0]), want[0]), (kind, N, mul, group)


# ---- formats ----------------------------------------------------------------------------------------------------------------------------
def test_formats_give_da_in_the_callers_order_and_a_second_call_builds_nothing(monkeypatch):
    import sparse_amd
    from sparse_amd import _attention as A, _ffi

    built, names = [], []
    real, real_call = A._build_grad_plan, _ffi.call
    monkeypatch.setattr(A, "_build_grad_plan", lambda *a: built.append(1) or real(*a))
    monkeypatch.setattr(_ffi, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    dtype, N, add, mul = np.float32, 17, "max", "times"
    indptr, indices, vals, shape, b, init, g = _mask("rows", dtype)
    tb, tg = _dev(_cut(b, N)), _dev(_cut(g, N))
    targ = _dev(_arg("rows", dtype, add, mul, N, False))
    want = _want("rows", dtype, add, mul, N, False)
    coo = _coo(indptr, indices, vals, shape)
    csc = coo.asformat("gcxs", compressed_axes=(1,))
    assert csc.compressed_axes == (1,)
    # the caller's order of the CSC: its own data, column by column
    order = np.lexsort((sr.coords_of(indptr, indices)[0], indices))
    assert np.array_equal(_np(csc.data), vals[order])
    for x, perm in ((coo, None), (_csr(indptr, indices, vals, shape), None), (csc, order)):
        del built[:]
        first = sparse_amd.semiring_matmul_grad(x, tb, targ, tg, mul=mul)
        assert all(isinstance(t, torch.Tensor) for t in first) and built == [1]
        plan = x._attention_grad_plan
        del names[:]
        second = sparse_amd.semiring_matmul_grad(x, tb, targ, tg, mul=mul)
        # the kernel's one call; for the column-compressed array one more, the gather of da into the caller's order
        assert names.count("spamd_semiring_grad") == 1 and len(names) == (1 if perm is None else 2), names
        assert built == [1] and x._attention_grad_plan is plan
        assert all(torch.equal(p, q) for p, q in zip(first, second))
        assert _same(second, (want[0] if perm is None else want[0][perm], want[1]))
        # the plan is the one attention's backward uses: it builds nothing either
        q = torch.zeros(shape[0], 4, device=DEV)
        k = torch.zeros(shape[1], 4, device=DEV)
        sparse_amd.sparse_attention_grad(x, q, k, k, q)
        assert built == [1] and x._attention_grad_plan is plan


# ---- values and layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", [np.bool_, np.int32, np.float32, np.float64])
def test_values_of_other_types_are_converted_and_values_replace_them(vdtype):
    import sparse_amd

    dtype, N, add, mul = np.float64, 5, "min", "times"
    indptr, indices, _, shape = sr.csr_mask(60, [0, 3, 9, 1, 70, 0, 5], np.float64)
    rng = np.random.default_rng(61)
    vals = sr.values(rng, len(indices), vdtype)
    b, g = sr.operand(62, (shape[1], N), dtype), _grad_operand(63, (shape[0], N), dtype)
    arg = sr.semiring_restated(indptr, indices, vals, b, add, mul)[1]
    want = sg.grad_restated(indptr, indices, vals, b, arg, g, mul)
    a = _coo(indptr, indices, vals, shape)
    assert _same(sparse_amd.semiring_matmul_grad(a, b, arg, g, mul=mul), want[:2])
    # `values=` takes the place of the stored values: an array of ones with the real values handed in
    ones = _coo(indptr, indices, np.ones(len(indices), np.float32), shape)
    assert _same(sparse_amd.semiring_matmul_grad(ones, b, arg, g, mul=mul, values=vals), want[:2])
    got = sparse_amd.semiring_matmul_grad(ones, b, arg, g, mul=mul, values=_dev(vals))
    assert all(isinstance(t, torch.Tensor) for t in got) and _same(got, want[:2])
    # on a column-compressed array `values` and da are in ITS order
    csc = ones.asformat("gcxs", compressed_axes=(1,))
    order = np.lexsort((sr.coords_of(indptr, indices)[0], indices))
    got = sparse_amd.semiring_matmul_grad(csc, b, arg, g, mul=mul, values=vals[order])
    assert _same(got, (want[0][order], want[1]))


def test_pitched_transposed_and_misaligned_operands():
    import sparse_amd

    dtype, add, mul = np.float32, "max", "times"
    indptr, indices, vals, shape, b, init, g = _mask("rows", dtype)
    a = _coo(indptr, indices, vals, shape)
    M, Kd = shape
    for N in (4, 17, 64):
        arg = _arg("rows", dtype, add, mul, N, True)
        want = _want("rows", dtype, add, mul, N, True)
        bb, gg = _cut(b, N), _cut(g, N)

        def pitched(x, pad, off):      # rows of N inside rows of N + pad, starting `off` elements into the buffer
            buf = torch.zeros(x.shape[0] * (N + pad) + off, dtype=_dev(x).dtype, device=DEV)
            view = buf[off:].reshape(x.shape[0], N + pad)[:, :N]
            view.copy_(_dev(x))
            return view

        for pad, off in ((0, 0), (3, 0), (4, 0), (4, 1), (0, 1), (8, 2)):
            tb, tg, ta = pitched(bb, pad, off), pitched(gg, pad, off), pitched(arg, pad, off)
            keep = [t.clone() for t in (tb, tg, ta)]
            got = sparse_amd.semiring_matmul_grad(a, tb, ta, tg, mul=mul, with_init=True)
            assert _same(got, want), (N, pad, off)
            assert all(torch.equal(t, k) for t, k in zip((tb, tg, ta), keep))                      # inputs untouched
        # transposed (column-major) operands: one copy inside, the same bits
        tb, tg, ta = (_dev(np.ascontiguousarray(x.T)).T for x in (bb, gg, arg))
        assert not tb.is_contiguous() and _same(sparse_amd.semiring_matmul_grad(a, tb, ta, tg, mul=mul, with_init=True), want)
        # the forward with a pitched init gives the arg the backward was checked with
        ti = pitched(_cut(init, N), 3, 1)
        out, targ = sparse_amd.semiring_matmul(a, _dev(bb), add=add, mul=mul, init=ti, return_arg=True)
        assert np.array_equal(_np(targ), arg)


# ---- cases and invariants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sg.DTYPES)
def test_hand_written_cases(dtype):
    import sparse_amd

    for name, indptr, indices, vals, b, arg, g, mul, da, db, dinit in sg.hand_cases(dtype):
        a = _csr(indptr, indices, vals, (len(indptr) - 1, b.shape[0]))
        got = sparse_amd.semiring_matmul_grad(a, b, arg, g, mul=mul, with_init=True)
        assert _same(got, (da, db, dinit)), (name, got)
    for mul in sg.MULS:
        indptr, indices, vals, b, arg, g, want = sg.n130_case(dtype, mul)
        a = _csr(indptr, indices, vals, (1, 2))
        da, db = sparse_amd.semiring_matmul_grad(a, b, arg, g, mul=mul)
        assert sr.same_bits(da, want) and _same((da, db), sg.grad_restated(indptr, indices, vals, b, arg, g, mul)[:2])


@pytest.mark.parametrize("n", [65, 129])
def test_hand_written_situations_at_the_edges_of_rows_and_columns(n):
    """the hand-written situations (a lone hit, g = -0.0, NaN and inf in g, a stored zero, an arg the row does not store, arg -1, a
    duplicate) at the positions 0, G - 1, G, n - 1 of a row - and of a column - of 65 and 129 elements: every width, the wave
    form and the pieces (chunk 64)"""
    from sparse_amd import _attention as A, _kernels as K

    dtype = np.float64
    for mul in sg.MULS:
        for where in sorted({0, n - 1} | {G - 1 for G in GROUPS} | set(GROUPS)):
            widths = [G for G in GROUPS if where in (0, G - 1, G, n - 1)]
            for kind in sg.PLACED:
                indptr, indices, vals, b, arg, g = sg.place_in(n, where, dtype, mul, kind)
                a = _csr(indptr, indices, vals, (1, n + 2))
                want = sg.grad_restated(indptr, indices, vals, b, arg, g, mul, 64)
                credited = {"arg not stored": 0, "arg all -1": 0, "duplicate": 2}.get(kind, 1)
                if kind not in ("g = -0.0", "nan and inf in g"):
                    assert np.count_nonzero(want[0]) == (credited if not (kind == "stored zero" and mul == "plus") else 1)
                plan = A._column_grouping(a, a.indices, a.indptr)
                tptr, tidx, tvals, tb, targ, tg = sg.place_in_column(n, where, dtype, mul, kind)
                t = _csr(tptr, tidx, tvals, (n, 3))
                tplan = A._column_grouping(t, t.indices, t.indptr)
                wants = {c: sg.grad_restated(tptr, tidx, tvals, tb, targ, tg, mul, c) for c in (64, 1024)}
                for G in widths:
                    got = K.semiring_grad(a.indptr, a.indices, a.data, plan["colptr"], plan["colperm"], plan["colrows"], _dev(b),
                                          _dev(arg), _dev(g), plan["max_col"], mul=mul, want=(True, True, True), group=G, col_group=G,
                                          chunk=64)
                    assert _same(got, want), ("row", mul, G, where, kind)
                    for kw in (dict(short_max=0, chunk=1024), dict(chunk=64), dict(chunk=64, col_group=1)):
                        got = K.semiring_grad(t.indptr, t.indices, t.data, tplan["colptr"], tplan["colperm"], tplan["colrows"],
                                              _dev(tb), _dev(targ), _dev(tg), tplan["max_col"], mul=mul, want=(True, True, True),
                                              **dict(dict(group=G, col_group=G), **kw))
                        assert _same(got, wants[kw["chunk"]]), ("column", mul, G, where, kind, kw)


def test_two_calls_give_the_same_bits_and_degenerate_shapes_run_without_a_launch():
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    dtype, N, add, mul = np.float32, 65, "min", "plus"
    indptr, indices, vals, shape, b, init, g = _mask("cols", dtype)
    a = _coo(indptr, indices, vals, shape)
    tb, tg, targ = _dev(_cut(b, N)), _dev(_cut(g, N)), _dev(_arg("cols", dtype, add, mul, N, True))
    first = sparse_amd.semiring_matmul_grad(a, tb, targ, tg, mul=mul, with_init=True)
    second = sparse_amd.semiring_matmul_grad(a, tb, targ, tg, mul=mul, with_init=True)
    assert all(torch.equal(p, q) for p, q in zip(first, second)) and _same(first, _want("cols", dtype, add, mul, N, True))

    def coo(shape):
        return sparse_amd.COO(np.zeros((2, 0), np.int64), np.zeros(0, np.float32), shape=shape, device=DEV)

    c0 = _ffi.CALLS
    g64 = np.arange(24, dtype=np.float32).reshape(6, 4) - 7
    da, db, di = sparse_amd.semiring_matmul_grad(coo((6, 9)), np.ones((9, 4), np.float32), np.full((6, 4), -1), g64, with_init=True)      # nnz = 0
    assert da.shape == (0,) and db.shape == (9, 4) and not db.any() and not np.signbit(db).any() and np.array_equal(di, g64)
    da, db = sparse_amd.semiring_matmul_grad(coo((0, 9)), np.ones((9, 4), np.float32), np.zeros((0, 4), np.int64), np.zeros((0, 4), np.float32))
    assert da.shape == (0,) and db.shape == (9, 4) and not db.any()                                                                       # M = 0
    da, db, di = sparse_amd.semiring_matmul_grad(coo((6, 0)), np.ones((0, 4), np.float32), np.full((6, 4), -1), g64, mul="times", with_init=True)
    assert db.shape == (0, 4) and np.array_equal(di, g64)                                                                                 # K = 0
    tda, tdb, tdi = sparse_amd.semiring_matmul_grad(coo((6, 9)), torch.ones(9, 4), torch.full((6, 4), -1), _dev(g64), with_init=True)
    assert all(isinstance(t, torch.Tensor) for t in (tda, tdb, tdi)) and torch.equal(tdi, _dev(g64)) and tdi.data_ptr() != _dev(g64).data_ptr()
    assert _ffi.CALLS == c0
    one = _coo(np.array([0, 1, 1]), np.array([2]), np.ones(1, np.float32), (2, 9))                                                        # N = 0
    da, db, di = sparse_amd.semiring_matmul_grad(one, np.ones((9, 0), np.float32), np.zeros((2, 0), np.int64), np.zeros((2, 0), np.float32), with_init=True)
    assert da.shape == (1,) and da[0] == 0 and not np.signbit(da[0]) and db.shape == (9, 0) and di.shape == (2, 0)
    assert K.SEMIRING_GRAD_STATS == dict(da=False, db=False, dinit=False)      # no pass of the backward was launched
    # a 1-D b: db is 1-D
    da, db = sparse_amd.semiring_matmul_grad(one, np.ones(9, np.float32), np.array([2, -1]), np.array([3.0, 4.0], np.float32))
    assert db.shape == (9,) and db[2] == 3.0 and da[0] == 3.0 and np.count_nonzero(db) == 1


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def _tie_free_device(mul, seed=21):
    indptr, indices, vals, b, init = sg.tie_free(seed, [0, 1, 2, 3, 5, 4, 5, 0, 2, 3, 1, 4], 9, 5, np.float64, mul)
    assert sg.products_distinct(indptr, indices, vals, b, mul, init, gap=1e-3)
    return indptr, indices, vals, b, init


@pytest.mark.parametrize("add,mul", sr.SEMIRINGS)
def test_gradcheck(add, mul):
    """float64, 12 x 9 x 5, tie-free with gaps of at least 1e-3 at eps 1e-6: b, init and values require gradients"""
    import sparse_amd

    indptr, indices, vals, b, init = _tie_free_device(mul)
    a = _coo(indptr, indices, np.ones(len(indices)), (12, 9))
    tb, ti, tv = (_dev(x).requires_grad_() for x in (b, init, vals))
    fn = lambda bb, ii, vv: sparse_amd.semiring_matmul_autograd(a, bb, add=add, mul=mul, init=ii, values=vv)
    assert torch.autograd.gradcheck(fn, (tb, ti, tv), eps=1e-6, atol=1e-6, rtol=1e-6)
    out, arg = sparse_amd.semiring_matmul_autograd(a, tb, add=add, mul=mul, init=ti, values=tv, return_arg=True)
    assert out.requires_grad and not arg.requires_grad and arg.dtype == torch.int64
    assert (arg == -1).any() and (arg >= 0).any()


def test_autograd_carries_the_bits_of_the_grad_function_and_skips_what_is_not_needed(monkeypatch):
    import sparse_amd
    from sparse_amd import _kernels as K

    wants = []
    real = K.semiring_grad
    monkeypatch.setattr(K, "semiring_grad", lambda *a, **kw: wants.append(tuple(kw["want"])) or real(*a, **kw))
    dtype, N = np.float32, 17
    indptr, indices, vals, shape, b, init, g = _mask("rows", dtype)
    a = _coo(indptr, indices, vals, shape)
    for add, mul in sr.SEMIRINGS:
        tb, ti, tg = _dev(_cut(b, N)), _dev(_cut(init, N)), _dev(_cut(g, N))
        tv = _dev(vals)
        fwd = sparse_amd.semiring_matmul(a, tb, add=add, mul=mul, init=ti, return_arg=True)
        for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            xb, xi, xv = (t.clone().requires_grad_(n) for t, n in zip((tb, ti, tv), need))
            out, arg = sparse_amd.semiring_matmul_autograd(a, xb, add=add, mul=mul, init=xi, values=xv, return_arg=True)
            assert torch.equal(out, fwd[0]) and torch.equal(arg, fwd[1])                        # the forward's bits
            del wants[:]
            out.backward(tg)
            assert wants == [(need[2], need[0], need[1])]                                       # (da, db, dinit) of (values, b, init)
            assert K.SEMIRING_GRAD_STATS == dict(da=need[2], db=need[0], dinit=need[1])
            ref = sparse_amd.semiring_matmul_grad(a, tb, fwd[1], tg, mul=mul, values=tv, with_init=True)
            for x, r, n in zip((xv, xb, xi), ref, (need[2], need[0], need[1])):
                assert (x.grad is None) == (not n) and (not n or torch.equal(x.grad, r))
    # no input requires a gradient: nothing to differentiate, nothing launched
    del wants[:]
    out = sparse_amd.semiring_matmul_autograd(a, _dev(_cut(b, N)))
    assert not out.requires_grad and wants == []
    # without init and values the function differentiates b alone
    xb = _dev(_cut(b, N)).requires_grad_()
    sparse_amd.semiring_matmul_autograd(a, xb, add="max", mul="times").backward(_dev(_cut(g, N)))
    assert wants == [(False, True, False)]
    assert sr.same_bits(_np(xb.grad), _want("rows", dtype, "max", "times", N, False)[1])

"""The kernels and host code that move data between layouts against the plain NumPy references of tests/layout_cases.py, at
every place where they take another path: the slab merge (`spamd_keys_lead_last`) at its four limits, at the hand-over between
its two table passes and with empty runs; the one-pass broadcast (`spamd_coo_broadcast`) with runs of every length the
galloping search treats differently; the transpose with leading dimensions of its own; the hub-row combine on its own and
the smallest operands that take the hub-row split; indexing with an array index in every combination, and every slice of a
5-element axis; `concatenate` by each of its three routes, compared with each other.  Everything but the floating-point
products moves bits: those comparisons are exact, NaN payloads and the sign of zero included.  Entry points are called
directly with their outputs inside larger buffers of sentinels: nothing outside the output may change."""
import functools

import numpy as np
import pytest
import torch

import layout_cases as lc
from invariants import assert_canonical

pytestmark = pytest.mark.gpu

GUARD = 64
_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
_TSIGNED = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def dev(a):
    """NumPy array -> device tensor with the same bits (unsigned words travel as signed ones)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u":
        a = a.view(_SIGNED[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


def bits(t):
    """the unsigned bit view of a device tensor, on the host"""
    return lc.bits_of(t.cpu().numpy())


class _Guarded:
    """an output of n elements inside a buffer of sentinels"""

    def __init__(self, n, dtype, sentinel=-77):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
        self.out = self.buf[GUARD:GUARD + n]

    def check(self, what=""):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sentinel).all(), f"{what}: written in front of the output"
        assert (b[GUARD + self.n:] == self.sentinel).all(), f"{what}: written behind the output"
        return b[GUARD:GUARD + self.n]

    def untouched(self):
        return bool((self.buf == self.sentinel).all())


def _lib():
    from sparse_amd import _ffi

    return _ffi.lib()


def _stream():
    from sparse_amd._device import stream_ptr

    return stream_ptr(torch.device("cuda", torch.cuda.current_device()))


def _sp():
    import sparse_amd as sp

    return sp


# ---- A. spamd_keys_lead_last ------------------------------------------------------------------------------------------------
def _lead_call(case, val_bytes):
    """-> (return code, failed, out_keys, out_vals as bits, table) with every buffer guarded"""
    keys, S, P, cells = case.keys, case.S, case.P, case.cells
    n = keys.size
    vals = lc.payload_bits(n, val_bytes, seed=n)
    words = S * (-(-P // cells) + 1)
    g_tab, g_keys, g_vals = _Guarded(words, torch.int32), _Guarded(n, torch.int64), _Guarded(n, _TSIGNED[val_bytes])
    failed = torch.full((3,), -77, dtype=torch.int64, device="cuda")
    tk, tv = dev(keys), dev(vals)
    rc = _lib().spamd_keys_lead_last(val_bytes, n, tk.data_ptr(), tv.data_ptr(), S, P, cells, g_tab.out.data_ptr(),
                                     g_keys.out.data_ptr(), g_vals.out.data_ptr(), failed[1:].data_ptr(), _stream())
    torch.cuda.synchronize()
    f = failed.tolist()
    assert f[0] == -77 and f[2] == -77, "written beside the `failed` word"
    assert np.array_equal(tk.cpu().numpy(), keys) and np.array_equal(bits(tv), vals), "an input was changed"
    return rc, f[1], g_keys.check("out_keys"), lc.bits_of(g_vals.check("out_vals")), g_tab.check("bounds"), vals


def test_lead_last_is_the_stable_argsort_of_the_rotated_keys():
    """every case of `layout_cases.LEAD_CASES` (a failure names its case).  Limit 2 (elements per range) comes from
    `spamd_keys_lead_last_limits`; 64 elements per output cell is RL_MAX_PER_CELL of csrc/lead_rotate.hip, which has no getter"""
    for name in lc.LEAD_CASES:
        _check_lead_case(name)


def _check_lead_case(name):
    case = lc.lead_case(name)
    lim = _lib().spamd_keys_lead_last_limits
    assert (lim(0), lim(1), lim(2)) == (lc.RL_MAX_SLABS, lc.RL_MAX_CELLS, lc.RL_CAP)
    predicted = lc.lead_predicts_failed(case.keys, case.S, case.P, case.cells, cap=int(lim(2)), per_cell=64)
    for val_bytes in (4, 8):
        rc, failed, out_keys, out_vals, table, vals = _lead_call(case, val_bytes)
        assert rc == 0, name
        assert (failed != 0) == predicted, f"{name}: failed = {failed}, predicted {predicted}"
        assert np.array_equal(table, lc.lead_table(case.keys, case.S, case.P, case.cells)), f"{name}: the boundary table"
        if failed == 0:
            want_keys, want_vals = lc.ref_lead_last(case.keys, vals, case.S, case.P)
            assert np.array_equal(out_keys, want_keys), f"{name}: keys, {val_bytes}-byte values"
            assert np.array_equal(out_vals, want_vals), f"{name}: {val_bytes}-byte values"


def test_lead_last_declines_arguments_with_the_documented_code():
    for case in lc.LEAD_ERRORS:
        _check_lead_error(*case)
    _check_lead_of_nothing()


def _check_lead_error(what, val_bytes, n, S, P, cells, code):
    keys = dev(np.arange(n, dtype=np.int64))
    vals = dev(np.arange(n, dtype=np.int64))
    g_tab, g_keys, g_vals = _Guarded(4096, torch.int32), _Guarded(n, torch.int64), _Guarded(n, torch.int64)
    failed = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    rc = _lib().spamd_keys_lead_last(val_bytes, n, keys.data_ptr(), vals.data_ptr(), S, P, cells, g_tab.out.data_ptr(),
                                     g_keys.out.data_ptr(), g_vals.out.data_ptr(), failed.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == code, what
    assert g_tab.untouched() and g_keys.untouched() and g_vals.untouched() and failed.item() == -77, what


def _check_lead_of_nothing():
    """n = 0 returns 0 with `failed` zeroed and nothing else written"""
    g_tab, g_keys, g_vals = _Guarded(64, torch.int32), _Guarded(4, torch.int64), _Guarded(4, torch.int64)
    failed = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    rc = _lib().spamd_keys_lead_last(8, 0, g_keys.out.data_ptr(), g_vals.out.data_ptr(), 8, 16, 4, g_tab.out.data_ptr(),
                                     g_keys.out.data_ptr(), g_vals.out.data_ptr(), failed.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and failed.item() == 0
    assert g_tab.untouched() and g_keys.untouched() and g_vals.untouched()


def test_reductions_over_the_leading_axis_at_and_over_the_merge_limits():
    """`x.sum(axis=0)`, `max` and `prod` of the at-limit and over-limit inputs as (S, P) arrays: as NumPy's on the dense form,
    whether the slab merge takes them, refuses them (`failed`: the sort follows) or is not asked"""
    for name in lc.LEAD_PRODUCT_CASES:
        _check_lead_product(name)


def _check_lead_product(name):
    sp = _sp()
    case = lc.lead_case(name)
    s, c = np.divmod(case.keys, case.P)
    rng = np.random.default_rng(5)
    for dtype in (np.float64, np.int32):
        d = np.zeros((case.S, case.P), dtype=dtype)
        # values +-1 and +-2: sums are exact, products are signed powers of two (exact in float64 in any order, infinite in any
        # order once they pass the largest double); integer products wrap around as NumPy's do
        d[s, c] = rng.integers(1, 3, size=s.size)
        if dtype == np.float64:
            d[s, c] *= rng.choice([-1.0, 1.0], size=s.size)
        x = sp.COO.from_numpy(d)
        for op in ("sum", "max", "prod"):
            with np.errstate(over="ignore"):
                want = getattr(d, op)(axis=0)
            got = getattr(x, op)(axis=0)
            assert_canonical(got)
            got = got.todense()
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, op, dtype)


# ---- B. spamd_coo_broadcast -------------------------------------------------------------------------------------------------
def test_broadcast_replicates_every_element_in_sorted_order():
    for name in lc.BCAST_CASES:
        _check_broadcast_case(name)


def _check_broadcast_case(name):
    c = lc.bcast_case(name)
    n = c.keys.size
    n_out = n * c.b0 * c.b1 * c.b2
    tk = dev(c.keys)
    for val_bytes in lc.BCAST_VAL_BYTES:
        vals = lc.payload_bits(n, val_bytes, seed=n)
        tv = dev(vals)
        g_keys, g_vals = _Guarded(n_out, torch.int64), _Guarded(n_out, _TSIGNED[val_bytes])
        rc = _lib().spamd_coo_broadcast(val_bytes, n, tk.data_ptr(), tv.data_ptr(), c.b0, c.k1, c.b1, c.k2, c.b2,
                                        g_keys.out.data_ptr(), g_vals.out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, name
        want_keys, want_vals = lc.ref_broadcast(c.keys, vals, c.b0, c.k1, c.b1, c.k2, c.b2)
        assert np.array_equal(g_keys.check(f"{name}: out_keys"), want_keys), (name, val_bytes)
        assert np.array_equal(lc.bits_of(g_vals.check(f"{name}: out_vals")), want_vals), (name, val_bytes)


def test_broadcast_to_and_an_elementwise_op_on_the_same_inputs():
    for name in lc.BCAST_CASES:
        _check_broadcast_public(name)


def _check_broadcast_public(name):
    sp = _sp()
    from sparse_amd import _broadcast

    c = lc.bcast_case(name)
    d = np.zeros(c.k1 * c.k2, dtype=np.float32)
    d[c.keys] = np.arange(1, c.keys.size + 1)
    d = d.reshape(c.k1, 1, c.k2, 1)
    shape = (c.b0, c.k1, c.b1, c.k2, c.b2)
    x = sp.COO.from_numpy(d)
    before = _broadcast.BROADCAST_STATS.get("fused", 0)
    r = sp.broadcast_to(x, shape)
    if shape != (1,) + d.shape:
        assert _broadcast.BROADCAST_STATS.get("fused", 0) == before + 1, name    # (the kernel under test, not the general route)
    assert_canonical(r)
    assert r.shape == shape and np.array_equal(r.todense(), np.broadcast_to(d, shape)), name
    other = np.zeros(shape, dtype=np.float32)
    other.reshape(-1)[::3] = 2.0
    y = sp.COO.from_numpy(other)
    for got, want in ((x * y, d * other), (x + y, d + other)):
        assert_canonical(got)
        assert got.shape == want.shape and np.array_equal(got.todense(), want), name


# ---- C. spamd_transpose_2d --------------------------------------------------------------------------------------------------
def test_transpose_with_leading_dimensions_writes_the_block_and_nothing_else():
    for rows in lc.TRANSPOSE_EXTENTS:
        for cols in lc.TRANSPOSE_EXTENTS:
            _check_transpose(rows, cols)
    _check_transpose_errors()


def _check_transpose(rows, cols):
    for nbytes in lc.TRANSPOSE_ELEM_BYTES:
        wide, sentinel = lc.transpose_case(rows, cols, nbytes)
        ld_in, ld_out = cols + lc.TRANSPOSE_LD_IN_EXTRA, rows + lc.TRANSPOSE_LD_OUT_EXTRA
        tin = dev(wide)
        sent = int(sentinel.view(_SIGNED[nbytes]))
        g = _Guarded(cols * ld_out, _TSIGNED[nbytes], sentinel=sent)
        rc = _lib().spamd_transpose_2d(nbytes, rows, cols, tin.data_ptr(), ld_in, g.out.data_ptr(), ld_out, _stream())
        torch.cuda.synchronize()
        what = f"{rows} x {cols}, {nbytes}-byte elements"
        assert rc == 0, what
        got = lc.bits_of(g.check(what)).reshape(cols, ld_out)
        want = lc.ref_transpose_into(wide, cols, sentinel)
        assert np.array_equal(got[:, :rows], want[:, :rows]), what
        assert np.array_equal(got, want), f"{what}: written between the rows of the result"
        assert np.array_equal(bits(tin), wide)


def _check_transpose_errors():
    """short leading dimensions are declined, empty extents return 0, and nothing is written"""
    tin = dev(np.arange(64, dtype=np.int32))
    g = _Guarded(64, torch.int32)
    call = functools.partial(_lib().spamd_transpose_2d)
    assert call(4, 4, 8, tin.data_ptr(), 7, g.out.data_ptr(), 4, _stream()) == lc.EINVAL        # ld_in < cols
    assert call(4, 4, 8, tin.data_ptr(), 8, g.out.data_ptr(), 3, _stream()) == lc.EINVAL        # ld_out < rows
    assert call(4, 0, 8, tin.data_ptr(), 8, g.out.data_ptr(), 4, _stream()) == 0
    assert call(4, 4, 0, tin.data_ptr(), 8, g.out.data_ptr(), 4, _stream()) == 0
    assert call(3, 4, 8, tin.data_ptr(), 8, g.out.data_ptr(), 4, _stream()) == lc.ETYPE
    torch.cuda.synchronize()
    assert g.untouched()


# ---- D. hub rows ------------------------------------------------------------------------------------------------------------
_CODES = {"float32": 0, "float64": 1, "int32": 2, "int64": 3}          # include/sparse_amd.h


def _combine(dtype, n_cols, part_wide, vfirst, rows, out_wide):
    """one call on [*, ld] host arrays (their leading n_cols columns are the operands); -> the whole `out` buffer afterwards"""
    tp, to = dev(part_wide), dev(out_wide)
    tf, tr = dev(np.asarray(vfirst, dtype=np.int64)), dev(np.asarray(rows, dtype=np.int64))
    rc = _lib().spamd_hot_rows_combine(_CODES[dtype], len(rows), n_cols, tp.data_ptr(), part_wide.shape[1], tf.data_ptr(), tr.data_ptr(),
                                       to.data_ptr(), out_wide.shape[1], _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(bits(tp), lc.bits_of(part_wide))
    return to.cpu().numpy()


def _wide(a, extra, sentinel):
    w = np.full((a.shape[0], a.shape[1] + extra), sentinel, dtype=a.dtype)
    w[:, :a.shape[1]] = a
    return w


def test_combine_adds_a_hot_rows_pieces_in_piece_order():
    """hot rows of 1, 7, 8, 9, 128 and 129 pieces - and one without pieces, whose row becomes zero - in one call, into rows of
    `out` given out of order, for 1, 255, 256, 257 and 513 columns; bit for bit `acc = T(0); acc = acc + part[v, c]`, integers
    wrapping around"""
    for dtype in lc.COMBINE_DTYPES:
        for n_cols in lc.COMBINE_N_COLS:
            _check_combine(n_cols, dtype)
    _check_combine_errors()


def _check_combine(n_cols, dtype):
    counts = list(lc.COMBINE_PIECES) + [0]
    vfirst = np.concatenate([[0], np.cumsum(counts)])
    rows = np.array([5, 0, 9, 2, 7, 3, 11])
    part = lc.combine_parts(int(vfirst[-1]), n_cols, dtype)
    out0 = lc.combine_parts(13, n_cols, dtype, seed=9)
    e_part, e_out = lc.COMBINE_LD_EXTRA
    sent = np.dtype(dtype).type(-123)
    got = _combine(dtype, n_cols, _wide(part, e_part, sent), vfirst, rows, _wide(out0, e_out, sent))
    want = _wide(lc.ref_combine(part, vfirst, rows, out0), e_out, sent)
    assert np.array_equal(lc.bits_of(got), lc.bits_of(want)), (dtype, n_cols)      # (rows not named, columns behind n_cols included)


def test_combine_in_two_levels_as_the_hub_product_chains_it():
    """rows of 129, 300 and 5 pieces: first every group of at most `fan` pieces into a row of its own (`g1` + identity rows),
    then the groups of each hot row (`vfirst`) - exactly `_hot_product`'s two calls"""
    for dtype in lc.COMBINE_DTYPES:
        _check_two_level_combine(dtype)


def _check_two_level_combine(dtype):
    from sparse_amd import _dot

    fan, n_cols = _dot.HOT_COMBINE_FAN, 257
    counts = [129, 300, 5]
    lens = [32 * c for c in counts]
    p0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    vptr, vfirst, g1 = _dot.hot_piece_plan(p0, p0 + np.asarray(lens))
    assert g1 is not None and len(vptr) - 1 == sum(counts) and vfirst.tolist() == [0, 2, 5, 6]
    part = lc.combine_parts(sum(counts), n_cols, dtype)
    ident = np.arange(len(g1) - 1)
    zero = np.zeros((len(g1) - 1, n_cols), dtype=dtype)
    tmp = _combine(dtype, n_cols, part, g1, ident, zero)
    assert np.array_equal(lc.bits_of(tmp), lc.bits_of(lc.ref_combine(part, g1, ident, zero)))
    rows = np.array([4, 1, 2])
    out0 = lc.combine_parts(6, n_cols, dtype, seed=2)
    got = _combine(dtype, n_cols, tmp, vfirst, rows, out0)
    assert np.array_equal(lc.bits_of(got), lc.bits_of(lc.ref_combine(tmp, vfirst, rows, out0)))


def _check_combine_errors():
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    f = torch.zeros(2, dtype=torch.int64, device="cuda")
    call = _lib().spamd_hot_rows_combine
    assert call(0, 1, 8, t.data_ptr(), 7, f.data_ptr(), f.data_ptr(), t.data_ptr(), 8, _stream()) == lc.EINVAL
    assert call(0, 1, 8, t.data_ptr(), 8, f.data_ptr(), f.data_ptr(), t.data_ptr(), 7, _stream()) == lc.EINVAL
    assert call(4, 1, 8, t.data_ptr(), 8, f.data_ptr(), f.data_ptr(), t.data_ptr(), 8, _stream()) == lc.ETYPE
    assert call(0, 0, 8, t.data_ptr(), 8, f.data_ptr(), f.data_ptr(), t.data_ptr(), 8, _stream()) == 0


@functools.lru_cache(maxsize=None)
def _hub(dtype):
    from sparse_amd import _dot

    indptr, indices, long_rows = lc.hub_matrix(hot_min=_dot.HOT_ROW_MIN, min_nnz=_dot.HOT_ROW_MIN_NNZ)
    data = lc.hub_values(int(indptr[-1]), dtype)
    bs = {}
    for N in (16, 128):
        rng = np.random.default_rng(N)
        bs[N] = (rng.integers(-5, 6, size=(6000, N)) if np.dtype(dtype).kind == "i" else rng.random((6000, N)) - 0.5).astype(dtype)
    refs = {}
    for N, b in bs.items():
        if np.dtype(dtype).kind == "i":
            import scipy.sparse as ss

            refs[N] = (ss.csr_matrix((data, indices, indptr), shape=(len(indptr) - 1, 6000)) @ b, None)
        else:
            refs[N] = lc.hub_bound(indptr, indices, data, b, dtype)
    return indptr, indices, data, long_rows, bs, refs


def _hub_operand(form, dtype):
    import scipy.sparse as ss

    sp = _sp()
    indptr, indices, data = _hub(dtype)[:3]
    host = ss.csr_matrix((data, indices, indptr), shape=(len(indptr) - 1, 6000))
    if form == "csr":
        return sp.GCXS.from_scipy_sparse(host)
    return sp.GCXS.from_scipy_sparse(host.tocsc()) if form == "csc" else sp.COO.from_scipy_sparse(host)


def _hub_check(got, ref, dtype, what):
    want, bound = ref
    got = np.asarray(got)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape, what
    if bound is None:
        assert np.array_equal(got, want), what
    else:
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), f"{what}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}"


def test_the_smallest_hub_rows_are_split_and_combined(monkeypatch):
    """About 600 x 6000 with rows of exactly HOT_ROW_MIN, HOT_ROW_MIN - 1 and 4129 elements: the split names the first and
    the last, cuts them into pieces of 32 (128 and 130 pieces: more than the fan, a two-level combine), and `_hot_product` and
    `a @ b` agree with the float64 product for 16 and 128 columns.  Integers are exact.  Floats are held to
    |got - want| <= (n_r + 2) eps sum_k |a_rk| |b_kj| (n_r the row's stored length, eps = 2u: every stored element costs one
    rounding at most in any summation order, twice that as margin).  What this bound sees: a lost piece of 32 elements of
    magnitude ~0.5 x 0.25 each is ~4 against a bound of ~1e-1 (float32, the longest row) - far outside; a single lost element
    (~0.1) is visible in float64 (bound ~1e-10) and in the integer runs, not in float32.  That is why the combine itself is
    tested bit for bit above.  Without the split (`HOT_ROW_SPLIT = False`) the results are within the same bound."""
    for dtype in (np.float32, np.float64, np.int64):
        for form in ("csr", "csc", "coo"):
            with monkeypatch.context() as patch:
                _check_hub(dtype, form, patch)


def _check_hub(dtype, form, monkeypatch):
    from sparse_amd import _dot

    indptr, indices, data, long_rows, bs, refs = _hub(np.dtype(dtype).name)
    hot = sorted(r for r, n in long_rows.items() if n >= _dot.HOT_ROW_MIN)
    assert len(hot) == 2
    a = _hub_operand(form, np.dtype(dtype).name)
    calls = []
    real = _dot._hot_product
    monkeypatch.setattr(_dot, "_hot_product", lambda *args: (calls.append(1), real(*args))[1])
    for N, b in bs.items():
        _hub_check(a @ b, refs[N], dtype, f"a @ b, N = {N}")
    split = a.__dict__.get("_hot_split")
    if form == "csr":
        assert len(calls) == len(bs), "the hub-row route was not taken"
    if form != "csc" or split is not None:       # (a CSC operand may go through its own inspector, which needs no CSR twin)
        assert split is not None
    if split is None:
        split = _dot._hot_row_split(a, *_dot._csr_triplet(a))
    light, hotv, vfirst, rows, mid, longest = split
    assert sorted(rows.tolist()) == hot and longest == 4129
    assert mid is not None and light.nnz + hotv.nnz == a.nnz and light.shape == a.shape
    assert hotv.shape[0] == 128 + 130 and vfirst.tolist() == [0, 1, 3]
    for N, b in bs.items():
        got = real(split, torch.from_numpy(b).cuda(), (a.shape[0], N))
        _hub_check(got.cpu().numpy(), refs[N], dtype, f"_hot_product, N = {N}")
    monkeypatch.setattr(_dot, "HOT_ROW_SPLIT", False)
    plain = _hub_operand(form, np.dtype(dtype).name)
    n_before = len(calls)
    for N, b in bs.items():
        _hub_check(plain @ b, refs[N], dtype, f"unsplit a @ b, N = {N}")
    assert len(calls) == n_before and plain.__dict__.get("_hot_split") is None


# ---- E. indexing ------------------------------------------------------------------------------------------------------------
_FORMS = ("coo int32", "coo int64", "gcxs (0,)", "gcxs (1,)", "gcxs (0, 1)", "coo int64 fill 2")


def _as_form(d, form):
    sp = _sp()
    if form.startswith("coo"):
        x = sp.COO.from_numpy(d, idx_dtype=np.int32 if "int32" in form else np.int64)
        return x + 2 if "fill 2" in form else x
    ca = tuple(int(c) for c in form[form.index("(") + 1:form.index(")")].split(",") if c.strip())
    return sp.GCXS.from_numpy(d, compressed_axes=ca)


def _real_index(index):
    """the index expression with every `Arr` as its kind says (a torch tensor included)"""
    def one(i):
        if isinstance(i, lc.Arr):
            if i.kind == "list":
                return list(i.values)
            if i.kind == "tensor":
                return torch.tensor(i.values, dtype=torch.int64)
            return np.asarray(i.values, dtype=bool if i.kind == "bool" else np.int32)
        return i
    return tuple(one(i) for i in index)


def _check_indexed(x, d, index, want, fill, what):
    got = x[index]
    if want.ndim == 0:
        assert np.asarray(got).shape == () and got == want, what
        return
    assert isinstance(got, type(x)), f"{what}: {type(x).__name__} became {type(got).__name__}"
    assert_canonical(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, NumPy's {want.shape}"
    assert got.dtype == want.dtype and got.fill_value == fill
    assert np.array_equal(got.todense(), want), what
    if fill == 0:
        assert got.nnz == np.count_nonzero(want), what


def test_an_array_index_alone_and_combined_is_numpys():
    """NumPy on the dense array is the reference.  In one family NumPy's placement of the result's axes is not the library's:
    an integer BEFORE the array with a slice between them (`x[2, :, [5, 5, 1]]`) sends the array's axis to the front in NumPy;
    the library keeps it in the array's place, as the reference it is modelled on does and as the golden case "index with an
    integer and an array" pins it.  `layout_cases.index_expected` is NumPy's result with that one axis put back
    (22 of the 396 expressions), and tests/test_layout_cases.py checks it against an axis-by-axis evaluation."""
    for form in _FORMS:
        _check_index_form(form)
    _check_index_errors()


def _check_index_form(form):
    d = lc.index_dense()
    x = _as_form(d, form)
    fill = 2 if "fill 2" in form else 0
    dd = d + fill
    assert type(x).__name__ == ("COO" if form.startswith("coo") else "GCXS") and np.array_equal(x.todense(), dd)
    n = 0
    for name, index in lc.index_cases().items():
        _check_indexed(x, dd, _real_index(index), lc.index_expected(dd, index), fill, f"{form}: {name}")
        n += 1
    assert n == 3 * 11 * (1 + 2 * 4 + 3)


def _check_index_errors():
    """two array indices, an element out of range, a mask of the wrong length ...: what `_indexing.py` documents"""
    d = lc.index_dense()
    for form in ("coo int64", "gcxs (1,)"):
        x = _as_form(d, form)
        with pytest.raises(NotImplementedError, match="several array indices"):
            x[[0, 1], [1, 2]]
        with pytest.raises(NotImplementedError, match="several array indices"):
            x[[0, 1], :, np.array([True] * 7)]
        with pytest.raises(IndexError, match="index 5 is out of bounds for axis 0 with size 5"):
            x[[0, 5]]
        with pytest.raises(IndexError, match="index -7 is out of bounds for axis 1 with size 6"):
            x[:, [1, -7]]
        with pytest.raises(IndexError, match="boolean index did not match indexed array along axis 2; size of axis is 7"):
            x[:, :, np.array([True] * 6)]
        with pytest.raises(NotImplementedError, match="1-D array indices"):
            x[np.zeros((2, 2), dtype=np.int64)]
        with pytest.raises(IndexError, match="must be of integer"):
            x[np.array([0.5, 1.0])]
        with pytest.raises(IndexError, match="too many indices"):
            x[0, 0, 0, [0]]


def test_every_slice_of_a_five_element_axis_is_numpys():
    for step in lc.SLICE_STEPS:
        _check_slices(step)


def _check_slices(step):
    sp = _sp()
    d1, d2 = lc.SLICE_DENSE_1D, lc.SLICE_DENSE_2D
    x1 = sp.COO.from_numpy(d1)
    x2 = sp.GCXS.from_numpy(d2, compressed_axes=(0,))
    x2c = sp.GCXS.from_numpy(d2, compressed_axes=(1,))
    x3 = sp.COO.from_numpy(d2)
    n = 0
    for start in lc.SLICE_POINTS:
        for stop in lc.SLICE_POINTS:
            s = slice(start, stop, step)
            # (the 1-D COO and the rows of the 2-D GCXS at every step; the column-compressed and the 2-D COO forms at +-1)
            for x, d in ((x1, d1), (x2, d2)) if abs(step) > 1 else ((x1, d1), (x2, d2), (x2c, d2), (x3, d2)):
                got, want = x[s], d[s]
                assert isinstance(got, type(x)) and got.shape == want.shape, (s, type(x).__name__)
                assert np.array_equal(got.todense(), want), (s, type(x).__name__, getattr(x, "compressed_axes", None))
                assert got.nnz == np.count_nonzero(want)
            n += 1
    assert n == 14 * 14
    for s in (slice(None, None, step), slice(4, None, step), slice(1, -1, step), slice(-1, 0, step)):
        for x in (x1, x2, x2c, x3):
            assert_canonical(x[s])


# ---- F. joins ---------------------------------------------------------------------------------------------------------------
def _operand(op, fmt="coo", ca=None, fill=0):
    sp = _sp()
    d = lc.operand_dense(op, fill=fill)
    idt = np.int32 if op.idx == "int32" else np.int64
    if fmt == "coo":
        return sp.COO.from_numpy(d, idx_dtype=idt, fill_value=fill), d
    return sp.GCXS.from_numpy(d, compressed_axes=ca, idx_dtype=idt, fill_value=fill), d


def _host_form(r):
    """what a result is made of, on the host: coordinates (their width included), values as bits, fill value"""
    sp = _sp()
    if isinstance(r, sp.COO):
        return ("coo", r.shape, str(r._index_dtype), r.coords.cpu().numpy(), bits(r.data), str(r.dtype), np.asarray(r.fill_value).tobytes())
    return ("gcxs", r.shape, r.compressed_axes, str(r.indices.dtype), r.indices.cpu().numpy(), str(r.indptr.dtype), r.indptr.cpu().numpy(),
            bits(r.data), str(r.dtype), np.asarray(r.fill_value).tobytes())


def _same_form(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))


class _Spy:
    """counts the calls of `_umath.union_merge` and `_kernels.sort_keys`"""

    def __init__(self, monkeypatch):
        from sparse_amd import _kernels, _umath

        self.merges = self.sorts = 0
        real_merge, real_sort = _umath.union_merge, _kernels.sort_keys

        def merge(*a, **k):
            self.merges += 1
            return real_merge(*a, **k)

        def sort(*a, **k):
            self.sorts += 1
            return real_sort(*a, **k)

        monkeypatch.setattr(_umath, "union_merge", merge)
        monkeypatch.setattr(_kernels, "sort_keys", sort)

    def reset(self):
        self.merges = self.sorts = 0


_JOIN_CASES = lc.join_cases()


def test_concatenate_by_the_route_its_case_names_and_as_the_sort_route(monkeypatch):
    """every case of `layout_cases.join_cases()` (a failure names its case)"""
    for case in _JOIN_CASES:
        with monkeypatch.context() as patch:
            _check_join(case, patch)
    with monkeypatch.context() as patch:
        _check_join_with_a_fill_value(patch)
    _check_join_refuses_a_promotion_the_device_cannot_convert()


def _check_join(case, monkeypatch):
    sp = _sp()
    from sparse_amd import _batched

    pairs = [_operand(o) for o in case.operands]
    xs, ds = [p[0] for p in pairs], [p[1] for p in pairs]
    want = np.concatenate(ds, axis=case.axis)
    spy = _Spy(monkeypatch)
    got = sp.concatenate(xs, axis=case.axis)
    nonempty = sum(1 for x in xs if x.nnz)
    if case.route == "merge":
        assert (spy.merges, spy.sorts) == (nonempty - 1, 0), f"{case.name}: not the merge route"
    elif case.route == "sort":
        assert spy.merges == 0, case.name
        assert (spy.sorts >= 1) == lc.concat_keys_unsorted(case.operands, case.axis % want.ndim), f"{case.name}: not the sort route"
    else:
        assert (spy.merges, spy.sorts) == (0, 0), f"{case.name}: joined along axis 0, the operands one after the other"
    assert_canonical(got)
    assert isinstance(got, sp.COO) and got.shape == want.shape and got.dtype == want.dtype, case.name
    assert np.array_equal(got.todense(), want) and got.nnz == np.count_nonzero(want), case.name
    want_idx = torch.int64 if any(o.idx == "int64" for o in case.operands) else torch.int32
    assert got._index_dtype == want_idx, case.name
    spy.reset()
    monkeypatch.setattr(_batched, "CONCAT_MERGE", False)
    by_sort = sp.concatenate(xs, axis=case.axis)
    assert spy.merges == 0, case.name
    assert _same_form(_host_form(got), _host_form(by_sort)), f"{case.name}: the routes disagree"


def _check_join_with_a_fill_value(monkeypatch):
    sp = _sp()
    from sparse_amd import _batched

    ops = lc._ops(3, (3, 4, 5), "float64", 1, idxs=("int32", "int64"))
    pairs = [_operand(o, fill=2) for o in ops]
    want = np.concatenate([p[1] for p in pairs], axis=1)
    got = sp.concatenate([p[0] for p in pairs], axis=1)
    assert_canonical(got)
    assert got.fill_value == 2 and np.array_equal(got.todense(), want)
    monkeypatch.setattr(_batched, "CONCAT_MERGE", False)
    assert _same_form(_host_form(got), _host_form(sp.concatenate([p[0] for p in pairs], axis=1)))
    with pytest.raises(ValueError, match="consistent fill-values"):
        sp.concatenate([pairs[0][0], _operand(ops[1])[0]], axis=1)


def _check_join_refuses_a_promotion_the_device_cannot_convert():
    """int8 and int16 values are stored and moved, but `_kernels.convert` has no conversion from them: a join that needs one
    says so instead of computing on the host"""
    sp = _sp()
    ops = lc._ops(2, (3, 4, 5), None, 1, dtypes=("int8", "float32"))
    assert all(o.dtype in lc.CONVERTIBLE for o in ops) is False
    with pytest.raises(TypeError, match="cannot convert"):
        sp.concatenate([_operand(o)[0] for o in ops], axis=1)


_GCXS_CASES = lc.gcxs_join_cases()


def test_concatenate_of_compressed_operands_by_pointers_and_by_the_general_route(monkeypatch):
    """every case of `layout_cases.gcxs_join_cases()` (a failure names its case)"""
    for case in _GCXS_CASES:
        with monkeypatch.context() as patch:
            _check_gcxs_join(*case, patch)


def _check_gcxs_join(name, ops, ca, axis, asked, fast, monkeypatch):
    sp = _sp()
    from sparse_amd import _batched

    pairs = [_operand(o, "gcxs", (ca,)) for o in ops]
    xs, ds = [p[0] for p in pairs], [p[1] for p in pairs]
    want = np.concatenate(ds, axis=axis)
    taken = []
    real = _batched._concatenate_compressed
    monkeypatch.setattr(_batched, "_concatenate_compressed", lambda *a: (taken.append(real(*a)), taken[-1])[1])
    got = sp.concatenate(xs, axis=axis, compressed_axes=asked)
    assert (taken[-1] is not None) == fast, f"{name}: not the route the case names"
    assert_canonical(got)
    assert isinstance(got, sp.GCXS) and got.compressed_axes == ((axis % 2,) if asked is None else tuple(asked)), name
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.todense(), want), name
    assert got.nnz == np.count_nonzero(want), name
    monkeypatch.setattr(_batched, "_concatenate_compressed", lambda *a: None)
    general = sp.concatenate(xs, axis=axis, compressed_axes=asked)
    assert_canonical(general)
    a, b = _host_form(got), _host_form(general)
    # (the general route builds its pointers anew, in the width the result needs; the pointer route keeps int64 where an operand
    # has it: the structure and the values must agree, widths compared after widening)
    assert a[:3] == b[:3] and a[8:] == b[8:], name
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[6], b[6]) and np.array_equal(a[7], b[7]), name
    monkeypatch.setattr(_batched, "CONCAT_MERGE", False)
    by_sort = sp.concatenate(xs, axis=axis, compressed_axes=asked)
    assert _same_form(_host_form(general), _host_form(by_sort)), f"{name}: the general route's merge and sort disagree"


def test_stack_along_every_axis_is_numpys():
    for fmt in ("coo", "gcxs"):
        for shape in lc.STACK_SHAPES:
            _check_stack(fmt, shape)


def _check_stack(fmt, shape):
    sp = _sp()
    nd = len(shape)
    ops = lc._ops(3, shape, "float64", 0, idxs=("int32", "int64"))
    pairs = [_operand(o, fmt, None if fmt == "coo" or nd == 1 else (0,)) for o in ops]
    xs, ds = [p[0] for p in pairs], [p[1] for p in pairs]
    for axis in range(-(nd + 1), nd + 1):
        want = np.stack(ds, axis=axis)
        got = sp.stack(xs, axis=axis)
        assert_canonical(got)
        assert got.shape == want.shape and got.dtype == want.dtype, axis
        assert np.array_equal(got.todense(), want) and got.nnz == np.count_nonzero(want), axis
        assert isinstance(got, sp.GCXS if fmt == "gcxs" and nd > 1 else sp.COO), axis

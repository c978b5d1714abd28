"""sparse_amd.sparse_attention_grad and sparse_attention_autograd on the device (csrc/attention_grad.hip).

Yardsticks, all from tests/attention_grad_cases.py:
  * `grad_restated` - the order contract of include/sparse_amd.h A16 written in NumPy - in the result type, BIT FOR BIT (any NaN
    equals any NaN: a payload is no result);
  * every kernel form, sub-group width and chunk against every other, bit for bit, for the lengths it accepts, for the row pass
    (row lengths) and the column pass (column lengths);
  * `sparse_amd.softmax` on the restated scores: with g = the identity, dv holds the probabilities of two independently written
    kernels, bit for bit;
  * torch.autograd.gradcheck at torch's own default tolerances."""
import functools

import numpy as np
import pytest
import torch

import attention_cases as ac
import attention_grad_cases as gc
import softmax_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNKS = (64, 128, None)          # None: the default, `_kernels.ATTENTION_CHUNK`


def _chunk(monkeypatch, chunk):
    from sparse_amd import _kernels as K

    if chunk is not None:
        monkeypatch.setattr(K, "ATTENTION_CHUNK", chunk)
    return K.ATTENTION_CHUNK


def _coo(indptr, indices, vals, shape, idx=None, **kw):
    import sparse_amd

    kw = dict(dict(has_duplicates=False, sorted=True), **kw)
    return sparse_amd.COO(ac.coords_of(indptr, indices), vals, shape=shape, idx_dtype=idx, device=DEV, **kw)


def _csr(indptr, indices, vals, shape):
    import sparse_amd

    return sparse_amd.GCXS((vals, indices, indptr), shape=shape, compressed_axes=(0,), device=DEV)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _dev(*xs):
    return tuple(torch.from_numpy(x).to(DEV) for x in xs)


def _same(got, want):
    return len(got) == 3 and all(sc.same_bits(_np(a), b) for a, b in zip(got, want))


@pytest.fixture
def spy(monkeypatch):
    """records the CSR triple every `attention_grad_rows` call was given"""
    from sparse_amd import _kernels as K

    seen = []
    real = K.attention_grad_rows

    def wrapped(indptr, indices, svals, *a, **kw):
        seen.append((indptr, indices, svals))
        return real(indptr, indices, svals, *a, **kw)

    monkeypatch.setattr(K, "attention_grad_rows", wrapped)
    return seen


# ---- row and column lengths, layouts -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lengths_case(chunk, dtype, columns):
    """the listed lengths as the ROW lengths of one mask, or (`columns`) as its COLUMN lengths; D = 17, Dv = 5, a scale; the
    restated gradient, computed once per chunk and type"""
    make = gc.transposed_mask if columns else ac.csr_mask
    indptr, indices, vals, shape = make(40 + chunk, sc.listed_lengths(chunk), dtype)
    q, k, v = ac.operands(41 + chunk, shape, 17, 5, dtype)
    g = gc.grad_operand(42 + chunk, shape, 5, dtype)
    want = gc.grad_restated(indptr, indices, vals, q, k, v, g, chunk, 0.3)[:3]
    for a in (indptr, indices, vals, q, k, v, g) + want:
        a.setflags(write=False)
    return indptr, indices, vals, shape, q, k, v, g, want


@pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_listed_lengths_bit_for_bit_in_every_layout(dtype, idx, chunk, columns, monkeypatch, spy):
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    indptr, indices, vals, shape, q, k, v, g, want = _lengths_case(chunk, np.dtype(dtype), columns)
    tidx = torch.int32 if np.dtype(idx) == np.int32 else torch.int64
    ptr_i, ind_i = indptr.astype(idx), indices.astype(idx)

    def same_csr(triple):
        """the triple the kernel read is the canonical CSR order the reference was restated on"""
        return (np.array_equal(_np(triple[0]), indptr) and np.array_equal(_np(triple[1]), indices)
                and np.array_equal(_np(triple[2]), vals))

    # a canonical COO
    coo = _coo(ptr_i, ind_i, vals, shape, idx)
    got = sparse_amd.sparse_attention_grad(coo, q, k, v, g, scale=0.3)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype) for a in got)
    assert [a.shape for a in got] == [(shape[0], 17), (shape[1], 17), (shape[1], 5)]
    assert _same(got, want) and same_csr(spy[-1]) and spy[-1][0].dtype == tidx
    # a row-compressed GCXS: its own arrays, untouched, at its own index width
    x = _csr(ptr_i, ind_i, vals, shape)
    got = sparse_amd.sparse_attention_grad(x, q, k, v, g, scale=0.3)
    assert spy[-1][0] is x.indptr and spy[-1][1] is x.indices and spy[-1][2] is x.data and x.indptr.dtype == tidx
    assert _same(got, want)
    # a column-compressed GCXS: the memoised CSR twin (stable, so the CSR order is the canonical one)
    xc = coo.asformat("gcxs", compressed_axes=(1,))
    got = sparse_amd.sparse_attention_grad(xc, q, k, v, g, scale=0.3)
    assert same_csr(spy[-1]) and spy[-1][0] is not xc.indptr and _same(got, want)
    # a COO built unsorted
    perm = np.random.default_rng(5).permutation(len(indices))
    coords = ac.coords_of(indptr, indices)[:, perm].astype(idx)
    un = sparse_amd.COO(coords, vals[perm], shape=shape, idx_dtype=idx, device=DEV)
    got = sparse_amd.sparse_attention_grad(un, q, k, v, g, scale=0.3)
    assert same_csr(spy[-1]) and _same(got, want)


# ---- widths ---------------------------------------------------------------------------------------------------------------------------
DS = [1, 3, 16, 17, 63, 64, 65, 128, 130]
DVS = [1, 5, 63, 64, 65, 130]
WIDTH_PAIRS = sorted({(D, DVS[(i + j) % 6]) for i, D in enumerate(DS) for j in (0, 3)} |
                     {(DS[(i + j) % 9], Dv) for i, Dv in enumerate(DVS) for j in (2, 6)})


@pytest.mark.parametrize("D,Dv", WIDTH_PAIRS)
def test_widths(D, Dv):
    """every D with at least two Dv and the reverse, float32 and float64, on rows of 0, 1, 2, 7, 8, 9, 33, 64, 65 and 100"""
    import sparse_amd

    for dtype in (np.float32, np.float64):
        indptr, indices, vals, shape = ac.csr_mask(50, ac.SHORT_LENGTHS, dtype)
        q, k, v = ac.operands(51 + D, shape, D, Dv, dtype)
        g = gc.grad_operand(52 + Dv, shape, Dv, dtype)
        got = sparse_amd.sparse_attention_grad(_coo(indptr, indices, vals, shape), q, k, v, g)
        assert _same(got, gc.grad_restated(indptr, indices, vals, q, k, v, g, 1024)[:3]), dtype


# ---- heads ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (1,), (3,), (2, 2)])
def test_heads_share_one_mask(lead):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(60, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(61, shape, 20, 9, np.float32, lead=lead)
    g = gc.grad_operand(62, shape, 9, np.float32, lead=lead)
    s = _coo(indptr, indices, vals, shape)
    got = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=0.5)
    assert [a.shape for a in got] == [lead + (shape[0], 20), lead + (shape[1], 20), lead + (shape[1], 9)]
    assert _same(got, gc.grad_heads(indptr, indices, vals, q, k, v, g, 1024, 0.5))
    for h in np.ndindex(*lead):
        assert _same(sparse_amd.sparse_attention_grad(s, q[h], k[h], v[h], g[h], scale=0.5), [a[h] for a in got])
    tout = sparse_amd.sparse_attention_grad(s, *_dev(q, k, v, g), scale=0.5)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tout) and _same(tout, got)


# ---- strides --------------------------------------------------------------------------------------------------------------------------
def test_strided_operands_and_a_sliced_grad():
    """row-strided views (a slice of a wider tensor: read in place), a transposed last axis (the one copy), a `grad` that is a
    non-contiguous slice, torch and NumPy"""
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(70, ac.SHORT_LENGTHS, np.float32)
    M, N = shape
    D, Dv, lead = 19, 7, (2,)
    q, k, v = ac.operands(71, shape, D, Dv, np.float32, lead=lead)
    g = gc.grad_operand(72, shape, Dv, np.float32, lead=lead)
    s = _coo(indptr, indices, vals, shape)
    want = sparse_amd.sparse_attention_grad(s, q, k, v, g)
    assert _same(want, gc.grad_heads(indptr, indices, vals, q, k, v, g, 1024))

    def wide(x):                       # a slice of a wider tensor: the row pitch exceeds the width
        w = torch.zeros(x.shape[:-1] + (x.shape[-1] + 9,), device=DEV)
        w[..., 4:4 + x.shape[-1]] = torch.from_numpy(x).to(DEV)
        return w[..., 4:4 + x.shape[-1]]

    def turned(x):                     # the last axis strided: a transposed buffer
        return torch.from_numpy(x).to(DEV).transpose(-1, -2).contiguous().transpose(-1, -2)

    for make in (wide, turned):
        tq, tk, tv, tg = make(q), make(k), make(v), make(g)
        assert not tg.is_contiguous()
        got = sparse_amd.sparse_attention_grad(s, tq, tk, tv, tg)
        assert all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in got) and _same(got, want)
    big = np.zeros((2, 2 * M, Dv + 3), np.float32)
    big[:, ::2, 1:1 + Dv] = g
    got = sparse_amd.sparse_attention_grad(s, q, np.asfortranarray(k), v, big[:, ::2, 1:1 + Dv])       # every second row of a wider array
    assert all(isinstance(a, np.ndarray) for a in got) and _same(got, want)
    mixed = sparse_amd.sparse_attention_grad(s, q, k, v, torch.from_numpy(g).to(DEV))                    # any torch operand: tensors out
    assert all(isinstance(t, torch.Tensor) for t in mixed) and _same(mixed, want)


# ---- every form against every other ------------------------------------------------------------------------------------------------
def _plan_np(indptr, indices, N):
    perm, rows, cols = gc.column_order(indptr, indices)
    return np.searchsorted(cols, np.arange(N + 1)), perm, rows


@pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_groups_and_chunks_change_no_bit(dtype, idx, columns):
    """`idx`: the width of the pointers and indices the kernels read; `columns`: the lengths are the column lengths"""
    from sparse_amd import _kernels as K

    make = gc.transposed_mask if columns else ac.csr_mask

    def runs(lengths, seed, variants, lead=(2,)):
        indptr, indices, vals, shape = make(seed, lengths, dtype)
        q, k, v = ac.operands(seed + 1, shape, 21, 6, dtype, lead=lead)
        g = gc.grad_operand(seed + 2, shape, 6, dtype, lead=lead)
        cptr, cperm, crow = _plan_np(indptr, indices, shape[1])
        ti = lambda a, t=idx: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(t)      # noqa: E731
        args = (ti(indptr), ti(indices), torch.from_numpy(vals).to(DEV), ti(cptr), ti(cperm, torch.int64), ti(crow)) + _dev(q, k, v, g)
        max_row, max_col = int(np.diff(indptr).max()), int(np.diff(cptr).max())
        outs = {str(kw): [_np(t) for t in K.attention_grad_rows(*args, max_row, max_col, scale=0.7, **kw)] for kw in variants}
        first = next(iter(outs.values()))
        assert all(_same(o, first) for o in outs.values()), [name for name, o in outs.items() if not _same(o, first)]
        return (indptr, indices, vals, q, k, v, g), first

    widths = [dict(group=a, col_group=b) for a, b in zip(K.ATTENTION_GROUPS, K.ATTENTION_GROUPS[::-1])]
    # lengths every form accepts (the other axis of these masks is short too: every row and column has at most 64 elements)
    short = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 5]
    variants = [dict(form="short", **w) for w in widths] + [dict(form="wide", chunk=c) for c in (64, 1024)]
    variants += [dict(form="long"), dict(), dict(group=8, col_group=8), dict(group=64, col_group=64, chunk=128), dict(short_max=16),
                 dict(short_max=0, group=32, col_group=32)]
    case, got = runs(short, 71, variants)
    assert _same(got, gc.grad_heads(*case, 64, 0.7))
    # up to 128: a wave each at chunks 128 and 1024, the default split at 64 with every width, the piece form at 128
    mid = short + [65, 100, 127, 128]
    variants = [dict(form="wide", chunk=c) for c in (128, 1024)] + [dict(chunk=c, **w) for w in widths for c in (128, 256)]
    variants += [dict(form="long", chunk=128)]
    runs(mid, 72, variants)
    # pieces (chunk is part of the order here, so one chunk at a time): the piece form against the default split, every width
    long_ = mid + [129, 191, 192, 193, 64 * 5, 700]
    for chunk in (64, 128):
        variants = [dict(form="long", chunk=chunk)] + [dict(chunk=chunk, **w) for w in widths]
        case, got = runs(long_, 73, variants, lead=())
        assert _same(got, gc.grad_heads(*case, chunk, 0.7))


def test_forced_forms_refuse_longer_rows_and_columns():
    from sparse_amd import _kernels as K

    for columns in (False, True):
        indptr, indices, vals, shape = (gc.transposed_mask if columns else ac.csr_mask)(74, [65, 1], np.float32)
        cptr, cperm, crow = _plan_np(indptr, indices, shape[1])
        ti = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                   # noqa: E731
        args = (ti(indptr), ti(indices), ti(vals), ti(cptr), ti(cperm), ti(crow)) + tuple(
            torch.zeros(n, 4, device=DEV) for n in (shape[0], shape[1], shape[1], shape[0]))
        lens = (int(np.diff(indptr).max()), int(np.diff(cptr).max()))
        assert max(lens) == 65
        with pytest.raises(ValueError, match="short"):
            K.attention_grad_rows(*args, *lens, form="short")
        with pytest.raises(ValueError, match="wide"):
            K.attention_grad_rows(*args, *lens, form="wide", chunk=64)


# ---- the probabilities of two kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dv_of_the_identity_equals_softmax_of_the_restated_scores(dtype, monkeypatch):
    """g = the identity (Dv = M): dv[c, r] = fma(p(r, c), 1, +0) and every other term adds a zero, so the backward kernels hand
    out their recomputed probabilities themselves - they equal `sparse_amd.softmax` of a COO of the restated scores, and the
    forward's restated p"""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    monkeypatch.setattr(K, "SOFTMAX_CHUNK", 64)
    lengths = [0, 1, 5, 33, 64, 65, 128, 200, 3]
    indptr, indices, vals, shape = ac.csr_mask(80, lengths, dtype)
    q, k, _ = ac.operands(81, shape, 24, 1, dtype)
    v = gc.grad_operand(82, (shape[1], 0), shape[0], dtype)
    eye = np.eye(shape[0], dtype=dtype)
    _, t, p = ac.attention_restated(indptr, indices, vals, q, k, v, 64, 0.6)
    dq, dk, dv = sparse_amd.sparse_attention_grad(_coo(indptr, indices, vals, shape), q, k, v, eye, scale=0.6)
    rows, cols = ac.coords_of(indptr, indices)
    sm = sparse_amd.softmax(_coo(indptr, indices, t, shape), 1)
    assert sc.same_bits(_np(sm.data), p) and sc.same_bits(dv[cols, rows], _np(sm.data))
    assert np.count_nonzero(dv) <= len(p)


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def test_stored_zeros_take_part():
    """a stored zero of the mask is the score 0 and has a probability; its y is s * z = 0, so it adds nothing to dq and dk, but
    its probability reaches dv"""
    import sparse_amd

    indptr, indices = np.array([0, 2, 3]), np.array([1, 3, 0])
    q, k, v = ac.operands(95, (2, 4), 8, 3, np.float32)
    g = gc.grad_operand(96, (2, 4), 3, np.float32)
    vals = np.array([0.0, 1.5, 1.0], np.float32)
    s = _coo(indptr, indices, vals, (2, 4))
    assert s.nnz == 3
    got = sparse_amd.sparse_attention_grad(s, q, k, v, g)
    want = gc.grad_restated(indptr, indices, vals, q, k, v, g, 1024)
    assert _same(got, want[:3]) and 0 < want[3][0] < 1 and want[4][0] == 0
    assert got[2][1].any() and not got[1][1].any() and not got[1][2].any() and not got[2][2].any()


def test_empty_mask_rows_and_columns():
    import sparse_amd
    from sparse_amd import _ffi

    q, k, v = ac.operands(100, (6, 9), 5, 4, np.float64, lead=(2,))
    g = gc.grad_operand(101, (6, 9), 4, np.float64, lead=(2,))
    empty = sparse_amd.COO(np.zeros((2, 0), np.int64), np.zeros(0, np.float32), shape=(6, 9), device=DEV)
    c0 = _ffi.CALLS
    outs = sparse_amd.sparse_attention_grad(empty, q, k, v, g)
    assert _ffi.CALLS == c0 and [a.shape for a in outs] == [(2, 6, 5), (2, 9, 5), (2, 9, 4)]
    assert all(a.dtype == np.float64 and not a.any() and not np.signbit(a).any() for a in outs)
    touts = sparse_amd.sparse_attention_grad(empty, *_dev(q, k, v, g))
    assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.any() for t in touts)
    none = sparse_amd.sparse_attention_grad(empty, q[:0], k[:0], v[:0], g[:0])
    assert [a.shape for a in none] == [(0, 6, 5), (0, 9, 5), (0, 9, 4)]
    indptr, indices, vals, shape = ac.csr_mask(102, [0, 0, 3, 70, 0, 1100, 2, 0], np.float64, ncols=1200)   # empty rows and columns
    q, k, v = ac.operands(103, shape, 5, 4, np.float64)
    g = gc.grad_operand(104, shape, 4, np.float64)
    got = sparse_amd.sparse_attention_grad(_coo(indptr, indices, vals, shape), q, k, v, g)
    assert _same(got, gc.grad_restated(indptr, indices, vals, q, k, v, g, 1024)[:3])
    unused = np.setdiff1d(np.arange(1200), indices)
    assert len(unused) and not got[0][[0, 1, 4, 7]].any() and not np.signbit(got[0][[0, 1, 4, 7]]).any()
    assert not got[1][unused].any() and not got[2][unused].any() and not np.signbit(got[1][unused]).any() and not np.signbit(got[2][unused]).any()
    assert all(np.isfinite(a).all() for a in got)


@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype, chunk, monkeypatch):
    """a NaN, a +inf score, nothing but -inf scores, -inf beside finite scores, at row lengths of every form; with a positive
    and a negative scale; and a NaN and an infinity in g.  The infinities enter through the mask values, with the sign that
    gives the score its sign"""
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    inf = np.inf
    lengths = [6, 40, 130, 2 * chunk + 9] * 4 + [5, 7, 7]
    indptr, indices, vals, shape = ac.csr_mask(120, lengths, dtype)
    q, k, v = ac.operands(121, shape, 10, 6, dtype)
    g = gc.grad_operand(122, shape, 6, dtype)
    g[17, 2], g[18, 0] = np.nan, inf
    w = np.sign(np.concatenate([ac.dot64(q[r], k[indices[indptr[r]:indptr[r + 1]]]) for r in range(shape[0])])).astype(dtype)
    assert (w != 0).all()
    for j in range(4):
        b, n = indptr[j], lengths[j]
        vals[b + n // 2] = np.nan                                           # rows 0-3: one NaN
        b = indptr[4 + j]
        vals[b + n - 1] = inf * w[b + n - 1]                                # rows 4-7: one score of +inf
        b = indptr[8 + j]
        vals[b:b + n] = -inf * w[b:b + n]                                   # rows 8-11: nothing but -inf
        b = indptr[12 + j]
        vals[b + 1:b + n:3] = -inf * w[b + 1:b + n:3]                       # rows 12-15: -inf beside finite scores
    s = _coo(indptr, indices, vals, shape)
    for scale in (0.5, -0.75):
        got = sparse_amd.sparse_attention_grad(s, q, k, v, g, scale=scale)
        want = gc.grad_restated(indptr, indices, vals, q, k, v, g, chunk, scale)[:3]
        assert _same(got, want)
        assert np.isnan(got[0][:4]).all() and np.isfinite(got[0][16]).all() and np.isnan(got[0][17]).all()
        touched = np.zeros(shape[1], bool)
        touched[indices[indptr[0]:indptr[1]]] = True                        # the columns of the NaN row 0 take its NaN
        assert np.isnan(got[2][touched]).all() and np.isnan(got[1][touched]).all()


def test_gradients_near_the_underflow_threshold():
    """float64 rows of two elements whose probabilities are 1 and down to 1e-320: y, and with it the whole dq row, is a few
    hundred orders below 1, its products with k are subnormal - the fma rounds them once, as the contract says"""
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(125, [2] * 300 + [3] * 100, np.float64)
    q, k, v = ac.operands(126, shape, 4, 3, np.float64)
    g = gc.grad_operand(127, shape, 3, np.float64)
    want = gc.grad_restated(indptr, indices, vals, q, k, v, g, 1024, 300.0)
    tiny = (np.abs(want[0]).max(axis=1) < 1e-290) & (np.abs(want[0]).max(axis=1) > 0)
    assert tiny.sum() >= 5 and np.isfinite(want[0]).all()
    got = sparse_amd.sparse_attention_grad(_coo(indptr, indices, vals, shape), q, k, v, g, scale=300.0)
    assert _same(got, want[:3])


# ---- caches -----------------------------------------------------------------------------------------------------------------------------
def test_second_call_builds_and_converts_nothing(monkeypatch):
    import sparse_amd
    from sparse_amd import _attention, _dot, _ffi

    built, converted = [], []
    real_plan, real_csr = _attention._build_grad_plan, _dot._csr_triplet
    monkeypatch.setattr(_attention, "_build_grad_plan", lambda *a: built.append(1) or real_plan(*a))

    def csr_spy(a):
        had = a.__dict__.get("_csr_view") is not None or a.__dict__.get("_csr_twin") is not None
        converted.append(not had)
        return real_csr(a)

    monkeypatch.setattr(_dot, "_csr_triplet", csr_spy)
    indptr, indices, vals, shape = ac.csr_mask(130, ac.SHORT_LENGTHS + [1500], np.float32)
    q, k, v = ac.operands(131, shape, 16, 8, np.float32)
    g = gc.grad_operand(132, shape, 8, np.float32)
    tq, tk, tv, tg = _dev(q, k, v, g)
    want = gc.grad_restated(indptr, indices, vals, q, k, v, g, 1024)[:3]
    for x in (_coo(indptr, indices, vals, shape), _coo(indptr, indices, vals, shape).asformat("gcxs", compressed_axes=(1,)),
              _csr(indptr, indices, vals, shape)):
        del built[:], converted[:]
        first = sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg)
        assert built == [1] and sum(converted) <= 1
        plan, c1 = x._attention_grad_plan, _ffi.CALLS
        second = sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg)
        assert _ffi.CALLS - c1 == 1                                          # the kernel's one call: nothing converted, no plan
        assert built == [1] and sum(converted) <= 1 and x._attention_grad_plan is plan and plan["max_col"] >= 1
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and _same(first, want)
        x.data *= 2                                                          # a write to the values is followed
        doubled = sparse_amd.sparse_attention_grad(x, tq, tk, tv, tg)
        assert _same(doubled, gc.grad_restated(indptr, indices, 2 * vals, q, k, v, g, 1024)[:3])


def test_python_argument_errors_that_need_a_mask():
    import sparse_amd

    q, k, v, g = (np.zeros(s, np.float32) for s in ((5, 4), (6, 4), (6, 3), (5, 3)))
    coords = np.array([[0, 1], [2, 3]])
    s = sparse_amd.COO(coords, np.ones(2, np.float32), shape=(5, 6), device=DEV)
    with pytest.raises(ValueError, match="2-D mask"):
        sparse_amd.sparse_attention_grad(sparse_amd.COO(np.zeros((3, 1), np.int64), np.ones(1, np.float32), shape=(2, 5, 6), device=DEV), q, k, v, g)
    with pytest.raises(ValueError, match="zero fill"):
        sparse_amd.sparse_attention_grad(sparse_amd.COO(coords, np.ones(2, np.float32), shape=(5, 6), fill_value=1.0, device=DEV), q, k, v, g)
    with pytest.raises(TypeError, match="scale"):
        sparse_amd.sparse_attention_grad(s, q, k, v, g, scale="1")
    with pytest.raises(TypeError, match="complex"):
        sparse_amd.sparse_attention_grad(sparse_amd.COO(coords, np.ones(2, np.complex64), shape=(5, 6), device=DEV), q, k, v, g)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.sparse_attention_grad(s, q[:4], k, v, g)
    with pytest.raises(TypeError, match="all float32 or all float64"):
        sparse_amd.sparse_attention_grad(s, q, k.astype(np.float64), v, g)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.sparse_attention_grad(s, q, k, v, g[:, :2])
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.sparse_attention_grad(s, q, k, v, g[None])
    with pytest.raises(TypeError, match="`grad` must have the type"):
        sparse_amd.sparse_attention_grad(s, q, k, v, g.astype(np.float64))
    with pytest.raises(TypeError, match="`grad` must be"):
        sparse_amd.sparse_attention_grad(s, q, k, v, g.tolist())


# ---- hubs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", [False, True], ids=["row", "column"])
def test_hub(columns):
    """one row, or one column, of 5000 elements among short ones at the default chunk: five pieces through the workspace, two heads"""
    import sparse_amd
    from sparse_amd import _kernels as K

    lengths = [3, 0, 17, 5000, 64, 9, 70]
    indptr, indices, vals, shape = (gc.transposed_mask if columns else ac.csr_mask)(140, lengths, np.float32)
    q, k, v = ac.operands(141, shape, 16, 8, np.float32, lead=(2,))
    g = gc.grad_operand(142, shape, 8, np.float32, lead=(2,))
    got = sparse_amd.sparse_attention_grad(_coo(indptr, indices, vals, shape), q, k, v, g, scale=0.25)
    assert _same(got, gc.grad_heads(indptr, indices, vals, q, k, v, g, K.ATTENTION_CHUNK, 0.25))
    assert all(np.isfinite(a).all() for a in got) and (got[1][:, 3].any() if columns else got[0][:, 3].any())


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_function_has_the_bits_of_both_calls():
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(150, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(151, shape, 12, 7, np.float32, lead=(3,))
    g = gc.grad_operand(152, shape, 7, np.float32, lead=(3,))
    s = _coo(indptr, indices, vals, shape)
    tq, tk, tv, tg = _dev(q, k, v, g)
    tq.requires_grad_()
    tv.requires_grad_()
    out = sparse_amd.sparse_attention_autograd(s, tq, tk, tv, scale=0.4)
    assert out.requires_grad and torch.equal(out.detach(), sparse_amd.sparse_attention(s, tq.detach(), tk, tv.detach(), scale=0.4))
    out.backward(tg)
    dq, dk, dv = sparse_amd.sparse_attention_grad(s, tq.detach(), tk, tv.detach(), tg, scale=0.4)
    assert torch.equal(tq.grad, dq) and torch.equal(tv.grad, dv) and tk.grad is None
    assert _same((dq, dk, dv), gc.grad_heads(indptr, indices, vals, q, k, v, g, 1024, 0.4))
    tk.requires_grad_()
    sparse_amd.sparse_attention_autograd(s, tq.detach(), tk, tv.detach(), scale=0.4).backward(tg)
    assert torch.equal(tk.grad, dk)
    with pytest.raises(TypeError, match="torch tensor"):
        sparse_amd.sparse_attention_autograd(s, q, tk, tv)


def test_gradcheck():
    """float64, a mask of 5 x 6 without an empty row, D = 3, Dv = 2, two heads, at torch's own default tolerances; operands drawn
    by `attention_cases.operands`, so that no score sits at a tie of the maximum"""
    import sparse_amd

    rng = np.random.default_rng(160)
    dense = rng.random((5, 6)) < 0.5
    dense[np.arange(5), rng.integers(0, 6, 5)] = True
    indptr = np.concatenate(([0], np.cumsum(dense.sum(axis=1))))
    indices = np.nonzero(dense)[1]
    vals = rng.uniform(0.5, 1.5, len(indices)) * rng.choice([-1, 1], len(indices))
    s = _coo(indptr, indices, vals, (5, 6))
    tq, tk, tv = (t.requires_grad_() for t in _dev(*ac.operands(161, (5, 6), 3, 2, np.float64, lead=(2,))))
    assert torch.autograd.gradcheck(lambda a, b, c: sparse_amd.sparse_attention_autograd(s, a, b, c, scale=0.7), (tq, tk, tv))

"""sparse_amd.sparse_attention on the device (csrc/attention.hip).

Yardsticks, all from tests/attention_cases.py:
  * `attention_restated` - the order contract of include/sparse_amd.h A15 written in NumPy - in the result type, BIT FOR BIT
    (any NaN equals any NaN: a payload is no result);
  * every kernel form, sub-group width and chunk against every other, bit for bit, for the lengths it accepts;
  * `sparse_amd.softmax` on the restated scores: the probabilities of two independently written kernels, bit for bit;
  * the three-call expression matmul(softmax(sddmm(s, q, bt=k), scale=c), v) within the derived bounds (`other_form_bound`).
Every comparison against a bound prints the largest share of it that it saw."""
import functools

import numpy as np
import pytest
import torch

import attention_cases as ac
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


@pytest.fixture
def spy(monkeypatch):
    """records the CSR triple every `attention_rows` call was given"""
    from sparse_amd import _kernels as K

    seen = []
    real = K.attention_rows

    def wrapped(indptr, indices, svals, *a, **kw):
        seen.append((indptr, indices, svals))
        return real(indptr, indices, svals, *a, **kw)

    monkeypatch.setattr(K, "attention_rows", wrapped)
    return seen


# ---- row lengths, layouts -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lengths_case(chunk, dtype):
    """the listed lengths in one mask, D = 17 and Dv = 5, a scale; the restated result, computed once per chunk and type"""
    indptr, indices, vals, shape = ac.csr_mask(40 + chunk, sc.listed_lengths(chunk), dtype)
    q, k, v = ac.operands(41 + chunk, shape, 17, 5, dtype)
    out, t, p = ac.attention_restated(indptr, indices, vals, q, k, v, chunk, 0.3)
    for a in (indptr, indices, vals, q, k, v, out):
        a.setflags(write=False)
    return indptr, indices, vals, shape, q, k, v, out


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_listed_lengths_bit_for_bit_in_every_layout(dtype, idx, chunk, monkeypatch, spy):
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    indptr, indices, vals, shape, q, k, v, want = _lengths_case(chunk, np.dtype(dtype))
    tidx = torch.int32 if np.dtype(idx) == np.int32 else torch.int64
    ptr_i, ind_i = indptr.astype(idx), indices.astype(idx)

    def same_csr(triple):
        """the triple the kernel read is the canonical CSR order the reference was restated on"""
        return (np.array_equal(_np(triple[0]), indptr) and np.array_equal(_np(triple[1]), indices)
                and np.array_equal(_np(triple[2]), vals))

    # a canonical COO
    coo = _coo(ptr_i, ind_i, vals, shape, idx)
    got = sparse_amd.sparse_attention(coo, q, k, v, scale=0.3)
    assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype) and got.shape == (shape[0], 5)
    assert sc.same_bits(got, want) and same_csr(spy[-1]) and spy[-1][0].dtype == tidx
    # a row-compressed GCXS: its own arrays, untouched, at its own index width
    g = _csr(ptr_i, ind_i, vals, shape)
    got = sparse_amd.sparse_attention(g, q, k, v, scale=0.3)
    assert spy[-1][0] is g.indptr and spy[-1][1] is g.indices and spy[-1][2] is g.data and g.indptr.dtype == tidx
    assert sc.same_bits(got, want)
    # a column-compressed GCXS: the memoised CSR twin (stable, so the CSR order is the canonical one)
    gc = coo.asformat("gcxs", compressed_axes=(1,))
    got = sparse_amd.sparse_attention(gc, q, k, v, scale=0.3)
    assert same_csr(spy[-1]) and spy[-1][0] is not gc.indptr and sc.same_bits(got, want)
    # a COO built unsorted
    perm = np.random.default_rng(5).permutation(len(indices))
    coords = ac.coords_of(indptr, indices)[:, perm].astype(idx)
    un = sparse_amd.COO(coords, vals[perm], shape=shape, idx_dtype=idx, device=DEV)
    got = sparse_amd.sparse_attention(un, q, k, v, scale=0.3)
    assert same_csr(spy[-1]) and sc.same_bits(got, want)


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
        got = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, v)
        want, _, _ = ac.attention_restated(indptr, indices, vals, q, k, v, 1024)
        assert got.shape == (shape[0], Dv) and sc.same_bits(got, want), dtype


# ---- heads ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (1,), (3,), (2, 2)])
def test_heads_share_one_mask(lead):
    import sparse_amd

    indptr, indices, vals, shape = ac.csr_mask(60, ac.SHORT_LENGTHS + [130], np.float32)
    q, k, v = ac.operands(61, shape, 20, 9, np.float32, lead=lead)
    s = _coo(indptr, indices, vals, shape)
    got = sparse_amd.sparse_attention(s, q, k, v, scale=0.5)
    assert got.shape == lead + (shape[0], 9) and got.dtype == np.float32
    assert sc.same_bits(got, ac.attention_heads(indptr, indices, vals, q, k, v, 1024, 0.5))
    for h in np.ndindex(*lead):
        assert sc.same_bits(got[h], sparse_amd.sparse_attention(s, q[h], k[h], v[h], scale=0.5))
    tq, tk, tv = _dev(q, k, v)
    tout = sparse_amd.sparse_attention(s, tq, tk, tv, scale=0.5)
    assert isinstance(tout, torch.Tensor) and tout.is_cuda and tuple(tout.shape) == got.shape and sc.same_bits(_np(tout), got)


# ---- strides --------------------------------------------------------------------------------------------------------------------------
def test_strided_operands():
    """row-strided views (a slice of a wider tensor: read in place) and a transposed last axis (the one copy), torch and NumPy"""
    import sparse_amd
    from sparse_amd import _kernels as K

    indptr, indices, vals, shape = ac.csr_mask(70, ac.SHORT_LENGTHS, np.float32)
    M, N = shape
    D, Dv, lead = 19, 7, (2,)
    q, k, v = ac.operands(71, shape, D, Dv, np.float32, lead=lead)
    s = _coo(indptr, indices, vals, shape)
    want = sparse_amd.sparse_attention(s, q, k, v)
    assert sc.same_bits(want, ac.attention_heads(indptr, indices, vals, q, k, v, 1024))

    def wide(x):                       # a slice of a wider tensor: the row pitch exceeds the width
        w = torch.zeros(x.shape[:-1] + (x.shape[-1] + 9,), device=DEV)
        w[..., 4:4 + x.shape[-1]] = torch.from_numpy(x).to(DEV)
        return w[..., 4:4 + x.shape[-1]]

    def turned(x):                     # the last axis strided: a transposed buffer
        return torch.from_numpy(x).to(DEV).transpose(-1, -2).contiguous().transpose(-1, -2)

    for make, copies in ((wide, False), (turned, True)):
        tq, tk, tv = make(q), make(k), make(v)
        assert not tq.is_contiguous()
        for t in (tq, tk, tv):
            t3, pitch, head = K._rows3(t, t.device)
            assert (t3.data_ptr() != t.data_ptr()) == copies and t3.stride(2) == 1 and pitch >= t.shape[-1]
        got = sparse_amd.sparse_attention(s, tq, tk, tv)
        assert isinstance(got, torch.Tensor) and sc.same_bits(_np(got), want)
    nq = np.zeros((2, M, D + 3), np.float32)
    nq[..., 1:1 + D] = q
    got = sparse_amd.sparse_attention(s, nq[..., 1:1 + D], np.asfortranarray(k), v[:, ::-1][:, ::-1])
    assert isinstance(got, np.ndarray) and sc.same_bits(got, want)
    mixed = sparse_amd.sparse_attention(s, q, torch.from_numpy(k).to(DEV), v)                  # any torch operand: a tensor out
    assert isinstance(mixed, torch.Tensor) and sc.same_bits(_np(mixed), want)


# ---- every form against every other ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_groups_and_chunks_change_no_bit(dtype, idx):
    """`idx`: the width of the row pointers and column indices the kernels read"""
    from sparse_amd import _kernels as K

    def runs(lengths, seed, variants, lead=(2,)):
        indptr, indices, vals, shape = ac.csr_mask(seed, lengths, dtype)
        q, k, v = ac.operands(seed + 1, shape, 21, 6, dtype, lead=lead)
        tq, tk, tv = _dev(q, k, v)
        ptr, ind, val = torch.from_numpy(indptr).to(DEV).to(idx), torch.from_numpy(indices).to(DEV).to(idx), torch.from_numpy(vals).to(DEV)
        outs = {str(kw): _np(K.attention_rows(ptr, ind, val, tq, tk, tv, max(lengths), scale=0.7, **kw)) for kw in variants}
        first = next(iter(outs.values()))
        assert all(sc.same_bits(first, o) for o in outs.values()), [name for name, o in outs.items() if not sc.same_bits(first, o)]
        return (indptr, indices, vals, q, k, v), first

    # lengths every form accepts: sub-groups of every width, a wave per row at two chunks, the piece form's wave per row
    short = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 5]
    variants = [dict(form="short", group=g) for g in K.ATTENTION_GROUPS] + [dict(form="wide", chunk=c) for c in (64, 1024)]
    variants += [dict(form="long"), dict(), dict(group=8), dict(group=64, chunk=128), dict(short_max=16), dict(short_max=0, group=32)]
    case, got = runs(short, 71, variants)
    assert sc.same_bits(got, ac.attention_heads(*case, 64, 0.7))
    # up to 128: a wave per row at chunks 128 and 1024, the default split at 64 with every width, the piece form at 128
    mid = short + [65, 100, 127, 128]
    variants = [dict(form="wide", chunk=c) for c in (128, 1024)] + [dict(group=g, chunk=c) for g in K.ATTENTION_GROUPS for c in (128, 256)]
    variants += [dict(form="long", chunk=128)]
    runs(mid, 72, variants)
    # pieces (chunk is part of the order here, so one chunk at a time): the piece form against the default split, every width
    long_ = mid + [129, 191, 192, 193, 64 * 5, 700]
    for chunk in (64, 128):
        variants = [dict(form="long", chunk=chunk)] + [dict(group=g, chunk=chunk) for g in K.ATTENTION_GROUPS]
        case, got = runs(long_, 73, variants, lead=())
        assert sc.same_bits(got, ac.attention_heads(*case, chunk, 0.7))
    z = torch.zeros(65, device=DEV, dtype=torch.float32)
    one = (torch.tensor([0, 65], device=DEV), torch.zeros(65, dtype=torch.int64, device=DEV), z, torch.zeros(1, 4, device=DEV),
           torch.zeros(1, 4, device=DEV), torch.zeros(1, 4, device=DEV), 65)
    with pytest.raises(ValueError, match="short"):
        K.attention_rows(*one, form="short")
    with pytest.raises(ValueError, match="wide"):
        K.attention_rows(*one, form="wide", chunk=64)


# ---- the probabilities of two kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_probabilities_equal_softmax_of_the_restated_scores(dtype, monkeypatch):
    """v = the identity: out[r, c_i] = fma(p_i, 1, +0) and every other term adds +0, so the fused kernel hands out its
    probabilities themselves - they equal `sparse_amd.softmax` of a COO of the restated scores, and the restated p"""
    import sparse_amd
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "ATTENTION_CHUNK", 64)
    monkeypatch.setattr(K, "SOFTMAX_CHUNK", 64)
    lengths = [0, 1, 5, 33, 64, 65, 128, 200, 3]
    indptr, indices, vals, shape = ac.csr_mask(80, lengths, dtype)
    q, k, _ = ac.operands(81, shape, 24, 1, dtype)
    eye = np.eye(shape[1], dtype=dtype)
    _, t, p = ac.attention_restated(indptr, indices, vals, q, k, eye, 64, 0.6)
    got = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, eye, scale=0.6)
    rows, cols = ac.coords_of(indptr, indices)
    sm = sparse_amd.softmax(_coo(indptr, indices, t, shape), 1)
    assert sc.same_bits(_np(sm.data), p) and sc.same_bits(got[rows, cols], _np(sm.data))
    assert np.count_nonzero(got) <= len(p)


# ---- the three-call expression ----------------------------------------------------------------------------------------------------------
def _three_calls(s, q, k, v, scale):
    import sparse_amd

    out = sparse_amd.matmul(sparse_amd.softmax(sparse_amd.sddmm(s, q, bt=k), -1, scale=scale), v)
    return out if isinstance(out, np.ndarray) else _np(out.todense() if hasattr(out, "todense") else out)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_call_expression_within_the_bounds(dtype):
    """continuous random operands and non-zero mask values, so that no score is 0 and sddmm prunes nothing.  D = 16: a dot
    product of 16 terms in any order of fmas plus the two multiplies has at most 18 roundings of u = eps / 2 each, the 9 eps
    of the score bound; the rest is `other_form_bound`, and the comparison value's own 4 eps |value|"""
    import sparse_amd

    lengths = [1, 2, 5, 17, 40, 64, 65, 130, 300, 1100, 0, 9]
    indptr, indices, vals, shape = ac.csr_mask(90, lengths, dtype)
    q, k, v = ac.operands(91, shape, 16, 8, dtype)
    scale = 0.25
    s = _coo(indptr, indices, vals, shape)
    got = sparse_amd.sparse_attention(s, q, k, v, scale=scale)
    three = _three_calls(s, q, k, v, scale)
    _, t, _ = ac.attention_restated(indptr, indices, vals, q, k, v, 1024, scale)
    assert (t != 0).all()
    want, bound = ac.other_form_bound(indptr, indices, vals, q, k, v, t, scale)
    bound = bound + 4 * np.finfo(dtype).eps * np.abs(three)
    err = np.abs(got.astype(np.longdouble) - three.astype(np.longdouble))
    rows = np.diff(indptr) > 0
    assert not err[~rows].any()                                                # a row without stored elements: +0.0 from both
    worst = float((err[rows] / bound[rows]).max())
    print(f"attention {np.dtype(dtype)}: fused against the three-call expression, largest share of the bound {worst:.3f}; "
          f"against the exact value {ac.share(got, *ac.output_exact_and_bound(indptr, indices, t, v)[:2]):.3f}")
    assert worst <= 1 and three.shape == got.shape


def test_stored_zeros_take_part():
    """a stored zero of the mask is the score 0 here; the three-call expression drops it (sddmm prunes zeros), so its row is
    the softmax of the remaining element alone: v[c] itself"""
    import sparse_amd

    indptr, indices = np.array([0, 2, 3]), np.array([1, 3, 0])
    q, k, v = ac.operands(95, (2, 4), 8, 3, np.float32)
    zero = np.copysign(np.float32(0), ac.dot64(q[0], k[[1]])[0])              # the zero whose score is +0.0: sddmm prunes all-zero bits
    vals = np.array([zero, 1.5, 1.0], np.float32)
    s = _coo(indptr, indices, vals, (2, 4))
    assert s.nnz == 3
    got = sparse_amd.sparse_attention(s, q, k, v)
    want, t, p = ac.attention_restated(indptr, indices, vals, q, k, v, 1024)
    assert sc.same_bits(got, want) and t[0] == 0 and not np.signbit(t[0]) and 0 < p[0] < 1
    three = _three_calls(s, q, k, v, None)
    assert np.allclose(three[0], v[3], rtol=1e-6) and not np.allclose(got[0], v[3], rtol=1e-3)
    assert np.allclose(three[1], got[1], rtol=1e-6)


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def test_empty_mask_and_empty_rows():
    import sparse_amd
    from sparse_amd import _ffi

    q, k, v = ac.operands(100, (6, 9), 5, 4, np.float64, lead=(2,))
    empty = sparse_amd.COO(np.zeros((2, 0), np.int64), np.zeros(0, np.float32), shape=(6, 9), device=DEV)
    c0 = _ffi.CALLS
    out = sparse_amd.sparse_attention(empty, q, k, v)
    assert _ffi.CALLS == c0 and out.shape == (2, 6, 4) and out.dtype == np.float64 and not out.any() and not np.signbit(out).any()
    tout = sparse_amd.sparse_attention(empty, *_dev(q, k, v))
    assert isinstance(tout, torch.Tensor) and tout.dtype == torch.float64 and not tout.any()
    assert sparse_amd.sparse_attention(_coo(np.array([0, 1]), np.array([2]), np.ones(1, np.float32), (1, 9)), q[:, :1], k, v[..., :0]).shape == (2, 1, 0)
    indptr, indices, vals, shape = ac.csr_mask(101, [0, 0, 3, 70, 0, 1100, 2, 0], np.float64)      # empty first and last rows
    q, k, v = ac.operands(102, shape, 5, 4, np.float64)
    got = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, v)
    assert sc.same_bits(got, ac.attention_restated(indptr, indices, vals, q, k, v, 1024)[0])
    assert not got[[0, 1, 4, 7]].any() and not np.signbit(got[[0, 1, 4, 7]]).any() and np.isfinite(got).all()


@pytest.mark.parametrize("mask_dtype", [np.int32, np.int64, np.bool_])
def test_integer_and_boolean_mask_values(mask_dtype, monkeypatch):
    import sparse_amd

    chunk = _chunk(monkeypatch, 64)
    for dtype in (np.float32, np.float64):
        indptr, indices, vals, shape = ac.csr_mask(110, [0, 3, 70, 200, 9], mask_dtype)
        q, k, v = ac.operands(111, shape, 12, 6, dtype)
        got = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, v, scale=0.5)
        assert got.dtype == np.dtype(dtype)                                                   # the type of q, k, v: the mask is converted
        assert sc.same_bits(got, ac.attention_restated(indptr, indices, vals, q, k, v, chunk, 0.5)[0])


@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype, chunk, monkeypatch):
    """a NaN, a +inf score, nothing but -inf scores, -inf beside finite scores, at lengths of every form; with a positive and
    a negative scale.  The infinities enter through the mask values, with the sign that gives the score its sign"""
    import sparse_amd

    chunk = _chunk(monkeypatch, chunk)
    inf = np.inf
    lengths = [6, 40, 130, 2 * chunk + 9] * 4 + [5]
    indptr, indices, vals, shape = ac.csr_mask(120, lengths, dtype)
    q, k, v = ac.operands(121, shape, 10, 6, dtype)
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
        got = sparse_amd.sparse_attention(s, q, k, v, scale=scale)
        want, t, p = ac.attention_restated(indptr, indices, vals, q, k, v, chunk, scale)
        assert sc.same_bits(got, want)
        assert np.isnan(got[:4]).all() and np.isfinite(got[16]).all()
        if scale > 0:
            assert np.isnan(got[4:12]).all() and np.isfinite(got[12:16]).all()
        else:           # scale < 0: +inf becomes -inf (+0.0 beside finite scores), -inf becomes +inf (NaN throughout)
            assert np.isfinite(got[4:8]).all() and np.isnan(got[8:16]).all()


# ---- caches -----------------------------------------------------------------------------------------------------------------------------
def test_second_call_converts_nothing_and_follows_value_writes():
    import sparse_amd
    from sparse_amd import _ffi

    indptr, indices, vals, shape = ac.csr_mask(130, ac.SHORT_LENGTHS + [1500], np.float32)
    q, k, v = ac.operands(131, shape, 16, 8, np.float32)
    tq, tk, tv = _dev(q, k, v)
    for x in (_coo(indptr, indices, vals, shape), _coo(indptr, indices, vals, shape).asformat("gcxs", compressed_axes=(1,)),
              _csr(indptr, indices, vals, shape)):
        c0 = _ffi.CALLS
        first = sparse_amd.sparse_attention(x, tq, tk, tv)
        c1 = _ffi.CALLS
        memo = x.__dict__.get("_csr_view") or x.__dict__.get("_csr_twin")
        plan = x._attention_plan
        second = sparse_amd.sparse_attention(x, tq, tk, tv)
        c2 = _ffi.CALLS
        assert c2 - c1 == 1 <= c1 - c0                                       # the kernel's one call: nothing converted, no plan
        assert (x.__dict__.get("_csr_view") or x.__dict__.get("_csr_twin")) is memo and x._attention_plan is plan
        assert plan["max_len"] == 1500 and torch.equal(first, second)
        assert sc.same_bits(_np(first), ac.attention_restated(indptr, indices, vals, q, k, v, 1024)[0])
        x.data *= 2
        doubled = sparse_amd.sparse_attention(x, tq, tk, tv)
        assert sc.same_bits(_np(doubled), ac.attention_restated(indptr, indices, 2 * vals, q, k, v, 1024)[0])


def test_python_argument_errors_that_need_a_mask():
    """a 3-D mask, a non-zero fill value, a bad scale, complex mask values and a shape mismatch, through the public function"""
    import sparse_amd

    q, k, v = np.zeros((5, 4), np.float32), np.zeros((6, 4), np.float32), np.zeros((6, 3), np.float32)
    coords = np.array([[0, 1], [2, 3]])
    s = sparse_amd.COO(coords, np.ones(2, np.float32), shape=(5, 6), device=DEV)
    with pytest.raises(ValueError, match="2-D mask"):
        sparse_amd.sparse_attention(sparse_amd.COO(np.zeros((3, 1), np.int64), np.ones(1, np.float32), shape=(2, 5, 6), device=DEV), q, k, v)
    with pytest.raises(ValueError, match="zero fill"):
        sparse_amd.sparse_attention(sparse_amd.COO(coords, np.ones(2, np.float32), shape=(5, 6), fill_value=1.0, device=DEV), q, k, v)
    with pytest.raises(TypeError, match="scale"):
        sparse_amd.sparse_attention(s, q, k, v, scale="1")
    with pytest.raises(TypeError, match="complex"):
        sparse_amd.sparse_attention(sparse_amd.COO(coords, np.ones(2, np.complex64), shape=(5, 6), device=DEV), q, k, v)
    with pytest.raises(ValueError, match="shape-mismatch"):
        sparse_amd.sparse_attention(s, q[:4], k, v)
    with pytest.raises(TypeError, match="all float32 or all float64"):
        sparse_amd.sparse_attention(s, q, k.astype(np.float64), v)


# ---- a hub row --------------------------------------------------------------------------------------------------------------------------
def test_hub_row():
    """one row of 5000 elements among short rows at the default chunk: five pieces through the workspace, two heads"""
    import sparse_amd
    from sparse_amd import _kernels as K

    lengths = [3, 0, 17, 5000, 64, 9, 70]
    indptr, indices, vals, shape = ac.csr_mask(140, lengths, np.float32)
    q, k, v = ac.operands(141, shape, 16, 8, np.float32, lead=(2,))
    got = sparse_amd.sparse_attention(_coo(indptr, indices, vals, shape), q, k, v, scale=0.25)
    assert sc.same_bits(got, ac.attention_heads(indptr, indices, vals, q, k, v, K.ATTENTION_CHUNK, 0.25))
    assert np.isfinite(got).all() and got[:, 3].any()

"""semiring_matmul_grad without a device: the restatement of include/sparse_amd.h A18 (tests/semiring_grad_cases.py) against torch's
CPU autograd of the dense statement and against central differences, the hand-written cases, the C interface and every
argument error of the C entry, the kernel layer and the public functions."""
import numpy as np
import pytest

import semiring_cases as sr
import semiring_grad_cases as sg


def _forward(indptr, indices, vals, b, add, mul, init):
    return sr.semiring_restated(indptr, indices, vals, b, add, mul, init=init)


# ---- the restatement against torch's CPU autograd of the dense statement ---------------------------------------------------------------
@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("dtype", sg.DTYPES)
@pytest.mark.parametrize("add,mul", sr.SEMIRINGS)
def test_restatement_equals_torch_autograd_of_the_dense_statement(add, mul, dtype, with_init, capsys):
    """`where(stored, a op b, identity).amax / amin(1)` (with the init as one more candidate) differentiated by torch on the CPU.
    Both sum the same terms - g b over an element's hits, a g over a column's hits - in another order, so they agree within
    2 n eps sum|terms| per element, the bound for a reordered sum of n terms (every term is itself rounded once by both: one
    more eps per term, inside the factor 2).  Tie-free inputs: the test asserts that the terms of every output are pairwise
    distinct and NaN-free."""
    import torch

    M, K, N = 24, 20, 67
    lengths = [0, 1, 2, 7, 8, 9, 19, 20, 0, 5, 3, 12] * 2
    indptr, indices, vals, b, init = sg.tie_free(7, lengths, K, N, dtype, mul, with_init)
    assert sg.products_distinct(indptr, indices, vals, b, mul, init)
    out, arg = _forward(indptr, indices, vals, b, add, mul, init)
    g = np.random.default_rng(9).standard_normal((M, N)).astype(dtype)      # full mantissas: the sums do round
    da, db, dinit = sg.grad_restated(indptr, indices, vals, b, arg, g, mul)

    rows = sr.coords_of(indptr, indices)[0]
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    tv = torch.tensor(vals, dtype=tdt, requires_grad=True)
    tb = torch.tensor(b, dtype=tdt, requires_grad=True)
    dense = torch.zeros(M, K, dtype=tdt).index_put((torch.tensor(rows), torch.tensor(indices)), tv)
    stored = torch.zeros(M, K, dtype=torch.bool)
    stored[rows, indices] = True
    t = dense[:, :, None] + tb[None] if mul == "plus" else dense[:, :, None] * tb[None]
    ident = float("inf") if add == "min" else -float("inf")
    t = torch.where(stored[:, :, None], t, torch.full_like(t, ident))
    ti = None
    if with_init:
        ti = torch.tensor(init, dtype=tdt, requires_grad=True)
        t = torch.cat([ti[:, None, :], t], dim=1)
    res = t.amin(1) if add == "min" else t.amax(1)
    assert sr.same_bits(res.detach().numpy(), out)                      # one operation per term: the same forward
    res.backward(torch.tensor(g, dtype=tdt))

    eps = np.finfo(dtype).eps
    hit = arg[rows] == indices[:, None]                                 # (nnz, N): element e credited at column j
    LD = np.longdouble
    term_a = np.abs(g[rows].astype(LD) * (b[indices].astype(LD) if mul == "times" else 1)) * hit
    bound_a = 2 * hit.sum(1) * eps * term_a.sum(1)
    term_b = np.abs(g[rows].astype(LD) * (vals[:, None].astype(LD) if mul == "times" else 1)) * hit
    n_b, s_b = np.zeros((K, N)), np.zeros((K, N), LD)
    np.add.at(n_b, indices, hit)
    np.add.at(s_b, indices, term_b)
    bound_b = 2 * n_b * eps * s_b
    err_a = np.abs(da.astype(LD) - tv.grad.numpy().astype(LD))
    err_b = np.abs(db.astype(LD) - tb.grad.numpy().astype(LD))
    with np.errstate(all="ignore"):
        share = max(np.nanmax(np.where(bound_a > 0, err_a / bound_a, 0), initial=0), np.nanmax(np.where(bound_b > 0, err_b / bound_b, 0), initial=0))
    with capsys.disabled():
        print(f"\n[semiring_grad] {add}.{mul} {np.dtype(dtype).name} init={with_init}: largest share of the bound {float(share):.3f}")
    assert (err_a <= bound_a).all() and (err_b <= bound_b).all()
    if with_init:
        assert np.array_equal(dinit, ti.grad.numpy())                   # a copy of g or a zero (torch's zero may be -0.0): no arithmetic
    else:
        assert not dinit.any() or (arg == -1).any()


# ---- central differences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add,mul", sr.SEMIRINGS)
def test_restatement_equals_central_differences(add, mul):
    """float64, 6 x 5 x 3.  With gaps of at least 1e-3 between the terms of an output and a step of 1e-6 no pick changes, and the
    loss sum(w * out) is then linear in every single input: the central difference is exact up to the rounding of the two loss
    values, at most 2 * (M N + 1) * eps * sum|w out| / (2 h)."""
    M, K, N, h = 6, 5, 3, 1e-6
    indptr, indices, vals, b, init = sg.tie_free(11, [0, 1, 2, 3, 5, 4], K, N, np.float64, mul)
    assert sg.products_distinct(indptr, indices, vals, b, mul, init, gap=1e-3)
    w = sr.operand(12, (M, N), np.float64) + 1 / 16
    out, arg = _forward(indptr, indices, vals, b, add, mul, init)
    da, db, dinit = sg.grad_restated(indptr, indices, vals, b, arg, w, mul)
    assert (arg == -1).any() and (arg >= 0).any()
    tol = 2 * (M * N + 1) * np.finfo(np.float64).eps * np.abs(w * out).sum() / (2 * h)

    def loss(v, bb, ii):
        return float((w * _forward(indptr, indices, v, bb, add, mul, ii)[0]).sum())

    for name, x, got in (("da", vals, da), ("db", b, db), ("dinit", init, dinit)):
        for at in np.ndindex(x.shape):
            lo, hi = x.copy(), x.copy()
            lo[at] -= h
            hi[at] += h
            args = {"da": (lambda y: (y, b, init)), "db": (lambda y: (vals, y, init)), "dinit": (lambda y: (vals, b, y))}[name]
            num = (loss(*args(hi)) - loss(*args(lo))) / (hi[at] - lo[at])
            assert abs(num - got[at]) <= tol + 4 * np.finfo(np.float64).eps * abs(got[at]), (name, at, num, got[at])


# ---- the hand-written cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sg.DTYPES)
def test_restatement_obeys_the_rules_on_hand_written_cases(dtype):
    for name, indptr, indices, vals, b, arg, g, mul, da, db, dinit in sg.hand_cases(dtype):
        got = sg.grad_restated(indptr, indices, vals, b, arg, g, mul)
        assert sr.same_bits(got[0], da) and sr.same_bits(got[1], db) and sr.same_bits(got[2], dinit), (name, got)
    for mul in sg.MULS:
        indptr, indices, vals, b, arg, g, want = sg.n130_case(dtype, mul)
        da, db, dinit = sg.grad_restated(indptr, indices, vals, b, arg, g, mul)
        assert sr.same_bits(da, want) and not dinit.any()
        # the column pass takes ONE element per output: a * g (times) or g (plus), rounded once
        assert sr.same_bits(db[1], (vals[0] * g[0] if mul == "times" else g[0] + 0)) and not db[0].any()


def test_generators_cover_the_listed_lengths_in_rows_and_columns():
    indptr, indices, vals, shape = sr.csr_mask(50, sg.LENGTHS, np.float32)
    tptr, tidx, tvals, tshape = sg.transposed(indptr, indices, vals, shape)
    assert sorted(np.diff(indptr)) == sorted(sg.LENGTHS) and tshape == shape[::-1]
    dense = np.zeros(shape, np.float32)
    dense[sr.coords_of(indptr, indices)[0], indices] = vals
    tdense = np.zeros(tshape, np.float32)
    tdense[sr.coords_of(tptr, tidx)[0], tidx] = tvals
    assert np.array_equal(tdense, dense.T)
    col_lengths = np.bincount(tidx, minlength=tshape[1])                 # the columns of the transposed: the listed lengths
    assert sorted(col_lengths) == sorted(sg.LENGTHS)


# ---- the interface ----------------------------------------------------------------------------------------------------------------------
def test_c_abi_public_functions_and_constants(hiplib):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    for name in ("spamd_semiring_grad", "spamd_semiring_grad_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_semiring_grad"][1]) == 32 and len(_ffi.SIGNATURES["spamd_semiring_grad_ws_bytes"][1]) == 4
    for name in ("semiring_matmul_grad", "semiring_matmul_autograd"):
        assert callable(getattr(sparse_amd, name)) and name in sparse_amd.__all__
    assert K.SEMIRING_GRAD_COL_FORMS == ("short", "wide", "long") and K.SEMIRING_GRAD_COL_GROUPS == (1, 8, 16, 32, 64)
    # the shipped defaults (the sweep tables stand in DESIGN.md A18): a change goes with a new sweep
    assert K.SEMIRING_GRAD_GROUP == 8 and K.SEMIRING_GRAD_SHORT_MAX == 64 and K.SEMIRING_GRAD_CHUNK == 1024 == sg.CHUNK
    assert K.SEMIRING_GRAD_LANE_MAX_N == 4
    assert [K._semiring_grad_col_group(N, size) for N, size in ((1, 4), (4, 8), (5, 4), (16, 4), (64, 4), (64, 8), (130, 8))] == [1, 1, 8, 8, 16, 32, 64]


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch (the pointers are null)"""
    from sparse_amd import _ffi

    f = hiplib.spamd_semiring_grad
    one = 1      # a non-null output pointer that is never written: every call below returns before a launch

    def call(val=_ffi.F32, idx=_ffi.I64, mul=0, M=3, K=4, N=5, nnz=200, pitch=8, group=16, col_group=32, short_max=64, chunk=64,
             max_col=100, ws_bytes=0, da=one, db=one, dinit=one):
        return f(val, idx, mul, M, K, N, nnz, None, None, None, None, None, None, None, pitch, None, pitch, None, pitch, group,
                 col_group, short_max, chunk, max_col, None, ws_bytes, da, db, pitch, dinit, pitch, None)

    for val in (_ffi.C64, _ffi.F16, _ffi.BF16, _ffi.U8, _ffi.I32, _ffi.I64):      # the integer value types too
        assert call(val=val) == -2
    assert call(idx=_ffi.F32) == -2 and call(idx=_ffi.U8) == -2
    assert call(mul=2) == -1 and call(mul=-1) == -1
    for name in ("M", "K", "N", "nnz", "max_col"):
        assert call(**{name: -1}) == -1, name
    assert call(max_col=201) == -1 and call(pitch=4) == -1
    assert call(group=0) == -1 and call(group=12) == -1 and call(group=128) == -1 and call(group=1) == -1
    assert call(col_group=0) == -1 and call(col_group=12) == -1 and call(col_group=128) == -1 and call(col_group=2) == -1
    assert call(col_group=1) == -1 and call(col_group=1, N=4) == -1 and call(col_group=1, N=4, da=None, db=None, dinit=None) == 0
    assert call(short_max=-1) == -1 and call(short_max=65) == -1
    assert call(chunk=0) == -1 and call(chunk=32) == -1 and call(chunk=100) == -1 and call(chunk=(1 << 30) + 64) == -1
    for val in (_ffi.F32, _ffi.F64):
        for idx in (_ffi.I32, _ffi.I64):
            assert call(val=val, idx=idx, da=None, db=None, dinit=None) == 0                       # nothing is wanted
            assert call(val=val, idx=idx, nnz=0, max_col=0, N=0, pitch=0) == 0                     # every output is empty
            assert call(val=val, idx=idx, M=0, K=0, nnz=0, max_col=0) == 0
    assert call() == -1 and call(mul=1) == -1                                                      # null pointers with work to do
    assert call(da=None, db=None) == -1 and call(da=None, dinit=None) == -1 and call(db=None, dinit=None) == -1
    ws = hiplib.spamd_semiring_grad_ws_bytes
    assert ws(_ffi.F32, 64, 3, 64) == 0 and ws(_ffi.F64, 1024, 8, 1024) == 0
    assert ws(_ffi.F32, 65, 3, 64) == 2 * 2 * 3 * 4 and ws(_ffi.F64, 1000, 7, 128) == 2 * 8 * 7 * 8      # two slots a window
    for val in (_ffi.C64, _ffi.I32, _ffi.I64, _ffi.F16):
        assert ws(val, 10, 1, 64) == -2
    assert ws(_ffi.F32, 10, 1, 0) == -1 and ws(_ffi.F32, 10, 1, 96) == -1 and ws(_ffi.F32, -1, 1, 64) == -1 and ws(_ffi.F32, 10, -1, 64) == -1


def _stub(cls_name="COO", **attrs):
    """a container that holds nothing but the attributes the checks read (no device: nothing is stored)"""
    import sparse_amd

    base = getattr(sparse_amd, cls_name)
    body = dict(dict(shape=(5, 6), ndim=2, dtype=np.dtype("float32"), fill_value=np.float32(0), size=30, nnz=3), **attrs)
    body["__init__"] = lambda self: None
    return type("Stub" + cls_name, (base,), body)()


def test_python_argument_errors_of_the_public_functions():
    import torch

    import sparse_amd

    b = np.zeros((6, 4), np.float32)
    arg, g = np.zeros((5, 4), np.int64), np.zeros((5, 4), np.float32)
    grad, auto = sparse_amd.semiring_matmul_grad, sparse_amd.semiring_matmul_autograd
    tb = torch.zeros(6, 4)
    for bad in (np.zeros((5, 6)), None, torch.zeros(5, 6)):                                         # wrong container
        with pytest.raises(TypeError, match="COO or GCXS"):
            grad(bad, b, arg, g)
        with pytest.raises(TypeError, match="COO or GCXS"):
            auto(bad, tb)
    for cls in ("COO", "GCXS"):
        a = _stub(cls)
        with pytest.raises(ValueError, match="2-D"):
            grad(_stub(cls, ndim=3, shape=(5, 6, 2)), b, arg, g)
        with pytest.raises(ValueError, match="zero fill value"):
            grad(_stub(cls, fill_value=np.float32(1)), b, arg, g)
        with pytest.raises(ValueError, match="zero fill value"):
            auto(_stub(cls, fill_value=np.float32(1)), tb)
        # an integer b: min / max of integers has no gradient here
        for ib in (b.astype(np.int32), b.astype(np.int64), torch.zeros(6, 4, dtype=torch.int64)):
            with pytest.raises(TypeError, match="no gradient"):
                grad(a, ib, arg, g)
        with pytest.raises(TypeError, match="no gradient"):
            auto(a, torch.zeros(6, 4, dtype=torch.int32))
        for kw in (dict(mul="min"), dict(mul=None), dict(mul="TIMES")):
            with pytest.raises(ValueError, match="min.plus, min.times, max.plus and max.times"):
                grad(a, b, arg, g, **kw)
        with pytest.raises(ValueError, match="min.plus, min.times, max.plus and max.times"):
            auto(a, tb, add="sum")
        with pytest.raises(TypeError, match="16-bit"):
            grad(a, b.astype(np.float16), arg, g.astype(np.float16))
        with pytest.raises(ValueError, match="shape-mismatch"):
            grad(a, np.zeros((5, 4), np.float32), arg, g)
        for bad_arg in (arg[:4], arg[:, :3], np.zeros((5, 4, 1), np.int64)):
            with pytest.raises(ValueError, match="`arg`.*is not the shape"):
                grad(a, b, bad_arg, g)
        for bad_g in (g[:4], g.T, np.zeros(5, np.float32)):
            with pytest.raises(ValueError, match="`grad`.*is not the shape"):
                grad(a, b, arg, bad_g)
        with pytest.raises(ValueError, match="is not the shape"):
            grad(a, b[:, 0], arg, g)                                                                # a 1-D b: results of shape (M,)
        for bad_arg in (arg.astype(np.int32), arg.astype(np.float64), torch.zeros(5, 4, dtype=torch.int32)):
            with pytest.raises(TypeError, match="`arg` must be int64"):
                grad(a, b, bad_arg, g)
        with pytest.raises(TypeError, match="`grad` must have the type"):
            grad(a, b, arg, g.astype(np.float64))
        for name, kw in (("arg", dict(arg=arg.tolist(), grad=g)), ("grad", dict(arg=arg, grad=None))):
            with pytest.raises(TypeError, match=f"`{name}` must be a NumPy array or a torch tensor"):
                grad(a, b, kw["arg"], kw["grad"])
        with pytest.raises(TypeError, match="`values` must be a NumPy array or a torch tensor"):
            grad(a, b, arg, g, values=[1.0, 2.0, 3.0])
        for bad_v in (np.zeros(4, np.float32), np.zeros((3, 1), np.float32), torch.zeros(2)):
            with pytest.raises(ValueError, match="`values`.*is not aligned"):
                grad(a, b, arg, g, values=bad_v)
        with pytest.raises(ValueError, match="`values`.*is not aligned"):
            auto(a, tb, values=torch.zeros(4))
        with pytest.raises(TypeError, match="cannot be converted"):
            grad(a, b, arg, g, values=np.zeros(3, np.complex64))
        for name, kw in (("b", dict(b=b)), ("init", dict(b=tb, init=np.zeros((5, 4), np.float32))), ("values", dict(b=tb, values=np.zeros(3, np.float32)))):
            with pytest.raises(TypeError, match=f"`{name}` must be a torch tensor"):
                auto(a, kw.pop("b"), **kw)
        with pytest.raises(ValueError, match="shape-mismatch"):
            auto(a, tb, init=torch.zeros(5, 3))
        with pytest.raises(TypeError, match="`init` must have the type"):
            auto(a, tb, init=torch.zeros(5, 4, dtype=torch.float64))


def test_python_argument_errors_of_the_kernel_layer():
    """CPU tensors: every one of these is raised before the layer asks for a device"""
    import torch

    from sparse_amd import _ffi, _kernels as K

    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1])
    colptr, colperm, colrows = torch.tensor([0, 1, 3, 3, 3]), torch.tensor([0, 1, 2]), torch.tensor([0, 0, 1])
    vals, b = torch.ones(3), torch.ones(4, 5)
    arg, g = torch.zeros(2, 5, dtype=torch.int64), torch.ones(2, 5)

    def call(**kw):
        a = dict(dict(indptr=indptr, indices=indices, vals=vals, colptr=colptr, colperm=colperm, colrows=colrows, b=b, arg=arg, g=g,
                      max_col=2, mul="plus"), **kw)
        pos = [a.pop(n) for n in ("indptr", "indices", "vals", "colptr", "colperm", "colrows", "b", "arg", "g", "max_col")]
        return K.semiring_grad(*pos, **a)

    for mul in ("min", None, "mul"):
        with pytest.raises(ValueError, match="mul must be"):
            call(mul=mul)
    for form in ("rows", "lanes", "piece", 1):
        with pytest.raises(ValueError, match="col_form must be"):
            call(col_form=form)
    for group in (0, 1, 4, 12, 128):
        with pytest.raises(ValueError, match="group must be"):
            call(group=group)
    for cg in (0, 2, 4, 12, 128):
        with pytest.raises(ValueError, match="col_group must be"):
            call(col_group=cg)
    with pytest.raises(ValueError, match="col_group 1 takes"):
        call(col_group=1)
    for sm in (-1, 65, 3.5):
        with pytest.raises(ValueError, match="short_max must"):
            call(short_max=sm)
    for chunk in (0, 32, 100, -64, (1 << 30) + 64, 64.5):
        with pytest.raises(ValueError, match="chunk must be"):
            call(chunk=chunk)
    for ints in (torch.int32, torch.int64):
        with pytest.raises(TypeError, match="no gradient"):
            call(b=b.to(ints), vals=vals.to(ints), g=g.to(ints))
    for bad in (dict(vals=vals.double()), dict(g=g.double()), dict(b=b.half(), vals=vals.half(), g=g.half())):
        with pytest.raises(TypeError, match="one type"):
            call(**bad)
    with pytest.raises(TypeError, match="arg must be int64"):
        call(arg=arg.int())
    with pytest.raises(TypeError, match="int32 or both int64"):
        call(indptr=indptr.int())
    for bad in (dict(colptr=None), dict(colperm=colperm.int()), dict(colrows=colrows.int()), dict(colptr=colptr.int())):
        with pytest.raises(TypeError, match="column grouping"):
            call(**bad)
    with pytest.raises(ValueError, match="1 or 2 dimensions"):
        call(b=torch.ones(4, 5, 1))
    for bad in (dict(indices=indices[:2]), dict(b=torch.ones(0, 5), arg=arg, g=g)):
        with pytest.raises(ValueError, match="shape mismatch between the CSR"):
            call(**bad)
    for bad in (dict(arg=arg[:1]), dict(g=g[:, :4]), dict(arg=arg[:, 0], g=g[:, 0])):
        with pytest.raises(ValueError, match="result's shape"):
            call(**bad)
    for bad in (dict(colptr=colptr[:4]), dict(colperm=colperm[:2]), dict(colrows=colrows[:2])):
        with pytest.raises(ValueError, match="column grouping"):
            call(**bad)
    for form, max_col in (("short", 65), ("wide", 1025)):
        with pytest.raises(ValueError, match="does not take a column"):
            call(col_form=form, max_col=max_col)
    with pytest.raises(_ffi.HipBackendError, match="device"):                       # every check passed: now it wants a device
        call()
    with pytest.raises(_ffi.HipBackendError, match="device"):                       # without db the grouping is not needed
        call(colptr=None, colperm=None, colrows=None, want=(True, False, True))

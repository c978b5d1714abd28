"""semiring_matmul without a GPU: the NumPy restatement of the contract (tests/semiring_cases.py) - which judges the kernels bit
for bit in tests/test_semiring_gpu.py - equals a dense brute force where one is unambiguous and obeys the tie / NaN / signed-zero /
empty-row / init rules on hand-written sequences; the C ABI and the public surface are in place; every argument error of both
layers is raised before anything touches a device."""
import numpy as np
import pytest

import semiring_cases as sr


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sr.DTYPES)
@pytest.mark.parametrize("add,mul", sr.SEMIRINGS)
def test_restatement_equals_the_dense_brute_force_without_ties(add, mul, dtype):
    """9 x 12 with 1 to 12 stored elements per row, N = 5: values drawn so that every product of a row is distinct, finite and
    not zero - checked here -, which is where `where(stored, a op b, identity).min(axis=1)` says the same as the contract"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(7)
    M, K, N = 9, 12, 5
    stored = np.zeros((M, K), bool)
    for r in range(M):
        stored[r, rng.choice(K, 1 + r % K, replace=False)] = True
    # distinct primes on the left, distinct powers of two (floats: with distinct odd offsets under plus) on the right
    primes = np.array([3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107,
                       109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199, 211, 223, 227, 229,
                       233, 239, 241, 251, 257, 263, 269, 271, 277, 281, 283, 293, 307, 311, 313, 317, 331, 337, 347, 349, 353, 359,
                       367, 373, 379, 383, 389, 397, 401, 409, 419, 421, 431, 433, 439, 443, 449, 457, 461, 463, 467, 479, 487, 491,
                       499, 503, 509, 521, 523, 541, 547, 557, 563, 569, 571, 577, 587, 593, 599])
    dense = np.zeros((M, K), dtype)
    dense[stored] = rng.permutation(primes)[:stored.sum()] * rng.choice([-1, 1], stored.sum())
    b = (1000 * rng.permutation(K * N).reshape(K, N) + 1000).astype(dtype) if mul == "plus" else \
        (rng.permutation(np.arange(1, K * N + 1)).reshape(K, N) * 2 + 1000).astype(dtype)
    indptr = np.concatenate(([0], np.cumsum(stored.sum(axis=1))))
    indices = np.nonzero(stored)[1]
    vals = dense[stored]
    want, warg = sr.brute_force(dense, stored, b, add, mul)
    for r in range(M):                                           # the brute force is unambiguous here
        for j in range(N):
            t = sr.products(vals[indptr[r]:indptr[r + 1]], np.ascontiguousarray(b[indices[indptr[r]:indptr[r + 1]], j]), mul)
            assert len(set(t.tolist())) == len(t) and (t != 0).all() and (t != sr.identity(add, dtype)).all()
            assert dtype.kind != "f" or np.isfinite(t).all()
    out, arg = sr.semiring_restated(indptr, indices, vals, b, add, mul)
    assert out.dtype == dtype and arg.dtype == np.int64
    assert sr.same_bits(out, want) and np.array_equal(arg, warg)
    # a 1-D b is column 0, and an init of identities changes no value (the rows here are not empty)
    o1, a1 = sr.semiring_restated(indptr, indices, vals, np.ascontiguousarray(b[:, 0]), add, mul)
    assert sr.same_bits(o1, want[:, 0]) and np.array_equal(a1, warg[:, 0])
    oi, ai = sr.semiring_restated(indptr, indices, vals, b, add, mul, init=np.full((M, N), sr.identity(add, dtype)))
    assert sr.same_bits(oi, want) and np.array_equal(ai, warg)


@pytest.mark.parametrize("case", sr.ADVERSARIAL, ids=[c[0] for c in sr.ADVERSARIAL])
def test_restatement_obeys_the_rules_on_hand_written_sequences(case):
    for dtype in (np.float32, np.float64):
        indptr, indices, vals, b, init, add, mul, at, value = sr.adversarial_case(case, dtype)
        out, arg = sr.semiring_restated(indptr, indices, vals, b, add, mul, init=init)
        assert out.shape == (1, 1) and sr.same_bits(out[0, 0], value), (out, value)
        assert np.signbit(out[0, 0]) == np.signbit(value) or np.isnan(value)
        if init is None:
            assert arg[0, 0] == indices[at]
        else:
            assert arg[0, 0] == (-1 if at == 0 else indices[at - 1])


def test_restatement_empty_rows_stored_zeros_and_absent_positions():
    for dtype in sr.DTYPES:
        dtype = np.dtype(dtype)
        b = np.array([[4, -4], [5, -5], [-6, 6]], dtype)
        indptr, indices, vals = np.array([0, 0, 2, 3]), np.array([0, 2, 1]), np.array([0, 1, 0], dtype)
        for add in sr.ADDS:
            out, arg = sr.semiring_restated(indptr, indices, vals, b, add, "plus")
            assert (out[0] == sr.identity(add, dtype)).all() and (arg[0] == -1).all()          # an empty row: the identity
            # row 1 holds a STORED zero at k = 0 and a one at k = 2; position k = 1 is absent, although 0 + b[1] would win
            assert out[1].tolist() == ([-5, -4] if add == "min" else [4, 7]) and arg[1].tolist() == ([2, 0] if add == "min" else [0, 2])
            assert out[2].tolist() == [5, -5] and arg[2].tolist() == [1, 1]
            init = np.array([[1, 2], [-9, 9], [5, -5]], dtype)
            out, arg = sr.semiring_restated(indptr, indices, vals, b, add, "plus", init=init)
            assert out[0].tolist() == [1, 2] and (arg[0] == -1).all()                        # an empty row: the init
            assert out[2].tolist() == [5, -5] and (arg[2] == -1).all()                       # a tie with the init: the init
            assert out[1].tolist() == ([-9, -4] if add == "min" else [4, 9])
            assert arg[1].tolist() == ([-1, 0] if add == "min" else [0, -1])
            assert init.tolist() == [[1, 2], [-9, 9], [5, -5]]


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_c_abi_public_function_and_constants(hiplib):
    import sparse_amd
    from sparse_amd import _ffi, _kernels as K

    for name in ("spamd_semiring_spmm", "spamd_semiring_spmm_ws_bytes"):
        assert name in _ffi.SIGNATURES and name in _ffi.header_symbols() and hasattr(hiplib, name)
    assert set(_ffi.header_symbols()) == set(_ffi.SIGNATURES)
    assert len(_ffi.SIGNATURES["spamd_semiring_spmm"][1]) == 26 and len(_ffi.SIGNATURES["spamd_semiring_spmm_ws_bytes"][1]) == 5
    assert callable(sparse_amd.semiring_matmul) and "semiring_matmul" in sparse_amd.__all__
    assert K.SEMIRING_ADDS == sr.ADDS and K.SEMIRING_MULS == sr.MULS and K.SEMIRING_GROUPS == (8, 16, 32, 64)
    assert K.SEMIRING_FORMS == ("rows", "lanes", "long")
    assert K.SEMIRING_CHUNK % 64 == 0 and 64 <= K.SEMIRING_CHUNK <= K.SEMIRING_MAX_CHUNK and K.SEMIRING_LANES_MAX_N >= 1
    # the measured defaults (the sweep tables stand next to the constants and in DESIGN.md A17): a change goes with a new sweep
    assert K.SEMIRING_LANES_MAX_N == 4 and K.SEMIRING_CHUNK == 2048
    assert [K._semiring_group(True, 1, 4, 32 * 1000, 1000), K._semiring_group(False, 64, 4, 1, 1), K._semiring_group(False, 130, 8, 1, 1)] == [8, 16, 64]
    assert callable(K.semiring_spmm)


def test_argument_checks_of_the_c_entry_return_before_any_launch(hiplib):
    """no device is touched: every one of these returns before a launch"""
    from sparse_amd import _ffi

    f = hiplib.spamd_semiring_spmm

    def call(val=_ffi.F32, idx=_ffi.I64, add=0, mul=0, M=3, K=4, N=5, nnz=200, pitch=8, narrow=0, group=16, chunk=64, max_len=100,
             ws_bytes=0):
        return f(val, idx, add, mul, M, K, N, nnz, None, None, None, None, pitch, None, pitch, narrow, group, chunk, max_len, None,
                 ws_bytes, None, pitch, None, pitch, None)

    for val in (_ffi.C64, _ffi.F16, _ffi.BF16, _ffi.U8):
        assert call(val=val) == -2
    assert call(idx=_ffi.F32) == -2 and call(idx=_ffi.U8) == -2
    assert call(add=2) == -1 and call(add=-1) == -1 and call(mul=2) == -1 and call(mul=-1) == -1
    for name in ("M", "K", "N", "nnz", "max_len"):
        assert call(**{name: -1}) == -1, name
    assert call(max_len=201) == -1 and call(pitch=4) == -1
    assert call(group=0) == -1 and call(group=12) == -1 and call(group=128) == -1
    assert call(chunk=0) == -1 and call(chunk=32) == -1 and call(chunk=100) == -1 and call(chunk=(1 << 30) + 64) == -1
    for val in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.I64):
        for idx in (_ffi.I32, _ffi.I64):
            assert call(val=val, idx=idx, M=0) == 0 and call(val=val, idx=idx, N=0, pitch=0) == 0      # nothing to do
    assert call() == -1 and call(nnz=0, max_len=0) == -1                       # null pointers with work to do
    ws = hiplib.spamd_semiring_spmm_ws_bytes
    assert ws(_ffi.F32, 64, 3, 64, 1) == 0 and ws(_ffi.F64, 1024, 8, 1024, 0) == 0
    assert ws(_ffi.F32, 65, 3, 64, 0) == 2 * 2 * 3 * 4 and ws(_ffi.F32, 65, 3, 64, 1) == 2 * 2 * 3 * 12      # two slots a window
    assert ws(_ffi.I64, 1000, 7, 128, 1) == 2 * 8 * 7 * 16
    assert ws(_ffi.C64, 10, 1, 64, 0) == -2 and ws(_ffi.F32, 10, 1, 0, 0) == -1 and ws(_ffi.F32, 10, 1, 96, 0) == -1
    assert ws(_ffi.F32, -1, 1, 64, 0) == -1 and ws(_ffi.F32, 10, -1, 64, 0) == -1


def _stub(cls_name="COO", **attrs):
    """a container that holds nothing but the attributes the checks read (no device: nothing is stored)"""
    import sparse_amd

    base = getattr(sparse_amd, cls_name)
    body = dict(dict(shape=(5, 6), ndim=2, dtype=np.dtype("float32"), fill_value=np.float32(0), size=30, nnz=3), **attrs)
    body["__init__"] = lambda self: None
    return type("Stub" + cls_name, (base,), body)()


def test_python_argument_errors_of_the_public_function():
    import torch

    import sparse_amd
    from sparse_amd._semiring import _check_arguments as check

    b = np.zeros((6, 4), np.float32)
    for bad in (np.zeros((5, 6)), None, [[1.0]], torch.zeros(5, 6)):                                     # wrong container
        with pytest.raises(TypeError, match="COO or GCXS"):
            sparse_amd.semiring_matmul(bad, b)
    for cls in ("COO", "GCXS"):
        for ndim, shape in ((1, (6,)), (3, (5, 6, 2))):
            with pytest.raises(ValueError, match="2-D"):
                sparse_amd.semiring_matmul(_stub(cls, ndim=ndim, shape=shape), b)
        with pytest.raises(ValueError, match="zero fill value"):
            sparse_amd.semiring_matmul(_stub(cls, fill_value=np.float32(1)), b)
        # the semiring, the types and the shapes are checked before the stub's (missing) arrays are touched
        for kw in (dict(add="sum"), dict(add="MIN"), dict(mul="min"), dict(mul=None), dict(add="plus", mul="min")):
            with pytest.raises(ValueError, match="min.plus, min.times, max.plus and max.times"):
                sparse_amd.semiring_matmul(_stub(cls), b, **kw)
        with pytest.raises(TypeError, match="16-bit"):
            sparse_amd.semiring_matmul(_stub(cls), b.astype(np.float16))
        with pytest.raises(ValueError, match="shape-mismatch"):
            sparse_amd.semiring_matmul(_stub(cls), np.zeros((5, 4), np.float32))
    assert check((5, 6), np.float32, b, "min", "plus", None) == torch.float32
    assert check((5, 6), bool, np.zeros(6, np.int64), "max", "times", torch.zeros(5, dtype=torch.int64)) == torch.int64
    assert check((5, 6), np.int32, torch.zeros(6, 2, dtype=torch.float64), "max", "plus", np.zeros((5, 2))) == torch.float64
    assert check((5, 6), np.int32, np.zeros((6, 0), np.int64), "min", "times", None) == torch.int64
    assert check((5, 6), np.float64, b, "min", "plus", None) == torch.float32                            # same kind: converted
    assert check((5, 6), np.int64, np.zeros((6, 1), np.int32), "min", "plus", None) == torch.int32
    # the dtype rules
    for bdt in (np.float16, np.complex64, np.complex128, np.int16, np.uint8, bool):
        with pytest.raises(TypeError, match="float32, float64, int32 or int64"):
            check((5, 6), np.float32, b.astype(bdt), "min", "plus", None)
    with pytest.raises(TypeError, match="float32, float64, int32 or int64"):
        check((5, 6), np.float32, torch.zeros(6, 4, dtype=torch.bfloat16), "min", "plus", None)
    for adt, bdt in ((np.complex64, np.float32), (np.complex128, np.float64), (np.float16, np.float32), (np.float32, np.int32),
                     (np.float64, np.int64), (np.complex64, np.int64)):
        with pytest.raises(TypeError, match="cannot be converted"):
            check((5, 6), adt, b.astype(bdt), "min", "plus", None)
    for bad in (b.tolist(), 3.0, None):
        with pytest.raises(TypeError, match="NumPy array or a torch tensor"):
            check((5, 6), np.float32, bad, "min", "plus", None)
    with pytest.raises(TypeError, match="NumPy array or a torch tensor"):
        check((5, 6), np.float32, b, "min", "plus", [[0.0] * 4] * 5)
    with pytest.raises(TypeError, match="`init` must have the type"):
        check((5, 6), np.float32, b, "min", "plus", np.zeros((5, 4), np.float64))
    # the shapes of b and init
    for bad in (np.zeros((5, 4), np.float32), np.zeros(5, np.float32), np.zeros((4, 6), np.float32)):
        with pytest.raises(ValueError, match="shape-mismatch"):
            check((5, 6), np.float32, bad, "min", "plus", None)
    for bad in (np.zeros((), np.float32), np.zeros((6, 4, 2), np.float32)):
        with pytest.raises(ValueError, match="1 or 2 dimensions"):
            check((5, 6), np.float32, bad, "min", "plus", None)
    for bad in (np.zeros((5,), np.float32), np.zeros((4, 5), np.float32), np.zeros((5, 4, 1), np.float32), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError, match="shape-mismatch"):
            check((5, 6), np.float32, b, "min", "plus", bad)
    with pytest.raises(ValueError, match="shape-mismatch"):
        check((5, 6), np.float32, b[:, 0], "min", "plus", np.zeros((5, 1), np.float32))


def test_python_argument_errors_of_the_kernel_layer():
    """CPU tensors: every one of these is raised before the layer asks for a device"""
    import torch

    from sparse_amd import _ffi, _kernels as K

    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1])
    vals, b = torch.ones(3), torch.ones(4, 5)
    ok = dict(add="min", mul="plus")
    for kw in (dict(add="sum", mul="plus"), dict(add="min", mul="mul"), dict(add=None, mul=None)):
        with pytest.raises(ValueError, match="min.plus"):
            K.semiring_spmm(indptr, indices, vals, b, 2, **kw)
    for form in ("short", "wide", "row", 1):
        with pytest.raises(ValueError, match="form must be"):
            K.semiring_spmm(indptr, indices, vals, b, 2, form=form, **ok)
    for group in (0, 4, 12, 128, -8):
        with pytest.raises(ValueError, match="group must be"):
            K.semiring_spmm(indptr, indices, vals, b, 2, group=group, **ok)
    for chunk in (0, 32, 100, -64, (1 << 30) + 64, 64.5):
        with pytest.raises(ValueError, match="chunk must be"):
            K.semiring_spmm(indptr, indices, vals, b, 2, chunk=chunk, **ok)
    for bad in (dict(vals=vals.double()), dict(b=b.half(), vals=vals.half()), dict(b=b.to(torch.complex64), vals=vals.to(torch.complex64)),
                dict(init=torch.zeros(2, 5, dtype=torch.float64))):
        args = dict(dict(vals=vals, b=b, init=None), **bad)
        with pytest.raises(TypeError, match="one type"):
            K.semiring_spmm(indptr, indices, args["vals"], args["b"], 2, init=args["init"], **ok)
    with pytest.raises(TypeError, match="int32 or both int64"):
        K.semiring_spmm(indptr.int(), indices, vals, b, 2, **ok)
    with pytest.raises(TypeError, match="int32 or both int64"):
        K.semiring_spmm(indptr.double(), indices.double(), vals, b, 2, **ok)
    with pytest.raises(ValueError, match="1 or 2 dimensions"):
        K.semiring_spmm(indptr, indices, vals, torch.ones(4, 5, 1), 2, **ok)
    with pytest.raises(ValueError, match="shape mismatch"):
        K.semiring_spmm(indptr, indices[:2], vals, b, 2, **ok)
    with pytest.raises(ValueError, match="shape mismatch"):
        K.semiring_spmm(indptr, indices, vals, torch.ones(0, 5), 2, **ok)
    for init in (torch.zeros(2), torch.zeros(5, 2), torch.zeros(2, 5, 1)):
        with pytest.raises(ValueError, match="init must have the result's shape"):
            K.semiring_spmm(indptr, indices, vals, b, 2, init=init, **ok)
    with pytest.raises(ValueError, match="init must have the result's shape"):
        K.semiring_spmm(indptr, indices, vals, b[:, 0], 2, init=torch.zeros(2, 1), **ok)
    with pytest.raises(_ffi.HipBackendError, match="device"):                    # everything is in order: now it wants a device
        K.semiring_spmm(indptr, indices, vals, b, 2, **ok)

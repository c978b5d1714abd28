"""Complex elementwise operations and reductions on the device.

* every case of tests/golden/complex_ew.npz (the reference's own results, tools/gen_complex_ew_golden.py) replayed with the
  HIP backend: structure exact, values bit-identical (NaN sign / payload aside) except `absolute`;
* the same ops against NumPy on the dense twins over a value grid;
* the C ABI called directly (8-byte-aligned complex128 buffers, odd lengths, SPAMD_EINVAL for the host-only ops);
* no host evaluation for the ops of the device list, host evaluation (and NumPy's result) for the others;
* determinism and the summation order at 10^7 stored values against `np.add.reduceat` on the host.

`absolute` is the one ulp-bounded op: hypot(re, im) of the device library against mpmath at 128 bits rounded to the result
type.  Bound 4 ulp (the `hypot` row of the conformance table); measured maximum on this grid: see ABS_ULP.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "complex_ew.npz")
ABS_ULP = {"c8": (4, 1.0), "c16": (4, 1.0)}      # dtype -> (bound, measured maximum on the MI355X)


def _generator():
    spec = importlib.util.spec_from_file_location("gen_complex_ew_golden", os.path.join(ROOT, "tools", "gen_complex_ew_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def sp():
    import sparse_amd

    return sparse_amd


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return z, {k[4:]: z[k] for k in z.files if k.startswith("in__")}


def _npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_values(got, want):
    """bit-identical, component by component; a NaN matches any NaN (sign and payload are not compared)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "c":
        if got.dtype.kind == "f":
            g, w = got.reshape(-1), want.reshape(-1)
            return bool(np.all((np.isnan(g) & np.isnan(w)) | (g.view(f"u{g.itemsize}") == w.view(f"u{w.itemsize}"))))
        return bool(np.array_equal(got, want))
    return same_values(np.ascontiguousarray(got.real), np.ascontiguousarray(want.real)) and \
        same_values(np.ascontiguousarray(got.imag), np.ascontiguousarray(want.imag))


_MP_CACHE = {}
_WORST = {}


def abs_within_bound(got, want_np, z):
    """|z| on the device: special results (non-finite, zero, a non-finite part) are NumPy's exactly, the others within the
    bound of the mpmath value rounded to the result type"""
    import mpmath

    got, want_np, z = np.asarray(got).reshape(-1), np.asarray(want_np).reshape(-1), np.asarray(z).reshape(-1)
    assert got.dtype == want_np.dtype and got.shape == want_np.shape
    key = "c8" if got.dtype == np.float32 else "c16"
    special = ~np.isfinite(want_np) | (want_np == 0) | ~np.isfinite(z.real) | ~np.isfinite(z.imag)
    ok = (np.isnan(got) & np.isnan(want_np)) | (got == want_np)
    assert ok[special].all(), ("absolute", key, z[special & ~ok][:4], got[special & ~ok][:4], want_np[special & ~ok][:4])
    idx = np.flatnonzero(~special)
    if not idx.size:
        return
    ref = np.empty(idx.size, dtype=got.dtype)
    with mpmath.workprec(128):
        for j, k in enumerate(idx):
            ck = (key, z[k].real.tobytes(), z[k].imag.tobytes())
            r = _MP_CACHE.get(ck)
            if r is None:
                r = _MP_CACHE[ck] = np.asarray(float(mpmath.hypot(mpmath.mpf(float(z[k].real)), mpmath.mpf(float(z[k].imag))))).astype(got.dtype)[()]
            ref[j] = r
    g = got[idx]
    assert np.isfinite(g).all() or not np.isfinite(ref[~np.isfinite(g)]).any()
    with np.errstate(all="ignore"):
        err = np.abs(g.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    err = np.where(np.isfinite(ref) | np.isfinite(g), err, 0.0)
    worst = float(np.nanmax(err))
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    print(f"absolute {key}: max ulp distance {worst:.3f} over {idx.size} values (bound {ABS_ULP[key][0]})")
    k = int(np.nanargmax(err))
    assert worst <= ABS_ULP[key][0], ("absolute", key, z[idx][k], g[k], ref[k], worst)


def canonical(sp, r):
    c = r.tocoo() if isinstance(r, sp.GCXS) else r
    data = _npy(c.data)
    coords = _npy(c.coords).astype(np.int64).reshape(len(c.shape), data.size)
    if coords.shape[1]:
        order = np.lexsort(coords[::-1]) if coords.shape[0] else np.arange(coords.shape[1])
        coords, data = coords[:, order], data[order]
    return coords, data


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", GEN.case_names())
def test_fixture_case(sp, gold, name):
    z, I = gold
    fn = dict(GEN.cases())[name]
    with np.errstate(all="ignore"):
        r = fn(sp, I)
    is_abs = name.startswith("absolute_")
    if f"{name}__out" in z.files:
        want = z[f"{name}__out"]
        got = _npy(r.todense()) if isinstance(r, sp.SparseArray) else _npy(r)
        assert got.shape == want.shape and got.dtype == want.dtype, name
        assert same_values(got, want), (name, got, want)
        return
    assert isinstance(r, sp.SparseArray), (name, type(r))
    meta, wfill = z[f"{name}__meta"], z[f"{name}__fill"]
    nnz, fmt, shape = int(meta[0]), int(meta[1]), tuple(int(v) for v in meta[2:])
    if fmt == 2:
        assert isinstance(r, sp.COO), (name, type(r))
    else:
        assert isinstance(r, sp.GCXS), (name, type(r))
        assert (r.compressed_axes[0] if r.compressed_axes else -1) == fmt, (name, r.compressed_axes)
    assert tuple(r.shape) == shape and r.nnz == nnz, (name, r.shape, r.nnz, shape, nnz)
    assert np.dtype(r.dtype) == z[f"{name}__data"].dtype, (name, r.dtype)
    gfill = np.asarray(r.fill_value)
    assert gfill.dtype == wfill.dtype, (name, gfill.dtype, wfill.dtype)
    coords, data = canonical(sp, r)
    assert np.array_equal(coords, z[f"{name}__coords"].reshape(coords.shape)), name
    if is_abs:
        tag = name.rsplit("_", 1)[1]
        src = I[f"b_{tag}"] if "_gcxs_" in name else I[f"a_{tag}"]
        abs_within_bound(data, z[f"{name}__data"], src[tuple(coords)])
        fsrc = np.asarray(-1.5 + 2j if "_fill_" in name else 0).astype(src.dtype)
        abs_within_bound(gfill.reshape(1), wfill.reshape(1), fsrc.reshape(1))
    else:
        assert same_values(gfill, wfill), (name, gfill, wfill)
        assert same_values(data, z[f"{name}__data"]), (name, data[:8], z[f"{name}__data"][:8])


# ---- 2. NumPy on the dense twins ----------------------------------------------------------------------------------------------
def cgrid(dt):
    real = np.float32 if np.dtype(dt) == np.complex64 else np.float64
    fi = np.finfo(real)
    rng = np.random.default_rng(21)
    parts = [0.0, -0.0, 1.0, -1.5, 2.5, float(fi.smallest_subnormal), -float(fi.tiny), 3.0e-5, -7.0e4, float(fi.max), -float(fi.max) / 4,
             np.inf, -np.inf, np.nan] + list((rng.random(4) - 0.5) * 8)
    parts = np.array(parts, dtype=real)
    v = np.empty(parts.size * parts.size, dtype=dt)
    v.real, v.imag = np.repeat(parts, parts.size), np.tile(parts, parts.size)
    return v


BIN_OPS = ("add", "subtract", "multiply", "divide", "true_divide", "equal", "not_equal")
UN_OPS = ("negative", "positive", "conjugate", "conj", "square", "absolute", "abs", "real", "imag", "isnan", "isinf", "isfinite")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", BIN_OPS)
def test_binary_against_numpy(sp, name, dt):
    f = getattr(np, name)
    v = cgrid(dt)
    A, B = np.repeat(v[:, None], v.size, 1), np.repeat(v[None, :], v.size, 0)
    with np.errstate(all="ignore"):
        want = f(A, B)
        a, b = sp.COO.from_numpy(A), sp.COO.from_numpy(B)
        for x, y in ((a, b), (sp.GCXS(a), sp.GCXS(b))):                      # the fused merge on COO keys / on GCXS keys
            r = f(x, y)
            assert np.dtype(r.dtype) == want.dtype
            assert same_values(_npy(r.todense()), want), name
        # scalars on either side (NumPy's array x scalar loop), every grid value as the scalar would be 324 launches: a few
        for s in (v[5], v[40], v[200], dt(2j), 2j, 3, 0.5):
            assert same_values(_npy(f(a, s).todense()), f(A, s)), (name, s)
            assert same_values(_npy(f(s, a).todense()), f(s, A)), (name, s)
        # sparse with dense: the result is dense when func(fill, dense) is not constant
        r = f(a, B)
        assert same_values(_npy(r.todense()) if isinstance(r, sp.SparseArray) else _npy(r), want), name


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", UN_OPS)
def test_unary_against_numpy(sp, name, dt):
    f = getattr(np, name)
    v = cgrid(dt)
    X = np.tile(v, (3, 1))
    with np.errstate(all="ignore"):
        want = f(X)
        for fv in (0, 1.5 - 2j):
            x = sp.COO.from_numpy(X, fill_value=dt(fv))
            for arr in (x, sp.GCXS(x)):
                r = f(arr)
                assert np.dtype(r.dtype) == want.dtype, (name, r.dtype)
                got = _npy(r.todense())
                if name in ("absolute", "abs"):
                    abs_within_bound(got, want, X)
                else:
                    assert same_values(got, want), name
                    assert same_values(np.asarray(r.fill_value), np.asarray(f(dt(fv)))), name


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_mixed_operands_promote_as_numpy(sp, dt):
    v = cgrid(dt)[:300].reshape(15, 20)
    rng = np.random.default_rng(3)
    real = np.float32 if dt == np.complex64 else np.float64
    R = np.where(rng.random((15, 20)) < 0.6, rng.random((15, 20)) - 0.5, 0).astype(real)
    Ii = rng.integers(-3, 4, (15, 20))
    Bo = rng.random((15, 20)) < 0.5
    x = sp.COO.from_numpy(v)
    with np.errstate(all="ignore"):
        for other, O in ((sp.COO.from_numpy(R), R), (sp.COO.from_numpy(Ii), Ii), (sp.COO.from_numpy(Bo), Bo)):
            for f in (np.add, np.multiply, np.subtract, np.divide, np.equal):
                for got, want in ((f(x, other), f(v, O)), (f(other, x), f(O, v))):
                    assert np.dtype(got.dtype) == want.dtype
                    assert same_values(_npy(got.todense()), want), (f.__name__, O.dtype)
        r = sp.COO.from_numpy(R)
        for s in (2j, dt(1 - 1j), np.complex128(0.5 + 0.25j)):
            for f in (np.multiply, np.add, np.divide):
                got, want = f(r, s), f(R, s)
                assert np.dtype(got.dtype) == want.dtype, (f.__name__, s, got.dtype, want.dtype)       # NEP 50: 2j keeps the narrow type
                assert same_values(_npy(got.todense()), want), (f.__name__, s)
        for target in (np.complex64, np.complex128):
            assert same_values(_npy(x.astype(target).todense()), v.astype(target))
            assert same_values(_npy(r.astype(target).todense()), R.astype(target))
        # where() with complex values (16-byte select)
        got = sp.where(sp.COO.from_numpy(Bo), x, sp.COO.from_numpy(v.T.copy().reshape(15, 20)))
        assert same_values(_npy(got.todense()), np.where(Bo, v, v.T.copy().reshape(15, 20)))


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 4099])
@pytest.mark.parametrize("shift", [0, 1])
def test_c_abi_value_kernels(hiplib, dt, n, shift):
    """`shift` = 1 starts every complex buffer one 8-byte word into its allocation: complex128 arrays that are 8-byte aligned
    only, complex64 arrays that start in the middle of a 16-byte packet"""
    from sparse_amd import _ffi

    d = torch.device("cuda", 0)
    code = _ffi.C64 if dt == np.complex64 else _ffi.C128
    v = cgrid(dt)
    rng = np.random.default_rng(n)
    a, b = v[rng.integers(0, v.size, n)], v[rng.integers(0, v.size, n)]
    real_t = torch.float32 if dt == np.complex64 else torch.float64

    class dev:     # a device copy of `arr` that starts `shift` 8-byte words into its buffer (torch cannot view such memory as complex)
        def __init__(self, arr):
            words = np.ascontiguousarray(arr).view(np.float64).copy()
            self.n = words.size
            self.buf = torch.zeros(self.n + 4, dtype=torch.float64, device=d)
            self.buf[shift:shift + self.n].copy_(torch.from_numpy(words))
            assert self.data_ptr() % 16 == (8 * shift) % 16

        def data_ptr(self):
            return self.buf.data_ptr() + 8 * shift

        def numpy(self):
            return self.buf[shift:shift + self.n].cpu().numpy().view(dt)

    ta, tb = dev(a), dev(b)
    s = torch.cuda.current_stream().cuda_stream
    with np.errstate(all="ignore"):
        for op, f in ((0, np.add), (1, np.subtract), (2, np.multiply), (3, np.divide)):
            out = dev(np.zeros(n, dt))
            assert hiplib.spamd_cplx_binary(op, code, n, ta.data_ptr(), 0, tb.data_ptr(), 0, out.data_ptr(), s) == 0
            assert same_values(out.numpy(), f(a, b)), (op, n, shift)
            assert hiplib.spamd_cplx_binary(op, code, n, ta.data_ptr(), 0, tb.data_ptr(), 1, out.data_ptr(), s) == 0
            assert same_values(out.numpy(), f(a, b[0])), (op, n, shift, "scalar b")
            assert hiplib.spamd_cplx_binary(op, code, n, ta.data_ptr(), 1, tb.data_ptr(), 0, out.data_ptr(), s) == 0
            assert same_values(out.numpy(), f(a[0], b)), (op, n, shift, "scalar a")
        for op, f in ((36, np.equal), (37, np.not_equal)):
            out = torch.zeros(n, dtype=torch.uint8, device=d)
            assert hiplib.spamd_cplx_binary(op, code, n, ta.data_ptr(), 0, ta.data_ptr(), 0, out.data_ptr(), s) == 0
            assert np.array_equal(_npy(out).astype(bool), f(a, a))
        for op, f in ((0, np.negative), (20, np.square), (22, np.positive), (96, np.conjugate)):
            out = dev(np.zeros(n, dt))
            assert hiplib.spamd_cplx_unary(op, code, n, ta.data_ptr(), out.data_ptr(), s) == 0
            assert same_values(out.numpy(), f(a)), (op, n, shift)
        for op, f in ((97, np.real), (98, np.imag)):
            out = torch.zeros(n, dtype=real_t, device=d)
            assert hiplib.spamd_cplx_unary(op, code, n, ta.data_ptr(), out.data_ptr(), s) == 0
            assert same_values(_npy(out), np.ascontiguousarray(f(a)))
        out = torch.zeros(n, dtype=real_t, device=d)
        assert hiplib.spamd_cplx_unary(1, code, n, ta.data_ptr(), out.data_ptr(), s) == 0
        abs_within_bound(_npy(out), np.abs(a), a)
        for op, f in ((64, np.isnan), (65, np.isinf), (66, np.isfinite)):
            out = torch.zeros(n, dtype=torch.uint8, device=d)
            assert hiplib.spamd_cplx_unary(op, code, n, ta.data_ptr(), out.data_ptr(), s) == 0
            assert np.array_equal(_npy(out).astype(bool), f(a))
        # conversions
        other = np.complex128 if dt == np.complex64 else np.complex64
        out = torch.zeros(n, dtype=torch.complex128 if dt == np.complex64 else torch.complex64, device=d)
        assert hiplib.spamd_cplx_convert(code, _ffi.C128 if dt == np.complex64 else _ffi.C64, n, ta.data_ptr(), out.data_ptr(), s) == 0
        assert same_values(_npy(out), a.astype(other))
        ints = torch.arange(-2, n - 2, dtype=torch.int64, device=d)
        out = dev(np.zeros(n, dt))
        assert hiplib.spamd_cplx_convert(_ffi.I64, code, n, ints.data_ptr(), out.data_ptr(), s) == 0
        assert same_values(out.numpy(), np.arange(-2, n - 2).astype(dt))
    # the ops that stay on the host are refused, not approximated; so are real dtypes
    out = dev(np.zeros(n, dt))
    for op in (4, 5, 6, 7, 8, 32, 33, 34, 35, 38, 39, 40):      # maximum, minimum, power, fmax, fmin, the ordered comparisons, logical_*
        assert hiplib.spamd_cplx_binary(op, code, n, ta.data_ptr(), 0, tb.data_ptr(), 0, out.data_ptr(), s) == -1
    for op in (2, 3, 5, 7, 19, 21):                              # sqrt, exp, log, sin, sign, reciprocal
        assert hiplib.spamd_cplx_unary(op, code, n, ta.data_ptr(), out.data_ptr(), s) == -1
    assert hiplib.spamd_cplx_binary(0, _ffi.F64, n, ta.data_ptr(), 0, tb.data_ptr(), 0, out.data_ptr(), s) == -2
    assert hiplib.spamd_cplx_segment_reduce(2, code, n, ta.data_ptr(), 0, 1, 0, out.data_ptr(), s) == -1      # maximum
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_c_abi_reductions(hiplib, dt):
    """runs of every length 1..140 and a few long ones, sum in reduceat's order (both entry points) and the product"""
    from sparse_amd import _ffi
    from sparse_amd._reduce import pairwise_order_sum

    d = torch.device("cuda", 0)
    code = _ffi.C64 if dt == np.complex64 else _ffi.C128
    lengths = list(range(1, 141)) + [255, 256, 257, 513, 1000, 4097, 20_001, 70_000]
    rng = np.random.default_rng(5)
    starts = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n = int(starts[-1])
    x = ((rng.standard_normal(n) * 4) + 1j * rng.standard_normal(n)).astype(dt)
    tx, ts = torch.from_numpy(x).to(d), torch.from_numpy(starts).to(d)
    s = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(len(lengths), dtype=tx.dtype, device=d)
    assert hiplib.spamd_cplx_segment_reduce(0, code, n, tx.data_ptr(), ts.data_ptr(), len(lengths), 0, out.data_ptr(), s) == 0
    want = np.add.reduceat(x, starts[:-1])
    got = _npy(out)
    bad = [lengths[g] for g in range(len(lengths)) if got[g].tobytes() != want[g].tobytes()]
    assert not bad, ("run lengths that differ from np.add.reduceat", bad[:10])
    for g in (3, 64, 65, 130):       # the arbiter where NumPy on this host is only the second witness
        assert got[g].tobytes() == pairwise_order_sum(x[starts[g]:starts[g + 1]]).tobytes()
    esz = x.itemsize
    for g, m in enumerate(lengths):
        if m in (2, 66, 67, 130, 257, 1000, 4097, 20_001, 70_000):
            one = torch.zeros(1, dtype=tx.dtype, device=d)
            wsb = int(hiplib.spamd_cplx_sum_long_ws_bytes(m))
            ws = torch.zeros(wsb, dtype=torch.uint8, device=d)
            assert hiplib.spamd_cplx_sum_long(code, m, tx.data_ptr() + int(starts[g]) * esz, one.data_ptr(), ws.data_ptr(), wsb, s) == 0
            assert _npy(one)[0].tobytes() == want[g].tobytes(), ("spamd_cplx_sum_long", m)
    assert hiplib.spamd_cplx_sum_long(code, 1000, tx.data_ptr(), out.data_ptr(), ws.data_ptr(), 8, s) == -3
    # the product: left to right, unfused
    small = np.concatenate(([0], np.cumsum([1, 2, 7, 8, 9, 64, 129, 300]))).astype(np.int64)
    y = (x[: small[-1]] / 2 + dt(0.9)).astype(dt)
    ty, tss = torch.from_numpy(y).to(d), torch.from_numpy(small).to(d)
    out = torch.zeros(len(small) - 1, dtype=tx.dtype, device=d)
    assert hiplib.spamd_cplx_segment_reduce(1, code, int(small[-1]), ty.data_ptr(), tss.data_ptr(), len(small) - 1, 0, out.data_ptr(), s) == 0
    with np.errstate(all="ignore"):
        assert same_values(_npy(out), np.multiply.reduceat(y, small[:-1]))


# ---- 4. nothing is evaluated on the host ----------------------------------------------------------------------------------
@pytest.fixture
def host_counter(monkeypatch):
    """Counts evaluations on the host: the general elementwise route (ufuncs), the host reduction, the tracer's fallbacks;
    and the names of the C-ABI entry points called."""
    import sparse_amd as spm
    from sparse_amd import _ffi, _reduce, _umath

    ew, red, abi = [], [], []
    orig_e, orig_r, orig_c = _umath._elemwise_general, _reduce._reduce_on_host, _ffi.call

    def counting_e(func, *a, **k):
        if isinstance(func, np.ufunc) or func in (np.real, np.imag):
            ew.append(getattr(func, "__name__", str(func)))
        return orig_e(func, *a, **k)

    def counting_r(x, method, *a, **k):
        red.append(method.__name__)
        return orig_r(x, method, *a, **k)

    def counting_c(name, *a):
        abi.append(name)
        return orig_c(name, *a)

    monkeypatch.setattr(_umath, "_elemwise_general", counting_e)
    monkeypatch.setattr(_reduce, "_reduce_on_host", counting_r)
    monkeypatch.setattr(_ffi, "call", counting_c)

    def snapshot():
        return len(ew), len(red), {k: v for k, v in spm.fallback_stats().items() if k != "recent"}

    snapshot.abi = abi
    snapshot.ew, snapshot.red = ew, red
    return snapshot


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_no_host_evaluation(sp, host_counter, dt):
    rng = np.random.default_rng(9)
    shape = (30, 40)
    X = np.where(rng.random(shape) < 0.4, rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5), 0).astype(dt)
    Y = np.where(rng.random(shape) < 0.4, rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5), 0).astype(dt)
    R = np.where(rng.random(shape) < 0.4, rng.random(shape), 0)
    D = (rng.random(shape) + 1j * rng.random(shape)).astype(dt)
    x, y, r = sp.COO.from_numpy(X), sp.COO.from_numpy(Y), sp.COO.from_numpy(R)
    row = sp.COO.from_numpy(Y[:1])
    gx, gy, gc = sp.GCXS(x), sp.GCXS(y), sp.GCXS(x, compressed_axes=(1,))
    n0 = host_counter()
    with np.errstate(all="ignore"):
        for f in (np.add, np.subtract, np.multiply, np.divide, np.true_divide, np.equal, np.not_equal):
            f(x, y), f(x, row), f(x, 2j), f(0.5 - 1j, x), f(x, r), f(r, x), f(gx, gy), f(gc, 1.5), f(gx, gc), f(x, 3)
        x * D, D[:1] * x, x / D, r * 2j, r + dt(1j)
        for f in (np.negative, np.positive, np.conjugate, np.conj, np.square, np.absolute, np.abs, np.real, np.imag, np.isnan,
                  np.isinf, np.isfinite):
            f(x), f(gx), f(gc)
        x.real, x.imag, x.conj(), abs(x), -x, gx.real
        x.astype(np.complex128), x.astype(np.complex64), r.astype(dt)
        sp.elemwise(lambda u, v: (u - v) * u + 2j, x, y)
        sp.elemwise(lambda u: np.conj(u) * u - u / 3, x)
        xf = sp.COO.from_numpy(X, fill_value=dt(0.5 - 0.25j))
        x1 = sp.COO.from_numpy(np.where(X == 0, 1, X).astype(dt), fill_value=dt(1))
        for a in (x, gx, gc, xf):
            a.sum(), a.sum(axis=0), a.sum(axis=1), a.sum(axis=(0, 1), keepdims=True), a.mean(axis=0), a.mean()
        x.prod(axis=0), x.prod(), x1.prod(axis=1), gx.prod(axis=1), sp.nansum(x, axis=0)
        np.add.reduce(x, axis=1, dtype=dt)
    assert host_counter() == n0, ("evaluated on the host", host_counter.ew, host_counter.red, host_counter())
    assert any(c.startswith("spamd_cplx_") for c in host_counter.abi) and "spamd_merge_union_complex" in host_counter.abi
    assert "spamd_cplx_segment_reduce" in host_counter.abi
    # the host-only functions still arrive on the host path and still give NumPy's result
    with np.errstate(all="ignore"):
        for f in (np.exp, np.sqrt, np.sign, np.reciprocal, np.log1p):
            before = len(host_counter.ew)
            got = f(x)
            assert len(host_counter.ew) == before + 1, f.__name__
            assert same_values(_npy(got.todense()), f(X)), f.__name__
        for f in (np.power, np.maximum, np.minimum, np.greater, np.less_equal, np.logical_and, np.logical_or):
            before = len(host_counter.ew)
            got = f(x, y)
            assert len(host_counter.ew) == before + 1, f.__name__
            assert same_values(_npy(got.todense()), f(X, Y)), f.__name__
        before = len(host_counter.red)
        got = (x + dt(1 + 0.5j)).prod(axis=0)          # a multiply reduction with a fill value that is neither 0 nor 1
        np.maximum.reduce(x, axis=0)
        np.add.reduce(x, axis=0, dtype=np.complex128 if dt == np.complex64 else np.complex64)
        assert len(host_counter.red) == before + 3
        assert np.allclose(_npy(got.todense()), (X + dt(1 + 0.5j)).prod(axis=0), rtol=1e-4, equal_nan=True)


@pytest.mark.gpu
def test_real_operands_never_reach_the_complex_kernels(sp, host_counter):
    rng = np.random.default_rng(10)
    X = np.where(rng.random((30, 40)) < 0.4, rng.random((30, 40)), 0)
    x, y = sp.COO.from_numpy(X), sp.COO.from_numpy(X.T.copy().reshape(30, 40))
    x + y, x * y, x * 2.0, abs(x), x.sum(axis=0), x.sum(), sp.GCXS(x) + sp.GCXS(y), x.astype(np.float32), np.isnan(x)
    sp.elemwise(lambda u, v: u * v + 1, x, y)
    assert not [c for c in host_counter.abi if "cplx" in c or "complex" in c]


# ---- 5. determinism and the order at size ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_large_sums_equal_reduceat_and_repeat(sp, dt):
    n, runs = 10_000_000, 100_000
    rng = np.random.default_rng(77)
    real = np.float32 if dt == np.complex64 else np.float64
    v = np.empty(n, dtype=dt)
    v.real, v.imag = rng.standard_normal(n, dtype=real), rng.standard_normal(n, dtype=real)
    v[v == 0] = 1
    # one run: a 1-D array summed whole; 10^5 runs: (runs, n / runs) summed over its second axis
    one = sp.COO(np.arange(n, dtype=np.int64)[None, :], v, shape=(n,))
    many = sp.COO(np.stack([np.arange(n) // (n // runs), np.arange(n) % (n // runs)]).astype(np.int64), v, shape=(runs, n // runs))
    g1, g2 = one.sum(), one.sum()
    a1, a2 = np.asarray(g1.todense()), np.asarray(g2.todense())
    assert a1.tobytes() == a2.tobytes()
    want_one = np.add.reduceat(v, [0])[0]
    print(f"{np.dtype(dt).name}: one run of 10^7: device {a1[()]!r}, reduceat {want_one!r}")
    assert a1.dtype == want_one.dtype and a1.tobytes() == want_one.tobytes()
    m1, m2 = many.sum(axis=1), many.sum(axis=1)
    d1, d2 = _npy(m1.todense()), _npy(m2.todense())
    assert d1.tobytes() == d2.tobytes()
    want_many = np.add.reduceat(v, np.arange(0, n, n // runs))
    assert d1.tobytes() == want_many.tobytes(), int((d1 != want_many).sum())
    e1, e2 = (one * one), (one * one)
    assert _npy(e1.data).tobytes() == _npy(e2.data).tobytes()
    with np.errstate(all="ignore"):
        assert same_values(_npy(e1.data), v * v)

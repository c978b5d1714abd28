"""Ufunc conformance: every device elementwise op (`_umath._BIN`, `_umath._UN`) and the reductions, on every dtype the device
computes, at the values where kernels go wrong (signed zeros, denormals, the float integer limits, ±max, ±inf, NaN, integer
extremes, u8 / bool operands), through every path that reaches the kernels: the kernel-level wrappers, the fused merge, the
union + value kernel, sparse (x) scalar, sparse (x) dense (same shape and broadcast row), GCXS operands and traced lambdas.

The reference is NumPy on the dense twins.  Ops of the `ULP` class are compared with mpmath (128 bits, rounded to the target
dtype) instead, within the bound of `TABLE`; every other op must match NumPy bit for bit (`EXACT`).  These exceptions are
the only ones granted:
  - the sign and payload of a NaN are not compared (x86 and the device produce different NaN bits for the same invalid op);
  - the sign of a zero produced by a ±0 tie of maximum / minimum / fmax / fmin is not compared (NumPy's own scalar and array
    loops disagree on it: np.maximum(0.0, -0.0) is -0.0, the SIMD array loop may return either operand);
  - a sparse result of sparse (x) dense stands for func(fill, dense) with ONE fill value, judged constant with == as the
    reference does: where that is a zero of either sign (copysign(0, ±y)) the sign of the zero is not compared (`check`).
"""
import math
import warnings

import numpy as np
import pytest
import torch

from sparse_amd import _umath

EXACT = "exact"
# name -> EXACT, or {dtype: (bound in ulp, measured maximum on the MI355X)} for the ulp-bounded class.  The measured maxima are
# over the value grid below (every path: they all evaluate one kernel); refresh them with SPARSE_AMD_ULP_REPORT=<file>.
TABLE = {
    # binary
    "add": EXACT, "subtract": EXACT, "multiply": EXACT, "divide": EXACT, "true_divide": EXACT,
    "maximum": EXACT, "minimum": EXACT, "fmax": EXACT, "fmin": EXACT,
    "greater": EXACT, "greater_equal": EXACT, "less": EXACT, "less_equal": EXACT, "equal": EXACT, "not_equal": EXACT,
    "logical_and": EXACT, "logical_or": EXACT, "logical_xor": EXACT,
    "bitwise_and": EXACT, "bitwise_or": EXACT, "bitwise_xor": EXACT, "left_shift": EXACT, "right_shift": EXACT,
    "floor_divide": EXACT, "remainder": EXACT, "mod": EXACT, "fmod": EXACT, "copysign": EXACT,
    "power": {"f4": (4, 1), "f8": (4, 1)},           # (integer power: exact, by squaring)
    "float_power": {"f8": (4, 1)},
    "hypot": {"f4": (4, 1), "f8": (4, 1)},
    "arctan2": {"f4": (4, 2), "f8": (4, 1)},
    # unary
    "negative": EXACT, "absolute": EXACT, "abs": EXACT, "fabs": EXACT, "positive": EXACT,
    "conjugate": EXACT, "conj": EXACT, "real": EXACT,
    "floor": EXACT, "ceil": EXACT, "rint": EXACT, "trunc": EXACT, "sign": EXACT, "square": EXACT, "reciprocal": EXACT,
    "sqrt": EXACT,                                          # correctly rounded (the build uses -ffp-contract=off)
    "deg2rad": EXACT, "radians": EXACT, "rad2deg": EXACT, "degrees": EXACT,   # one multiply by NumPy's constant
    "isnan": EXACT, "isinf": EXACT, "isfinite": EXACT, "logical_not": EXACT, "signbit": EXACT,
    "exp": {"f4": (2, 1), "f8": (2, 0)},
    "expm1": {"f4": (2, 1), "f8": (2, 0)},
    "exp2": {"f4": (2, 1), "f8": (2, 1)},
    "log": {"f4": (2, 1), "f8": (2, 1)},
    "log1p": {"f4": (2, 0), "f8": (2, 1)},
    "log2": {"f4": (2, 1), "f8": (2, 0)},
    "log10": {"f4": (2, 1), "f8": (2, 1)},
    "sin": {"f4": (2, 1), "f8": (2, 1)},
    "cos": {"f4": (2, 1), "f8": (2, 0)},
    "tan": {"f4": (4, 1), "f8": (4, 1)},
    "arcsin": {"f4": (2, 0), "f8": (2, 0)},
    "arctan": {"f4": (2, 1), "f8": (2, 1)},
    "sinh": {"f4": (2, 1), "f8": (2, 1)},
    "cosh": {"f4": (2, 0), "f8": (2, 0)},
    "tanh": {"f4": (2, 1), "f8": (2, 1)},
    "arcsinh": {"f4": (2, 0), "f8": (2, 0)},
    "arctanh": {"f4": (2, 1), "f8": (2, 0)},
    "cbrt": {"f4": (2, 1), "f8": (2, 0)},
}
_TIE_ZERO_SIGN_FREE = {"maximum", "minimum", "fmax", "fmin"}
DTYPES = ["f4", "f8", "i4", "i8", "u1", "?"]


def test_exactness_table_covers_every_device_op():
    """A new device op without a declared exactness class fails here (CPU test)."""
    assert set(TABLE) == set(_umath._BIN) | set(_umath._UN)
    for name, cls in TABLE.items():
        if cls != EXACT:
            for dt, (bound, _measured) in cls.items():
                assert dt in ("f4", "f8") and 1 <= bound <= 4, (name, dt)


# ---- value grid ------------------------------------------------------------------------------------------------------
def grid(dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        fi = np.finfo(dt)
        big = 2.0 ** (24 if dt == np.float32 else 53)
        tiny_den = float(fi.smallest_subnormal)
        mag = [0.0, tiny_den, float(fi.tiny) - tiny_den, float(fi.tiny), 0.5, 1.0, 1.5, 2.5,
               big, float(np.nextafter(dt.type(big), dt.type(0))), float(np.nextafter(dt.type(big), dt.type(np.inf))),
               float(fi.max), math.inf]
        rng = np.random.default_rng(11)
        lo, hi = (-140, 120) if dt == np.float32 else (-1060, 1000)
        seeded = list(rng.random(12) * 2.0 ** rng.integers(lo, hi, 12).astype(np.float64))
        seeded += list(rng.random(6) * 4 - 2)       # the interesting range of the trig / inverse functions
        vals = [s * m for m in mag + seeded for s in (1.0, -1.0)] + [math.nan]
        with np.errstate(all="ignore"):
            return np.array(vals, dtype=np.float64).astype(dt)
    if dt.kind == "i":
        ii = np.iinfo(dt)
        rng = np.random.default_rng(12)
        return np.array([0, 1, -1, 2, -2, ii.min, ii.min + 1, ii.max, ii.max - 1] + list(rng.integers(-1000, 1000, 5))
                        + list(rng.integers(ii.min, ii.max, 5)), dtype=dt)
    if dt.kind == "u":
        return np.array([0, 1, 127, 128, 255], dtype=dt)
    return np.array([True, False])


def cross(dt):
    v = grid(dt)
    return np.repeat(v[:, None], v.size, 1), np.repeat(v[None, :], v.size, 0)


# ---- comparison ------------------------------------------------------------------------------------------------------
_MP = {"exp": "exp", "expm1": "expm1", "log": "log", "log1p": "log1p", "sin": "sin", "cos": "cos", "tan": "tan",
       "sinh": "sinh", "cosh": "cosh", "tanh": "tanh", "arcsin": "asin", "arctan": "atan", "arcsinh": "asinh",
       "arctanh": "atanh", "hypot": "hypot"}
_MEASURED = {}     # (op, dtype) -> the largest ulp distance seen; SPARSE_AMD_ULP_REPORT=<file> writes it as JSON at the end


@pytest.fixture(scope="module", autouse=True)
def _ulp_report():
    yield
    import json
    import os

    path = os.environ.get("SPARSE_AMD_ULP_REPORT")
    if path and _MEASURED:
        with open(path, "w") as fh:
            json.dump({f"{k[0]}|{k[1]}": v for k, v in sorted(_MEASURED.items())}, fh, indent=1)


def _mp_value(name, args):
    import mpmath

    with mpmath.workprec(128):
        x = [mpmath.mpf(float(a)) for a in args]
        if name in _MP:
            return getattr(mpmath, _MP[name])(*x)
        if name == "log2":
            return mpmath.log(x[0], 2)
        if name == "log10":
            return mpmath.log10(x[0])
        if name == "exp2":
            return mpmath.power(2, x[0])
        if name == "cbrt":
            return mpmath.cbrt(abs(x[0])) * (1 if x[0] >= 0 else -1)
        if name in ("power", "float_power"):
            if not mpmath.isfinite(x[1]) or abs(x[0]) == 1 and not mpmath.isfinite(x[1]):
                return mpmath.mpf(1) if abs(x[0]) == 1 else mpmath.power(abs(x[0]), x[1])
            if x[0] < 0:          # (a finite result means an integral exponent: its parity gives the sign)
                return mpmath.power(-x[0], x[1]) * (-1 if int(x[1]) % 2 else 1)
            return mpmath.power(x[0], x[1])
        if name == "arctan2":
            return mpmath.atan2(x[0], x[1])
    raise KeyError(name)


_MP_CACHE = {}


def _mp_rounded(name, dt, args):
    key = (name, dt.str) + tuple((np.asarray(a).dtype.str, np.asarray(a).tobytes()) for a in args)
    r = _MP_CACHE.get(key)
    if r is None:
        r = _MP_CACHE[key] = np.asarray(float(_mp_value(name, args))).astype(dt)[()]
    return r


def _ulp_check(name, got, want_np, args):
    """got / want_np: arrays of the result dtype; args: the operand arrays (same shape).  Special results (NumPy's result
    non-finite or zero, or a non-finite or zero operand) must match NumPy exactly (NaN-ness, inf and its sign, the sign of zero); the others are within the
    table's bound of the mpmath value."""
    dt = np.dtype(want_np.dtype)
    key = "f4" if dt == np.float32 else "f8"
    bound = TABLE[name][key][0]
    args = [np.broadcast_to(a, want_np.shape).reshape(-1) for a in args]
    got, want_np = got.reshape(-1), want_np.reshape(-1)
    special = ~np.isfinite(want_np) | (want_np == 0)
    for a in args:           # (C99 Annex F special cases such as pow(inf, 0) and atan2(0, -0): NumPy's value exactly)
        special |= ~np.isfinite(a) | (a == 0)
    nan_w, nan_g = np.isnan(want_np), np.isnan(got)
    assert np.array_equal(nan_w, nan_g), (name, dt, "NaN", [a[nan_w != nan_g][:4] for a in args])
    sp_ok = nan_w | ((got == want_np) & (np.signbit(got) == np.signbit(want_np)))
    bad = special & ~sp_ok
    assert not bad.any(), (name, dt, "special value", [a[bad][:4] for a in args], got[bad][:4], want_np[bad][:4])
    idx = np.flatnonzero(~special)
    if not idx.size:
        return
    ref_t = np.array([_mp_rounded(name, dt, tuple(a[k] for a in args)) for k in idx], dtype=dt)
    g = got[idx]
    fin = np.isfinite(g)
    assert fin.all(), (name, dt, "non-finite result", [a[idx][~fin][:4] for a in args], g[~fin][:4])
    with np.errstate(all="ignore"):
        err = np.abs(g.astype(np.float64) - ref_t.astype(np.float64)) / np.spacing(np.abs(ref_t)).astype(np.float64)
    worst = float(err.max())
    _MEASURED[(name, key)] = max(_MEASURED.get((name, key), 0.0), worst)
    k = int(np.argmax(err))
    assert worst <= bound, (name, dt, [a[idx][k] for a in args], g[k], ref_t[k], worst)


def check(name, got, want, args=None, loose_zero=False):
    """`got` (sparse result, dense device / host array) against NumPy's `want` (dense ndarray) on the dense twins.
    `loose_zero`: a sparse result of sparse (x) dense, whose fill value is func(fill, dense) judged constant with == (the
    reference's `_get_fill_value`, deliberately kept): where func(fill, dense) is a zero of either sign the result holds the
    fill's zero, so the sign of zeros is not compared there (copysign(0, -1) = -0.0 and copysign(0, 1) = 0.0 share one fill)."""
    sparse_result = hasattr(got, "fill_value")
    if hasattr(got, "todense"):
        gd = got.todense()
    elif isinstance(got, torch.Tensor):
        gd = got.cpu().numpy()
    else:
        gd = np.asarray(got)
    want = np.asarray(want)
    assert gd.dtype == want.dtype, (name, gd.dtype, want.dtype)
    assert gd.shape == want.shape, (name, gd.shape, want.shape)
    if want.dtype.kind != "f":
        assert np.array_equal(gd, want), (name, want.dtype, np.argwhere(gd != want)[:4])
        return
    if TABLE[name] != EXACT and args is not None:
        _ulp_check(name, gd, want, args)
        return
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(gd)), (name, want.dtype, "NaN positions")
    same = (gd == want) | nan
    assert same.all(), (name, want.dtype, np.argwhere(~same)[:4])
    sign = nan | (np.signbit(gd) == np.signbit(want))
    if name in _TIE_ZERO_SIGN_FREE or (loose_zero and sparse_result):
        sign |= want == 0
    assert sign.all(), (name, want.dtype, "sign of zero", np.argwhere(~sign)[:4])


def check_fill(name, got, want_fill, fill_args):
    if not hasattr(got, "fill_value"):
        return
    fv, wf = np.asarray(got.fill_value), np.asarray(want_fill)
    assert fv.dtype == wf.dtype, (name, "fill dtype", fv.dtype, wf.dtype)
    if wf.dtype.kind == "f" and np.isnan(wf):
        assert np.isnan(fv), (name, fv, wf)
    elif wf.dtype.kind == "f" and TABLE[name] != EXACT:
        _ulp_check(name, fv.reshape(1), wf.reshape(1), [np.asarray(a).reshape(1) for a in fill_args])
    else:
        assert fv == wf and (wf.dtype.kind != "f" or name in _TIE_ZERO_SIGN_FREE or np.signbit(fv) == np.signbit(wf)), \
            (name, fv, wf)


def np_call(f, *args):
    """(result, exception type) of a NumPy call."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return f(*args), None
        except (TypeError, ValueError, OverflowError) as e:
            return None, type(e)


def sp_call(f, *args):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*args)


def same_call(name, f, want_args, got_args, uargs=None, fill_args=None, loose_zero=False):
    """NumPy on want_args, the library on got_args: same exception type, or the same values / dtype / fill value."""
    want, err = np_call(f, *want_args)
    if err is not None:
        with pytest.raises(err):
            sp_call(f, *got_args)
        return
    got = sp_call(f, *got_args)
    check(name, got, want, uargs, loose_zero)
    if fill_args is not None:
        wf, ferr = np_call(f, *fill_args)
        if ferr is None:
            check_fill(name, got, wf, fill_args)


# ---- which combinations are DECLARED host-evaluated ---------------------------------------------------------------------
_NARROW_HOST_BIN = {"floor_divide", "remainder", "mod", "fmod", "left_shift", "right_shift"}


def host_expected_binary(name, dt):
    """The device computes f4 / f8 / i4 / i8 for everything NumPy defines; u8 and bool operands only where NumPy's result is
    bool, u8, f4 or f8 and the op is not one of the late value kernels instantiated for f4 / f8 / i4 / i8 alone."""
    if np.dtype(dt).kind in "fi":
        return False
    a, _ = cross(dt)
    r, err = np_call(getattr(np, name), a[:1, :1], a[:1, :1])
    if err is not None:
        return True
    return r.dtype.str not in ("|b1", "|u1", "<f4", "<f8") or name in _NARROW_HOST_BIN


def host_expected_unary(name, dt):
    """Declared host: NumPy results of a type the kernel does not compute (float16 from u8 / bool, int8 from bool) and
    integer reciprocal (NumPy's 1.0 / x cast back to the integer type)."""
    r, err = np_call(getattr(np, name), grid(dt)[:1])
    if err is not None:
        return True
    return r.dtype.str in ("<f2", "|i1") or (name == "reciprocal" and np.dtype(dt).kind in "iub")


@pytest.fixture
def host_counter(monkeypatch):
    """Counts evaluations on the host: the general elementwise route and the tracer's fallbacks."""
    import sparse_amd as sp

    calls = []
    orig = _umath._elemwise_general

    def counting(func, *a, **k):
        if isinstance(func, np.ufunc):      # (a ufunc on the general route is evaluated by NumPy; callables are traced first)
            calls.append(func.__name__)
        return orig(func, *a, **k)

    monkeypatch.setattr(_umath, "_elemwise_general", counting)

    def snapshot():
        return len(calls), {k: v for k, v in sp.fallback_stats().items() if k != "recent"}

    return snapshot


# ---- binary -------------------------------------------------------------------------------------------------------------
_SCALARS = {"f": [0.0, -0.0, 1.5, -2.5, math.inf, math.nan], "i": ["min", -1, 0, 2], "u": [0, 255], "b": [True, False]}


def _scalars(dt):
    dt = np.dtype(dt)
    out = []
    for s in _SCALARS[dt.kind]:
        if s == "min":
            s = np.iinfo(dt).min
        out.append(dt.type(s))
    return out


def _fills(dt):
    """(fill_a, fill_b) pairs: zero fills, a non-zero fill on one side, a NaN fill on the other (floats)."""
    dt = np.dtype(dt)
    z = dt.type(0)
    if dt.kind == "f":
        return [(z, z), (dt.type(1.5), z), (z, dt.type(np.nan)), (dt.type(-np.inf), dt.type(2.5))]
    if dt.kind == "i":
        return [(z, z), (dt.type(-1), z), (z, dt.type(2))]
    if dt.kind == "u":
        return [(z, z), (dt.type(255), dt.type(1))]
    return [(z, z), (np.True_, np.False_)]


def _unary_fills(dt):
    dt = np.dtype(dt)
    return [dt.type(v) for v in {"f": [0, 1.5, np.nan, -np.inf], "i": [0, -1], "u": [0, 255], "b": [False, True]}[dt.kind]]


def _bin_ids():
    return [(n, dt) for n in sorted(_umath._BIN) for dt in DTYPES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", _bin_ids())
def test_binary_ufunc_conformance(name, dt, host_counter, monkeypatch):
    import sparse_amd as sp

    f = getattr(np, name)
    A, B = cross(dt)
    n0 = host_counter()
    for fa, fb in _fills(dt):
        a = sp.COO.from_numpy(A, fill_value=fa)
        b = sp.COO.from_numpy(B, fill_value=fb)
        fill_args = (np.asarray(fa), np.asarray(fb))
        # (b) sparse (x) sparse: the fused merge, its partition-kernel form, and the union + value kernel
        same_call(name, f, (A, B), (a, b), (A, B), fill_args)
        with monkeypatch.context() as m:
            m.setattr(_umath, "MERGE_FUSED", False)
            same_call(name, f, (A, B), (a, b), (A, B), fill_args)
        with monkeypatch.context() as m:
            m.setattr(_umath, "_UNFUSED", set(range(128)))
            m.setattr(_umath, "_SAME_SHAPE_PLANS", {})
            same_call(name, f, (A, B), (a, b), (A, B), fill_args)
        # (e) GCXS operands: the same-layout route and the COO route from two layouts
        ga, gb = sp.GCXS(a), sp.GCXS(b)
        same_call(name, f, (A, B), (ga, gb), (A, B), fill_args)
        same_call(name, f, (A, B), (ga, sp.GCXS(b, compressed_axes=(1,))), (A, B), fill_args)
    a, b = sp.COO.from_numpy(A), sp.COO.from_numpy(B)
    zero = np.zeros((), dtype=dt)
    # (c) sparse (x) scalar, on both sides; a GCXS operand too
    for s in _scalars(dt):
        same_call(name, f, (A, s), (a, s), (A, s), (zero, s))
        same_call(name, f, (s, B), (s, b), (s, B), (s, zero))
        same_call(name, f, (A, s), (sp.GCXS(a), s), (A, s), (zero, s))
    # (d) sparse (x) dense: same shape, and a row that broadcasts into the sparse shape
    same_call(name, f, (A, B), (a, B), (A, B), loose_zero=True)
    same_call(name, f, (A, B), (A, b), (A, B), loose_zero=True)
    row = B[:1]
    want_fill, err = np_call(f, zero, row)
    if err is None and _umath._loose_all_equal(np.asarray(want_fill).reshape(-1)[0], want_fill):
        same_call(name, f, (A, row), (a, row), (A, row), loose_zero=True)
    elif err is None:
        with pytest.raises(ValueError):
            sp_call(f, a, row)
    # (f) traced lambda (the tracer records the ops its device kernels reproduce exactly)
    from sparse_amd import _trace

    if name in _trace._ARITH | _trace._TO_BOOL | _trace._BITWISE:
        want, err2 = np_call(f, A, B)
        if err2 is None:
            check(name, sp_call(lambda: sp.elemwise(lambda u, v: f(u, v), a, b)), want, (A, B))
    n1 = host_counter()
    if not host_expected_binary(name, dt):
        assert n1 == n0, (name, dt, "evaluated on the host", n0, n1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, (1 << 20) + 3])
@pytest.mark.parametrize("dt", DTYPES)
def test_binary_kernels_flat(dt, n):
    """(a) `_umath.binary_arrays` on flat device arrays: the cross product tiled to n elements (n = 2^20 + 3 is past the
    4096 x 256 grid-stride cap), and the 1-element scalar operand on either side."""
    A, B = (x.reshape(-1) for x in cross(dt))
    reps = -(-n // A.size)
    a, b = np.tile(A, reps)[:n], np.tile(B, reps)[:n]
    devi = torch.device("cuda", 0)
    for name in sorted(_umath._BIN):
        f = getattr(np, name)
        want, err = np_call(f, a, b)
        if err is not None:
            continue
        comp = np.dtype(dt) if want.dtype == np.dtype(bool) else want.dtype
        kname = _umath._BOOL_ARITH.get(name, name) if comp == np.dtype(bool) else name
        if comp.str not in ("<f4", "<f8", "<i4", "<i8", "|u1", "|b1") or (name in _NARROW_HOST_BIN and comp.kind not in "fi"):
            continue
        if comp.kind == "f" and name in ("left_shift", "right_shift", "bitwise_and", "bitwise_or", "bitwise_xor"):
            continue
        with np.errstate(all="ignore"):
            ac, bc = a.astype(comp), b.astype(comp)
        ta, tb = torch.from_numpy(ac).to(devi), torch.from_numpy(bc).to(devi)
        got = _umath.binary_arrays(kname, ta, tb).cpu().numpy()
        if got.dtype == np.uint8 and want.dtype == np.dtype(bool):
            got = got.view(bool)
        if TABLE[name] != EXACT and n > A.size:
            # the grid itself is checked at n <= 257 against mpmath; past it every element must equal the grid's result
            small = _umath.binary_arrays(kname, ta[:A.size], tb[:A.size]).cpu().numpy()
            assert np.array_equal(got.view(f"u{got.itemsize}"), np.tile(small, reps)[:n].view(f"u{got.itemsize}")), name
        else:
            check(name, got, want, (a, b) if n <= A.size else None)
        # the scalar operand on either side
        for k in (0, min(7, n - 1)):
            s = torch.from_numpy(ac[k:k + 1].copy()).to(devi)
            got_l = _umath.binary_arrays(kname, s, tb, a_scalar=True).cpu().numpy()
            got_r = _umath.binary_arrays(kname, ta, s, b_scalar=True).cpu().numpy()
            if want.dtype == np.dtype(bool):
                got_l, got_r = got_l.view(bool), got_r.view(bool)
            wl, _ = np_call(f, a[k], b)
            wr, _ = np_call(f, a, a[k])
            if n <= 257:
                check(name, got_l, np.asarray(wl).astype(want.dtype), (np.full(n, a[k]), b))
                check(name, got_r, np.asarray(wr).astype(want.dtype), (a, np.full(n, a[k])))
            else:
                assert got_l.shape == (n,) and got_r.shape == (n,)


# ---- unary --------------------------------------------------------------------------------------------------------------
def _un_ids():
    return [(n, dt) for n in sorted(_umath._UN) for dt in DTYPES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", _un_ids())
def test_unary_ufunc_conformance(name, dt, host_counter):
    import sparse_amd as sp

    f = getattr(np, name)
    v = grid(dt)
    X = np.tile(v, (3, 1))
    n0 = host_counter()
    for fv in _unary_fills(dt):
        x = sp.COO.from_numpy(X, fill_value=fv)
        for arr in (x, sp.GCXS(x)):
            same_call(name, f, (X,), (arr,), (X,), (np.asarray(fv),))
    from sparse_amd import _trace

    if name in _trace._UNARY:
        want, err = np_call(f, X)
        if err is None:
            check(name, sp_call(lambda: sp.elemwise(lambda u: f(u), sp.COO.from_numpy(X))), want, (X,))
    if not host_expected_unary(name, dt):
        assert host_counter() == n0, (name, dt, "evaluated on the host")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, (1 << 20) + 3])
@pytest.mark.parametrize("dt", DTYPES)
def test_unary_kernels_flat(dt, n):
    """(a) `_umath.unary_array` on flat arrays of the grid, tiled to n elements; integer / bool data go in as the kernel's
    compute type (NumPy's float result type, or the data type for the integer forms of `un_tt`)."""
    v = grid(dt)
    reps = -(-n // v.size)
    a = np.tile(v, reps)[:n]
    devi = torch.device("cuda", 0)
    for name in sorted(_umath._UN):
        f = getattr(np, name)
        want, err = np_call(f, a)
        if err is not None:
            continue
        code = _umath._UN[name]
        if code >= 64:
            comp = a.dtype
        elif want.dtype.str in ("<f4", "<f8"):
            comp = want.dtype
        elif want.dtype == a.dtype and code in _umath._UN_INT:
            comp = a.dtype
        else:
            continue
        t = torch.from_numpy(a.astype(comp)).to(devi)
        got = _umath.unary_array(name, t).cpu().numpy()
        if TABLE[name] != EXACT and n > v.size:
            small = _umath.unary_array(name, t[:v.size]).cpu().numpy()
            assert np.array_equal(got.view(f"u{got.itemsize}"), np.tile(small, reps)[:n].view(f"u{got.itemsize}")), name
        else:
            check(name, got, want, (a.astype(comp),) if n <= v.size else None)


# ---- the fixed findings, one named test each ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u1", "?"])
@pytest.mark.parametrize("name", ["sqrt", "exp", "log", "sin", "rint", "cbrt", "deg2rad"])
def test_float_ufunc_of_u8_and_bool_is_float16(name, dt):
    """NumPy returns float16 for these on uint8 / bool data: u8 data used to go into the integer kernel (zeros of the
    wrong dtype) and bool data raised TypeError."""
    import sparse_amd as sp

    X = np.tile(grid(dt), (2, 1))
    f = getattr(np, name)
    want, _ = np_call(f, X)
    got = sp_call(f, sp.COO.from_numpy(X))
    assert got.dtype == want.dtype == np.float16
    assert np.array_equal(got.todense(), want, equal_nan=True)
    assert np.asarray(got.fill_value).dtype == np.float16


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["i4", "i8", "u1"])
def test_integer_reciprocal(dt):
    """np.reciprocal of integers is 1 / x for ±1 (the kernel's integer branch gave 0), NumPy's value for a stored 0."""
    import sparse_amd as sp

    X = np.array([[1, 0, 2, 5, 1], [0, 3, 1, 0, 0]], dtype=dt)
    if np.dtype(dt).kind == "i":
        X[1, 0] = -1
    want, _ = np_call(np.reciprocal, X)
    for x in (sp.COO.from_numpy(X), sp.COO.from_numpy(X, fill_value=X.dtype.type(1))):
        got = sp_call(np.reciprocal, x)
        assert got.dtype == want.dtype and np.array_equal(got.todense(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["square", "reciprocal", "conjugate"])
def test_bool_square_reciprocal_dtype(name):
    """NumPy returns int8 for these on bool data: the result dtype follows NumPy, not the data."""
    import sparse_amd as sp

    X = np.array([[True, False, True], [False, False, True]])
    f = getattr(np, name)
    want, _ = np_call(f, X)
    got = sp_call(f, sp.COO.from_numpy(X))
    assert got.dtype == want.dtype == np.int8
    assert np.asarray(got.fill_value).dtype == np.int8
    assert np.array_equal(got.todense(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["i4", "i8"])
def test_integer_power_negative_exponent_raises(dt):
    """NumPy refuses negative integer exponents; sparse (x) sparse and sparse (x) dense returned 1 for them."""
    import sparse_amd as sp

    A = np.array([[2, 0, 3], [0, 4, 5]], dtype=dt)
    E = np.array([[1, 0, -1], [0, 2, 0]], dtype=dt)
    a, e = sp.COO.from_numpy(A), sp.COO.from_numpy(E)
    with pytest.raises(ValueError, match="negative integer powers"):
        np.power(A, E)
    for args in ((a, e), (a, E), (A, e), (np.int64(2).astype(dt), e), (sp.GCXS(a), sp.GCXS(e))):
        with pytest.raises(ValueError, match="negative integer powers"):
            sp_call(np.power, *args)
    with pytest.raises(ValueError, match="negative integer powers"):
        sp_call(lambda: a ** e)
    # a negative exponent only where the sparse base holds its fill value: met by the fill computation over the dense operand
    Ef = np.array([[1, -1, 2], [0, 2, 1]], dtype=dt)
    assert A[0, 1] == 0
    with pytest.raises(ValueError, match="negative integer powers"):
        sp_call(np.power, a, Ef)
    # non-negative exponents are unaffected
    Ep = np.abs(E)
    got = sp_call(np.power, a, sp.COO.from_numpy(Ep))
    assert np.array_equal(got.todense(), np.power(A, Ep)) and got.dtype == A.dtype


# ---- reductions at special values -------------------------------------------------------------------------------------------
_REDUCTIONS = ["sum", "prod", "max", "min", "any", "all", "nansum", "nanprod", "nanmax", "nanmin", "mean"]


def _red_values(dt, name):
    dt = np.dtype(dt)
    if dt.kind == "f":
        v = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.5, 3.0]
        if name not in ("prod", "nanprod"):     # (a product of max and a denormal depends on the order of the factors)
            v += [np.finfo(dt).max, np.finfo(dt).smallest_subnormal]
        return np.array(v, dtype=dt)
    if dt.kind in "iu":
        ii = np.iinfo(dt)
        return np.array([ii.min, ii.max, ii.max, 1, 2, 0, ii.min + (ii.min < 0), 3], dtype=dt)
    return np.array([True, False, True])


def _red_arrays(dt, name):
    """(dense, fill) pairs of shape (4, 3, 5): special values stored sparsely, with zero and non-zero fills."""
    rng = np.random.default_rng(5)
    v = _red_values(dt, name)
    shape = (4, 3, 5)
    out = []
    for fill in ([np.zeros((), dt)[()]] + ([np.asarray(v[-1])[()]] if np.dtype(dt).kind != "b" else [np.True_])):
        for mix in ("sparse", "nan_free", "extreme"):
            d = np.full(shape, fill, dtype=dt)
            mask = rng.random(shape) < 0.45
            vals = v
            if mix == "nan_free" and np.dtype(dt).kind == "f":
                vals = v[~np.isnan(v)]
            if mix == "extreme" and np.dtype(dt).kind in "iu":
                vals = v[:3]
            d[mask] = rng.choice(vals, int(mask.sum()))
            out.append((d, fill))
    return out


def _red_call(name, x, axis):
    import sparse_amd as sp

    if name.startswith("nan"):
        return getattr(sp, name)(x, axis=axis)
    return getattr(x, name)(axis=axis)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", [(n, dt) for n in _REDUCTIONS for dt in DTYPES])
def test_reductions_at_special_values(name, dt):
    """axis=None (`spamd_reduce_all`), a leading axis (the slab merge), the last axis (`group_reduce`), on COO and GCXS;
    integers and max / min / any / all exactly (dtype and value, int64 wrap included), float sums within n * eps * sum|v| of
    a math.fsum reference."""
    import sparse_amd as sp

    for d, fill in _red_arrays(dt, name):
        coo = sp.COO.from_numpy(d, fill_value=fill)
        for axis in (None, 0, 2):
            for x in (coo, sp.GCXS(coo), sp.GCXS(coo.reshape((12, 5)))):
                xd = d if x.shape == d.shape else d.reshape(12, 5)
                ax = axis if x.shape == d.shape or axis is None else (0 if axis == 0 else 1)
                w, err = np_call(lambda z: getattr(np, name)(z, axis=ax), xd)
                if err is not None:
                    with pytest.raises(err):
                        sp_call(lambda: _red_call(name, x, ax))
                    continue
                got = sp_call(lambda: _red_call(name, x, ax))
                gd = got.todense() if hasattr(got, "todense") else np.asarray(got)
                w = np.asarray(w)
                if w.dtype == np.uint64:
                    # deliberate: NumPy sums / multiplies uint8 in uint64, a value type the containers do not have (torch has
                    # no general uint64 arithmetic; `_device._NP2T` maps it to int64) - the same 64 bits, typed int64
                    assert gd.dtype == np.int64, (name, dt, ax, gd.dtype)
                    gd = gd.view(np.uint64)
                assert gd.dtype == w.dtype and gd.shape == w.shape, (name, dt, ax, gd.dtype, w.dtype)
                if w.dtype.kind != "f" or name in ("max", "min", "nanmax", "nanmin"):
                    nan = np.isnan(w) if w.dtype.kind == "f" else np.zeros(w.shape, bool)
                    assert np.array_equal(np.isnan(gd) if w.dtype.kind == "f" else nan, nan), (name, dt, ax)
                    assert np.array_equal(gd[~nan], w[~nan]), (name, dt, ax, gd, w)
                    continue
                # floats: non-finite results exactly (NaN-ness, inf and its sign), the others within m * eps of the exact
                # value - for sums and means relative to sum |v| (math.fsum reference), for products to the product
                fin = np.isfinite(w)
                assert np.array_equal(np.isnan(gd), np.isnan(w)), (name, dt, ax, gd, w)
                assert np.array_equal(gd[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (name, dt, ax, gd, w)
                src = np.where(np.isnan(xd), 0 if name != "nanprod" else 1, xd) if name.startswith("nan") else xd
                red_ax = tuple(range(xd.ndim)) if ax is None else (ax,)
                moved = np.moveaxis(src.astype(np.float64), red_ax, tuple(range(-len(red_ax), 0)))
                flat = moved.reshape(moved.shape[:moved.ndim - len(red_ax)] + (-1,))[fin]
                m = flat.shape[-1]
                eps = np.finfo(w.dtype).eps
                if name in ("prod", "nanprod"):
                    ref = np.prod(flat, axis=-1)       # (the factors are small: exact enough in float64)
                    tol = m * eps * np.abs(ref)
                else:
                    ref = np.array([math.fsum(r) for r in flat]).reshape(-1)
                    tol = m * eps * np.abs(flat).sum(-1)
                    if name == "mean":
                        ref, tol = ref / m, tol / m
                tol = tol + np.finfo(w.dtype).smallest_subnormal
                assert np.all(np.abs(gd[fin].astype(np.float64) - ref) <= tol), (name, dt, ax, gd, w)

"""SDDMM with complex64 / complex128 operands and complex mask values (csrc/sddmm_complex.hip).

The yardstick is the complex128 NumPy evaluation of `s * einsum("ik,ik->i", a[rows], bt[cols])` on the values the kernel
saw (complex64 inputs widened), per component (re and im separately):

    |got - want| <= tol * absum + 1e-300,   absum = (|s.re| + |s.im|) * sum_k (|a.re| + |a.im|)(|b.re| + |b.im|)

with the project's constants tol = 2e-6 (fp32 accumulation) and 1e-14 (fp64): (terms + 10) * u covers up to about 22 real terms
per lane and component, the butterfly and the mask product, u = 2^-24 / 2^-53.  The one case with more terms per lane -
complex64 K = 1000 in the gather form, 8 vectors of 2 complex values of 2 real terms = 32 - takes its bound from the same
formula, 42 u = 2.5e-6.  Every test prints the measured maximum of |got - want| / absum."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CDT = {"c64": (np.complex64, torch.complex64), "c128": (np.complex128, torch.complex128)}
U = {"c64": 2.0 ** -24, "c128": 2.0 ** -53}
TOL = {"c64": 2e-6, "c128": 1e-14}
MASK_TYPES = (np.float32, np.float64, np.int64, np.bool_, np.complex64, np.complex128)


def _cplx(rng, shape, npdt):
    return ((rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)).astype(npdt)


def _mask_values(rng, n, vt):
    if vt is np.bool_:
        return rng.random(n) < 0.7
    if vt is np.int64:
        return rng.integers(-3, 4, n)
    if np.dtype(vt).kind == "c":
        return _cplx(rng, n, vt)
    return (rng.random(n) - 0.5).astype(vt)


def _mask(rng, M, N, nnz, idx=np.int64):
    lin = np.sort(rng.choice(M * N, nnz, replace=False))
    return np.stack([lin // N, lin % N]).astype(idx)


def _l1(z):
    return np.abs(z.real) + np.abs(z.imag)


def _reference(s, a, bt, rows, cols):
    """(want, absum) in complex128 / float64 for operands given as NumPy arrays of the values the kernel saw."""
    s, a, bt = s.astype(np.complex128), a.astype(np.complex128), bt.astype(np.complex128)
    la, lb = _l1(a), _l1(bt)
    want, absum = np.empty(s.size, np.complex128), np.empty(s.size, np.float64)
    for lo in range(0, s.size, 8192):        # (in pieces: a[rows] of 60 013 rows of 512 complex128 is 490 MB)
        r, c = rows[lo:lo + 8192], cols[lo:lo + 8192]
        want[lo:lo + 8192] = s[lo:lo + 8192] * np.einsum("ik,ik->i", a[r], bt[c])
        absum[lo:lo + 8192] = _l1(s[lo:lo + 8192]) * np.einsum("ik,ik->i", la[r], lb[c])
    return want, absum


def _assert_close(got, want, absum, tol, what):
    got = np.asarray(got).astype(np.complex128)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    print(f"{what}: max component error / absum = {(err / (absum + 1e-300)).max() if err.size else 0.0:.3e} (bound {tol:.2e})")
    assert np.all(np.abs(got.real - want.real) <= tol * absum + 1e-300), what
    assert np.all(np.abs(got.imag - want.imag) <= tol * absum + 1e-300), what


def _real_view(t):
    return torch.view_as_real(t)


# ---- gather form ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gather_case(dt, Kd):
    """Operands, coordinates and one reference per (type, K): shared by the index widths and mask types."""
    rng = np.random.default_rng(1000 + Kd)
    M, N, nnz = 300, 250, 4001
    coords = _mask(rng, M, N, nnz)
    a, bt = _cplx(rng, (M, Kd), CDT[dt][0]), _cplx(rng, (N, Kd), CDT[dt][0])
    unit, absum1 = _reference(np.ones(nnz), a, bt, coords[0], coords[1])     # the dot products and their sum|terms|
    return coords, a, bt, unit, absum1


def _gather_tol(dt, Kd):
    # complex64 K = 1000: 500 vectors over 64 lanes = up to 8 vectors per lane = 32 real terms per component
    return 42 * U[dt] if (dt, Kd) == ("c64", 1000) else TOL[dt]


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("Kd", [1, 3, 7, 33, 100, 200, 1000])
@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_gather_form_against_complex128(dt, Kd, idx):
    """Odd K (pitch padding for complex64), every lane-group width from 4 to 64, nnz a multiple of no group size; the mask
    value type rotates through the six with K and the index width."""
    import sparse_amd as sp

    coords, a, bt, unit, absum1 = _gather_case(dt, Kd)
    M, N, nnz = 300, 250, coords.shape[1]
    vt = MASK_TYPES[([1, 3, 7, 33, 100, 200, 1000].index(Kd) + (idx is np.int64) * 3) % 6]
    sval = _mask_values(np.random.default_rng(Kd), nnz, vt)
    s = sp.COO(coords.astype(idx), sval, shape=(M, N))
    at, btt = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    r = sp.sddmm(s, at, bt=btt)
    assert r.dtype == CDT[dt][0] and r.shape == (M, N)
    seen = sval.astype(CDT[dt][0]).astype(np.complex128)       # the mask values in the operands' type
    got = r.todense()[coords[0], coords[1]]
    _assert_close(got, seen * unit, _l1(seen) * absum1, _gather_tol(dt, Kd), f"gather {dt} K={Kd} {np.dtype(idx)} mask {np.dtype(vt)}")
    assert r.nnz == np.count_nonzero(got)


@pytest.mark.parametrize("vt", MASK_TYPES)
@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_every_mask_value_type(dt, vt):
    import sparse_amd as sp

    coords, a, bt, unit, absum1 = _gather_case(dt, 33)
    sval = _mask_values(np.random.default_rng(5), coords.shape[1], vt)
    s = sp.COO(coords, sval, shape=(300, 250))
    r = sp.sddmm(s, torch.from_numpy(a).cuda(), bt=torch.from_numpy(bt).cuda())
    assert r.dtype == CDT[dt][0]
    seen = sval.astype(CDT[dt][0]).astype(np.complex128)
    got = r.todense()[coords[0], coords[1]]
    _assert_close(got, seen * unit, _l1(seen) * absum1, TOL[dt], f"mask {np.dtype(vt)} over {dt}")
    assert r.nnz == np.count_nonzero(got)
    if vt in (np.bool_, np.int64):
        assert r.nnz < coords.shape[1]          # zero mask values give (0, 0) pairs, which are pruned


def test_scalar_tail_of_the_gather_kernel_through_the_c_abi():
    """complex64 rows of an odd K on a 16-byte pitch, K passed as it is: the element past the whole vectors is taken by the
    scalar tail (the host layer pads the operands and never passes an odd K)."""
    from sparse_amd import _ffi
    from sparse_amd._device import ptr, stream_ptr

    rng = np.random.default_rng(77)
    M, N, nnz = 60, 50, 1203
    coords = _mask(rng, M, N, nnz, np.int32)
    for Kd in (1, 7, 33, 201):
        a, bt = np.zeros((M, Kd + 1), np.complex64), np.zeros((N, Kd + 1), np.complex64)
        a[:, :Kd], bt[:, :Kd] = _cplx(rng, (M, Kd), np.complex64), _cplx(rng, (N, Kd), np.complex64)
        a[:, Kd], bt[:, Kd] = 1e3, 1e3                      # the pad column must not be read
        sval = _cplx(rng, nnz, np.complex64)
        at, btt, st, ct = (torch.from_numpy(x).cuda() for x in (a, bt, sval, coords))
        out = torch.empty(nnz, dtype=torch.complex64, device="cuda")
        _ffi.call("spamd_sddmm_complex", _ffi.C64, _ffi.I32, nnz, ptr(ct[0]), ptr(ct[1]), ptr(st), ptr(at), Kd + 1, ptr(btt), Kd + 1,
                  Kd, ptr(out), None, 0, None, 0, stream_ptr(out.device))
        want, absum = _reference(sval, a[:, :Kd], bt[:, :Kd], coords[0], coords[1])
        _assert_close(out.cpu().numpy(), want, absum, TOL["c64"], f"tail K={Kd}")


# ---- row-cached form --------------------------------------------------------------------------------------------------------
# (type, K, lanes per element, vectors per lane): every pair the dispatch takes - the first L of 16, 32, 64 that factors the row
ROWCACHE = [("c64", 32, 16, 1), ("c64", 64, 16, 2), ("c64", 96, 16, 3), ("c64", 128, 16, 4), ("c64", 192, 32, 3), ("c64", 256, 32, 4),
            ("c64", 384, 64, 3), ("c64", 512, 64, 4),
            ("c128", 16, 16, 1), ("c128", 32, 16, 2), ("c128", 48, 16, 3), ("c128", 64, 16, 4), ("c128", 96, 32, 3), ("c128", 128, 32, 4),
            ("c128", 192, 64, 3), ("c128", 256, 64, 4)]


@functools.lru_cache(maxsize=None)
def _rowcache_case(dt, Kd):
    rng = np.random.default_rng(Kd)
    M, N, nnz = 700, 5000, 60_013
    coords = _mask(rng, M, N, nnz)
    a, bt, sval = _cplx(rng, (M, Kd), CDT[dt][0]), _cplx(rng, (N, Kd), CDT[dt][0]), _cplx(rng, nnz, CDT[dt][0])
    want, absum = _reference(sval, a, bt, coords[0], coords[1])
    subset = np.sort(rng.choice(nnz, 20_001, replace=False))
    return coords, a, bt, sval, want, absum, subset


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dt, Kd, L, KS", ROWCACHE)
def test_row_cached_form_and_its_panel_order_are_bit_identical(dt, Kd, L, KS, idx):
    """The row-cached kernel against the complex128 evaluation, and bit for bit against itself in column-panel order - ragged
    sizes (nnz no multiple of the step), several panel widths with and without XCD-private pieces, several chunk lengths - and
    for a subset of the elements written into a pre-filled result."""
    from sparse_amd import _ffi
    from sparse_amd import _kernels as K

    esz = 8 if dt == "c64" else 16
    assert Kd * esz == L * KS * 16 and _ffi.lib().spamd_sddmm_complex_has_rowcache(K.sddmm_complex_code(CDT[dt][1]), Kd) == 1
    assert all((Kd * esz // 16) % l or not 1 <= Kd * esz // 16 // l <= 4 for l in (16, 32, 64) if l < L)    # L is the first that fits
    coords_h, a, bt, sval_h, want, absum, subset_h = _rowcache_case(dt, Kd)
    M, N, nnz = 700, 5000, coords_h.shape[1]
    coords = torch.from_numpy(coords_h.astype(idx)).cuda()
    at, btt, sval = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda(), torch.from_numpy(sval_h).cuda()
    ref = K.sddmm_coo(coords, sval, at, btt)
    assert ref.dtype == CDT[dt][1]
    _assert_close(ref.cpu().numpy(), want, absum, TOL[dt], f"row-cached {dt} K={Kd} L={L} KS={KS} {np.dtype(idx)}")
    assert torch.equal(_real_view(K.sddmm_coo(coords, sval, at, btt)), _real_view(ref))      # run to run
    for width, xcd in ((64, False), (64, True), (300, True), (1000, False), (4999, False), (5000, True)):
        plan = K.sddmm_panels(coords, (M, N), width, xcd=xcd)
        assert (plan.xstate is not None) == (xcd and (N - 1) // width + 1 >= 8)
        for chunk in (0, 16, 48, 1000):
            plan.chunk = chunk
            got = K.sddmm_coo(coords, sval, at, btt, panels=plan)
            assert torch.equal(_real_view(got), _real_view(ref)), (width, xcd, chunk)
    # a subset of the elements, written into a caller-provided result
    subset = torch.from_numpy(subset_h).cuda()
    plan = K.sddmm_panels(coords, (M, N), 300, subset=subset)
    out = torch.full((nnz,), -7.0 + 3.0j, dtype=ref.dtype, device="cuda")
    K._sddmm_panels_into(plan, sval, sval, at, btt, out)
    keep = torch.zeros(nnz, dtype=torch.bool, device="cuda")
    keep[subset] = True
    assert torch.equal(_real_view(out[keep]), _real_view(ref[keep])) and bool((out[~keep] == -7.0 + 3.0j).all())


@pytest.mark.parametrize("dt, Kd", [("c64", 100), ("c128", 7), ("c64", 128), ("c128", 192)])
def test_two_runs_are_equal(dt, Kd):
    """Determinism of both forms: no atomics, a fixed lane order."""
    import sparse_amd as sp

    rng = np.random.default_rng(Kd)
    M, N, nnz = 300, 250, 4001
    coords = _mask(rng, M, N, nnz)
    s = sp.COO(coords, _cplx(rng, nnz, CDT[dt][0]), shape=(M, N))
    at, btt = torch.from_numpy(_cplx(rng, (M, Kd), CDT[dt][0])).cuda(), torch.from_numpy(_cplx(rng, (N, Kd), CDT[dt][0])).cuda()
    r1, r2 = sp.sddmm(s, at, bt=btt), sp.sddmm(s, at, bt=btt)
    assert r1.nnz == r2.nnz == nnz and torch.equal(_real_view(r1.data), _real_view(r2.data))


# ---- edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kd", [5, 32])
@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_edges(dt, Kd):
    import sparse_amd as sp

    npdt, tdt = CDT[dt]
    rng = np.random.default_rng(3)
    M, N = 20, 30
    a, bt = _cplx(rng, (M, Kd), npdt), _cplx(rng, (N, Kd), npdt)
    at, btt = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    # fewer stored elements than one lane group, and none at all
    for nnz in (0, 1, 3):
        coords = _mask(rng, M, N, nnz)
        sval = _cplx(rng, nnz, npdt)
        r = sp.sddmm(sp.COO(coords, sval, shape=(M, N)), at, bt=btt)
        assert r.nnz == nnz and r.shape == (M, N) and r.dtype == npdt
        want, absum = _reference(sval, a, bt, coords[0], coords[1])
        _assert_close(r.todense()[coords[0], coords[1]], want, absum, TOL[dt], f"nnz={nnz} {dt} K={Kd}")
    # a mask row whose A row is all zeros: pruned
    coords = _mask(rng, M, N, 200)
    sval = _cplx(rng, 200, npdt)
    a0 = a.copy()
    a0[coords[0][17]] = 0
    r = sp.sddmm(sp.COO(coords, sval, shape=(M, N)), torch.from_numpy(a0).cuda(), bt=btt)
    dead = int((coords[0] == coords[0][17]).sum())
    assert dead >= 1 and r.nnz == 200 - dead
    assert np.all(r.todense()[coords[0][17]] == 0)
    want, absum = _reference(sval, a0, bt, coords[0], coords[1])
    _assert_close(r.todense()[coords[0], coords[1]], want, absum, TOL[dt], f"zero row {dt} K={Kd}")
    # an operand of -0.0 in both parts: every result is (+0, +0) and pruned
    neg = torch.full((M, Kd), -0.0, dtype=torch.float64 if dt == "c128" else torch.float32, device="cuda")
    az = torch.complex(neg, neg)
    assert sp.sddmm(sp.COO(coords, sval, shape=(M, N)), az, bt=btt).nnz == 0
    # shape errors and operand types
    with pytest.raises(ValueError, match="shape-mismatch"):
        sp.sddmm(sp.COO(coords, sval, shape=(M, N)), at, bt=btt[:, :-1])
    other = torch.complex128 if dt == "c64" else torch.complex64
    with pytest.raises(TypeError, match="share a dtype"):
        sp.sddmm(sp.COO(coords, sval, shape=(M, N)), at, bt=btt.to(other))
    with pytest.raises(TypeError):
        sp.sddmm(sp.COO(coords, sval, shape=(M, N)), at, bt=btt.real.contiguous())
    with pytest.raises(TypeError):
        sp.sddmm(sp.COO(coords, sval, shape=(M, N)), at.real.contiguous().float(), bt=btt)


@pytest.mark.parametrize("Kd", [6, 64])
def test_operand_layouts(Kd):
    """Views at a storage offset of 8 bytes (complex64: one element) are cloned, a non-contiguous bt is packed, b may come
    untransposed: the values of the aligned, contiguous call, bit for bit."""
    import sparse_amd as sp

    rng = np.random.default_rng(8)
    M, N, nnz = 90, 70, 2003
    coords = _mask(rng, M, N, nnz)
    s = sp.COO(coords, _cplx(rng, nnz, np.complex64), shape=(M, N))
    at, btt = torch.from_numpy(_cplx(rng, (M, Kd), np.complex64)).cuda(), torch.from_numpy(_cplx(rng, (N, Kd), np.complex64)).cuda()
    ref = sp.sddmm(s, at, bt=btt)
    assert ref.nnz == nnz

    def same(r):
        return r.nnz == nnz and torch.equal(_real_view(r.data), _real_view(ref.data))

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8
        return v

    assert same(sp.sddmm(s, shifted(at), bt=shifted(btt)))
    wide = torch.zeros((N, 2 * Kd), dtype=torch.complex64, device="cuda")
    wide[:, ::2] = btt
    assert not wide[:, ::2].is_contiguous() and same(sp.sddmm(s, at, bt=wide[:, ::2]))
    assert same(sp.sddmm(s, at, btt.t().contiguous()))       # b (K x N)
    assert same(sp.sddmm(s, at, btt.t()))                    # and as a transposed view
    assert same(sp.sddmm(s, at.cpu().numpy(), bt=btt.cpu().numpy()))     # NumPy complex arrays in


# ---- public interface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, Kd", [("c64", 64), ("c128", 64)])
def test_product_path_uses_panels_and_follows_the_mask(dt, Kd, monkeypatch):
    """`sparse_amd.sddmm` with complex operands builds the panel plan once per mask (COO, or the kept COO view of a GCXS mask),
    re-gathers the mask values when they change in place, and takes NumPy arrays."""
    import sparse_amd as sp
    from sparse_amd import _ffi
    from sparse_amd import _kernels as K

    npdt, tdt = CDT[dt]
    monkeypatch.setattr(K, "sddmm_panels_pay", lambda n, a, bt, width: bool(width))   # (the traffic model would keep so small a mask in its own order)
    monkeypatch.setattr(K, "SDDMM_PANEL_BYTES", 64 * Kd * np.dtype(npdt).itemsize)    # 64 Bt rows per panel
    calls = []
    orig = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *a: (calls.append((name, a)), orig(name, *a))[1])
    rng = np.random.default_rng(11)
    M, N, nnz = 500, 3000, 40_000
    coords = _mask(rng, M, N, nnz, np.int32)
    sval = _cplx(rng, nnz, npdt)
    a, bt = _cplx(rng, (M, Kd), npdt), _cplx(rng, (N, Kd), npdt)
    unit, absum1 = _reference(np.ones(nnz), a, bt, coords[0], coords[1])

    def check(r, values, what):
        v = values.astype(np.complex128)
        _assert_close(r.todense()[coords[0], coords[1]], v * unit, _l1(v) * absum1, TOL[dt], what)

    s = sp.COO(coords, sval, shape=(M, N))
    at, btt = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    plain = K.sddmm_coo(s.coords, s.data, at, btt)
    r = sp.sddmm(s, at, bt=btt)
    check(r, sval, f"panels {dt}")
    key = ("panels", "all", K.sddmm_panel_width(btt))
    assert key[2] == 64 and key in s._sddmm_plan and s._sddmm_plan[key].count == nnz
    panel_calls = [c for n, c in calls if n == "spamd_sddmm_complex"]
    assert panel_calls[-1][12] is not None and panel_calls[0][12] is None       # perm given: the panel order ran
    assert torch.equal(_real_view(r.data), _real_view(plain))                    # the same bits as the mask's own order
    first = s._sddmm_plan[key]
    sp.sddmm(s, a, bt=bt)                          # NumPy operands
    assert s._sddmm_plan[key] is first             # built once
    s.data.mul_(2.0)                               # in-place change of the mask values: new result, no stale values
    check(sp.sddmm(s, at, bt=btt), 2 * sval, "after an in-place change")
    g = s.asformat("gcxs", compressed_axes=(0,))
    rg = sp.sddmm(g, at, bt=btt)
    assert isinstance(rg, sp.GCXS) and rg.dtype == npdt
    check(rg, 2 * sval, "gcxs mask")
    view = g._coo_view
    sp.sddmm(g, at, bt=btt)
    assert g._coo_view is view and key in view._sddmm_plan


# ---- N-D masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("la, lb", [((3,), ()), ((3,), (3,)), ((), ())])
@pytest.mark.parametrize("dt, Kd", [("c64", 5), ("c64", 32), ("c128", 16), ("c128", 9)])
def test_nd_masks_equal_the_loop_of_2d_calls(dt, Kd, la, lb):
    """A (3, 40, 50) mask over a (3, 40, K) / (40, K) and bt (50, K) / (3, 50, K): the fold is independent of the value type, so
    the stack is bit-identical to the loop of 2-D calls; with both operands broadcast several samples share one pair of rows."""
    import sparse_amd as sp

    npdt, tdt = CDT[dt]
    rng = np.random.default_rng(Kd + len(la) + 2 * len(lb))
    lead, M, N = (3,), 40, 50
    shape = lead + (M, N)
    nnz = 2100
    lin = np.sort(rng.choice(int(np.prod(shape)), nnz, replace=False))
    coords = np.stack(np.unravel_index(lin, shape)).astype(np.int64)
    sval = _cplx(rng, nnz, npdt)
    a, bt = _cplx(rng, la + (M, Kd), npdt), _cplx(rng, lb + (N, Kd), npdt)
    s = sp.COO(coords, sval, shape=shape)
    at, btt = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    r = sp.sddmm(s, at, bt=btt)
    assert r.shape == shape and r.dtype == npdt and r.nnz == nnz
    ab, bb = np.broadcast_to(a, lead + (M, Kd)).reshape(-1, Kd), np.broadcast_to(bt, lead + (N, Kd)).reshape(-1, Kd)
    want, absum = _reference(sval, ab, bb, coords[0] * M + coords[1], coords[0] * N + coords[2])
    got = r.todense()
    _assert_close(got[tuple(coords)], want, absum, TOL[dt], f"N-D {dt} K={Kd} a{la} b{lb}")
    loop = np.zeros(shape, dtype=npdt)
    for b in range(3):
        loop[b] = sp.sddmm(s[b], at[b] if la else at, bt=btt[b] if lb else btt).todense()
    assert np.array_equal(got.view(np.float64 if dt == "c128" else np.float32), loop.view(np.float64 if dt == "c128" else np.float32))
    rg = sp.sddmm(s.asformat("gcxs"), at, bt=btt)
    assert isinstance(rg, sp.GCXS) and np.array_equal(rg.todense(), got)


# ---- complex mask values over real operands ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", [np.complex64, np.complex128])
@pytest.mark.parametrize("rdt, Kd", [(np.float32, 100), (np.float32, 64), (np.float64, 33), (np.float64, 32)])
def test_complex_mask_over_real_operands(rdt, Kd, mt):
    """The real dot products under a unit mask, then one device multiply by the mask values: complex64 for float32 operands,
    complex128 for float64, each component within the real kernels' bound over |s component| * sum|a||b|.  (The parent commit
    dropped the imaginary part of the mask.)"""
    import sparse_amd as sp

    rng = np.random.default_rng(Kd)
    M, N, nnz = 300, 250, 4001
    coords = _mask(rng, M, N, nnz)
    sval = _cplx(rng, nnz, mt)
    a, bt = (rng.random((M, Kd)) - 0.5).astype(rdt), (rng.random((N, Kd)) - 0.5).astype(rdt)
    cdt = np.complex64 if rdt is np.float32 else np.complex128
    for s in (sp.COO(coords, sval, shape=(M, N)), sp.COO(coords, sval, shape=(M, N)).asformat("gcxs")):
        r = sp.sddmm(s, torch.from_numpy(a).cuda(), bt=torch.from_numpy(bt).cuda())
        assert r.dtype == cdt and type(r) is type(s) and r.nnz == nnz
        got = r.todense()[coords[0], coords[1]].astype(np.complex128)
        seen = sval.astype(cdt).astype(np.complex128)
        a64, b64 = a.astype(np.float64), bt.astype(np.float64)
        dots = np.einsum("ik,ik->i", a64[coords[0]], b64[coords[1]])
        absd = np.einsum("ik,ik->i", np.abs(a64[coords[0]]), np.abs(b64[coords[1]]))
        tol = 2e-6 if rdt is np.float32 else 1e-14
        for part in ("real", "imag"):
            g, w, sc = getattr(got, part), getattr(seen, part) * dots, np.abs(getattr(seen, part))
            print(f"{np.dtype(mt)} mask over {np.dtype(rdt)} K={Kd} {part}: max error / sum|terms| = {(np.abs(g - w) / (sc * absd + 1e-300)).max():.3e}")
            assert np.all(np.abs(g - w) <= tol * sc * absd + 1e-300)
        assert np.all((got.imag != 0) == (seen.imag * dots != 0)) and np.count_nonzero(got.imag) > nnz // 2


def test_complex_mask_over_16_bit_operands_is_refused():
    import sparse_amd as sp

    rng = np.random.default_rng(2)
    coords = _mask(rng, 40, 50, 300)
    s = sp.COO(coords, _cplx(rng, 300, np.complex64), shape=(40, 50))
    for tdt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="complex mask"):
            sp.sddmm(s, torch.zeros((40, 64), dtype=tdt, device="cuda"), bt=torch.zeros((50, 64), dtype=tdt, device="cuda"))


# ---- nothing is computed on the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, Kd", [("c64", 7), ("c128", 64)])
def test_no_stored_value_reaches_the_host(dt, Kd, monkeypatch):
    """During `sddmm` no tensor of value type (floating point or complex: the mask values, the operands, the result) is copied
    to the host - only small integer read-backs (the pruning count, plan sizes) - and the general host routes are not entered."""
    import sparse_amd as sp
    from sparse_amd import _ffi, _kernels as K, _reduce, _umath

    npdt, tdt = CDT[dt]
    monkeypatch.setattr(K, "sddmm_panels_pay", lambda n, a, bt, width: bool(width))
    monkeypatch.setattr(K, "SDDMM_PANEL_BYTES", 64 * Kd * np.dtype(npdt).itemsize)
    rng = np.random.default_rng(4)
    M, N, nnz = 200, 900, 9001
    coords = _mask(rng, M, N, nnz)
    at, btt = torch.from_numpy(_cplx(rng, (M, Kd), npdt)).cuda(), torch.from_numpy(_cplx(rng, (N, Kd), npdt)).cuda()
    masks = [sp.COO(coords, _mask_values(rng, nnz, vt), shape=(M, N)) for vt in (np.float64, np.int64, np.complex64, np.complex128)]
    masks.append(masks[-1].asformat("gcxs"))
    rmask = sp.COO(coords, _cplx(rng, nnz, np.complex128), shape=(M, N))
    ra, rb = at.real.contiguous(), btt.real.contiguous()
    torch.cuda.synchronize()
    crossed, abi, host = [], [], []

    def watch(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                crossed.append((name, self.dtype, self.numel()))
            return orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, f)

    for name in ("cpu", "numpy", "tolist", "item", "__array__"):
        watch(name)
    orig_to = torch.Tensor.to

    def to(self, *a, **k):
        dev = k.get("device", a[0] if a and isinstance(a[0], (str, torch.device)) else None)
        if self.is_cuda and dev is not None and torch.device(dev).type == "cpu":
            crossed.append(("to", self.dtype, self.numel()))
        return orig_to(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "to", to)
    orig_call = _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *a: (abi.append(name), orig_call(name, *a))[1])
    monkeypatch.setattr(_umath, "_elemwise_general", lambda *a, **k: host.append("elemwise") or pytest.fail("host elementwise route"))
    monkeypatch.setattr(_reduce, "_reduce_on_host", lambda *a, **k: host.append("reduce") or pytest.fail("host reduction"))
    results = [sp.sddmm(m, at, bt=btt) for m in masks]
    results.append(sp.sddmm(rmask, ra, bt=rb))
    monkeypatch.undo()
    assert all(r.nnz > 0 for r in results) and not host
    assert "spamd_sddmm_complex" in abi and "spamd_cplx_convert" in abi and "spamd_cplx_binary" in abi
    assert "spamd_sddmm" in abi or "spamd_sddmm_panels" in abi          # the real dot products of the complex-mask case
    bad = [c for c in crossed if c[1].is_floating_point or c[1].is_complex or c[2] > 16]
    assert not bad, bad

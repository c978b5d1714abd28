"""float16 SDDMM on the device: tests/test_sddmm_gpu.py case for case with float16 in place of bfloat16 - the same float64
reference (`s * (a @ b)` on the values the kernel saw), the same bounds (2e-6 * sum|terms| sampled, 4e-6 tiles: an fp16 product
has a 22-bit significand and an exponent of at least 2^-48, so it is exact in fp32 and the error is the fp32 accumulation's,
as for bf16), the same bit-identities - plus operands that hold fp16 subnormals, which have no bf16 twin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = torch.float16


def _bounds(sval, a64, b64, r, c):
    want = sval * np.einsum("ik,ik->i", a64[r], b64[c])
    absum = np.abs(sval) * np.einsum("ik,ik->i", np.abs(a64[r]), np.abs(b64[c]))
    return want, absum


@pytest.mark.parametrize("K", [1, 7, 64, 192, 200, 256, 384, 1000])
def test_sddmm_f16_vs_dense_formulation(K):
    import sparse_amd as sp

    rng = np.random.default_rng(K)
    M, N, nnz = 300, 250, 4001
    lin = np.sort(rng.choice(M * N, nnz, replace=False))
    coords = np.stack([lin // N, lin % N])
    sval = rng.random(nnz) - 0.5
    a, b = rng.random((M, K)) - 0.5, rng.random((K, N)) - 0.5
    at, bt = torch.from_numpy(a).cuda().to(F16), torch.from_numpy(b.T.copy()).cuda().to(F16)
    s = sp.COO(coords, sval.astype(np.float32), shape=(M, N))
    r = sp.sddmm(s, at, bt=bt)
    assert r.dtype == np.float32
    a64, b64 = at.double().cpu().numpy(), bt.double().cpu().numpy()  # the values the kernel saw
    want, absum = _bounds(s.data.double().cpu().numpy(), a64, b64, coords[0], coords[1])
    got = r.todense()[coords[0], coords[1]]
    err = np.abs(got - want) / (absum + 1e-300)
    print(f"K={K}: max error / sum|terms| = {err.max():.3e}")
    assert np.all(np.abs(got - want) <= 2e-6 * absum + 1e-300)
    assert r.nnz == np.count_nonzero(got)
    # b given untransposed: the same values
    r2 = sp.sddmm(s, at, bt.t().contiguous())
    assert np.array_equal(r2.todense(), r.todense())


def test_sddmm_f16_numpy_operands_and_mixed_types():
    """NumPy float16 arrays (NumPy has no bfloat16: this is its only 16-bit SDDMM); operands of two types are refused."""
    import sparse_amd as sp

    rng = np.random.default_rng(2)
    M, N, K, nnz = 200, 300, 128, 3000
    lin = np.sort(rng.choice(M * N, nnz, replace=False))
    coords = np.stack([lin // N, lin % N])
    sval = (rng.random(nnz) - 0.5).astype(np.float32)
    a, b = (rng.random((M, K)) - 0.5).astype(np.float16), (rng.random((K, N)) - 0.5).astype(np.float16)
    s = sp.COO(coords, sval, shape=(M, N))
    r = sp.sddmm(s, a, b)
    want, absum = _bounds(sval.astype(np.float64), a.astype(np.float64), b.T.astype(np.float64), coords[0], coords[1])
    got = r.todense()[coords[0], coords[1]]
    assert np.all(np.abs(got - want) <= 2e-6 * absum + 1e-300)
    rt = sp.sddmm(s, torch.from_numpy(a).cuda(), bt=torch.from_numpy(b.T.copy()).cuda())
    assert np.array_equal(rt.todense(), r.todense())
    with pytest.raises(TypeError, match="share a dtype"):
        sp.sddmm(s, torch.from_numpy(a).cuda(), bt=torch.from_numpy(b.T.copy()).cuda().to(torch.bfloat16))
    with pytest.raises(TypeError, match="sddmm supports"):
        sp.sddmm(s, torch.zeros((M, K), dtype=torch.int32, device="cuda"), bt=torch.zeros((N, K), dtype=torch.int32, device="cuda"))


def test_sddmm_f16_gcxs_mask():
    import sparse_amd as sp

    rng = np.random.default_rng(4)
    M, N, K, nnz = 257, 129, 64, 5000
    lin = np.sort(rng.choice(M * N, nnz, replace=False))
    coords = np.stack([lin // N, lin % N])
    sval = (rng.random(nnz) - 0.5).astype(np.float32)
    at = (torch.rand((M, K), device="cuda") - 0.5).to(F16)
    bt = (torch.rand((N, K), device="cuda") - 0.5).to(F16)
    s = sp.COO(coords, sval, shape=(M, N))
    for axes in ((0,), (1,)):
        g = s.asformat("gcxs", compressed_axes=axes)
        r = sp.sddmm(g, at, bt=bt)
        assert isinstance(r, sp.GCXS) and tuple(r.compressed_axes) == axes
        assert np.array_equal(r.todense(), sp.sddmm(s, at, bt=bt).todense())
    want, absum = _bounds(sval.astype(np.float64), at.double().cpu().numpy(), bt.double().cpu().numpy(), coords[0], coords[1])
    assert np.all(np.abs(r.todense()[coords[0], coords[1]] - want) <= 2e-6 * absum + 1e-300)


# ---- dense-tile (matrix-core) form ----------------------------------------------------------------------------------------
def _clustered_mask(rng, M, N, n_blocks, block_density, sprinkle):
    """32 x 32 blocks filled at `block_density` plus a uniform sprinkle: (sorted unique linear indices)"""
    tr, tc = -(-M // 32), -(-N // 32)
    blocks = rng.choice(tr * tc, n_blocks, replace=False)
    lin = []
    for b in blocks:
        r0, c0 = (b // tc) * 32, (b % tc) * 32
        rr, cc = np.meshgrid(np.arange(r0, min(r0 + 32, M)), np.arange(c0, min(c0 + 32, N)), indexing="ij")
        keep = rng.random(rr.shape) < block_density
        lin.append((rr[keep] * N + cc[keep]).ravel())
    lin.append(rng.choice(M * N, sprinkle, replace=False))
    return np.unique(np.concatenate(lin))


@pytest.mark.parametrize("shape_k", [((2048, 2048), 256), ((1000, 777), 48), ((70, 3000), 16), ((513, 515), 400)])
@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_sddmm_f16_dense_tiles_on_the_matrix_cores(shape_k, idx, monkeypatch):
    """Populated tiles run as float16 MFMA tile products (v_mfma_f32_32x32x16_f16), the rest through the sampled kernel; both
    against the fp64 evaluation within 4e-6 * sum |terms|, and against each other within the same bound."""
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    (M, N), Kd = shape_k
    rng = np.random.default_rng(M + Kd)
    lin = _clustered_mask(rng, M, N, n_blocks=40, block_density=0.6, sprinkle=3000)
    coords = np.stack([lin // N, lin % N]).astype(idx)
    nnz = lin.size
    sval = (rng.random(nnz) - 0.5).astype(np.float32)
    at = torch.from_numpy(rng.random((M, Kd)) - 0.5).cuda().to(F16)
    bt = torch.from_numpy(rng.random((N, Kd)) - 0.5).cuda().to(F16)
    s = sp.COO(coords, sval, shape=(M, N))
    plan = K.sddmm_plan(s.coords, s.shape)
    assert plan.n_dense_samples > 0.5 * nnz and plan.rest.numel() > 0      # both paths are exercised
    got = K.sddmm_coo_mfma(plan, s.coords, s.shape, s.data, at, bt)
    assert got is not None, "the hybrid path declined a clustered mask"
    sampled = K.sddmm_coo(s.coords, s.data, at, bt)
    a64, b64 = at.double().cpu().numpy(), bt.double().cpu().numpy()
    want, absum = _bounds(sval.astype(np.float64), a64, b64, coords[0], coords[1])
    g = got.double().cpu().numpy()
    print(f"{shape_k}: tile path max error / sum|terms| = {(np.abs(g - want) / (absum + 1e-300)).max():.3e}")
    assert np.all(np.abs(g - want) <= 4e-6 * absum + 1e-300)
    assert np.all(np.abs(g - sampled.double().cpu().numpy()) <= 4e-6 * absum + 1e-300)
    # the samples left to the sampled kernel are bit-identical to the all-sampled result
    rest = plan.rest.cpu().numpy()
    assert np.array_equal(got.cpu().numpy()[rest], sampled.cpu().numpy()[rest])
    # product entry point (told that the tiles pay): same values, plan cached on the mask
    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: True)
    r = sp.sddmm(s, at, bt=bt)
    assert ("tiles", K.SDDMM_TILE_THRESHOLD) in s._sddmm_plan
    assert np.array_equal(r.todense()[coords[0], coords[1]], np.where(g == 0, 0, got.cpu().numpy()))


def test_sddmm_f16_and_bf16_tiles_agree_on_values_exact_in_both():
    """Operands that are exact in float16 AND bfloat16 (small integers / 8): the two MFMA forms and the two sampled forms
    compute the same sums of exact products, element for element on the tile path's fixed order."""
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(8)
    M = N = 256
    Kd = 128
    lin = _clustered_mask(rng, M, N, n_blocks=20, block_density=0.9, sprinkle=500)
    coords = torch.from_numpy(np.stack([lin // N, lin % N]).astype(np.int32)).cuda()
    sval = torch.from_numpy((rng.random(lin.size) - 0.5).astype(np.float32)).cuda()
    a = torch.from_numpy(rng.integers(-8, 9, (M, Kd)) / 8.0).cuda()
    b = torch.from_numpy(rng.integers(-8, 9, (N, Kd)) / 8.0).cuda()
    plan = K.sddmm_plan(coords, (M, N))
    assert plan.tiles.numel() > 0
    h = K.sddmm_coo_mfma(plan, coords, (M, N), sval, a.to(F16), b.to(F16), force=True)
    bf = K.sddmm_coo_mfma(plan, coords, (M, N), sval, a.to(torch.bfloat16), b.to(torch.bfloat16), force=True)
    assert torch.equal(h, bf)           # (sums of multiples of 1/64 below 2^24 / 64: exact in fp32 in any order)
    assert torch.equal(K.sddmm_coo(coords, sval, a.to(F16), b.to(F16)), K.sddmm_coo(coords, sval, a.float(), b.float()))


def test_sddmm_f16_uniform_mask_stays_on_the_sampled_kernel():
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(5)
    M = N = 4096
    lin = np.sort(rng.choice(M * N, 16000, replace=False))
    coords = np.stack([lin // N, lin % N])
    s = sp.COO(coords, rng.random(lin.size).astype(np.float32), shape=(M, N))
    at = torch.rand((M, 64), device="cuda").to(F16)
    bt = torch.rand((N, 64), device="cuda").to(F16)
    plan = K.sddmm_plan(s.coords, s.shape)
    assert plan.tiles.numel() == 0 and plan.rest.numel() == lin.size
    assert K.sddmm_coo_mfma(plan, s.coords, s.shape, s.data, at, bt) is None
    r = sp.sddmm(s, at, bt=bt)
    assert torch.equal(r.data, K.sddmm_coo(s.coords, s.data, at, bt))


def _mask(rng, M, N, nnz, idx=np.int32):
    lin = np.sort(rng.choice(M * N, nnz, replace=False))
    return np.stack([lin // N, lin % N]).astype(idx), lin


@pytest.mark.parametrize("Kd", [128, 256, 512, 2048,     # 16-, 32- and 64-lane groups, 1 / 2 / 4 vectors per lane (512: two passes)
                                384, 768, 1024, 1536])   # 3 vectors per lane; 32 x 4, 64 x 3
@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_sddmm_f16_column_panel_order_is_bit_identical(Kd, idx):
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(Kd)
    M, N, nnz = 700, 5000, 60_013
    coords_h, _ = _mask(rng, M, N, nnz, idx)
    at = (torch.rand((M, Kd), device="cuda", dtype=torch.float64) - 0.5).to(F16)
    bt = (torch.rand((N, Kd), device="cuda", dtype=torch.float64) - 0.5).to(F16)
    coords = torch.from_numpy(coords_h).cuda()
    sval = (torch.rand(nnz, device="cuda", dtype=torch.float64) - 0.5).to(torch.float32)
    assert K.sddmm_has_panels(F16, Kd)
    ref = K.sddmm_coo(coords, sval, at, bt)
    # (the row-cached kernel itself against the float64 evaluation, for every group width)
    ch = coords_h.astype(np.int64)
    want, absum = _bounds(sval.double().cpu().numpy(), at.double().cpu().numpy(), bt.double().cpu().numpy(), ch[0], ch[1])
    err = np.abs(ref.double().cpu().numpy() - want) / (absum + 1e-300)
    print(f"K={Kd}: row-cached kernel max error / sum|terms| = {err.max():.3e}")
    assert np.all(np.abs(ref.double().cpu().numpy() - want) <= 2e-6 * absum + 1e-300)
    for width, xcd in ((64, False), (64, True), (300, True), (1000, False), (4999, False), (5000, True)):
        plan = K.sddmm_panels(coords, (M, N), width, xcd=xcd)
        for chunk in (0, 16, 48, 1000):
            plan.chunk = chunk
            assert torch.equal(K.sddmm_coo(coords, sval, at, bt, panels=plan), ref), (width, chunk)
    # a subset of the elements, written into a caller-provided result
    subset = torch.from_numpy(np.sort(rng.choice(nnz, 20_001, replace=False))).cuda()
    plan = K.sddmm_panels(coords, (M, N), 300, subset=subset)
    out = torch.full((nnz,), -7.0, dtype=ref.dtype, device="cuda")
    K._sddmm_panels_into(plan, sval, sval, at, bt, out)
    keep = torch.zeros(nnz, dtype=torch.bool, device="cuda")
    keep[subset] = True
    assert torch.equal(out[keep], ref[keep]) and bool((out[~keep] == -7.0).all())


def test_sddmm_f16_product_path_uses_panels_and_follows_the_mask(monkeypatch):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "sddmm_panels_pay", lambda n, a, bt, width: bool(width))
    monkeypatch.setattr(K, "SDDMM_PANEL_BYTES", 64 * 256 * 2)   # 64 Bt rows per panel
    rng = np.random.default_rng(11)
    M, N, Kd, nnz = 500, 3000, 256, 40_000
    coords_h, _ = _mask(rng, M, N, nnz)
    sval = (rng.random(nnz) - 0.5).astype(np.float32)
    at = (torch.rand((M, Kd), device="cuda") - 0.5).to(F16)
    bt = (torch.rand((N, Kd), device="cuda") - 0.5).to(F16)
    a64, b64 = at.double().cpu().numpy(), bt.double().cpu().numpy()
    dots = np.einsum("ik,ik->i", a64[coords_h[0]], b64[coords_h[1]])
    absd = np.einsum("ik,ik->i", np.abs(a64[coords_h[0]]), np.abs(b64[coords_h[1]]))

    def check(r, values):
        got = r.todense()[coords_h[0], coords_h[1]]
        assert np.all(np.abs(got - values.astype(np.float64) * dots) <= 2e-6 * np.abs(values) * absd + 1e-300)

    s = sp.COO(coords_h, sval, shape=(M, N))
    check(sp.sddmm(s, at, bt=bt), sval)
    plans = s._sddmm_plan
    key = ("panels", "all", K.sddmm_panel_width(bt))
    assert key in plans and plans[key].count == nnz
    first = plans[key]
    check(sp.sddmm(s, at, bt=bt), sval)
    assert s._sddmm_plan[key] is first            # built once
    # the plan is the pattern's: bf16 operands of the same row length share it
    sp.sddmm(s, at.to(torch.bfloat16), bt=bt.to(torch.bfloat16))
    assert s._sddmm_plan[key] is first
    s.data.mul_(2.0)                               # in-place change of the mask values: new result, no stale values
    check(sp.sddmm(s, at, bt=bt), 2 * sval)
    g = s.asformat("gcxs", compressed_axes=(0,))
    r = sp.sddmm(g, at, bt=bt)
    assert isinstance(r, sp.GCXS)
    check(r, 2 * sval)
    view = g._coo_view
    sp.sddmm(g, at, bt=bt)
    assert g._coo_view is view and key in view._sddmm_plan


def test_sddmm_f16_mfma_rest_in_panel_order(monkeypatch):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(3)
    M = N = 2048
    Kd = 128
    tiles = rng.choice((M // 32) * (N // 32), 300, replace=False)
    pos = np.argsort(rng.random((300, 1024)), axis=1)[:, :600]
    r = (tiles // (N // 32))[:, None] * 32 + pos // 32
    c = (tiles % (N // 32))[:, None] * 32 + pos % 32
    lin = np.unique(np.concatenate([(r.astype(np.int64) * N + c).ravel(), rng.choice(M * N, 50_000, replace=False)]))
    coords_h = np.stack([lin // N, lin % N]).astype(np.int32)
    s = sp.COO(coords_h, (rng.random(lin.size) - 0.5).astype(np.float32), shape=(M, N))
    at = (torch.rand((M, Kd), device="cuda") - 0.5).to(F16)
    bt = (torch.rand((N, Kd), device="cuda") - 0.5).to(F16)
    plan = K.sddmm_plan(s.coords, s.shape)
    assert plan.tiles.numel() > 0 and plan.rest.numel() > 1000
    plain = K.sddmm_coo_mfma(plan, s.coords, s.shape, s.data, at, bt, force=True)
    restp = K.sddmm_panels(s.coords, s.shape, 100, subset=plan.rest)
    paneled = K.sddmm_coo_mfma(plan, s.coords, s.shape, s.data, at, bt, force=True, rest_panels=restp)
    assert torch.equal(plain, paneled)
    monkeypatch.setattr(K, "sddmm_panels_pay", lambda n, a, bt, width: bool(width))
    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: True)
    monkeypatch.setattr(K, "SDDMM_PANEL_BYTES", 100 * Kd * 2)
    out = sp.sddmm(s, at, bt=bt)
    assert ("panels", "rest", K.sddmm_panel_width(bt)) in s._sddmm_plan
    want = np.where(plain.cpu().numpy() == 0, 0, plain.cpu().numpy())
    assert np.array_equal(out.todense()[coords_h[0], coords_h[1]], want)


def test_sddmm_f16_dispatch_models_and_rowreuse_kernel():
    """The traffic models answer for float16 as for bfloat16 (they depend on the element size), and a block-sparse mask of
    16 384 tiles and more at K = 256 takes the row-reuse form of the tile kernel: against the fp64 evaluation."""
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(0)
    M = N = 16384
    a = torch.empty((M, 256), dtype=F16, device="cuda")
    bt = torch.empty((N, 256), dtype=F16, device="cuda")
    tiles = rng.choice((M // 32) * (N // 32), 2000, replace=False)
    full = np.arange(1024)
    lin = np.sort((((tiles // (N // 32))[:, None] * 32 + full // 32).astype(np.int64) * N + (tiles % (N // 32))[:, None] * 32 + full % 32).ravel())
    coords = torch.from_numpy(np.stack([lin // N, lin % N]).astype(np.int32)).cuda()
    plan = K.sddmm_plan(coords, (M, N))
    assert plan.tiles.numel() == 2000 and plan.rest.numel() == 0
    assert K.sddmm_tiles_pay(plan, a, bt, K.sddmm_panel_width(bt))
    w = K.sddmm_panel_width(torch.empty((100_000, 256), dtype=F16, device="cuda"))
    assert w == 6250
    # row-reuse kernel (ntiles >= 16 384): a banded block mask of 4096 x 4096 x ... tiles of 600 samples
    M = N = 8192
    tr = M // 32
    tl = np.array([(i, (i + d) % tr) for i in range(tr) for d in range(64)])            # 16 384 tiles, 64 per tile row
    pos = np.argsort(rng.random((tl.shape[0], 1024)), axis=1)[:, :520]
    r = tl[:, :1] * 32 + pos // 32
    c = tl[:, 1:] * 32 + pos % 32
    lin = np.unique((r.astype(np.int64) * N + c).ravel())
    ch = np.stack([lin // N, lin % N]).astype(np.int32)
    sval = (rng.random(lin.size) - 0.5).astype(np.float32)
    s = sp.COO(ch, sval, shape=(M, N))
    at = (torch.rand((M, 256), device="cuda") - 0.5).to(F16)
    btt = (torch.rand((N, 256), device="cuda") - 0.5).to(F16)
    plan = K.sddmm_plan(s.coords, s.shape)
    assert plan.tiles.numel() == tl.shape[0] >= 16384 and plan.rest.numel() == 0
    got = K.sddmm_coo_mfma(plan, s.coords, s.shape, s.data, at, btt, force=True).double().cpu().numpy()
    a64, b64 = at.double().cpu().numpy(), btt.double().cpu().numpy()
    sel = rng.choice(lin.size, 200_000, replace=False)
    want, absum = _bounds(sval[sel].astype(np.float64), a64, b64, ch[0][sel], ch[1][sel])
    assert np.all(np.abs(got[sel] - want) <= 4e-6 * absum + 1e-300)


@pytest.mark.parametrize("Kd", [200, 100, 33])
def test_sddmm_f16_inner_dimensions_without_a_row_cached_kernel_are_padded(Kd):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    M, N, nnz = 3000, 5000, 250_000
    s = sp.random((M, N), nnz=nnz, random_state=5, dtype=np.float32)
    at = (torch.rand((M, Kd), device="cuda", dtype=torch.float64) - 0.5).to(F16)
    bt = (torch.rand((N, Kd), device="cuda", dtype=torch.float64) - 0.5).to(F16)
    pa, pb = K.sddmm_pad_inner(at, bt, nnz)
    assert (pa.shape[1] > Kd) == (Kd != 33)        # (66-byte rows would become 256-byte ones: more than 1.5x, left alone)
    r = sp.sddmm(s, at, bt=bt)
    c = s.coords.cpu().numpy()
    want, absum = _bounds(s.data.double().cpu().numpy(), at.double().cpu().numpy(), bt.double().cpu().numpy(), c[0], c[1])
    got = r.todense()[c[0], c[1]]
    assert np.all(np.abs(got - want) <= 2e-6 * absum + 1e-300)


# ---- fp16 subnormals (|x| < 2^-14): no bf16 twin ---------------------------------------------------------------------------
def _with_subnormals(rng, shape):
    """float16 values of which every third (placed, not left to chance) is a subnormal: k * 2^-24, k in 1..1023, either sign;
    the others are normal and small enough (2^-10 .. 2^-6) that the subnormal terms are a visible share of a dot product"""
    x = (rng.integers(1, 1024, shape) * 2.0 ** -24) * rng.choice([-1.0, 1.0], shape)
    normal = rng.random(shape) * (2.0 ** -6 - 2.0 ** -10) + 2.0 ** -10
    flat = np.arange(x.size).reshape(shape)
    x = np.where(flat % 3 == 0, x, normal * rng.choice([-1.0, 1.0], shape))
    h = x.astype(np.float16)
    sub = (np.abs(h) < 2.0 ** -14) & (h != 0)
    assert sub.sum() >= x.size // 3 - 1
    return h


def _flushed(h):
    return np.where(np.abs(h) < 2.0 ** -14, np.float16(0), h)


@pytest.mark.parametrize("Kd", [7, 64, 200, 128, 256, 384, 512, 1024])   # generic gather (7, 64, 200) and every row-cached group width
def test_sddmm_f16_subnormal_operands_on_the_sampled_kernels(Kd):
    """One operand all subnormals against normal values of 2^-2 .. 2^0 (every term of every dot product has a subnormal
    factor: flushed inputs would give exactly 0), and both operands with every third value subnormal; own order and panel
    order.  Bound: 2e-6 * sum|terms| against the evaluation on the UNFLUSHED inputs."""
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(Kd)
    M, N, nnz = 300, 400, 20_000
    coords_h, _ = _mask(rng, M, N, nnz)
    coords = torch.from_numpy(coords_h).cuda()
    sval = torch.from_numpy((rng.random(nnz) + 0.5).astype(np.float32)).cuda()
    all_sub = ((rng.integers(1, 1024, (M, Kd)) * 2.0 ** -24) * rng.choice([-1.0, 1.0], (M, Kd))).astype(np.float16)
    normal = ((rng.random((N, Kd)) * 0.75 + 0.25) * rng.choice([-1.0, 1.0], (N, Kd))).astype(np.float16)
    for a_h, b_h, tag in ((all_sub, normal, "subnormal x normal"), (_with_subnormals(rng, (M, Kd)), _with_subnormals(rng, (N, Kd)), "mixed")):
        at, bt = torch.from_numpy(a_h).cuda(), torch.from_numpy(b_h).cuda()
        got = K.sddmm_coo(coords, sval, at, bt)
        want, absum = _bounds(sval.double().cpu().numpy(), a_h.astype(np.float64), b_h.astype(np.float64), coords_h[0], coords_h[1])
        g = got.double().cpu().numpy()
        wf, _ = _bounds(sval.double().cpu().numpy(), _flushed(a_h).astype(np.float64), _flushed(b_h).astype(np.float64), coords_h[0], coords_h[1])
        print(f"K={Kd} {tag}: max error / sum|terms| = {(np.abs(g - want) / absum).max():.3e} (against flushed inputs: "
              f"{(np.abs(g - wf) / absum).max():.3e})")
        assert np.all(np.abs(g - want) <= 2e-6 * absum)
        if K.sddmm_has_panels(F16, Kd):
            plan = K.sddmm_panels(coords, (M, N), 64)
            assert torch.equal(K.sddmm_coo(coords, sval, at, bt, panels=plan), got)


SUBNORMALS_FLUSHED_BY_THE_F16_MFMA = False     # measured on MI355X: v_mfma_f32_32x32x16_f16 keeps them, 1.5e-7 at most


@pytest.mark.parametrize("Kd", [16, 128, 256])
def test_sddmm_f16_subnormal_operands_on_the_tile_path(Kd):
    """The same operands through the matrix-core tiles (every tile sample against the evaluation on the unflushed inputs,
    4e-6 * sum|terms|); the left-over samples are the sampled kernel's and keep the unflushed form either way."""
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(Kd)
    M, N = 256, 320
    lin = _clustered_mask(rng, M, N, n_blocks=30, block_density=0.8, sprinkle=2000)
    coords_h = np.stack([lin // N, lin % N]).astype(np.int32)
    nnz = lin.size
    coords = torch.from_numpy(coords_h).cuda()
    sval = torch.from_numpy((rng.random(nnz) + 0.5).astype(np.float32)).cuda()
    all_sub = ((rng.integers(1, 1024, (M, Kd)) * 2.0 ** -24) * rng.choice([-1.0, 1.0], (M, Kd))).astype(np.float16)
    normal = ((rng.random((N, Kd)) * 0.75 + 0.25) * rng.choice([-1.0, 1.0], (N, Kd))).astype(np.float16)
    plan = K.sddmm_plan(coords, (M, N))
    assert plan.tiles.numel() > 0 and plan.rest.numel() > 0
    rest = plan.rest.cpu().numpy()
    tile = np.setdiff1d(np.arange(nnz), rest)
    for a_h, b_h, tag in ((all_sub, normal, "subnormal x normal"), (_with_subnormals(rng, (M, Kd)), _with_subnormals(rng, (N, Kd)), "mixed")):
        at, bt = torch.from_numpy(a_h).cuda(), torch.from_numpy(b_h).cuda()
        g = K.sddmm_coo_mfma(plan, coords, (M, N), sval, at, bt, force=True).double().cpu().numpy()
        sv = sval.double().cpu().numpy()
        want, absum = _bounds(sv, a_h.astype(np.float64), b_h.astype(np.float64), coords_h[0], coords_h[1])
        wf, _ = _bounds(sv, _flushed(a_h).astype(np.float64), _flushed(b_h).astype(np.float64), coords_h[0], coords_h[1])
        eu, ef = np.abs(g - want)[tile] / absum[tile], np.abs(g - wf)[tile] / absum[tile]
        print(f"K={Kd} {tag}: tile samples max error / sum|terms| = {eu.max():.3e} against the unflushed inputs, "
              f"{ef.max():.3e} against inputs with subnormals zeroed")
        ref = wf if SUBNORMALS_FLUSHED_BY_THE_F16_MFMA else want
        assert np.all(np.abs(g - ref)[tile] <= 4e-6 * absum[tile])
        assert np.all(np.abs(g - want)[rest] <= 2e-6 * absum[rest])

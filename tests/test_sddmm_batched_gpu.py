"""SDDMM with an N-D mask: the leading axes of `a` and `b` broadcast against the mask's, the whole stack is ONE product over the
folded coordinates (csrc/sddmm_batch.hip).  Two references: the float64 evaluation `s.todense() * (a64 @ b64)` at the stored
positions within the 2-D kernels' bounds (2e-6 * sum|terms| sampled, 4e-6 tiles, 1e-14 float64), and the Python loop of 2-D
`sddmm` calls over the batch, bit for bit (the folded call runs the same kernel over the same operand rows; where the route -
panels, tiles, padding - could differ between the folded call and a slice it is pinned, as tests/test_sddmm_gpu.py pins it)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}


def _nd_mask(rng, shape, nnz, idx=np.int64):
    lin = np.sort(rng.choice(int(np.prod(shape)), nnz, replace=False))
    return np.stack(np.unravel_index(lin, shape)).astype(idx)


def _reference(coords, sval, a64, b64t, lead):
    """float64 value and sum|terms| of every stored element; a64 [la..., M, K], b64t [lb..., N, K] broadcast to `lead`."""
    p = len(lead)
    ab = np.broadcast_to(a64, lead + a64.shape[-2:])
    bb = np.broadcast_to(b64t, lead + b64t.shape[-2:])
    li = tuple(coords[d] for d in range(p))
    ar, br = ab[li + (coords[p],)], bb[li + (coords[p + 1],)]
    return sval * np.einsum("ik,ik->i", ar, br), np.abs(sval) * np.einsum("ik,ik->i", np.abs(ar), np.abs(br))


def _loop_of_2d_calls(sp, s, at, btt, lead):
    """The loop the folded call replaces: one 2-D `sddmm` per batch index, operands sliced by NumPy's broadcasting rule."""
    p = len(lead)
    out = np.zeros(s.shape, dtype=np.float64 if at.dtype == torch.float64 else np.float32)

    def pick(x, index):
        xl = (1,) * (p - (x.dim() - 2)) + tuple(x.shape[:-2])
        x = x.reshape(xl + tuple(x.shape[-2:]))
        return x[tuple(0 if xl[d] == 1 else index[d] for d in range(p))]

    for index in itertools.product(*[range(n) for n in lead]):
        sl = s[index]
        out[index] = sp.sddmm(sl, pick(at, index), bt=pick(btt, index)).todense()
    return out


LEADS = [  # (mask's leading shape, a's, b's)
    ((3,), (3,), (3,)), ((3,), (), (3,)), ((3,), (3,), ()), ((3,), (), ()), ((3,), (1,), (3,)), ((3,), (3,), (1,)),
    ((2, 3), (2, 3), (2, 3)), ((2, 3), (3,), (2, 1)), ((2, 3), (2, 1), (1, 3)), ((2, 3), (1, 1), (2, 3)), ((2, 3), (), (3,)),
    ((1, 3), (1, 3), (3,)),
]


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32", "f64"])
@pytest.mark.parametrize("lead, la, lb", LEADS)
def test_batched_sddmm_against_float64_and_the_loop(dt, lead, la, lb, monkeypatch):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: False)      # one route for the stack and its slices
    seed = len(lead) * 100 + len(la) * 10 + len(lb) + sum(la) + 7 * sum(lb)
    rng = np.random.default_rng(seed)
    M, N, Kd = 70, 90, {"f16": 64, "bf16": 200, "f32": 64, "f64": 24}[dt]
    shape = lead + (M, N)
    nnz = 2500 * int(np.prod(lead))
    idx = np.int32 if seed % 2 else np.int64
    coords = _nd_mask(rng, shape, nnz, idx)
    vdt = np.float64 if dt == "f64" else np.float32
    sval = (rng.random(nnz) - 0.5).astype(vdt)
    at = (torch.rand(la + (M, Kd), device="cuda", dtype=torch.float64) - 0.5).to(TDT[dt])
    btt = (torch.rand(lb + (N, Kd), device="cuda", dtype=torch.float64) - 0.5).to(TDT[dt])
    s = sp.COO(coords, sval, shape=shape)
    r = sp.sddmm(s, at, bt=btt)
    assert isinstance(r, sp.COO) and r.shape == shape and r.dtype == vdt
    c64 = coords.astype(np.int64)
    want, absum = _reference(c64, sval.astype(np.float64), at.double().cpu().numpy(), btt.double().cpu().numpy(), lead)
    got = r.todense()
    g = got[tuple(c64)]
    tol = 1e-14 if dt == "f64" else 2e-6
    print(f"{dt} {lead} {la} {lb}: max error / sum|terms| = {(np.abs(g - want) / (absum + 1e-300)).max():.3e}")
    assert np.all(np.abs(g - want) <= tol * absum + 1e-300)
    assert np.count_nonzero(got) == np.count_nonzero(g) == r.nnz
    assert np.array_equal(got, _loop_of_2d_calls(sp, s, at, btt, lead))
    # b given as (..., K, N): transposed per batch
    rb = sp.sddmm(s, at, btt.transpose(-1, -2).contiguous())
    assert np.array_equal(rb.todense(), got)
    # a GCXS mask goes through its kept COO view and comes back as GCXS
    gx = s.asformat("gcxs")
    rg = sp.sddmm(gx, at, bt=btt)
    assert isinstance(rg, sp.GCXS) and tuple(rg.compressed_axes) == tuple(gx.compressed_axes)
    assert np.array_equal(rg.todense(), got)
    assert ("fold", la, lb) in gx._coo_view._sddmm_plan


def test_batched_sddmm_numpy_operands_and_4d_mask(monkeypatch):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: False)
    rng = np.random.default_rng(40)
    lead, M, N, Kd = (2, 1, 3), 40, 33, 128
    shape = lead + (M, N)
    coords = _nd_mask(rng, shape, 4000, np.int32)
    sval = (rng.random(4000) - 0.5).astype(np.float32)
    a = (rng.random((2, 1, 1, M, Kd)) - 0.5).astype(np.float16)
    b = (rng.random((3, Kd, N)) - 0.5).astype(np.float16)
    s = sp.COO(coords, sval, shape=shape)
    r = sp.sddmm(s, a, b)
    c64 = coords.astype(np.int64)
    want, absum = _reference(c64, sval.astype(np.float64), a.astype(np.float64), np.swapaxes(b, -1, -2).astype(np.float64), lead)
    assert np.all(np.abs(r.todense()[tuple(c64)] - want) <= 2e-6 * absum + 1e-300)
    at, btt = torch.from_numpy(a).cuda(), torch.from_numpy(np.ascontiguousarray(np.swapaxes(b, -1, -2))).cuda()
    assert np.array_equal(r.todense(), _loop_of_2d_calls(sp, s, at, btt, lead))


def test_batched_sddmm_shape_errors():
    import sparse_amd as sp

    s = sp.COO(np.zeros((3, 1), dtype=np.int64), np.ones(1, np.float32), shape=(3, 5, 6))
    z = lambda *shape: torch.zeros(shape, device="cuda")      # noqa: E731
    with pytest.raises(ValueError, match="more leading axes"):
        sp.sddmm(s, z(1, 3, 5, 8), bt=z(6, 8))
    with pytest.raises(ValueError, match="do not broadcast"):
        sp.sddmm(s, z(2, 5, 8), bt=z(6, 8))
    with pytest.raises(ValueError, match="do not broadcast"):
        sp.sddmm(s, z(5, 8), bt=z(4, 6, 8))
    with pytest.raises(ValueError, match="shape-mismatch"):
        sp.sddmm(s, z(3, 5, 8), bt=z(3, 6, 9))
    with pytest.raises(ValueError, match="shape-mismatch"):
        sp.sddmm(s, z(3, 6, 8), bt=z(3, 6, 8))
    s2 = sp.COO(np.zeros((2, 1), dtype=np.int64), np.ones(1, np.float32), shape=(5, 6))
    with pytest.raises(ValueError, match="more leading axes"):       # an operand may not be larger than the mask
        sp.sddmm(s2, z(3, 5, 8), bt=z(6, 8))


def test_batched_sddmm_empty_batch_and_empty_mask():
    import sparse_amd as sp

    e = sp.COO(np.zeros((3, 0), dtype=np.int64), np.zeros(0, np.float32), shape=(4, 5, 6))
    r = sp.sddmm(e, torch.zeros((4, 5, 8), device="cuda"), bt=torch.zeros((6, 8), device="cuda"))
    assert r.nnz == 0 and r.shape == (4, 5, 6)
    z = sp.COO(np.zeros((3, 0), dtype=np.int64), np.zeros(0, np.float32), shape=(0, 5, 6))
    r = sp.sddmm(z, torch.zeros((0, 5, 8), device="cuda", dtype=torch.float16), bt=torch.zeros((0, 6, 8), device="cuda", dtype=torch.float16))
    assert r.nnz == 0 and r.shape == (0, 5, 6)
    r = sp.sddmm(z, torch.zeros((5, 8), device="cuda"), bt=torch.zeros((6, 8), device="cuda"))
    assert r.nnz == 0 and r.shape == (0, 5, 6)
    # a mask one of whose batches is empty
    rng = np.random.default_rng(1)
    c = _nd_mask(rng, (3, 20, 30), 500)
    c = c[:, c[0] != 1]
    s = sp.COO(c, np.ones(c.shape[1], np.float32), shape=(3, 20, 30))
    at, btt = torch.rand((3, 20, 16), device="cuda"), torch.rand((3, 30, 16), device="cuda")
    got = sp.sddmm(s, at, bt=btt).todense()
    assert not got[1].any() and got[0].any() and got[2].any()
    assert np.array_equal(got, _loop_of_2d_calls(sp, s, at, btt, (3,)))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_batched_sddmm_duplicate_pairs_fill_a_tile_past_1024_samples(dt, monkeypatch):
    """A 2-D operand pair under a 3-D mask: every slice folds to the same (row', col') pairs, so a 32 x 32 tile of the folded
    problem holds B x 1024 samples.  Tile path forced on: the tile kernels' sample loops stride over a run of any length; the
    left-over samples (duplicates as well) go through the sampled kernel in panel order.  Bit-identical to the slices."""
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: True)
    rng = np.random.default_rng(6)
    B, M, N, Kd = 5, 128, 160, 128
    dense_tiles = [(0, 0), (1, 3), (3, 4)]
    lin = []
    for b in range(B):
        for (tr, tc) in dense_tiles:                            # full tiles in every slice: 5 x 1024 samples per folded tile
            rr, cc = np.meshgrid(np.arange(tr * 32, tr * 32 + 32), np.arange(tc * 32, tc * 32 + 32), indexing="ij")
            lin.append((b * M + rr.ravel()) * N + cc.ravel())
        lin.append(b * M * N + rng.choice(M * N, 1500, replace=False))
    lin = np.unique(np.concatenate(lin))
    coords = np.stack(np.unravel_index(lin, (B, M, N))).astype(np.int32)
    sval = (rng.random(lin.size) - 0.5).astype(np.float32)
    s = sp.COO(coords, sval, shape=(B, M, N))
    at = (torch.rand((M, Kd), device="cuda") - 0.5).to(TDT[dt])
    btt = (torch.rand((N, Kd), device="cuda") - 0.5).to(TDT[dt])
    r = sp.sddmm(s, at, bt=btt)
    fold = s._sddmm_plan[("fold", (), ())]
    plan = fold[("tiles", K.SDDMM_TILE_THRESHOLD)]
    seg = plan.seg_start.cpu().numpy()
    runs = np.array([seg[t + 1] - seg[t] for t in plan.tiles.cpu().numpy()])
    assert runs.size == len(dense_tiles) and runs.min() >= B * 1024 > 1024
    assert plan.rest.numel() > 0 and any(k[:2] == ("panels", "rest") for k in fold if isinstance(k, tuple))
    c64 = coords.astype(np.int64)
    want, absum = _reference(c64, sval.astype(np.float64), at.double().cpu().numpy(), btt.double().cpu().numpy(), (B,))
    got = r.todense()
    assert np.all(np.abs(got[tuple(c64)] - want) <= 4e-6 * absum + 1e-300)
    assert np.array_equal(got, _loop_of_2d_calls(sp, s, at, btt, (B,)))
    # the same duplicates through the sampled kernel alone, in the mask's own order and in panel order
    fc = fold["coords"]
    own = K.sddmm_coo(fc, s.data, at, btt)
    pan = K.sddmm_coo(fc, s.data, at, btt, panels=K.sddmm_panels(fc, (M, N), 64))
    assert torch.equal(own, pan)
    assert np.all(np.abs(own.double().cpu().numpy() - want) <= 2e-6 * absum + 1e-300)


def test_fold_kernel_against_numpy_and_int64_extents():
    """The fold kernel alone: int32 / int64 coordinates, and extents past 2^31 (Ba * M > 2^31 on a tiny mask: the 2-D kernels
    take contiguous operands, so the product itself is not run at that extent - no buffer of that size is allocated)."""
    from sparse_amd import _kernels as K

    rng = np.random.default_rng(9)
    for idx in (np.int32, np.int64):
        lead, M, N = (4, 3), 50, 60
        coords = _nd_mask(rng, lead + (M, N), 5000, idx)
        for la, lb in (((4, 3), (4, 3)), ((3,), (4, 1)), ((), ()), ((4, 1), (3,))):
            sa, nba = K.sddmm_fold_strides(lead, la, "a")
            sb, nbb = K.sddmm_fold_strides(lead, lb, "b")
            out = K.sddmm_fold(torch.from_numpy(coords).cuda(), 2, sa, sb, M, N, nba * M, nbb * N)
            assert out.dtype == torch.int32 and out.shape == (2, 5000)
            c = coords.astype(np.int64)
            assert np.array_equal(out[0].cpu().numpy(), (c[0] * sa[0] + c[1] * sa[1]) * M + c[2])
            assert np.array_equal(out[1].cpu().numpy(), (c[0] * sb[0] + c[1] * sb[1]) * N + c[3])
    # Ba * M = 70 000 * 40 000 = 2.8 x 10^9 > 2^31; b broadcast
    lead, M, N = (70_000,), 40_000, 50_000
    coords = np.array([[0, 1, 53_687, 53_688, 69_999], [0, 39_999, 3_648, 1, 39_999], [7, 0, 49_999, 2, 49_999]], dtype=np.int32)
    sa, nba = K.sddmm_fold_strides(lead, lead, "a")
    sb, nbb = K.sddmm_fold_strides(lead, (), "b")
    assert nba * M > 2 ** 31 and nbb * N < 2 ** 31
    out = K.sddmm_fold(torch.from_numpy(coords).cuda(), 1, sa, sb, M, N, nba * M, nbb * N)
    assert out.dtype == torch.int64
    c = coords.astype(np.int64)
    assert np.array_equal(out[0].cpu().numpy(), c[0] * M + c[1]) and out[0].max().item() == 69_999 * 40_000 + 39_999 > 2 ** 31
    assert np.array_equal(out[1].cpu().numpy(), c[2])


def test_batched_sddmm_builds_fold_and_plans_once_per_mask_and_leading_shapes(monkeypatch):
    import sparse_amd as sp
    from sparse_amd import _kernels as K

    monkeypatch.setattr(K, "sddmm_panels_pay", lambda n, a, bt, width: bool(width))
    monkeypatch.setattr(K, "sddmm_tiles_pay", lambda plan, a, bt, width: False)
    monkeypatch.setattr(K, "SDDMM_PANEL_BYTES", 64 * 256 * 2)   # 64 Bt rows per panel
    rng = np.random.default_rng(12)
    B, M, N, Kd, nnz = 4, 300, 800, 256, 30_000
    coords = _nd_mask(rng, (B, M, N), nnz, np.int32)
    sval = (rng.random(nnz) - 0.5).astype(np.float32)
    s = sp.COO(coords, sval, shape=(B, M, N))
    at = (torch.rand((B, M, Kd), device="cuda") - 0.5).to(torch.float16)
    btt = (torch.rand((B, N, Kd), device="cuda") - 0.5).to(torch.float16)
    calls = []
    real_fold = K.sddmm_fold
    monkeypatch.setattr(K, "sddmm_fold", lambda *a, **k: calls.append(1) or real_fold(*a, **k))
    r1 = sp.sddmm(s, at, bt=btt)
    fold = s._sddmm_plan[("fold", (B,), (B,))]
    pkey = ("panels", "all", K.sddmm_panel_width(btt.reshape(B * N, Kd)))
    assert pkey in fold and fold[pkey].count == nnz and fold["coords"].shape == (2, nnz)
    first_coords, first_panels = fold["coords"], fold[pkey]
    r2 = sp.sddmm(s, at, bt=btt)
    assert len(calls) == 1 and s._sddmm_plan[("fold", (B,), (B,))]["coords"] is first_coords and fold[pkey] is first_panels
    assert np.array_equal(r1.todense(), r2.todense())
    # other leading shapes of the operands: a fold of their own, next to the first
    sp.sddmm(s, at[0], bt=btt)
    assert len(calls) == 2 and ("fold", (), (B,)) in s._sddmm_plan and s._sddmm_plan[("fold", (B,), (B,))] is fold
    # panel order against the mask's own order on the folded coordinates: bit-identical, as in 2-D
    own = K.sddmm_coo(first_coords, s.data, at.reshape(B * M, Kd), btt.reshape(B * N, Kd))
    assert torch.equal(own, K.sddmm_coo(first_coords, s.data, at.reshape(B * M, Kd), btt.reshape(B * N, Kd), panels=first_panels))
    assert np.array_equal(r1.todense()[tuple(coords.astype(np.int64))], np.where(own.cpu().numpy() == 0, 0, own.cpu().numpy()))
    # the fold lives and dies with the mask's other derived layouts (`_validate_derived`): a stored buffer written in place or
    # replaced drops it, and the next call folds again - no stale values, no stale coordinates
    s.data.mul_(2.0)
    r3 = sp.sddmm(s, at, bt=btt)
    assert len(calls) == 3 and np.array_equal(r3.todense(), 2 * r1.todense())
    assert ("fold", (), (B,)) not in s._sddmm_plan
    s.coords = s.coords.clone()
    sp.sddmm(s, at, bt=btt)
    assert len(calls) == 4 and s._sddmm_plan[("fold", (B,), (B,))]["coords"] is not first_coords

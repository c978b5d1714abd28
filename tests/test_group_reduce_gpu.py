"""The grouped reduce (csrc/group_reduce.hip: `spamd_group_reduce`) and `spamd_segment_reduce` against the host
references of tests/reduce_cases.py.

Every layout there puts run boundaries on the kernel's units (4 elements per thread, 256 per wave, 2048 per tile, 32
head-less tiles per fast walk); every (op, dtype) of its table has data whose result is exact in any association, so the
comparison is EQUALITY and one dropped, duplicated or mis-assigned element shows.  The only tolerances are the two derived
ones: Higham's any-order bound gamma_(m-1) * sum|v| for float sums of real-valued data, and bit-for-bit agreement with a
left-to-right loop for the sequential kernel.  Group ids, run lengths and the group count are compared exactly everywhere.
Both id paths run: `key_bound` below 2^53 (double precision, `GroupOfD`) and 0 / above 2^53 (integer, `GroupOf`).
Keys of 2^62 or more are never put on the device: the top of the key range is settled on the host (test_group_of_host.py).
"""
import functools

import numpy as np
import pytest
import torch

import reduce_cases as RC

pytestmark = pytest.mark.gpu

LAYOUTS = RC.layouts()
DIVISOR = 100_003           # above the longest run of any layout (33 tiles + 2)
_IDS = [f"{op}-{np.dtype(dt).name}" for op, dt in RC.TABLE]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _group_reduce(keys, divisor, data, op, key_bound):
    """the C ABI through `_reduce.group_reduce`; everything read back: (group ids, values, run lengths, [groups, 0])"""
    from sparse_amd import _reduce as R

    gids, vals, counts, ng = R.group_reduce(_dev(keys), divisor, _dev(data), op, key_bound=key_bound, sync=False)
    torch.cuda.synchronize()
    ng = ng.cpu().tolist()
    c = max(0, min(int(ng[0]), len(keys)))
    return gids[:c].cpu().numpy(), vals[:c].cpu().numpy(), counts[:c].cpu().numpy(), ng


def _runs_of_keys(keys, divisor):
    """(heads, group ids) of sorted keys by Python integer floor division; element 0 starts a run whatever its group"""
    g = [int(k) // divisor for k in keys]
    heads = [i for i in range(len(g)) if i == 0 or g[i] != g[i - 1]]
    return np.asarray(heads, dtype=np.int64), np.asarray([g[i] for i in heads], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _layout_keys(name):
    heads, n = LAYOUTS[name]
    keys, gids = RC.make_keys(heads, n, DIVISOR, np.random.default_rng(len(name) + n))
    return keys, gids, (int(gids[-1]) + 1) * DIVISOR


def _check_structure(got, gids, heads, n, what):
    g, v, c, ng = got
    assert ng == [len(heads), 0], (what, ng, len(heads))
    assert np.array_equal(g, gids), what
    assert np.array_equal(c, RC.run_lengths(heads, n)), what


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_layout_op_and_dtype_on_both_id_paths(name):
    """layout x table x {double-precision ids, integer ids}: values, group ids, run lengths and the group count all equal
    the reference's; the two id paths give the same bytes"""
    heads, n = LAYOUTS[name]
    keys, gids, bound = _layout_keys(name)
    for op, dtype in RC.TABLE:
        data = RC.make_data(op, dtype, heads, n, np.random.default_rng(11))
        want = RC.reference(op, data, heads, n)
        outs = []
        for key_bound in (bound, 0):
            what = (name, op, np.dtype(dtype).name, key_bound)
            got = _group_reduce(keys, DIVISOR, data, op, key_bound)
            _check_structure(got, gids, heads, n, what)
            assert RC.same_values(got[1], want), (what, np.flatnonzero(~((got[1] == want) | ((got[1] != got[1]) & (want != want))))[:8])
            outs.append(got)
        assert outs[0][1].tobytes() == outs[1][1].tobytes(), (name, op, dtype)


@pytest.mark.parametrize("dtype", RC.FLOAT_DTYPES)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_float_sums_of_real_values_within_the_any_order_bound(name, dtype):
    """uniform values in [-1, 1): every run against math.fsum, within gamma_(m-1) * sum|v| + u |exact| (Higham: m terms added
    in any order in the value type; the second term is the rounding of the exact sum itself).  No other slack."""
    heads, n = LAYOUTS[name]
    keys, gids, bound = _layout_keys(name)
    data = RC.rounding_data(dtype, n, np.random.default_rng(13))
    exact, tol = RC.fsum_reference(data, heads, n)
    for key_bound in (bound, 0):
        got = _group_reduce(keys, DIVISOR, data, "add", key_bound)
        _check_structure(got, gids, heads, n, (name, key_bound))
        err = np.abs(got[1].astype(np.float64) - exact)
        worst = int(np.argmax(err - tol))
        print(f"{name} {np.dtype(dtype).name} key_bound={key_bound}: worst run {worst} error {err[worst]:.3e} bound {tol[worst]:.3e}")
        assert np.all(err <= tol), (name, key_bound, worst, err[worst], tol[worst])


def test_the_first_element_starts_a_run_whatever_its_group():
    """a first key of group -1 (no valid key; what an unwritten buffer may hold) equals the kernels' "nothing before" mark:
    it is a run all the same, with id -1, and every later run keeps its place"""
    heads, n = LAYOUTS["thread"]
    keys = _layout_keys("thread")[0].copy()   # (run 0 of the layout is element 0, run 1 elements 1 and 2)
    data = RC.make_data("add", np.int64, heads, n, np.random.default_rng(3))
    for first in (-1, -DIVISOR):
        keys[0] = first
        for at in (1, 3):                    # the odd key alone in its run / followed by two elements of another group
            k = keys.copy()
            k[1:at] = first
            want_heads, want_gids = _runs_of_keys(k, DIVISOR)
            assert want_gids[0] == -1 and want_heads[1] == at
            for key_bound in (int(k[-1]) + 1, 0):
                got = _group_reduce(k, DIVISOR, data, "add", key_bound)
                _check_structure(got, want_gids, want_heads, n, (first, at, key_bound))
                assert np.array_equal(got[1], RC.reference("add", data, want_heads, n)), (first, at, key_bound)


@pytest.mark.parametrize("top,key_bound", [(2 ** 53, 2 ** 53), (2 ** 62, 0), (2 ** 62, 2 ** 53 + 1)],
                         ids=["double-below-2^53", "integer-unknown-bound", "integer-bound-2^53+1"])
def test_group_ids_at_the_top_of_each_key_range(top, key_bound):
    """keys at q d - 1, q d, q d + 1 up to `top` - 1 for six divisors: ids from Python integers.  Below 2^53 the keys include
    those where the double-precision guess of the quotient is one too small (tests/test_reduce_cases.py asserts there are
    some): the `r >= d` correction decides them."""
    heads, n = LAYOUTS["thread"]
    data = RC.make_data("add", np.int64, heads, n, np.random.default_rng(5))
    want = RC.reference("add", data, heads, n)
    for d in RC.RANGE_DIVISORS:
        keys, _, _ = RC.range_keys(heads, n, d, top, np.random.default_rng(d % 1000))
        assert 0 <= int(keys.min()) and int(keys.max()) < min(top, 2 ** 62)
        want_heads, want_gids = _runs_of_keys(keys, d)
        assert np.array_equal(want_heads, heads)
        got = _group_reduce(keys, d, data, "add", key_bound)
        _check_structure(got, want_gids, heads, n, (d, top, key_bound))
        assert np.array_equal(got[1], want), (d, top, key_bound)


# ---- the scan and fix-up switch-overs ----------------------------------------------------------------------------------
SCALE_N = [16383 * RC.TILE, 16384 * RC.TILE, 16384 * RC.TILE + 1]
# (n, whether the array holds the run that raises the chain).  The chained fix-up redoes EVERY boundary run, the fast walk's
# included: the two-launch form runs once more without it, so that what `gr_fix_fast_kernel` wrote is what is compared.
SCALE_CASES = [(n, True) for n in SCALE_N] + [(SCALE_N[2], False)]


@functools.lru_cache(maxsize=1)
def _scale_case(n, chain):
    """runs of 1..40 elements, one run over 40 head-less tiles (the chained fix-up; only with `chain`) and one over 20 (the
    fast walk); keys `gid * DIVISOR + position in the run`"""
    rng = np.random.default_rng(n % 1009)
    lens = rng.integers(1, 41, size=n // 20 + 1000)
    if chain:
        lens[len(lens) // 3] = 41 * RC.TILE + 5       # wherever it starts, at least 40 whole tiles without a head
    lens[2 * len(lens) // 3] = 21 * RC.TILE + 5
    heads = np.concatenate([[0], np.cumsum(lens)])
    assert heads[-1] >= n
    heads = heads[heads < n].astype(np.int64)
    lens = RC.run_lengths(heads, n)
    assert np.sort(lens)[-2:].tolist() == ([21 * RC.TILE + 5, 41 * RC.TILE + 5] if chain else [40, 21 * RC.TILE + 5])    # whole, inside the array
    gids = np.cumsum(rng.integers(1, 3, size=len(heads))) - 1
    keys = np.repeat(gids * DIVISOR - heads, lens) + np.arange(n, dtype=np.int64)
    return heads, gids.astype(np.int64), keys, (int(gids[-1]) + 1) * DIVISOR


@pytest.mark.parametrize("dtype,id_path", [(np.int64, "double"), (np.float32, "integer")])
@pytest.mark.parametrize("n,chain", SCALE_CASES, ids=[f"{n}-{'chain' if c else 'walk-only'}" for n, c in SCALE_CASES])
def test_scan_and_fix_up_switch_overs_with_many_runs(n, chain, dtype, id_path):
    """16383 tiles: the small scan's last size; 16384: the library scan with the one-launch fix-up; 16384 tiles + 1 element:
    the two-launch fix-up, with and without a run long enough for the chain.  About 1.6 million runs each, every one compared
    (int64 sums wrap, float32 sums are exact)."""
    from sparse_amd import _reduce as R

    heads, gids, keys, bound = _scale_case(n, chain)
    data = RC.make_data("add", dtype, heads, n, np.random.default_rng(17))
    want = RC.reference("add", data, heads, n)
    g, v, c, ng = R.group_reduce(_dev(keys), DIVISOR, _dev(data), "add", key_bound=bound if id_path == "double" else 0, sync=False)
    torch.cuda.synchronize()
    assert ng.cpu().tolist() == [len(heads), 0]
    assert torch.equal(g[:len(heads)].cpu(), torch.from_numpy(gids))
    assert torch.equal(c[:len(heads)].cpu(), torch.from_numpy(RC.run_lengths(heads, n)))
    got = v[:len(heads)].cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_misaligned_operands_are_refused():
    """keys and data must be 16-byte aligned (include/sparse_amd.h): a pointer one element in is SPAMD_EINVAL, nothing runs"""
    from sparse_amd import _ffi
    from sparse_amd._device import ptr, stream_ptr

    n = 4099
    keys = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    out = [torch.full((n + 1,), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    ng = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for code, data in ((_ffi.I64, torch.ones(n + 1, dtype=torch.int64, device="cuda")), (_ffi.F32, torch.ones(n + 4, dtype=torch.float32, device="cuda")),
                       (_ffi.U8, torch.ones(n + 16, dtype=torch.uint8, device="cuda"))):
        ws_bytes = int(_ffi.lib().spamd_group_reduce_ws_bytes(code, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        assert ptr(keys) % 16 == 0 and ptr(data) % 16 == 0
        for k, d in ((keys[1:], data), (keys, data[1:]), (keys[1:], data[1:])):
            assert ptr(k) % 16 or ptr(d) % 16
            with pytest.raises(_ffi.HipBackendError, match="invalid argument") as e:
                _ffi.call("spamd_group_reduce", 0, code, n, ptr(k), 3, 0, ptr(d), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ng), ptr(ws),
                          ws_bytes, stream_ptr(keys.device))
            assert e.value.code == -1
    torch.cuda.synchronize()
    assert ng.tolist() == [-7, -7] and all(bool((o == -7).all()) for o in out)


# ---- spamd_segment_reduce ----------------------------------------------------------------------------------------------
def _segment_reduce(data, heads, n, op, sequential):
    from sparse_amd import _kernels as K
    from sparse_amd import _reduce as R

    flags = K.flag_heads(_dev(RC.run_of(heads, n)))
    offs = K.exclusive_scan(flags)
    assert int(offs[n]) == len(heads)
    out, counts = R.segment_reduce(_dev(data), flags, offs, len(heads), op, want_counts=True, sequential=sequential)
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy()


def _segment_layouts():
    out = dict(LAYOUTS)
    base = LAYOUTS["walk_31"]
    out["walk_31_quotient_23"] = RC.pad_to_quotient(*base, 23)          # one thread per run ...
    out["walk_31_quotient_24"] = RC.pad_to_quotient(*base, 24)          # ... and one wave per run: the switch is n / runs >= 24
    return out


SEGMENT_LAYOUTS = _segment_layouts()


@pytest.mark.parametrize("name", list(SEGMENT_LAYOUTS))
def test_segment_reduce_every_layout_op_and_dtype(name):
    """the same layouts and table through `spamd_segment_reduce`: the kernel its run lengths choose (thread per run below
    n / runs = 24, wave per run from there) and the thread-per-run kernel forced; run lengths compared exactly"""
    heads, n = SEGMENT_LAYOUTS[name]
    lens = RC.run_lengths(heads, n)
    for op, dtype in RC.TABLE:
        data = RC.make_data(op, dtype, heads, n, np.random.default_rng(19))
        want = RC.reference(op, data, heads, n)
        for sequential in (False, True):
            got, counts = _segment_reduce(data, heads, n, op, sequential)
            assert np.array_equal(counts, lens), (name, op, dtype, sequential)
            assert RC.same_values(got, want), (name, op, np.dtype(dtype).name, sequential)


@pytest.mark.parametrize("dtype", RC.FLOAT_DTYPES)
@pytest.mark.parametrize("name", ["thread", "edges", "walk_31_quotient_23", "walk_31_quotient_24", "open_end_8193", "tile_exact_10241"])
def test_segment_reduce_float_sums_of_real_values(name, dtype):
    """the thread-per-run kernel adds strictly left to right: bit for bit a loop in the value type; the wave-per-run tree is
    held to the any-order bound against math.fsum"""
    heads, n = SEGMENT_LAYOUTS[name]
    data = RC.rounding_data(dtype, n, np.random.default_rng(23))
    left_to_right = RC.sequential_reference(data, heads, n)
    exact, tol = RC.fsum_reference(data, heads, n)
    wave = n // len(heads) >= 24
    assert wave == (name in ("walk_31_quotient_24", "tile_exact_10241"))
    got, _ = _segment_reduce(data, heads, n, "add", True)
    assert got.tobytes() == left_to_right.tobytes(), name
    got, _ = _segment_reduce(data, heads, n, "add", False)
    if wave:
        err = np.abs(got.astype(np.float64) - exact)
        worst = int(np.argmax(err - tol))
        print(f"{name} {np.dtype(dtype).name}: worst run {worst} error {err[worst]:.3e} bound {tol[worst]:.3e}")
        assert np.all(err <= tol), (name, worst, err[worst], tol[worst])
    else:
        assert got.tobytes() == left_to_right.tobytes(), name


# ---- through the public API: arrays of 2^53 cells and more -------------------------------------------------------------
API_SHAPES = [(2 ** 26, 2 ** 27), (2 ** 26, 2 ** 27 + 1), (2 ** 31, 2 ** 31)]


@functools.lru_cache(maxsize=None)
def _api_coords(shape):
    """about 5000 stored elements in rows of 1..300, with rows 0 and max and columns 0 and max among them"""
    rng = np.random.default_rng(shape[1] % 977)
    rows = np.unique(np.concatenate([[0, shape[0] - 1], rng.integers(0, shape[0], size=31)]))
    rr, cc = [], []
    for i, r in enumerate(rows):
        cols = np.unique(rng.integers(0, shape[1], size=int(rng.integers(1, 301))))
        if i % 2 == 0:
            cols = np.unique(np.concatenate([[0, shape[1] - 1], cols]))
        if i % 5 == 0:
            cols = np.unique(np.concatenate([cols, np.minimum(cols[:40] + 1, shape[1] - 1)]))       # neighbours: columns shared by no other row
        rr.append(np.full(len(cols), r))
        cc.append(cols)
    shared = np.concatenate(cc)[::7][:200]                                     # and columns that several rows share
    for r in rows[1:4]:
        rr.append(np.full(len(shared), r))
        cc.append(shared)
    coords = np.unique(np.stack([np.concatenate(rr), np.concatenate(cc)]), axis=1)
    assert 3000 < coords.shape[1] < 8000
    return coords.astype(np.int64)


def _wrap(x, dtype):
    if np.dtype(dtype).kind != "i":
        return x
    bits = 8 * np.dtype(dtype).itemsize
    return (int(x) + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)


def _same_bits(a, b, dtype):
    """what the result container's prune compares: -0.0 is not the fill value 0.0"""
    return np.asarray(a, dtype=dtype).tobytes() == np.asarray(b, dtype=dtype).tobytes()


def _api_data(name, dtype, nnz, rng):
    """the exact-data choices of tests/reduce_cases.py, for a whole array at once"""
    if np.dtype(dtype).kind == "i":
        if name in ("sum", "prod"):      # (products of odd factors: units of the ring, never the 0 that 64 even factors wrap to)
            return rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, size=nnz, endpoint=True, dtype=dtype) | (name == "prod")
        return (rng.permutation(nnz) - nnz // 2).astype(dtype) * 2 + 1
    if name == "sum":
        return rng.integers(1, 9, size=nnz).astype(dtype) * rng.choice([-1, 1], size=nnz)
    if name == "prod":
        return rng.choice([1.0, -1.0, 2.0, 0.5, -2.0], size=nnz, p=[0.4, 0.4, 0.07, 0.07, 0.06]).astype(dtype)
    return (rng.permutation(nnz) - nnz // 2).astype(dtype) + 0.5


def _api_expected(name, coords, data, shape, axis, fill):
    """{kept index: value} by a host dictionary, the implicit entries folded in as the reference does (closed forms for sum
    and prod; integers in Python arithmetic wrapped to the dtype), results equal to the result's fill value dropped"""
    dtype = data.dtype
    n_red = shape[axis]
    groups = {}
    for k, v in zip(coords[1 - axis].tolist(), data.tolist()):
        groups.setdefault(k, []).append(v)
    integer = dtype.kind == "i"
    out = {}
    for k, vs in groups.items():
        n_fill = n_red - len(vs)
        if name == "sum":
            v = sum(vs) + fill * n_fill if integer else dtype.type(np.float64(sum(vs)) + np.float64(fill) * np.float64(n_fill))
        elif name == "prod":
            p = 1
            for x in vs:
                p = p * x
            if integer:
                v = p * pow(int(fill), n_fill, 2 ** 64)
            else:
                with np.errstate(all="ignore"):
                    v = dtype.type(np.float64(p) * np.power(np.float64(fill), np.float64(n_fill)))
        else:
            v = (max if name == "max" else min)(vs + ([fill] if n_fill else []))
        out[k] = _wrap(v, dtype)
    with np.errstate(all="ignore"):
        if name == "sum":
            result_fill = _wrap(int(fill) * n_red, dtype) if integer else dtype.type(np.float64(fill) * n_red)
        elif name == "prod":
            result_fill = _wrap(pow(int(fill), n_red, 2 ** 64), dtype) if integer else dtype.type(np.power(np.float64(fill), n_red))
        else:
            result_fill = fill
    return {k: v for k, v in out.items() if not _same_bits(v, result_fill, dtype)}, result_fill


@pytest.mark.parametrize("dtype,fill", [(np.int64, 0), (np.float64, 0.0), (np.int64, 3), (np.float64, 0.5), (np.float64, -1.0)],
                         ids=["int64", "float64", "int64-fill3", "float64-fill0.5", "float64-fill-1"])
@pytest.mark.parametrize("shape", API_SHAPES, ids=["2^53-cells", "2^53+2^26-cells", "2^62-cells"])
def test_reductions_of_arrays_of_2_to_53_cells_and_more(shape, dtype, fill):
    """sum / max / min / prod over each axis of COO arrays with exactly 2^53 cells (the double-precision id path's last
    size), just above it and with 2^62 cells (integer ids), zero and non-zero fill values: the fold-in of the implicit
    entries runs with about 2^27 / 2^31 of them per group.  Stored indices and values equal a host dictionary's."""
    import sparse_amd as sp

    coords = _api_coords(shape)
    nnz = coords.shape[1]
    dtype = np.dtype(dtype)
    for name in ("sum", "max", "min", "prod"):
        if fill and dtype.kind == "f" and ((name == "prod") != (fill == -1.0)):
            continue        # float fills: 0.5 for the sum's closed form, -1 for the product's (a power that is exact: the sign)
        data = _api_data(name, dtype, nnz, np.random.default_rng(29))
        x = sp.COO(coords, data, shape=shape, fill_value=dtype.type(fill))
        assert x.nnz == nnz
        for axis in (1, 0):
            want, want_fill = _api_expected(name, coords, data, shape, axis, dtype.type(fill).item())
            got = getattr(x, name)(axis=axis)
            what = (name, axis, shape, fill)
            assert got.shape == (shape[1 - axis],) and got.dtype == dtype, what
            assert np.asarray(got.fill_value).dtype == dtype and _same_bits(got.fill_value, want_fill, dtype), (what, got.fill_value, want_fill)
            idx = got.coords.cpu().numpy()[0].astype(np.int64)
            assert idx.tolist() == sorted(want), (what, len(idx), len(want))
            vals = got.data.cpu().numpy()
            expect = np.asarray([want[k] for k in sorted(want)], dtype=dtype)
            assert np.array_equal(vals, expect), (what, np.flatnonzero(vals != expect)[:8])

"""sparse @ sparse on every route - the one-launch small kernel on its first and second chance, the bucket kernels of
csrc/spgemm_rows.hip with rows skipped or declined and merged back, the global expand-sort-compress with row chunks and both
of its sums - against the plain NumPy reference of tests/spgemm_cases.py, on a table in which every case puts a row, a bucket, a
pass, a key width, a size or a fill exactly where the code switches path (tests/test_spgemm_cases.py checks, without a GPU,
that every case does).

Every case forces its route with the `SPGEMM_*` switches (restored by `monkeypatch`), and `SPGEMM_STATS` must report that
route, the `heavy_or_declined` rows and the `parts` the case states.  The row pointers and column indices must EQUAL the
reference's and the values its BITS: every output element is 0 + p1 + p2 + ... left to right in the order of A's elements, so
an element whose products are all -0.0 is +0.0, and NaN is NaN (its sign and payload are the hardware's).  The grouped reduce
re-associates by design: exact values stay bit-equal there, `ordered` floats lie within (n - 1) * eps * sum |p_i| of the
sequential reference, the bound for any two orders of the same rounded products.  The same operands then go through `a @ b`
as GCXS and as COO: the pruned result is the reference pruned bit-wise.

A test is one case with values of one type: every pool that applies to it, through the three entry points.  On an MI355X
the file's 349 tests take about 6 s; the slowest is the first class-boundary case (0.7 s, most of it the first use of the
kernels), no other one takes more than 0.15 s."""
import functools

import numpy as np
import pytest
import torch

import spgemm_cases as sc

pytestmark = pytest.mark.gpu

_PATCHABLE = ("SPGEMM_ROW_LOCAL", "SPGEMM_SMALL", "SPGEMM_SMALL_SECOND", "SPGEMM_BITMAP", "SPGEMM_SMALL_MAX_CELLS", "SPGEMM_SMALL_MAX_NNZ",
              "SPGEMM_CHUNK_PRODUCTS")
RUNS = sc.runs()


def _id(run):
    return f"{sc.slug(run[0])}-{run[1]}"


@pytest.fixture(scope="module")
def K():
    from sparse_amd import _kernels

    return _kernels


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # (a copy: the cached operands are read-only)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=2)
def _dev_operands(call):
    A, B = sc.case_operands(*call)
    return tuple(dev(a) for a in A), tuple(dev(b) for b in B)


def _force(monkeypatch, K, case):
    for name, value in {**case.switches, **case.patch}.items():
        assert name in _PATCHABLE and hasattr(K, name), name
        monkeypatch.setattr(K, name, value)


def _observed_route(stats):
    """the route from the other keys, as before `route` was one: `rows` is written when a row-local kernel delivered the
    product, and `max_prod` once the first chance of the small kernel is behind it; the global form writes neither"""
    if "rows" not in stats:
        return "global"
    if stats["kernel"] == "small":
        return "small/second" if "max_prod" in stats else "small/first"
    return stats["kernel"]


@pytest.fixture
def grouped(monkeypatch):
    """calls of `_reduce.group_reduce`, counted"""
    from sparse_amd import _reduce

    calls, orig = [], _reduce.group_reduce

    def counting(*a, **kw):
        calls.append(a[3])
        return orig(*a, **kw)

    monkeypatch.setattr(_reduce, "group_reduce", counting)
    return calls


def _check_values(call, case, got, want, x, keep=slice(None)):
    """`keep`: the output elements of the reference that `want` holds"""
    name, dtype, pool = call
    assert got.dtype == want.dtype
    if case.group_reduce and pool == "ordered":
        bound, single = sc.reassociation_bound(x)[keep], (x.length == 1)[keep]
        err = np.abs(got.astype(np.longdouble) - want.astype(np.longdouble))
        assert (err <= bound).all(), (float(err.max()), float(bound[np.argmax(err)]))
        assert np.array_equal(sc.bits_of(got)[single], sc.bits_of(want)[single])
        return
    same = sc.bits_of(got) == sc.bits_of(want)
    same = same.all(axis=1) if same.ndim == 2 else same
    assert same.all(), (int((~same).sum()), got[~same][:4], want[~same][:4])


def _dot_csr_csr(K, grouped, call):
    name, dtype, pool = call
    case = sc.CASES[name]
    st = sc.case_struct(name, sc.value_bytes(dtype))
    (ad, ai, ap), (bd, bi, bp) = _dev_operands(call)
    data, indices, indptr, x = sc.case_reference(*call)
    del grouped[:]
    K.SPGEMM_STATS.clear()
    gd, gi, gp = K.dot_csr_csr((st.n_row, st.n_col), ad, bd, ai, bi, ap, bp)
    torch.cuda.synchronize()
    stats = dict(K.SPGEMM_STATS)
    route = "global" if np.dtype(dtype).kind == "c" else case.route
    assert _observed_route(stats) == route and stats["route"] == route, stats
    if route != "global":
        assert stats["heavy_or_declined"] == case.heavy and stats["rows"] == st.n_row, stats
    assert stats.get("parts") is None, stats                      # (the bitmap kernel's word: no case of this table takes it)
    if case.group_reduce is not None:
        assert grouped == (["add"] if case.group_reduce else []), grouped
    gd, gi, gp = host(gd), host(gi), host(gp)
    assert gp.dtype == np.int64 and gi.dtype == np.int64
    assert np.array_equal(gp, indptr)
    assert np.array_equal(gi, indices)
    _check_values(call, case, gd, data, x)


def _matmul_of_containers(K, call, container):
    import sparse_amd as sp

    name, dtype, pool = call
    case = sc.CASES[name]
    st = sc.case_struct(name, sc.value_bytes(dtype))
    (ad, ai, ap), (bd, bi, bp) = _dev_operands(call)
    data, indices, indptr, x = sc.case_reference(*call)
    if container == "gcxs":
        a = sp.GCXS((ad, ai, ap), shape=(st.n_row, st.n_inner), compressed_axes=(0,))
        b = sp.GCXS((bd, bi, bp), shape=(st.n_inner, st.n_col), compressed_axes=(0,))
    else:
        def coo(d, i, p, shape):
            rows = torch.repeat_interleave(torch.arange(shape[0], device=d.device), (p[1:] - p[:-1]).to(torch.int64))
            return sp.COO(torch.stack([rows, i.to(torch.int64)]), d, shape=shape, has_duplicates=False, sorted=True)
        a, b = coo(ad, ai, ap, (st.n_row, st.n_inner)), coo(bd, bi, bp, (st.n_inner, st.n_col))
    K.SPGEMM_STATS.clear()
    c = a @ b
    torch.cuda.synchronize()
    route = "global" if np.dtype(dtype).kind == "c" else case.route
    assert _observed_route(dict(K.SPGEMM_STATS)) == route and K.SPGEMM_STATS["route"] == route, dict(K.SPGEMM_STATS)
    assert isinstance(c, sp.GCXS if container == "gcxs" else sp.COO) and c.shape == (st.n_row, st.n_col)
    bits = sc.bits_of(data)
    keep = bits.any(axis=1) if bits.ndim == 2 else bits != 0           # the bit-wise prune: -0.0 would stay
    want_d, want_r, want_c = sc.prune_bits(data, indices, indptr)
    if container == "gcxs":
        assert c.compressed_axes == (0,)
        gp = host(c.indptr).astype(np.int64)
        got_r, got_c, got_d = np.repeat(np.arange(st.n_row, dtype=np.int64), np.diff(gp)), host(c.indices), host(c.data)
    else:
        coords = host(c.coords)
        got_r, got_c, got_d = coords[0], coords[1], host(c.data)
    assert c.nnz == got_d.size == want_d.size, (c.nnz, got_d.size, want_d.size)
    assert np.array_equal(got_r, want_r) and np.array_equal(got_c, want_c)
    _check_values(call, case, got_d, want_d, x, keep)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_case(K, monkeypatch, grouped, run):
    """one case with values of one type, every pool that applies: `dot_csr_csr`, then `a @ b` as GCXS and as COO"""
    name, dtype = run
    _force(monkeypatch, K, sc.CASES[name])
    for pool in sc.CASES[name].pools or sc.pools_of(dtype):
        call = (name, dtype, pool)
        _dot_csr_csr(K, grouped, call)
        for container in ("gcxs", "coo"):
            _matmul_of_containers(K, call, container)


# C-ABI calls of one `dot_csr_csr` (differences of `_ffi.CALLS`), measured on the commit before `_spgemm_route`: the smallest
# case of every route with float32 values, and the smallest shape of tests/test_spgemm_bitmap_gpu.py with the bitmap kernel
# forced on as that file forces it
CALLS_BEFORE = {"small/first": 2, "small/second": 5, "buckets": 7, "buckets/heavy": 27, "global": 10, "bitmap": 4}


def test_no_route_makes_more_c_abi_calls_than_it_did(K, monkeypatch):
    from sparse_amd import _ffi
    from test_spgemm_bitmap_gpu import _csr

    def calls(shape, A, B):
        (ad, ai, ap), (bd, bi, bp) = (tuple(dev(x) for x in A), tuple(dev(x) for x in B))
        K.SPGEMM_STATS.clear()
        c0 = _ffi.CALLS
        K.dot_csr_csr(shape, ad, bd, ai, bi, ap, bp)
        return _ffi.CALLS - c0, dict(K.SPGEMM_STATS)

    assert set(sc.SMALLEST) | {"bitmap"} == set(CALLS_BEFORE)
    for key, name in sc.SMALLEST.items():
        case = sc.CASES[name]
        with monkeypatch.context() as m:
            _force(m, K, case)
            st = sc.case_struct(name, 4)
            got, stats = calls((st.n_row, st.n_col), *sc.case_operands(name, "float32", (case.pools or sc.pools_of("float32"))[0]))
        assert stats["route"] == case.route and (stats.get("heavy_or_declined", 0) > 0) == (key == "buckets/heavy"), (key, stats)
        assert got <= CALLS_BEFORE[key], (key, got)
    with monkeypatch.context() as m:
        for name, value in (("SPGEMM_BITMAP", True), ("SPGEMM_BITMAP_MIN_MEAN", 0), ("SPGEMM_BITMAP_MAX_DUPS", 10 ** 9), ("SPGEMM_BITMAP_SPLIT", False)):
            m.setattr(K, name, value)
        got, stats = calls((1, 1_048_576), _csr(1, 3_000, 120, 11), _csr(3_000, 1_048_576, 110, 11))
    assert stats["route"] == "bitmap" and stats["parts"] == 1, stats
    assert got <= CALLS_BEFORE["bitmap"], got


def test_switches_are_back_where_they_were(K):
    for name, value in sc.DEFAULT_SWITCHES.items():
        assert getattr(K, name) == value, name
    assert K.SPGEMM_CHUNK_PRODUCTS == 1 << 27

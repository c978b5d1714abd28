"""Audit of the structure and the cached state of every result container (tests/invariants.py).

(a) every case of the existing case tables, evaluated as their own tests evaluate them, with `assert_canonical` on every sparse
    array in the result - and a count that proves no case was left out;
(b) every producer at sizes where its kernels use more than one workgroup, more than one scan block and the radix sorts;
(c) a result is as good as a rebuilt one: a fixed set of consumers gives the same bits for a result and for a twin built from
    host copies of its public arrays through the public constructor - also on the second call (cached layouts) and after the
    three kinds of write `_dot._stamp` is documented to notice.

Values are eighths of small integers wherever sums are formed, so that every sum is exact in float32 whatever its order: the
expected structure (which sums cancel to an exact zero and are pruned) is then a matter of arithmetic, not of rounding.

UNSORTED_ROWS is the table of producers that return GCXS rows with unsorted indices on purpose.  It is empty: every producer
audited here returns strictly increasing rows.
"""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import array_api_cases as ac
import general_cases as gc
import invariants as inv
from invariants import assert_canonical

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
gpu = pytest.mark.gpu

# producer -> (line of the consumer that copes with unsorted rows | fixture showing the reference returns the same structure)
UNSORTED_ROWS = {}


@pytest.fixture(scope="module")
def sp():
    import sparse_amd

    return sparse_amd


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _sparse_in(obj):
    """every sparse array inside a result: tuples, lists and dicts are searched"""
    from sparse_amd import SparseArray

    if isinstance(obj, SparseArray):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from _sparse_in(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _sparse_in(o)


# =================================================================================================================================
# (a) the case tables
# =================================================================================================================================
def _table_counts(npz):
    """(cases, cases the fixture records as sparse) of a general_cases-style fixture"""
    g = np.load(os.path.join(GOLD, npz))
    kinds = [str(g[k]) for k in g.files if k.startswith("c") and k.endswith("_kind")]
    return len(kinds), sum(k == "sparse" for k in kinds)


def _complex_ew_sparse(z):
    return sorted({k.split("__")[0] for k in z.files if k.endswith("__meta")})


def _complex_dot_sparse(z):
    return sorted({k.split("__")[0] for k in z.files if k.endswith("__out_format")})


def test_fixtures_record_sparse_cases():
    """no device: the counts the sweeps below must reach are not zero, and every table has the cases its fixture has"""
    n, s = _table_counts("general.npz")
    assert n == len(gc.CASES) and s > 0
    n, s = _table_counts("array_api.npz")
    assert n == len(ac.CASES) and s > 0
    z = np.load(os.path.join(GOLD, "complex_ew.npz"))
    names = _tool("gen_complex_ew_golden").case_names()
    assert _complex_ew_sparse(z) and set(_complex_ew_sparse(z)) <= set(names)
    z = np.load(os.path.join(GOLD, "complex_dot.npz"))
    names = _tool("gen_complex_golden").case_names()
    assert _complex_dot_sparse(z) and set(_complex_dot_sparse(z)) <= set(names)
    assert UNSORTED_ROWS == {}
    kept = {n for n in _complex_dot_sparse(z) if _recorded_fill_values(z[f"{n}__out_data"], 0)}
    z = np.load(os.path.join(GOLD, "complex_ew.npz"))
    kept |= {n for n in _complex_ew_sparse(z) if _recorded_fill_values(z[f"{n}__data"], z[f"{n}__fill"])}
    assert kept == REFERENCE_KEPT_ZEROS


# cases whose fixture shows that the reference itself kept explicit fill values (its `einsum` sums the products of the aligned
# operands and never prunes: zeros of either sign stay stored, and its `nnz` counts them; tests/test_complex_products_gpu.py
# compares these two cases without their explicit zeros as well).  `test_fixtures_record_sparse_cases` proves from the fixtures
# that these are all of them.
REFERENCE_KEPT_ZEROS = {"einsum_c64", "einsum_c128"}


def _recorded_fill_values(values, fill):
    return int(inv.eq_bits(values.reshape(-1), fill).sum()) if values.size else 0


def _audit_recorded(name, r, nnz_recorded, recorded_values=None, recorded_fill=None):
    """One sparse result of a fixture case that records the reference's `nnz`: pruned, and that `nnz`.  For the cases of
    REFERENCE_KEPT_ZEROS the elements whose VALUE differs from the fill value are counted on both sides instead."""
    if name not in REFERENCE_KEPT_ZEROS:
        assert recorded_values is None or _recorded_fill_values(recorded_values, recorded_fill) == 0, name
        n = assert_canonical(r, pruned=True)
        assert r.nnz == nnz_recorded, (r.nnz, nnz_recorded)
    else:
        n = assert_canonical(r)
        assert recorded_values.size == nnz_recorded
        mine, theirs = int(np.count_nonzero(_npy(r.data) != r.fill_value)), int(np.count_nonzero(recorded_values != recorded_fill))
        assert mine == theirs, (r.nnz, mine, nnz_recorded, theirs)
    return n


def _sweep_case_table(sp, cases, npz):
    g = np.load(os.path.join(GOLD, npz))
    inp = {key[3:]: g[key] for key in g.files if key.startswith("in_")}
    audited = 0
    for k, (name, fn) in enumerate(cases):
        assert str(g[f"c{k}_name"]) == name
        kind = str(g[f"c{k}_kind"])
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = fn(sp, inp)
        except Exception as e:  # noqa: BLE001 - the recorded result of such a case is the exception's type
            assert kind == "error" and type(e).__name__ == str(g[f"c{k}_error"]), (name, e)
            continue
        assert kind != "error", (name, "no exception was raised")
        assert (kind == "sparse") == isinstance(r, sp.SparseArray), (name, kind, type(r))
        found = list(_sparse_in(r))
        for x in found:
            try:
                if x is r and f"c{k}_nnz" in g.files:
                    audited += _audit_recorded(name, x, int(g[f"c{k}_nnz"]))
                else:
                    audited += assert_canonical(x)
            except AssertionError as e:
                raise AssertionError(f"case {k} ({name}): {e}") from e
    return audited


@gpu
def test_general_case_table_gives_canonical_containers(sp):
    audited = _sweep_case_table(sp, gc.CASES, "general.npz")
    print(f"general.npz: {audited} containers audited, {_table_counts('general.npz')[1]} sparse cases recorded")
    assert audited >= _table_counts("general.npz")[1]


@gpu
def test_array_api_case_table_gives_canonical_containers(sp):
    audited = _sweep_case_table(sp, ac.CASES, "array_api.npz")
    print(f"array_api.npz: {audited} containers audited, {_table_counts('array_api.npz')[1]} sparse cases recorded")
    assert audited >= _table_counts("array_api.npz")[1]


@gpu
def test_complex_elementwise_cases_give_canonical_containers(sp):
    gen = _tool("gen_complex_ew_golden")
    z = np.load(os.path.join(GOLD, "complex_ew.npz"))
    inputs = {k[4:]: z[k] for k in z.files if k.startswith("in__")}
    fns = dict(gen.cases())
    audited = 0
    for name in gen.case_names():
        with np.errstate(all="ignore"):
            r = fns[name](sp, inputs)
        for x in _sparse_in(r):
            try:
                if x is r and f"{name}__meta" in z.files:
                    audited += _audit_recorded(name, x, int(z[f"{name}__meta"][0]), z[f"{name}__data"], z[f"{name}__fill"])
                else:
                    audited += assert_canonical(x)
            except AssertionError as e:
                raise AssertionError(f"case {name}: {e}") from e
    print(f"complex_ew.npz: {audited} containers audited, {len(_complex_ew_sparse(z))} sparse cases recorded")
    assert audited >= len(_complex_ew_sparse(z))


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fma"])
def test_complex_product_cases_give_canonical_containers(sp, exact, monkeypatch):
    import test_complex_products_gpu as cp          # (its `_operand` / `_call` are how the fixture's own test evaluates a case)
    from sparse_amd import _settings

    monkeypatch.setattr(_settings, "EXACT_MULADD", exact)
    z = np.load(os.path.join(GOLD, "complex_dot.npz"))
    names = cp._names(z)
    assert set(names) == set(_tool("gen_complex_golden").case_names())
    audited = 0
    for k, name in enumerate(names):
        a, b = cp._operand(sp, z, name, "a"), cp._operand(sp, z, name, "b")
        r = cp._call(sp, name, k, a, b)
        for x in _sparse_in(r):
            try:
                if x is r and f"{name}__out_nnz" in z.files:
                    audited += _audit_recorded(name, x, int(z[f"{name}__out_nnz"]), z[f"{name}__out_data"], np.zeros((), z[f"{name}__out_data"].dtype))
                else:
                    audited += assert_canonical(x)
            except AssertionError as e:
                raise AssertionError(f"case {name}: {e}") from e
        for operand in (a, b):                       # the operands are untouched
            for x in _sparse_in(operand):
                assert_canonical(x)
    print(f"complex_dot.npz: {audited} containers audited, {len(_complex_dot_sparse(z))} sparse cases recorded")
    assert audited >= len(_complex_dot_sparse(z))


# =================================================================================================================================
# (c) a result is as good as a rebuilt one  (the helpers come first: every test of (b) ends in them)
# =================================================================================================================================
DENSE_IMAGE_MAX = 1 << 24          # cells: beyond this no dense image is formed (the SpGEMM results of 10^6 columns)
DENSE_OPERAND_MAX_ROWS = 1 << 16   # rows of the dense operand of `r @ dense`


def _host_form(r):
    """a result as a tuple of host arrays: index arrays as int64 (the width is not what is compared), values as they are"""
    from sparse_amd import COO, GCXS

    if isinstance(r, COO):
        return ("coo", tuple(r.shape), np.asarray(r.fill_value), _npy(r.coords).astype(np.int64), _npy(r.data))
    if isinstance(r, GCXS):
        return ("gcxs", tuple(r.shape), r.compressed_axes, np.asarray(r.fill_value), _npy(r.indices).astype(np.int64),
                _npy(r.indptr).astype(np.int64), _npy(r.data))
    return ("dense", _npy(r))


def _same_form(a, b):
    if len(a) != len(b) or a[0] != b[0]:
        return False
    for x, y in zip(a[1:], b[1:]):
        if isinstance(x, np.ndarray):
            if not inv.same_bits(x, y):
                return False
        elif x != y:
            return False
    return True


def host_arrays(r):
    """(coords int64 [ndim, nnz], data) of a result from host copies of its PUBLIC arrays; nothing is computed on the device"""
    from sparse_amd import COO

    if isinstance(r, COO):
        return _npy(r.coords).astype(np.int64).reshape(len(r.shape), -1), _npy(r.data).copy()
    data, indices, indptr = _npy(r.data).copy(), _npy(r.indices).astype(np.int64), _npy(r.indptr).astype(np.int64)
    if r.ndim == 1:
        return indices[None, :], data
    if r.ndim == 0:
        return np.zeros((0, data.size), dtype=np.int64), data
    order = r._axis_order
    R, C = r._compressed_shape
    rc = np.stack(np.unravel_index(inv.gcxs_rows(indptr, data.size) * C + indices, tuple(r.shape[a] for a in order))) if data.size else \
        np.zeros((r.ndim, 0), dtype=np.int64)
    nat = np.empty_like(rc)
    nat[order] = rc
    return nat, data


def build_twin(sp, r, coords=None, data=None):
    """the same array through the public constructor with its default promises: it sorts and checks for itself"""
    if coords is None:
        coords, data = host_arrays(r)
    idt = np.int32 if (r._index_dtype if isinstance(r, sp.COO) else r.indices.dtype) == torch.int32 else np.int64
    t = sp.COO(coords.astype(idt), data, shape=r.shape, fill_value=r.fill_value)
    if isinstance(r, sp.GCXS):
        t = sp.GCXS(t, compressed_axes=r.compressed_axes)
    return t


def _pruned_copy(x):
    c = type(x)(x)                  # shares the buffers; a prune replaces them on the copy only
    c._prune()
    return c


def consumers_of(sp, r, seed=0):
    """the fixed set of consumers, each `fn(x)` for x = the result or its twin; the other operands are built once, on the
    host, from the result's own public arrays"""
    coords, data = host_arrays(r)
    rng = np.random.default_rng(seed)
    kind = np.dtype(r.dtype).kind
    out = {}
    if r.size <= DENSE_IMAGE_MAX:
        out["todense"] = lambda x: x.todense()
    if kind != "b":
        # an operand on every third position of the result (and nowhere else) of the result's format
        oc = coords[:, ::3]
        od = (rng.integers(1, 5, size=oc.shape[1]) * (1 if kind in "iu" else 0.5)).astype(r.dtype)
        other = build_twin(sp, r, oc, od)
        out["r + other"] = lambda x: x + other
        out["r * other"] = lambda x: x * other
    out["r.T"] = lambda x: x.T
    if r.ndim >= 1 and kind != "b":
        out["r.sum(axis=0)"] = lambda x: x.sum(axis=0)
    if r.ndim == 2 and kind in "fiu" and r.shape[1] <= DENSE_OPERAND_MAX_ROWS and r.shape[0] * 130 <= DENSE_IMAGE_MAX:
        for n in (3, 130):
            d = (rng.integers(-4, 5, size=(r.shape[1], n)) * (1 if kind in "iu" else 0.25)).astype(r.dtype)
            out[f"r @ dense[{n}]"] = lambda x, d=d: x @ d
    if r.ndim >= 1:
        out["r[1:]"] = lambda x: x[1:]
    out["prune"] = _pruned_copy
    return out


def same_as_rebuilt(sp, r, seed=0, runs=2):
    """every consumer `runs` times on the twin and on the result (the second call uses whatever the first one cached): the same
    bits.  Two runs on the twin prove first that the consumer is bit-reproducible run to run at all; every consumer of this set
    is, so there is no tolerance anywhere in this file."""
    twin = build_twin(sp, r)
    for name, fn in consumers_of(sp, r, seed).items():
        t1 = _host_form(fn(twin))
        for _ in range(runs - 1):
            assert _same_form(_host_form(fn(twin)), t1), f"{name} is not bit-reproducible run to run on one operand"
        for call in range(1, runs + 1):
            got = _host_form(fn(r))
            assert _same_form(got, t1), f"{name}, call {call}: a {type(r).__name__} result {r.shape} differs from its rebuilt twin"


def owns_its_values(r, operands):
    """a 2-D `GCXS.T`, a `reshape`, a conversion that keeps the order share the operand's value buffer: a write to such a result
    is a write to the operand"""
    mine = r.data.untyped_storage().data_ptr()
    return all(o.data.untyped_storage().data_ptr() != mine for o in operands if hasattr(o, "nnz"))


def follows_writes(sp, r):
    """the three writes `_dot._stamp` notices, each after the consumers have filled their caches: in-place arithmetic, an element
    write, a replaced buffer (other values: the old ones reversed and negated).  After each the zero-bit note is not believed,
    the consumers give what they give for a twin rebuilt from the NEW values (a layout cached before the write would give the
    old ones), and a prune drops exactly the elements that are zero now."""
    from sparse_amd import _kernels as K

    for step in ("*= 2", "[0] = 0", "replaced"):
        if step == "*= 2":
            r.data *= 2
        elif step == "[0] = 0":
            r.data[0] = 0
        else:
            r.data = torch.flip(r.data, [0]).neg()
        assert K.known_eq_bits(r.data, r.fill_value) is None, step
        same_as_rebuilt(sp, r, seed=1, runs=1)
        assert _pruned_copy(r).nnz == r.nnz - int(inv.eq_bits(_npy(r.data), r.fill_value).sum()), step
        assert_canonical(r)


def audit(sp, r, pruned=False, operands=()):
    """(b) + (c) for one result.  The writes are done on every result that owns its value buffer (`operands`: what it was made
    from), holds an element and is not boolean (`*= 2` is no operation on booleans)."""
    n = assert_canonical(r, pruned=pruned)
    same_as_rebuilt(sp, r)
    assert_canonical(r, pruned=pruned)            # (with whatever the consumers cached on it)
    if r.nnz and np.dtype(r.dtype).kind != "b" and owns_its_values(r, operands):
        follows_writes(sp, r)
    return n


class Untouched:
    """operands of a producer: settled (lazy coordinates / keys are produced, which is no write), stamped, and compared after"""

    def __init__(self, *operands):
        from sparse_amd import _dot

        self.ops = [o for o in operands if hasattr(o, "nnz")]
        for o in self.ops:
            if hasattr(o, "linear_loc"):
                o.coords, o.linear_loc()
        self.stamps = [_dot._stamp(o) for o in self.ops]

    def check(self):
        from sparse_amd import _dot

        for o, st in zip(self.ops, self.stamps):
            assert _dot._stamp(o) == st, f"an operand {type(o).__name__} {o.shape} was written to"
            assert_canonical(o)


# =================================================================================================================================
# (b) producers
# =================================================================================================================================
VALUE_TYPES = [np.float32, np.float64, np.int64]
INDEX_TYPES = [np.int32, np.int64]


def eighths(rng, n, dtype, zero=False):
    """non-zero multiples of 1/8 in [-0.5, 0.5] (integers: -4 .. 4): sums of thousands of them are exact in float32"""
    k = rng.integers(1, 5, size=n) * rng.choice([-1, 1], size=n)
    if zero:
        k[rng.random(n) < 0.1] = 0
    return k.astype(dtype) if np.dtype(dtype).kind in "iu" else (k / 8).astype(dtype)


def random_keys(rng, shape, n, margin_rows=2):
    """n distinct sorted linear keys of `shape`, none in the first and last `margin_rows` rows (empty leading / trailing rows)"""
    row = int(np.prod(shape[1:]))
    lo, hi = margin_rows * row, (shape[0] - margin_rows) * row
    return np.sort(rng.choice(hi - lo, size=n, replace=False)) + lo


def make(sp, fmt, keys, data, shape, idt, **kw):
    coords = np.stack(np.unravel_index(keys, shape)).astype(idt)
    x = sp.COO(coords, data, shape=shape)
    return sp.GCXS(x, **kw) if fmt == "gcxs" else x


# ---- the COO constructor -----------------------------------------------------------------------------------------------------------
# 1, 255 / 257 (a workgroup), 4095 / 4097 (SUM_RUNS_PROBE_MIN), 16385 (SMALL_SCAN_MAX of csrc/common.h is 16384: one beyond the
# one-workgroup scan), 300001 (beyond both radix thresholds of csrc/prims.hip)
COUNTS = [1, 255, 257, 4095, 4097, 16385, 300_001]


@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("mode", ["30 % duplicates", "one long run"])
def test_coo_constructor_from_unsorted_duplicated_coordinates(sp, mode, n, dtype, idt, monkeypatch):
    from sparse_amd import _coo, _kernels as K
    from sparse_amd.csrc import build as hbuild

    assert _coo.SUM_RUNS_PROBE_MIN == 4096 and "SMALL_SCAN_MAX = 16384" in open(os.path.join(os.path.dirname(hbuild.__file__), "common.h")).read()
    shape = (1000, 1201)
    rng = np.random.default_rng(n)
    if True:
        distinct = random_keys(rng, shape, max(1, n - (3 * n) // 10 if mode == "30 % duplicates" else n - min(n // 2, 2000)))
        if mode == "30 % duplicates":
            keys = np.concatenate([distinct, rng.choice(distinct, size=n - distinct.size)])
        else:
            keys = np.concatenate([distinct, np.full(n - distinct.size, distinct[distinct.size // 2])])
        keys = keys[rng.permutation(n)]
        for zeros in (False, True):
            data = eighths(rng, n, dtype, zero=zeros)
            coords = np.stack(np.unravel_index(keys, shape)).astype(idt)
            uk, inverse = np.unique(keys, return_inverse=True)
            sums = np.zeros(uk.size, dtype=np.float64)
            np.add.at(sums, inverse, data.astype(np.float64))           # exact: eighths
            for prune in (False, True):
                for count_first in (None, 1000):
                    if count_first is not None:
                        if not prune:
                            continue
                        monkeypatch.setattr(K, "PRUNE_COUNT_FIRST", count_first)
                    try:
                        x = sp.COO(coords, data, shape=shape, prune=prune)
                        keep = sums != 0 if prune else np.ones(uk.size, dtype=bool)
                        assert x.nnz == int(keep.sum()), (mode, zeros, prune, count_first)
                        assert x._index_dtype == (torch.int32 if idt == np.int32 else torch.int64)
                        assert np.array_equal(_npy(x.linear_loc()), uk[keep])
                        assert np.array_equal(_npy(x.data), sums[keep].astype(dtype))
                        audit(sp, x, pruned=prune)
                    finally:
                        if count_first is not None:
                            monkeypatch.undo()


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
def _pair(sp, fmt, shape, dtype, idt, nx=300_001, ny=200_003):
    """x and y of nx / ny stored elements sharing ny / 3 positions; (x, y, dense x, dense y)"""
    rng = np.random.default_rng(len(shape) * 7 + np.dtype(dtype).itemsize)
    shared = ny // 3
    pool = random_keys(rng, shape, nx + ny - shared)
    pool = pool[rng.permutation(pool.size)]
    kx, ky = np.sort(pool[:nx]), np.sort(pool[nx - shared:])
    vx, vy = eighths(rng, nx, dtype), eighths(rng, ny, dtype)
    dx, dy = np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype)
    dx.reshape(-1)[kx], dy.reshape(-1)[ky] = vx, vy
    return make(sp, fmt, kx, vx, shape, idt), make(sp, fmt, ky, vy, shape, idt), dx, dy


@gpu
@pytest.mark.parametrize("shape", [(2000, 1500), (100, 150, 200)], ids=["2d", "3d"])
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("fmt", ["coo", "gcxs"])
def test_elementwise_results_at_device_wide_sizes(sp, fmt, dtype, idt, shape):
    x, y, dx, dy = _pair(sp, fmt, shape, dtype, idt)
    row = eighths(np.random.default_rng(5), shape[-1], dtype)
    row = np.abs(row) + row.dtype.type(1)
    cases = {
        "x + y": (lambda: x + y, dx + dy),
        "x * y": (lambda: x * y, dx * dy),
        "x - x": (lambda: x - x, dx - dx),
        "maximum(x, y)": (lambda: np.maximum(x, y), np.maximum(dx, dy)),
        "x * dense_row": (lambda: x * row, dx * row),
        "x > y": (lambda: x > y, dx > dy),
        "where(x > y, x, y)": (lambda: sp.where(x > y, x, y), np.where(dx > dy, dx, dy)),
    }
    ops = Untouched(x, y)
    for name, (fn, want) in cases.items():
        r = fn()
        try:
            assert isinstance(r, sp.SparseArray), type(r)
            # (bit-wise: `negative * 0 = -0.0` is a stored element, as in the reference's `equivalent`)
            stored = int((~inv.eq_bits(want.reshape(-1), 0)).sum())
            assert r.nnz == stored, (r.nnz, stored)
            assert np.array_equal(r.todense(), want)
            audit(sp, r, pruned=True, operands=ops.ops)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    ops.check()


# ---- transposes, reshapes, slices, joins, casts, reductions --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("fmt", ["coo", "gcxs"])
def test_shape_manipulation_results(sp, fmt, dtype, idt):
    rng = np.random.default_rng(17)
    s2, s3 = (2000, 1500), (100, 150, 200)
    k2, k3 = random_keys(rng, s2, 300_001), random_keys(rng, s3, 300_001)
    v2, v3 = eighths(rng, k2.size, dtype), eighths(rng, k3.size, dtype)
    x2, x3 = make(sp, fmt, k2, v2, s2, idt), make(sp, fmt, k3, v3, s3, idt)
    d2, d3 = np.zeros(s2, dtype=dtype), np.zeros(s3, dtype=dtype)
    d2.reshape(-1)[k2], d3.reshape(-1)[k3] = v2, v3
    cases = {
        "x.T": (lambda: x2.T, d2.T),
        "x.transpose((2, 0, 1))": (lambda: x3.transpose((2, 0, 1)), d3.transpose((2, 0, 1))),
        "x.reshape 3-D -> 2-D": (lambda: x3.reshape((1500, 2000)), d3.reshape((1500, 2000))),
    }
    ops = Untouched(x2, x3)
    for name, (fn, want) in cases.items():
        r = fn()
        try:
            assert isinstance(r, sp.SparseArray), type(r)
            assert r.shape == want.shape and np.array_equal(r.todense(), want)         # (exact sums: eighths)
            audit(sp, r, pruned=True, operands=ops.ops)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    ops.check()


@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("fmt", ["coo", "gcxs"])
@pytest.mark.parametrize("group", ["slices and casts", "concatenate", "stack", "reductions"])
def test_slices_joins_casts_and_reductions(sp, group, fmt, dtype, idt):
    rng = np.random.default_rng(18)
    s2, s3 = (2000, 1500), (100, 150, 200)
    k2, k3 = random_keys(rng, s2, 300_001), random_keys(rng, s3, 300_001)
    v2, v3 = eighths(rng, k2.size, dtype), eighths(rng, k3.size, dtype)
    x2, x3 = make(sp, fmt, k2, v2, s2, idt), make(sp, fmt, k3, v3, s3, idt)
    d2, d3 = np.zeros(s2, dtype=dtype), np.zeros(s3, dtype=dtype)
    d2.reshape(-1)[k2], d3.reshape(-1)[k3] = v2, v3
    take = np.array([5, 1999, 5, 17, 0, 1000])
    other = np.float64 if dtype != np.float64 else np.float32
    cases = {
        "x.reshape 2-D -> 3-D": (lambda: x2.reshape((300, 50, 200)), d2.reshape((300, 50, 200))),
        "x[::2]": (lambda: x2[::2], d2[::2]),
        "x[:, 3:50]": (lambda: x2[:, 3:50], d2[:, 3:50]),
        "x[::2] 3-D": (lambda: x3[::2], d3[::2]),
        "x[:, 3:50] 3-D": (lambda: x3[:, 3:50], d3[:, 3:50]),
        "x[array]": (lambda: x2[take], d2[take]),
        "astype": (lambda: x2.astype(other), d2.astype(other)),
    }
    for ax in range(2):
        cases[f"concatenate axis {ax}"] = (lambda ax=ax: sp.concatenate([x2, x2, x2], axis=ax), np.concatenate([d2, d2, d2], axis=ax))
    for ax in range(3):
        cases[f"concatenate 3-D axis {ax}"] = (lambda ax=ax: sp.concatenate([x3, x3], axis=ax), np.concatenate([d3, d3], axis=ax))
        cases[f"stack axis {ax}"] = (lambda ax=ax: sp.stack([x2, x2], axis=ax), np.stack([d2, d2], axis=ax))
        cases[f"sum axis {ax}"] = (lambda ax=ax: x3.sum(axis=ax), d3.sum(axis=ax))
        cases[f"max axis {ax}"] = (lambda ax=ax: x3.max(axis=ax), d3.max(axis=ax))
    if fmt == "coo":
        cases["tril"] = (lambda: sp.tril(x2, k=-1), np.tril(d2, k=-1))
        cases["triu"] = (lambda: sp.triu(x2, k=3), np.triu(d2, k=3))
        cases["diagonal"] = (lambda: sp.diagonal(x2[:1500], offset=2), np.diagonal(d2[:1500], offset=2))
        cases["nansum"] = (lambda: sp.nansum(x3, axis=1), d3.sum(axis=1))
    ops = Untouched(x2, x3)
    for name, (fn, want) in cases.items():
        mine = name.split()[0] if name.startswith(("concatenate", "stack")) else "reductions" if name.startswith(("sum", "max", "nansum")) else "slices and casts"
        if mine != group:
            continue
        r = fn()
        try:
            assert isinstance(r, sp.SparseArray), type(r)
            assert r.shape == want.shape and np.array_equal(r.todense(), want)         # (exact sums: eighths)
            # (a reduction may keep a sum that cancelled to zero; everything else holds the operand's non-zero values)
            audit(sp, r, pruned=not name.startswith(("sum", "max", "nansum")), operands=ops.ops)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    ops.check()


# ---- conversions -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ca,new", [((0,), (1,)), ((1,), (0, 1)), ((0, 1), (2,)), ((2,), (0,))], ids=str)
def test_format_conversions(sp, ca, new, dtype, idt):
    """COO -> GCXS compressed along `ca` -> COO, and `change_compressed_axes` from `ca` to `new`"""
    rng = np.random.default_rng(23)
    s3 = (100, 150, 200)
    k3 = random_keys(rng, s3, 300_001)
    v3 = eighths(rng, k3.size, dtype)
    d3 = np.zeros(s3, dtype=dtype)
    d3.reshape(-1)[k3] = v3
    x = make(sp, "coo", k3, v3, s3, idt)
    ops = Untouched(x)
    g = sp.GCXS(x, compressed_axes=ca)
    assert g.compressed_axes == ca and g.indices.dtype == (torch.int32 if idt == np.int32 else torch.int64)
    audit(sp, g, pruned=True, operands=[x])
    ops.check()
    g = sp.GCXS(x, compressed_axes=ca)            # (the audit wrote to the first one where it owned its values)
    ops = Untouched(x, g)
    back = g.tocoo()
    assert np.array_equal(_npy(back.linear_loc()), k3) and inv.same_bits(_npy(back.data), v3)
    audit(sp, back, pruned=True, operands=[x, g])
    h = g.change_compressed_axes(new)
    assert h.compressed_axes == new and np.array_equal(h.todense(), d3)
    audit(sp, h, pruned=True, operands=[x, g])
    ops.check()


@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
def test_conversions_from_scipy_and_numpy(sp, dtype, idt):
    import scipy.sparse

    rng = np.random.default_rng(24)
    s3 = (100, 150, 200)
    k3 = random_keys(rng, s3, 300_001)
    d3 = np.zeros(s3, dtype=dtype)
    d3.reshape(-1)[k3] = eighths(rng, k3.size, dtype)
    d2 = d3.reshape(1500, 2000)
    for f in ("csr", "csc", "coo"):
        m = getattr(scipy.sparse, f + "_matrix")(d2)
        if f != "coo":
            m.indices, m.indptr = m.indices.astype(idt), m.indptr.astype(idt)
        r = (sp.COO if f == "coo" else sp.GCXS).from_scipy_sparse(m)
        assert np.array_equal(r.todense(), d2)
        audit(sp, r, pruned=True)
    for cls, kw in ((sp.COO, {}), (sp.GCXS, {"compressed_axes": (1,)}), (sp.GCXS, {"compressed_axes": (0, 2)})):
        r = cls.from_numpy(d3, idx_dtype=idt, **kw)
        assert r.nnz == k3.size and np.array_equal(r.todense(), d3)
        audit(sp, r, pruned=True)


# ---- sparse @ sparse through every SpGEMM route ------------------------------------------------------------------------------------
def _int_valued(sp, g, dtype, seed):
    """the pattern of `g` with eighths for values: products cancel to exact zeros, sums are exact"""
    v = eighths(np.random.default_rng(seed), g.nnz, dtype)
    return sp.GCXS((v, g.indices, g.indptr), shape=g.shape, compressed_axes=g.compressed_axes)


def _spgemm_audit(sp, a, b, kernel, stats_check=None, route=None):
    """the raw triple and its zero-bit note before the container prunes, then the container; `route`: what `SPGEMM_STATS`
    names beside `kernel` (the kernel's own name, "global" without one, unless given: the small kernel's two chances)"""
    from sparse_amd import _kernels as K

    ops = Untouched(a, b)
    K.SPGEMM_STATS.clear()
    data, indices, indptr = K.dot_csr_csr((a.shape[0], b.shape[1]), a.data, b.data, a.indices, b.indices, a.indptr, b.indptr)
    stats = dict(K.SPGEMM_STATS)
    route = route or kernel or "global"
    assert stats.get("kernel") == kernel, stats              # (None: no row-local kernel ran, the global form throughout)
    assert stats["route"] == route, stats
    if stats_check is not None:
        stats_check(stats)
    hd = _npy(data)
    inv.check_gcxs_arrays(hd, _npy(indices), _npy(indptr), (a.shape[0], b.shape[1]), (0,), hd.dtype.type(0))
    zeros = int(inv.eq_bits(hd, 0).sum())
    assert zeros > 0, "no product is an exact zero: the zero-bit note would be trivial"
    note = getattr(data, "_zero_bits_count", None)
    if kernel is not None:                                   # the small, bitmap and pack kernels count their exact zeros
        assert note is not None and note[1] == data._version, note
    if note is not None and note[1] == data._version:
        assert int(note[0]) == zeros, (note, zeros)
    K.SPGEMM_STATS.clear()
    c = a @ b
    assert K.SPGEMM_STATS.get("kernel") == kernel and K.SPGEMM_STATS["route"] == route, dict(K.SPGEMM_STATS)
    assert isinstance(c, sp.GCXS) and c.nnz == hd.size - zeros
    audit(sp, c, pruned=True, operands=ops.ops)
    ops.check()
    return zeros


@gpu
@pytest.mark.parametrize("dtype,idt", [(np.float32, np.int32), (np.float64, np.int64), (np.int64, np.int64)])
def test_spgemm_routes_give_canonical_products(sp, dtype, idt, monkeypatch):
    from sparse_amd import _kernels as K

    kw = dict(dtype=np.float64, idx_dtype=idt, format="gcxs", compressed_axes=(0,))

    def operand(shape, density, seed):
        return _int_valued(sp, sp.random(shape, density=density, random_state=seed, **kw), dtype, seed)

    # the one-launch kernel
    a, b = operand((200, 300), 0.05, 1), operand((300, 250), 0.05, 2)
    _spgemm_audit(sp, a, b, "small", route="small/first")
    # its second chance, once the row products are known (tests/test_round6_gpu.py, 700 x 900 with 120 per row)
    a, b = operand((700, 900), 120 / 900, 11), operand((900, 900), 120 / 900, 12)
    assert a.nnz > K.SPGEMM_SMALL_MAX_NNZ
    _spgemm_audit(sp, a, b, "small", route="small/second")
    monkeypatch.setattr(K, "SPGEMM_SMALL_SECOND", False)
    _spgemm_audit(sp, a, b, "buckets")
    monkeypatch.undo()
    # the bucket kernels with heavy rows merged in from the global form (tests/test_matrix_gpu.py, n = 2500)
    n = 2500
    rng = np.random.default_rng(4)
    da = np.where(rng.random((n, n)) < 0.01, 1.0, 0.0)
    da[7, :], da[1999, ::2] = 1.0, 1.0
    db = np.where(rng.random((n, n)) < 0.03, 1.0, 0.0)
    a = _int_valued(sp, sp.GCXS.from_numpy(da, compressed_axes=(0,), idx_dtype=idt), dtype, 5)
    b = _int_valued(sp, sp.GCXS.from_numpy(db, compressed_axes=(0,), idx_dtype=idt), dtype, 6)
    monkeypatch.setattr(K, "SPGEMM_SMALL", False)
    _spgemm_audit(sp, a, b, "buckets", lambda st: st["heavy_or_declined"] >= 1 or pytest.fail(str(st)))
    # the global expand-sort-compress throughout
    monkeypatch.setattr(K, "SPGEMM_ROW_LOCAL", False)
    a, b = operand((3000, 2500), 0.004, 1), operand((2500, 2000), 0.004, 2)
    _spgemm_audit(sp, a, b, None)
    monkeypatch.undo()


@gpu
@pytest.mark.parametrize("split,dtype,idt", [(False, np.float32, np.int32), (True, np.float32, np.int32), (True, np.float64, np.int64),
                                             (True, np.int64, np.int64)])
def test_spgemm_bitmap_forms_give_canonical_products(sp, dtype, idt, split, monkeypatch):
    """the shapes of tests/test_spgemm_bitmap_gpu.py (its `_csr` generator), the kernel forced on as that file forces it"""
    import test_spgemm_bitmap_gpu as tb
    from sparse_amd import _kernels as K

    # (40 rows of ~10^4 elements each: the host passes stay at a few 10^5 elements; 3 x 10^6 columns are beyond the wide form)
    m, k, n = 40, 3_000, (3_000_000 if split else 1_000_000)
    A = tb._csr(m, k, 120 if np.dtype(dtype).itemsize == 4 else 60, 10 + m, np.float32, idt, empty_every=7)
    B = tb._csr(k, n, 110, 11, np.float32, idt, empty_every=13)
    rng = np.random.default_rng(3)
    # (at 10^6 columns two products rarely meet in one element: A stores explicit zeros, so that exact zeros are produced)
    a = sp.GCXS((eighths(rng, A[0].size, dtype, zero=True), A[1], A[2]), shape=(m, k), compressed_axes=(0,))
    b = sp.GCXS((eighths(rng, B[0].size, dtype), B[1], B[2]), shape=(k, n), compressed_axes=(0,))
    for name, value in (("SPGEMM_BITMAP", True), ("SPGEMM_BITMAP_MIN_MEAN", 0), ("SPGEMM_BITMAP_MAX_DUPS", 10 ** 9), ("SPGEMM_BITMAP_SPLIT", split)):
        monkeypatch.setattr(K, name, value)
    _spgemm_audit(sp, a, b, "bitmap", lambda st: (st.get("parts", 1) > 1) == split or pytest.fail(str(st)))


# ---- tensordot, einsum, sddmm ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("dtype", VALUE_TYPES, ids=lambda t: np.dtype(t).name)
def test_tensordot_and_einsum_results(sp, dtype, idt):
    rng = np.random.default_rng(31)
    sx, sy = (60, 70, 80), (80, 70, 50)
    kx, ky = random_keys(rng, sx, 30_011, margin_rows=1), random_keys(rng, sy, 20_011, margin_rows=1)
    vx, vy = eighths(rng, kx.size, dtype), eighths(rng, ky.size, dtype)
    dx, dy = np.zeros(sx, dtype=dtype), np.zeros(sy, dtype=dtype)
    dx.reshape(-1)[kx], dy.reshape(-1)[ky] = vx, vy
    want = np.tensordot(dx.astype(np.float64), dy.astype(np.float64), axes=([1, 2], [1, 0])).astype(dtype)     # exact: eighths
    for fmt in ("coo", "gcxs"):
        x, y = make(sp, fmt, kx, vx, sx, idt), make(sp, fmt, ky, vy, sy, idt)
        ops = Untouched(x, y)
        for rt in (sp.COO, sp.GCXS):
            for call in (1, 2):                       # (the second product uses the 2-D forms the first one left on the operands)
                r = sp.tensordot(x, y, axes=([1, 2], [1, 0]), return_type=rt)
                assert isinstance(r, rt) and np.array_equal(r.todense(), want)
                audit(sp, r, pruned=True, operands=ops.ops)
                ops.check()                           # (the cached forms on x and y are audited with them)
        r = sp.einsum("ijk,kjl->il", x, y)
        assert isinstance(r, sp.SparseArray) and np.array_equal(r.todense(), want)
        audit(sp, r, operands=ops.ops)
        r = sp.einsum("ijk,ijk->ij", x, x)
        assert isinstance(r, sp.SparseArray) and np.array_equal(r.todense(), (dx.astype(np.float64) ** 2).sum(axis=2).astype(dtype))
        audit(sp, r, operands=ops.ops)
        ops.check()


@gpu
@pytest.mark.parametrize("operands", ["float32", "bfloat16", "float16", "complex64"])
@pytest.mark.parametrize("fmt", ["coo", "gcxs"])
def test_sddmm_results(sp, fmt, operands):
    tdt = getattr(torch, operands)
    rng = np.random.default_rng(41)
    for shape, inner in (((300, 250), 64), ((300, 250), 7), ((4, 90, 70), 48)):
        keys = random_keys(rng, shape, 20_011 if len(shape) == 2 else 9_001, margin_rows=1)
        sval, coords = eighths(rng, keys.size, np.float32), np.unravel_index(keys, shape)
        s = make(sp, fmt, keys, sval, shape, np.int64)
        # operands of small integers: every sampled product is exact, and many are exactly zero (pruned)
        a = torch.from_numpy(rng.integers(-1, 2, size=shape[:-2] + (shape[-2], inner)).astype(np.float32)).cuda().to(tdt)
        bt = torch.from_numpy(rng.integers(-1, 2, size=shape[:-2] + (shape[-1], inner)).astype(np.float32)).cuda().to(tdt)
        ops = Untouched(s)
        for call in (1, 2):                           # (the second call uses the plans kept on the mask)
            r = sp.sddmm(s, a, bt=bt)
            assert type(r) is type(s) and r.shape == s.shape
            wide = torch.complex64 if tdt.is_complex else torch.float32
            full = _npy(torch.matmul(a.to(wide), bt.to(wide).transpose(-1, -2)))
            want = (sval * full[tuple(coords)]).astype(r.dtype)             # at the mask's positions; exact
            assert np.array_equal(r.todense()[tuple(coords)], want)
            if not tdt.is_complex:        # (mask value x (+0.0) is -0.0 for a negative mask value: a stored element, bit-wise)
                assert r.nnz == int((~inv.eq_bits(want, 0)).sum())
            audit(sp, r, pruned=True, operands=ops.ops)
        ops.check()


# ---- the fast GCXS slices and joins --------------------------------------------------------------------------------------------------
def _sliceable(sp, ca, dtype=np.float64, idt=np.int64):
    """a 60 x 60 matrix compressed along `ca` whose rows 20..29 (of the compressed axis) are empty, as are the first and last"""
    rng = np.random.default_rng(3)
    d = np.where(rng.random((60, 60)) < 0.2, rng.integers(1, 9, size=(60, 60)) / 8, 0.0).astype(dtype)
    idx = [slice(None)] * 2
    for lo, hi in ((0, 1), (20, 30), (59, 60)):
        idx[ca] = slice(lo, hi)
        d[tuple(idx)] = 0
    return sp.GCXS.from_numpy(d, compressed_axes=(ca,), idx_dtype=idt), d


RANGES = {"a == b == 0": (0, 0), "a == b in the middle": (40, 40), "a == b == n": (60, 60), "b < a": (50, 20), "empty rows": (21, 29),
          "empty rows and one more": (20, 31), "the whole range": (0, 60), "from the middle": (35, 60), "one row": (41, 42)}


@gpu
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ca", [0, 1], ids=["csr", "csc"])
@pytest.mark.parametrize("rng_name", list(RANGES))
def test_gcxs_slices_keep_the_invariants(sp, rng_name, ca, idt):
    """`x[a:b]` and `x[:, a:b]` of CSR and CSC matrices.  `a == b in the middle` is the empty compressed-axis slice whose single
    pointer was `indptr[a]`, not zero (fixed in `_gcxs._compressed_axis_slice`)."""
    x, d = _sliceable(sp, ca, idt=idt)
    a, b = RANGES[rng_name]
    if rng_name == "a == b in the middle":
        assert int(x.indptr[a]) > 0                  # the row's pointer is not zero: this is the case that went wrong
    ops = Untouched(x)
    for index in ((slice(a, b),), (slice(None), slice(a, b))):
        r = x[index]
        assert isinstance(r, sp.GCXS) and r.compressed_axes == (ca,), (type(r), r.compressed_axes)
        assert r.shape == d[index].shape and np.array_equal(r.todense(), d[index])
        audit(sp, r, pruned=True, operands=ops.ops)
    ops.check()


@gpu
@pytest.mark.parametrize("ca", [0, 1], ids=["csr", "csc"])
def test_gcxs_joins_of_slices_keep_the_invariants(sp, ca):
    """pieces cut by the fast slices (empty ones included) joined along the compressed axis (`_concatenate_compressed`: the
    pointers shifted by what came before) and along the other axis"""
    x, d = _sliceable(sp, ca)
    cuts = [(0, 0), (0, 25), (25, 25), (25, 40), (40, 40), (40, 60), (60, 60)]

    def piece(axis, lo, hi):
        idx = [slice(None)] * 2
        idx[axis] = slice(lo, hi)
        return x[tuple(idx)]

    for axis in (0, 1):
        pieces = [piece(axis, lo, hi) for lo, hi in cuts]
        ops = Untouched(x, *pieces)
        r = sp.concatenate(pieces, axis=axis)
        assert isinstance(r, sp.GCXS) and np.array_equal(r.todense(), d)
        audit(sp, r, pruned=True, operands=ops.ops)
        r = sp.concatenate([pieces[2], pieces[4]], axis=axis)          # empty pieces only
        assert r.nnz == 0 and r.shape[axis] == 0
        audit(sp, r, pruned=True, operands=ops.ops)
        r = sp.concatenate([pieces[4], pieces[5], pieces[2], pieces[1]], axis=axis)
        lead = (slice(None),) * axis
        want = np.concatenate([d[lead + (slice(40, 60),)], d[lead + (slice(0, 25),)]], axis=axis)
        assert np.array_equal(r.todense(), want)
        audit(sp, r, pruned=True, operands=ops.ops)
        ops.check()


# ---- the zero-bit note a producer leaves, and a write after it ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("write", ["*= 2", "[0] = 0", "replaced"])
@pytest.mark.parametrize("container", ["gcxs", "coo"])
@pytest.mark.parametrize("route", ["small", "buckets"])
def test_zero_bit_note_of_a_product_is_not_believed_after_a_write(sp, route, container, write, monkeypatch):
    """A product without an exact zero: the kernel notes 0 zeros, the prune returns early on the note and the container keeps
    it (`known_eq_bits == 0`).  A write must end that: `known_eq_bits` is None, and a prune reads the values and drops the zero
    that was written - with a stale note it would return early and keep it."""
    from sparse_amd import _kernels as K

    kw = dict(dtype=np.float64, idx_dtype=np.int32, format="gcxs", compressed_axes=(0,))
    a, b = sp.random((200, 300), density=0.05, random_state=1, **kw), sp.random((300, 250), density=0.05, random_state=2, **kw)
    if route == "buckets":
        monkeypatch.setattr(K, "SPGEMM_SMALL", False)
    K.SPGEMM_STATS.clear()
    c = a @ b if container == "gcxs" else sp.tensordot(a, b, axes=1, return_type=sp.COO)       # (values in (0, 1): no zero)
    assert K.SPGEMM_STATS.get("kernel") == route and isinstance(c, sp.GCXS if container == "gcxs" else sp.COO)
    assert K.known_eq_bits(c.data, c.fill_value) == 0, "the product's note did not reach the container"
    assert_canonical(c, pruned=True)
    nnz = c.nnz
    if write == "*= 2":
        c.data *= 2
        c.data[3] = 0
    elif write == "[0] = 0":
        c.data[0] = 0
    else:
        fresh = c.data.clone()
        fresh[nnz - 1] = 0
        c.data = fresh
    assert K.known_eq_bits(c.data, c.fill_value) is None
    p = _pruned_copy(c)
    assert p.nnz == nnz - 1
    assert_canonical(p, pruned=True)
    if container == "gcxs":
        q = sp.GCXS(c, prune=True)
        assert q.nnz == nnz - 1
        assert_canonical(q, pruned=True)

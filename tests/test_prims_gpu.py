"""The key and index primitives (csrc/prims.hip through the `_kernels` wrappers) against the plain NumPy references of
tests/prims_cases.py, at every size and value where the code takes another path: the merge/radix switches and both key
width configurations of the sorts, the one-workgroup scan and the growth of the device-wide scan's workspace, both
rows_to_indptr kernels with empty stretches around the wave-wide fill's threshold at every lane position, the three division
classes of keys_to_csr, both csr_to_keys kernels, the CSR <-> CSC swap's 24 -> 25 bit step and its fallback routes,
dense_nonfill's tile edges in both comparison modes, and the second trip of every grid-stride loop.  Everything is integers
and bit patterns: every comparison is exact.

Entry points whose output length the kernel derives are also called directly with the output inside a larger buffer of
sentinels (`_Guarded`): nothing outside the output may change."""
import functools

import numpy as np
import pytest
import torch

import prims_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 256          # sentinel elements on each side of a guarded output
_TORCH = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32, "float64": torch.float64,
          "int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64, "bool": torch.bool,
          "complex64": torch.complex64, "complex128": torch.complex128}
_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
_TSIGNED = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
INDEX_TYPES = (np.int32, np.int64)


@pytest.fixture(scope="module")
def K():
    from sparse_amd import _kernels

    return _kernels


def dev(a, dtype=None):
    """NumPy array -> device tensor with the same bits (unsigned words travel as signed ones), viewed as `dtype`"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u":
        a = a.view(_SIGNED[a.dtype.itemsize])
    t = torch.from_numpy(a).cuda()
    if dtype is not None and t.dtype != dtype:
        t = t.view(torch.uint8).view(dtype) if dtype == torch.bool else t.view(dtype)
    return t


def host(t):
    return t.cpu().numpy()


def host_bits(t):
    """the unsigned bit view of a device tensor (bfloat16 and bool included)"""
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    elif t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return pc.bits_of(t.cpu().numpy())


class _Guarded:
    """an output of n elements inside a buffer of sentinels"""

    def __init__(self, n, dtype, sentinel=-77):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
        self.out = self.buf[GUARD:GUARD + n]

    def check(self, what=""):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sentinel).all(), f"{what}: written in front of the output"
        assert (b[GUARD + self.n:] == self.sentinel).all(), f"{what}: written behind the output"
        return b[GUARD:GUARD + self.n]


def _call(name, *args):
    from sparse_amd import _ffi

    _ffi.call(name, *args)


def _stream():
    from sparse_amd._device import stream_ptr

    return stream_ptr(torch.device("cuda", torch.cuda.current_device()))


def _ptr(t):
    return 0 if t is None or t.numel() == 0 else t.data_ptr()


def _code(np_index_type):
    from sparse_amd import _ffi

    return _ffi.I32 if np.dtype(np_index_type) == np.int32 else _ffi.I64


# ---- a. sorts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_key", pc.SORT_CASES, ids=lambda v: str(v))
def test_sorts_are_the_stable_argsort(K, n, max_key):
    assert K._key_bits(max_key) == pc.key_bits(max_key)
    keys = pc.sort_keys_case(n, max_key)
    want_keys, want_perm = pc.ref_sort(keys)
    tk = dev(keys)
    sk, perm = K.sort_keys(tk, max_key)
    assert np.array_equal(host(sk), want_keys)
    assert np.array_equal(host(perm), want_perm)               # equal keys keep their order
    assert np.array_equal(host(tk), keys)                      # the input is not sorted in place
    for nbytes, tdt in ((4, torch.float32), (8, torch.float64), (4, torch.int32), (8, torch.int64)):
        bits = pc.payload_bits(n, nbytes)
        sk, sv = K.sort_key_value(tk, dev(bits, tdt), max_key)
        assert sv.dtype == tdt
        assert np.array_equal(host(sk), want_keys)
        assert np.array_equal(host_bits(sv), bits[want_perm])  # NaN patterns included: the payload moves bit-wise


def test_sorts_and_scan_refuse_a_workspace_that_is_too_small(K):
    """The full workspace is handed over with a size one byte short: nothing can be overrun even if the check were wrong."""
    from sparse_amd import _ffi

    lib, n, s = _ffi.lib(), 5000, _stream()
    keys, vals = dev(pc.sort_keys_case(n, 1000)), dev(np.arange(n, dtype=np.int64))
    ko, vo = torch.full_like(keys, -5), torch.full_like(vals, -5)

    def refused(name, *args):
        with pytest.raises(_ffi.HipBackendError, match="workspace too small") as e:
            _ffi.call(name, *args)
        assert e.value.code == -3
        torch.cuda.synchronize()
        assert (ko == -5).all() and (vo == -5).all()           # nothing ran

    need = int(lib.spamd_sort_pairs_ws_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    refused("spamd_sort_pairs", n, _ptr(keys), _ptr(ko), _ptr(vals), _ptr(vo), 10, _ptr(ws), need - 1, s)
    for nbytes, v in ((8, vals), (4, vals.to(torch.int32))):
        need = int(lib.spamd_sort_kv_ws_bytes(nbytes, n))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        refused("spamd_sort_kv", nbytes, n, _ptr(keys), _ptr(ko), _ptr(v), _ptr(vo), 10, _ptr(ws), need - 1, s)
    m = pc.SMALL_SCAN_MAX + 5                                   # beyond the one-workgroup scan, which takes no workspace
    flags = torch.ones(m + 1, dtype=torch.int64, device="cuda")
    ko = torch.full_like(flags, -5)
    need = int(lib.spamd_scan_ws_bytes(m))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    refused("spamd_exclusive_scan", m, _ptr(flags), _ptr(ko), _ptr(ws), need - 1, s)
    _ffi.call("spamd_exclusive_scan", m, _ptr(flags), _ptr(ko), _ptr(ws), need, s)        # the size the query returns serves
    assert np.array_equal(host(ko), np.arange(m + 1))
    _ffi.call("spamd_exclusive_scan", 100, _ptr(flags), _ptr(ko), 0, 0, s)                 # short arrays need none
    assert np.array_equal(host(ko)[:101], np.arange(101))


# ---- b. scan -------------------------------------------------------------------------------------------------------
def _scan_guarded(values):
    """spamd_exclusive_scan with the output AND the workspace inside sentinels: the scan runs over len(values) items, and the
    size query has to cover them"""
    from sparse_amd import _ffi

    n = values.size - 1
    out = _Guarded(n + 1, torch.int64)
    need = int(_ffi.lib().spamd_scan_ws_bytes(n))
    assert need > 0
    ws = _Guarded(need, torch.uint8, sentinel=0xA5)
    _call("spamd_exclusive_scan", n, _ptr(dev(values)), _ptr(out.out), _ptr(ws.out), need, _stream())
    got = out.check("scan output")
    ws.check("scan workspace")
    return got


@pytest.mark.parametrize("length", pc.SCAN_LENGTHS)
def test_exclusive_scan(K, length):
    for big in (False, True):
        values = pc.scan_case(length, big=big)
        want = pc.ref_scan(values)
        assert np.array_equal(host(K.exclusive_scan(dev(values))), want)         # (the sentinel in[n] does not enter out[n])
        assert np.array_equal(_scan_guarded(values), want)


def test_exclusive_scan_where_its_workspace_grows(K):
    """The n (beyond the one-workgroup scan) at which the size query first returns more: the scan runs over n + 1 items, so
    that is where a query made for n items would have been one block short."""
    from sparse_amd import _ffi

    q = _ffi.lib().spamd_scan_ws_bytes
    base = int(q(pc.SMALL_SCAN_MAX))
    assert base > 0
    hi = pc.SMALL_SCAN_MAX
    while int(q(hi)) <= base:
        hi *= 2
        assert hi <= 2 ** 26, "the workspace of the scan never grows"
    lo = hi // 2                      # q(lo) == base < q(hi): bisect for the first n with more
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if int(q(mid)) > base else (mid, hi)
    first = hi
    assert int(q(first)) > base == int(q(first - 1))
    print(f"spamd_scan_ws_bytes: {base} bytes up to n = {first - 1}, {int(q(first))} from n = {first}")
    for n in (first - 1, first, first + 1):
        values = pc.scan_case(n + 1, seed=1)
        want = pc.ref_scan(values)
        assert np.array_equal(_scan_guarded(values), want)
        assert np.array_equal(host(K.exclusive_scan(dev(values))), want)


# ---- c. rows_to_indptr -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("name", list(pc.ROWS_CASES))
def test_rows_to_indptr(K, name, idt):
    rows, R = pc.ROWS_CASES[name]
    want = pc.ref_rows_to_indptr(rows, R)
    tr = dev(rows.astype(idt))
    got = K.rows_to_indptr(tr, R)
    assert got.dtype == torch.int64 and np.array_equal(host(got), want), name
    g = _Guarded(R + 1, torch.int64)
    _call("spamd_rows_to_indptr", _code(idt), rows.size, _ptr(tr), R, _ptr(g.out), _stream())
    assert np.array_equal(g.check(name), want)


def test_rows_to_indptr_is_the_same_on_either_side_of_its_dispatch(K):
    (rows, Ra), (_, Rb) = pc.ROWS_CASES["R = 8 nnz"], pc.ROWS_CASES["R = 8 nnz + 1"]
    tr = dev(rows)
    a, b = host(K.rows_to_indptr(tr, Ra)), host(K.rows_to_indptr(tr, Rb))
    assert np.array_equal(a, b[:Ra + 1]) and b[Rb] == rows.size


# ---- d. keys_to_csr --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.K2C_SHAPES, ids=str)
def test_keys_to_csr(K, shape):
    R, C = shape
    keys = pc.k2c_keys(R, C)
    want_ptr, want_idx = pc.ref_keys_to_csr(keys, R, C)
    tk = dev(keys)
    for idt in INDEX_TYPES:
        if idt == np.int32 and C >= 2 ** 31:
            continue
        tdt = _TSIGNED[np.dtype(idt).itemsize]
        indptr, indices = K.keys_to_csr(tk, R, C, tdt)
        assert indptr.dtype == tdt and indices.dtype == tdt
        assert np.array_equal(host(indptr), want_ptr) and np.array_equal(host(indices), want_idx), (shape, idt)
        gp, gi = _Guarded(R + 1, tdt), _Guarded(keys.size, tdt)
        _call("spamd_keys_to_csr", _code(idt), keys.size, _ptr(tk), R, C, _ptr(gp.out), _ptr(gi.out), _stream())
        assert np.array_equal(gp.check("indptr"), want_ptr) and np.array_equal(gi.check("indices"), want_idx)


# ---- e. csr_to_keys --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("R,nnz,C", pc.CSR_CASES)
def test_csr_to_keys(K, R, nnz, C, idt):
    indptr, indices = pc.csr_case(R, nnz, C, idt)
    want = pc.ref_csr_to_keys(indptr, indices, C)
    tp, ti = dev(indptr), dev(indices)
    assert np.array_equal(host(K.csr_to_keys(tp, ti, R, C)), want)
    g = _Guarded(nnz, torch.int64)
    _call("spamd_csr_to_keys", _code(idt), R, nnz, _ptr(tp), _ptr(ti), C, _ptr(g.out), _stream())
    assert np.array_equal(g.check("keys"), want)
    # the round trip through keys_to_csr (int64: C may pass 2^31)
    p2, i2 = K.keys_to_csr(dev(np.sort(want)), R, C, torch.int64)
    assert np.array_equal(host(p2), indptr.astype(np.int64)) and np.array_equal(host(i2), np.sort(want) % C)


# ---- f. csx_swap_2d --------------------------------------------------------------------------------------------------
VALUE_TYPES = ("float32", "float64", "int32", "int64")


def _values(nnz, name, seed=0):
    """nnz values of type `name` as a NumPy array, every bit pattern allowed (NaNs included)"""
    dt = np.dtype(name)
    words = pc.payload_bits(nnz * (dt.itemsize // 8), 8, seed) if dt.itemsize >= 8 else pc.payload_bits(nnz, 4, seed).astype(f"u{dt.itemsize}")
    return words.view(dt)


def _check_swap(K, case, name, idt, ptr_type=None, guarded=False):
    n_major, n_minor, nnz, mode = case
    indices, indptr = _csx(case)
    data = _values(nnz, name, seed=n_major)
    assert data.size == nnz
    want_data, want_idx, want_ptr = pc.ref_csx_swap(data, indices, indptr, n_minor)
    td, ti, tp = dev(data), dev(indices.astype(idt)), dev(indptr.astype(ptr_type or idt))
    nd, ni, nptr = K.csx_swap_2d(td, ti, tp, n_major, n_minor)
    what = (case, name, np.dtype(idt).name)
    assert nd.dtype == td.dtype and ni.dtype == ti.dtype and nptr.dtype == ti.dtype and nptr.numel() == n_minor + 1, what
    assert np.array_equal(host_bits(nd), pc.bits_of(want_data)), what
    assert np.array_equal(host(ni), want_idx), what
    assert np.array_equal(host(nptr), want_ptr), what
    if guarded:
        from sparse_amd import _ffi

        wide = data.dtype.itemsize == 8
        need = int((_ffi.lib().spamd_csx_swap8_ws_bytes if wide else _ffi.lib().spamd_csx_swap_ws_bytes)(nnz))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        gd, gi, gp = _Guarded(nnz, _TSIGNED[data.dtype.itemsize]), _Guarded(nnz, ti.dtype), _Guarded(n_minor + 1, ti.dtype)
        _call("spamd_csx_swap8" if wide else "spamd_csx_swap", _code(idt), n_major, n_minor, nnz, _ptr(td), _ptr(ti), _ptr(tp),
              _ptr(gd.out), _ptr(gi.out), _ptr(gp.out), _ptr(ws), need, _stream())
        assert np.array_equal(pc.bits_of(gd.check("data")), pc.bits_of(want_data)), what
        assert np.array_equal(gi.check("indices"), want_idx) and np.array_equal(gp.check("indptr"), want_ptr), what


@functools.lru_cache(maxsize=4)
def _csx(case):
    return pc.csx_case(*case)


@pytest.mark.parametrize("case", pc.CSX_SMALL, ids=str)
def test_csx_swap_fast_path_every_type(K, case):
    for name in VALUE_TYPES:
        for idt in INDEX_TYPES:
            _check_swap(K, case, name, idt, guarded=True)


_LARGE_TYPES = (("float32", np.int32), ("float64", np.int64), ("int32", np.int64), ("int64", np.int32))


@pytest.mark.parametrize("i", range(len(pc.CSX_LARGE)), ids=lambda i: str(pc.CSX_LARGE[i]))
def test_csx_swap_at_the_sort_switches(K, i):
    """the merge/radix switch of either configuration and the 24 -> 25 key bit step between them (2^24 and 2^24 + 1 minor
    indices, the last of which needs the 25th bit)"""
    name, idt = _LARGE_TYPES[i % len(_LARGE_TYPES)]
    _check_swap(K, pc.CSX_LARGE[i], name, idt)


@pytest.mark.parametrize("case", [(9, 257, 70, "ends"), (1, 256, 70, "ends"), (12, 5000, 3000, "gaps")], ids=str)
def test_csx_swap_fallback_routes(K, case):
    for name in ("complex64", "complex128", "float16", "int8"):
        for idt in INDEX_TYPES:
            _check_swap(K, case, name, idt)
    for name in ("float32", "float64"):                      # indices and pointers of different widths
        _check_swap(K, case, name, np.int32, ptr_type=np.int64)
        _check_swap(K, case, name, np.int64, ptr_type=np.int32)


# ---- g. dense_nonfill ------------------------------------------------------------------------------------------------
def _fill_value(name, fill_bits):
    """the fill value as the wrapper takes it: a NumPy scalar with exactly these bits"""
    nbytes, kind = pc.DENSE_TYPES[name]
    word = np.array([fill_bits], dtype=f"u{nbytes}")
    if name == "bfloat16":
        return word.view(np.int16)[0]                  # (no NumPy type: the tensor goes in as int16, bit-identity is the same)
    return word.view(np.bool_ if kind == "b" else ("int" + str(8 * nbytes) if kind == "i" else name))[0]


def _dense_direct(bits, fill_bits, mask, guarded=True):
    """spamd_dense_nonfill itself: outputs with room for n entries inside sentinels; (keys, value bits)"""
    from sparse_amd import _ffi

    n, nbytes = bits.size, bits.dtype.itemsize
    tdt = _TSIGNED[nbytes]
    work = torch.empty(int(_ffi.lib().spamd_dense_nonfill_work_words(n)), dtype=torch.int64, device="cuda")
    gk, gv = _Guarded(n, torch.int64), _Guarded(n, tdt, sentinel=-77)
    _call("spamd_dense_nonfill", nbytes, n, _ptr(dev(bits)), int(fill_bits), int(mask), _ptr(work), _ptr(gk.out), _ptr(gv.out), _stream())
    count = int(work[1])
    keys, vals = gk.check("keys"), gv.check("values")
    assert (keys[count:] == -77).all() and (vals[count:] == -77).all(), "written beyond the count"
    return keys[:count], pc.bits_of(vals[:count])


@pytest.mark.parametrize("n", pc.DENSE_N)
@pytest.mark.parametrize("name", list(pc.DENSE_TYPES))
def test_dense_nonfill(K, name, n):
    nbytes, kind = pc.DENSE_TYPES[name]
    sp = pc.float_specials(name) if kind == "f" else None
    nonzero_fill = 1 if kind == "b" else (0x3c if nbytes == 1 else (sp["+nan"] if nbytes == 2 else sp["1"]) if sp else 0x3c01)
    tdt = torch.int16 if name == "bfloat16" else _TORCH[name]
    ones = (1 << (8 * nbytes)) - 1
    for fill_bits in (0, nonzero_fill):
        fv = _fill_value(name, fill_bits)
        for density in (0.1, 0.9, 0.0, 1.0):                     # (0.1 / 0.9: either side of count * 4 < n * 3)
            bits = pc.dense_case(name, n, fill_bits, density)
            want_keys, want_vals = pc.ref_dense_nonfill(bits, fill_bits)
            assert density not in (0.0, 1.0) or want_keys.size == int(density) * n
            flat = dev(bits, tdt)
            got = K.dense_nonfill(flat, fv)
            assert got is not None and got[1].dtype == tdt
            assert np.array_equal(host(got[0]), want_keys) and np.array_equal(host_bits(got[1]), want_vals), (name, n, fill_bits, density)
            if n in (pc.DN_TILE - 1, pc.DN_TILE, pc.DN_TILE + 1) or density == 0.1:
                dk, dv = _dense_direct(bits, fill_bits, ones)
                assert np.array_equal(dk, want_keys) and np.array_equal(dv, want_vals)
            # value != 0: both zeros go, NaNs of either sign stay
            if fill_bits != 0:
                if name != "bfloat16":
                    assert K.dense_nonfill(flat, fv, numeric=True) is None
                continue
            nk, nv = pc.ref_dense_nonfill(bits, 0, float_numeric=kind == "f")
            if sp and density == 0.9 and n > 64:
                kept = set(nv.tolist())
                assert {sp["+nan"], sp["-nan"]} <= kept and sp["-0"] not in kept and sp["-0"] in set(bits.tolist())
            if name == "bfloat16":
                gk, gv = _dense_direct(bits, 0, ones >> 1)
            else:
                got = K.dense_nonfill(flat, fv, numeric=True)
                gk, gv = host(got[0]), host_bits(got[1])
            assert np.array_equal(gk, nk) and np.array_equal(gv, nv), (name, n, density, "numeric")


# ---- h. flags and movement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.MOVE_N)
def test_flag_heads(K, n):
    rng = np.random.default_rng(n)
    keys = np.cumsum(rng.integers(0, 2, size=n, dtype=np.int64) * rng.integers(1, 2 ** 40, size=n, dtype=np.int64))
    got = K.flag_heads(dev(keys))
    assert got.numel() == n + 1 and np.array_equal(host(got)[:n], pc.ref_flag_heads(keys))
    same = K.flag_heads(dev(np.full(n, 7, dtype=np.int64)))
    assert host(same)[:n].sum() == 1 and int(same[0]) == 1


_ELEM_TYPES = {1: "int8", 2: "float16", 4: "float32", 8: "float64", 16: "complex128"}


@pytest.mark.parametrize("n", pc.MOVE_N)
@pytest.mark.parametrize("nbytes", pc.ELEM_BYTES)
def test_flag_ne_bits_and_count_eq_bits(K, nbytes, n):
    name = _ELEM_TYPES[nbytes]
    rng = np.random.default_rng([nbytes, n])
    if nbytes == 1:
        fills = [np.int8(0), np.int8(-128)]
        pool = np.array([0, -128, 1, -1, 127], dtype=np.int8)
    elif nbytes == 16:
        nan, nan2 = np.array([pc.NAN64[0], pc.NAN64[4]], dtype=np.uint64).view(np.float64)
        pool = np.array([0j, complex(0.0, -0.0), complex(-0.0, 0.0), complex(nan, 1.0), complex(nan2, 1.0), complex(1.0, nan), 1 + 2j], dtype=np.complex128)
        fills = [pool[0], pool[3]]
        assert not np.array_equal(pc.bits_of(pool[3:4]), pc.bits_of(pool[4:5]))        # the same NaN-ness, another payload
    else:
        sp = pc.float_specials(name)
        pool = np.array([sp[k] for k in ("+0", "-0", "+nan", "-nan", "nan2", "1", "denormal")], dtype=f"u{nbytes}").view(name)
        fills = [pool[0], pool[2]]          # +0.0 (then -0.0 differs) and a NaN (then only its own bit pattern is equal)
    data = pool[rng.integers(0, pool.size, size=n)]
    data[0], data[-1] = pool[0], pool[min(3, pool.size - 1)]
    td = dev(data)
    for fill in fills:
        want = pc.ref_flag_ne_bits(pc.bits_of(data), pc.bits_of(np.array([fill], dtype=data.dtype))[0])
        got = K.flag_ne_bits(td, fill)
        assert got.numel() == n + 1 and np.array_equal(host(got)[:n], want), (name, n, fill)
        assert K.count_eq_bits(td, fill) == n - int(want.sum())


def _flags_case(n, seed):
    rng = np.random.default_rng([seed, n])
    flags = np.zeros(n + 1, dtype=np.int64)
    flags[:n] = rng.integers(0, 2, size=n)
    flags[n] = pc.SCAN_SENTINEL          # (the slot behind the flags: ignored)
    return flags, pc.ref_scan(flags)


@pytest.mark.parametrize("n", pc.MOVE_N)
def test_compact_gather_scatter_1d(K, n):
    flags, offs = _flags_case(n, 1)
    count = int(offs[n])
    rng = np.random.default_rng(n)
    m = n // 2 + 1
    perm = rng.integers(0, m, size=n, dtype=np.int64)          # repeats: a gather is not a permutation
    perm[0], perm[-1] = m - 1, 0
    tf, to, tperm = dev(flags), dev(offs), dev(perm)
    assert np.array_equal(host(K.exclusive_scan(tf)), offs)
    spots = rng.permutation(n + 100)[:n].astype(np.int64)       # distinct places of a larger destination
    for name in ("int8", "int16", "float32", "float64", "complex128"):
        src = _values(n, name, seed=3) if name in ("float32", "float64", "complex128") else rng.integers(-100, 100, size=n).astype(name)
        ts = dev(src)
        got = K.compact(ts, tf, to, count)
        assert got.numel() == count and np.array_equal(host_bits(got), pc.bits_of(src[flags[:n] == 1])), name
        got = K.gather(ts[:m], tperm)
        assert np.array_equal(host_bits(got), pc.bits_of(src[:m][perm])), name
        dst0 = _values(n + 100, name, seed=4) if name in ("float32", "float64", "complex128") else np.full(n + 100, 5, dtype=name)
        want = dst0.copy()
        want[spots] = src
        tdst = dev(dst0)
        assert K.scatter_into(tdst, dev(spots), ts) is tdst
        assert np.array_equal(host_bits(tdst), pc.bits_of(want)), name


@pytest.mark.parametrize("n", pc.MOVE_N)
@pytest.mark.parametrize("k", pc.MOVE_ROWS)
def test_compact_gather_rows(K, k, n):
    flags, offs = _flags_case(n, 2)
    count = int(offs[n])
    rng = np.random.default_rng([k, n])
    m = n // 2 + 1
    perm = rng.integers(0, m, size=n, dtype=np.int64)
    perm[0], perm[-1] = m - 1, 0
    tf, to, tperm = dev(flags), dev(offs), dev(perm)
    for name in ("int32", "int64") if n < pc.N1 or k < 16 else ("int32",):
        src = rng.integers(-2 ** 30, 2 ** 30, size=(k, n)).astype(name)
        ts = dev(src)
        got = K.compact(ts, tf, to, count)
        assert tuple(got.shape) == (k, count) and np.array_equal(host(got), src[:, flags[:n] == 1]), (name, k, n)
        small = np.ascontiguousarray(src[:, :m])
        got = K.gather(dev(small), tperm)
        assert tuple(got.shape) == (k, n) and np.array_equal(host(got), small[:, perm]), (name, k, n)


def test_more_rows_than_the_grid_takes_are_refused(K):
    from sparse_amd import _ffi

    src = torch.zeros((pc.TOO_MANY_ROWS, 4), dtype=torch.int64, device="cuda")
    flags, offs = _flags_case(4, 3)
    with pytest.raises(_ffi.HipBackendError, match="invalid argument"):
        K.compact(src, dev(flags), dev(offs), int(offs[4]))
    with pytest.raises(_ffi.HipBackendError, match="invalid argument"):
        K.gather(src, dev(np.array([3, 0, 0, 1], dtype=np.int64)))
    ok = K.gather(src[:65535], dev(np.array([3, 0, 0, 1], dtype=np.int64)))          # the last count that is taken
    assert tuple(ok.shape) == (65535, 4)


# ---- i. checks -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_keys():
    keys = np.arange(pc.CHECK_N, dtype=np.int64) * 3
    return keys, dev(keys)


def _diff_flags(keys):
    d = np.diff(keys)
    return bool((d < 0).any()), bool((d == 0).any())


def test_keys_check_finds_one_bad_pair_anywhere(K, check_keys):
    keys, tk = check_keys
    assert K.keys_check(tk) == _diff_flags(keys) == (False, False)
    for p in pc.CHECK_POSITIONS:
        for bad in (keys[p - 1] - 1, keys[p - 1]):          # one inversion; one equal pair
            old = keys[p]
            try:
                keys[p] = bad
                tk[p] = int(bad)
                want = _diff_flags(keys)
                assert want == ((True, False) if bad < keys[p - 1] else (False, True))
                assert K.keys_check(tk) == want, (p, "inversion" if want[0] else "equal pair")
            finally:
                keys[p] = old
                tk[p] = int(old)
    assert K.keys_check(tk) == (False, False)
    pairs = np.repeat(np.arange(1000, dtype=np.int64), 2)      # equal pairs only
    assert K.keys_check(dev(pairs)) == _diff_flags(pairs) == (False, True)
    assert K.keys_check(dev(pairs[::-1].copy())) == (True, True)
    assert K.keys_check(dev(pairs[:1])) == (False, False)


@pytest.mark.parametrize("idt", INDEX_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ndim", pc.COORD_NDIMS)
def test_coords_in_range(K, ndim, idt):
    shape = {1: (1_000_003,), 3: (1201, 7, 977), 16: (2, 3) * 8}[ndim]
    for nnz, spots in ((1000, (0, 300, 999)), (pc.N1 + 257, (pc.N1 + 5,))):
        if ndim == 16 and nnz > 1000:
            continue
        coords = pc.coords_case(shape, nnz, idt)
        tc = dev(coords)
        assert K.coords_in_range(tc, shape) is True
        for d in range(ndim):
            for spot in spots:
                for bad in (shape[d], -1):
                    old = int(coords[d, spot])
                    tc[d, spot] = bad
                    assert K.coords_in_range(tc, shape) is False, (ndim, d, spot, bad)
                    tc[d, spot] = old
        assert K.coords_in_range(tc, shape) is True


# ---- j. linearize ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", list(pc.LINEARIZE_SHAPES))
def test_linearize_every_axis_order(K, ndim):
    shape = pc.LINEARIZE_SHAPES[ndim]
    for idt in INDEX_TYPES:
        for nnz in (5000,) + ((pc.N1 + 257,) if ndim == 2 else ()):
            coords = pc.coords_case(shape, nnz, idt)
            tc = dev(coords)
            assert np.array_equal(host(K.linearize(tc, shape)), pc.ref_linearize(coords, shape, range(ndim)))
            for order in pc.axis_orders(ndim):
                got = K.linearize(tc, shape, axis_order=order)
                assert got.dtype == torch.int64 and np.array_equal(host(got), pc.ref_linearize(coords, shape, order)), (ndim, order)


def test_linearize_int32_coordinates_whose_key_passes_2_31(K):
    shape = pc.LINEARIZE_INT32_SHAPE
    coords = pc.coords_case(shape, 5000, np.int32)
    for order in pc.axis_orders(2):
        want = pc.ref_linearize(coords, shape, order)
        assert want.max() == shape[0] * shape[1] - 1 > 2 ** 31
        assert np.array_equal(host(K.linearize(dev(coords), shape, axis_order=order)), want)


# ---- k. convert ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.CONVERT_N)
@pytest.mark.parametrize("src", pc.CONVERT_TYPES)
def test_convert_matrix(K, src, n):
    v = pc.convert_values(src, n)
    tv = dev(v)
    for dst in pc.CONVERT_TYPES:
        got = K.convert(tv, _TORCH[dst])
        assert got.dtype == _TORCH[dst]
        assert np.array_equal(host_bits(got), pc.bits_of(v.astype(dst))), (src, dst)      # bits: -0.0 stays -0.0


def test_convert_special_values(K):
    for name in ("float32", "float64"):
        sp = pc.float_specials(name)
        v = np.array([sp[k] for k in ("+nan", "-nan", "-0", "+0", "denormal", "1")], dtype=f"u{np.dtype(name).itemsize}").view(name)
        got = host(K.convert(dev(v), torch.bool))
        assert got.tolist() == [True, True, False, False, True, True] == v.astype(bool).tolist()
    i = np.array([2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3, 2 ** 62 + 1, 0, -1], dtype=np.int64)
    for dst in ("float32", "float64"):                                  # round to nearest even, as NumPy
        assert np.array_equal(host_bits(K.convert(dev(i), _TORCH[dst])), pc.bits_of(i.astype(dst))), dst
    assert float(i.astype(np.float32)[0]) == 2.0 ** 24 and float(i.astype(np.float64)[3]) == 2.0 ** 53
    d = np.array([1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24, 1e39, -1e39, 3.5e38, 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150,
                  0.75 * 2.0 ** -149, 1e-50, np.inf, -np.inf, -0.0], dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        want = d.astype(np.float32)
    assert np.isinf(want[3]) and want[6] != 0 and want[9] == 0 and want[10] != 0
    assert np.array_equal(host_bits(K.convert(dev(d), torch.float32)), pc.bits_of(want))
    assert np.array_equal(host_bits(K.convert(dev(want), torch.float64)), pc.bits_of(want.astype(np.float64)))

"""The merge-path union (csrc/merge.hip, csrc/merge_complex.hip) and the older three-kernel union (csrc/ewise.hip) against
the plain NumPy references of tests/merge_cases.py, on a table in which every case puts a matched pair, a tile's last item or
a tile's output count exactly where the tile logic switches: thread, wave and tile diagonals, the look-ahead and look-behind
keys, one-sided and nearly empty tiles, both store routes, every look-back window count, the recipe switch at 2^22 items, the
extreme keys, every value type.  Everything is integers and single IEEE operations on small integers: every comparison is
exact, bit for bit.

Every case runs through `_umath.merge_union` in each launch recipe (fused single launch, partition + single pass, partition +
count + fill), and through the C ABI directly with every output inside a larger buffer of sentinels: nothing in front of or
behind the na + nb output elements may change, and the elements from `total` on keep the sentinel - a write there is a wrong
offset, whatever the trimmed result looks like.

On an MI355X the file's 798 cases take 6.6 s; the slowest are the 2^22-item recipe cases and the 1024-tile look-back case
through `merge_union` (0.2 - 0.3 s each, most of it the NumPy reference)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import merge_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 256
RECIPES = {"fused": {}, "single pass": {"MERGE_FUSED": False}, "two passes": {"MERGE_FUSED": False, "MERGE_SINGLE_PASS": False}}
_TORCH = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8,
          "bool": torch.bool, "complex64": torch.complex64, "complex128": torch.complex128}
_SENTINEL = {torch.uint8: 0xA5}


def _is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def _id(call):
    name, dtype, op, fa, fb = call
    return f"{name}|{dtype}|{op}|{fa}"


CALLS = mc.calls()
REAL_CALLS = [c for c in CALLS if not _is_complex(c[1])]
COMPLEX_CALLS = [c for c in CALLS if _is_complex(c[1])]
FUSED_CALLS = [c for c in REAL_CALLS if c[0] != "nothing"]       # (nothing to merge: the fused form declines, see the return codes)


@pytest.fixture(scope="module")
def U():
    from sparse_amd import _umath

    return _umath


@pytest.fixture
def abi(monkeypatch):
    """the names of the C-ABI entry points called"""
    from sparse_amd import _ffi

    names, orig = [], _ffi.call

    def recording(name, *a):
        names.append(name)
        return orig(name, *a)

    monkeypatch.setattr(_ffi, "call", recording)
    return names


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=2)
def _dev_operands(name, dtype):
    return tuple(dev(a) for a in mc.case_operands(name, dtype))


def _scalar(value, dtype):
    return np.array(value, dtype=dtype)[()]


def _same_values(got, want):
    """bit for bit (a bool result may come back as 0 / 1 bytes)"""
    got = got.view(np.uint8) if got.dtype == np.bool_ else got
    want = want.view(np.uint8) if want.dtype == np.bool_ else want
    return got.dtype == want.dtype and np.array_equal(mc.bits_of(got), mc.bits_of(want))


class _Guarded:
    """an output of n elements inside a buffer of sentinels"""

    def __init__(self, n, dtype, zero=False):
        self.n, self.sentinel = n, _SENTINEL.get(dtype, -77)
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda")
        self.out = self.buf[GUARD:GUARD + n]
        if zero:
            self.out.zero_()

    def ptr(self):
        return self.out.data_ptr()            # (never null: an empty output still has its guards around it)

    def check(self, what=""):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sentinel).all(), f"{what}: written in front of the output"
        assert (b[GUARD + self.n:] == self.sentinel).all(), f"{what}: written behind the output"
        return b[GUARD:GUARD + self.n]


def _stream():
    from sparse_amd._device import stream_ptr

    return stream_ptr(torch.device("cuda", torch.cuda.current_device()))


def _ptr(t):
    return 0 if t is None or t.numel() == 0 else t.data_ptr()


def _bits_word(value, dtype):
    dt = np.dtype("uint8") if np.dtype(dtype) == np.bool_ else np.dtype(dtype)
    return int(np.asarray(value).astype(dt).reshape(1).view(f"u{dt.itemsize}")[0])


# ---- 1. through `_umath.merge_union`, every case in every launch recipe -------------------------------------------------
def _expected_entry_points(recipe, n):
    """the spamd_merge_* calls of one `merge_union`"""
    if n == 0:
        return []
    if recipe == "fused" and n <= mc.MERGE_FUSED_MAX_ITEMS:
        return ["spamd_merge_union_fused"]
    if recipe == "two passes":
        return ["spamd_merge_partition", "spamd_merge_union", "spamd_merge_union"]
    return ["spamd_merge_partition", "spamd_merge_union"]


@pytest.mark.parametrize("recipe", list(RECIPES))
@pytest.mark.parametrize("call", REAL_CALLS, ids=_id)
def test_merge_union(U, monkeypatch, abi, call, recipe):
    name, dtype, op, fa, fb = call
    for k, v in RECIPES[recipe].items():
        monkeypatch.setattr(U, k, v)
    ka, va, kb, vb = _dev_operands(name, dtype)
    keys, vals, fo, st = mc.case_reference(*call)
    gk, gv = U.merge_union(op, ka, va, kb, vb, _scalar(fa, dtype), _scalar(fb, dtype), fo)
    torch.cuda.synchronize()
    ran = [n for n in abi if n.startswith("spamd_merge")]
    assert ran == _expected_entry_points(recipe, ka.numel() + kb.numel())         # the recipe that was asked for is the one that ran
    gk, gv = host(gk), host(gv)
    assert gk.size == keys.size == st.total, (gk.size, keys.size)
    assert np.array_equal(gk, keys)
    assert _same_values(gv, vals)
    assert gv.dtype == vals.dtype or (vals.dtype == np.bool_ and gv.dtype in (np.bool_, np.uint8))


@pytest.mark.parametrize("call", COMPLEX_CALLS, ids=_id)
def test_merge_union_complex(U, abi, call):
    name, dtype, op, fa, fb = call
    ka, va, kb, vb = _dev_operands(name, dtype)
    keys, vals, fo, st = mc.case_reference(*call)
    gk, gv = U.merge_union(op, ka, va, kb, vb, _scalar(fa, dtype), _scalar(fb, dtype), fo)       # -> `_cmerge_union`
    torch.cuda.synchronize()
    assert abi == ["spamd_merge_partition", "spamd_merge_union_complex"]
    assert np.array_equal(host(gk), keys) and _same_values(host(gv), vals)


# ---- 2. the C ABI itself, outputs inside sentinels ------------------------------------------------------------------------
class _Direct:
    """the arguments of one call of the table as the C ABI takes them"""

    def __init__(self, U, call):
        from sparse_amd import _ffi

        name, dtype, op, fa, fb = call
        self.ka, self.va, self.kb, self.vb = _dev_operands(name, dtype)
        if self.va.dtype == torch.bool:
            self.va, self.vb = self.va.view(torch.uint8), self.vb.view(torch.uint8)
        self.keys, self.vals, self.fo, self.st = mc.case_reference(*call)
        self.na, self.nb = int(self.ka.numel()), int(self.kb.numel())
        self.n = self.na + self.nb
        lib = _ffi.lib()
        self.nblocks = int(lib.spamd_merge_num_blocks(self.na, self.nb))
        assert self.nblocks == self.st.nblocks == int(lib.spamd_merge_fused_blocks(self.na, self.nb))
        out_np = np.dtype("uint8") if self.vals.dtype == np.bool_ else self.vals.dtype
        self.out_t = _TORCH[out_np.name]
        self.part = dev(self.st.part)                        # the reference's partition: the union is checked on its own
        if _is_complex(dtype):
            self.code = U._CBIN[op]
            self.type_code = U._CCODE[self.va.dtype]
            self.fills = [np.array([fa], dtype=dtype), np.array([fb], dtype=dtype), np.array([self.fo]).astype(out_np)]
            self.fill_args = tuple(f.ctypes.data_as(ctypes.c_void_p) for f in self.fills)
        else:
            self.code = U._BIN[op]
            self.type_code = U._CODE[self.va.dtype]
            self.fill_args = (_bits_word(fa, dtype), _bits_word(fb, dtype), _bits_word(self.fo, out_np))
        self.operands = (self.na, _ptr(self.ka), _ptr(self.va), self.nb, _ptr(self.kb), _ptr(self.vb))

    def outputs(self):
        return _Guarded(self.n, torch.int64), _Guarded(self.n, self.out_t)

    def check_outputs(self, gk, gv, total, what):
        k, v = gk.check(what + ": keys"), gv.check(what + ": values")
        assert total == self.st.total, (what, total, self.st.total)
        assert (k[total:] == gk.sentinel).all() and (v[total:] == gv.sentinel).all(), f"{what}: written beyond the {total} outputs"
        assert np.array_equal(k[:total], self.keys), what
        assert _same_values(v[:total], self.vals), what


def _call(name, *args):
    from sparse_amd import _ffi

    _ffi.call(name, *args)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_partition_direct(name):
    ka, _, kb, _ = _dev_operands(name, mc.CASES[name].dtypes[0])
    dtype = mc.CASES[name].dtypes[0]
    st = mc.case_reference(name, dtype, *mc.case_ops(name, dtype)[0])[3]
    part = _Guarded(st.nblocks + 1 if st.nblocks else 0, torch.int64)
    _call("spamd_merge_partition", ka.numel(), _ptr(ka), kb.numel(), _ptr(kb), part.ptr(), _stream())
    assert np.array_equal(part.check("part"), st.part if st.nblocks else st.part[:0])


@pytest.mark.parametrize("call", REAL_CALLS, ids=_id)
def test_union_count_and_fill_direct(U, call):
    d = _Direct(U, call)
    args = (d.code, d.type_code, *d.operands, *d.fill_args, _ptr(d.part))
    counts = _Guarded(d.nblocks, torch.int64)
    _call("spamd_merge_union", 0, *args, counts.ptr(), 0, 0, 0, _stream())
    assert np.array_equal(counts.check("counts"), d.st.tot)                    # per-tile outputs
    offs = np.zeros(d.nblocks, dtype=np.int64)
    np.cumsum(d.st.tot[:-1], out=offs[1:])
    gk, gv = d.outputs()
    toffs = dev(offs)
    _call("spamd_merge_union", 1, *args, 0, _ptr(toffs), gk.ptr(), gv.ptr(), _stream())
    d.check_outputs(gk, gv, d.st.total, "fill pass")


@pytest.mark.parametrize("call", REAL_CALLS, ids=_id)
def test_union_single_pass_direct(U, call):
    d = _Direct(U, call)
    counts = _Guarded(d.nblocks + 2 if d.nblocks else 0, torch.int64)
    gk, gv = d.outputs()
    _call("spamd_merge_union", 2, d.code, d.type_code, *d.operands, *d.fill_args, _ptr(d.part), counts.ptr(), 0, gk.ptr(), gv.ptr(),
          _stream())
    work = counts.check("counts")
    d.check_outputs(gk, gv, int(work[d.nblocks + 1]) if d.nblocks else 0, "single pass")


def _fused(d, ws, total_dev, pinned):
    gk, gv = d.outputs()
    _call("spamd_merge_union_fused", d.code, d.type_code, *d.operands, *d.fill_args, ws.ptr(), total_dev.ptr(),
          pinned.data_ptr() if pinned is not None else 0, gk.ptr(), gv.ptr(), _stream())
    torch.cuda.synchronize()                                   # (a stream synchronisation: never a spin on the pinned word)
    total = int(total_dev.check("total_dev")[0])
    assert (ws.check("workspace") == 0).all(), "the workspace is not left zero"
    if pinned is not None:
        assert int(pinned[0]) == total
    d.check_outputs(gk, gv, total, "fused")


@pytest.mark.parametrize("call", FUSED_CALLS, ids=_id)
def test_union_fused_direct(U, call):
    d = _Direct(U, call)
    assert d.nblocks > 0
    ws = _Guarded(3 + d.nblocks, torch.int64, zero=True)       # exactly 3 + spamd_merge_fused_blocks words
    _fused(d, ws, _Guarded(1, torch.int64), None)
    pinned = torch.full((1,), -1, dtype=torch.int64).pin_memory()
    _fused(d, ws, _Guarded(1, torch.int64), pinned)            # the same workspace again, as the first call left it


def test_fused_calls_share_one_workspace(U):
    """tile counts 130, 1, 65, 2 on one workspace: every call finds it zero and leaves it zero"""
    cases = ("look-back 130 tiles", "specials: multiply", "look-back 65 tiles", "look-back 2 tiles")
    assert [mc.case_reference(c, "float64", "multiply", 0, 0)[3].nblocks for c in cases] == [130, 1, 65, 2]
    ws = _Guarded(3 + 130, torch.int64, zero=True)
    pinned = torch.full((1,), -1, dtype=torch.int64).pin_memory()
    for c in cases:
        pinned[0] = -1
        _fused(_Direct(U, (c, "float64", "multiply", 0, 0)), ws, _Guarded(1, torch.int64), pinned)


@pytest.mark.parametrize("call", COMPLEX_CALLS, ids=_id)
def test_union_complex_direct(U, call):
    d = _Direct(U, call)
    counts = _Guarded(d.nblocks + 2, torch.int64)
    gk, gv = d.outputs()
    _call("spamd_merge_union_complex", d.code, d.type_code, *d.operands, *d.fill_args, _ptr(d.part), counts.ptr(), gk.ptr(), gv.ptr(),
          _stream())
    d.check_outputs(gk, gv, int(counts.check("counts")[d.nblocks + 1]), "complex single pass")


def test_return_codes_without_a_launch(U):
    """as include/sparse_amd.h states them; every buffer is a real one, and none of them is touched"""
    from sparse_amd import _ffi

    lib, s = _ffi.lib(), _stream()
    EINVAL, ETYPE = -1, -2
    call = ("(1, 1) equal keys", "float64", "add", 0, 0)
    d = _Direct(U, call)
    part, counts, ws, total = (_Guarded(2, torch.int64), _Guarded(3, torch.int64), _Guarded(4, torch.int64, zero=True),
                               _Guarded(1, torch.int64))
    gk, gv = d.outputs()
    ka, va, kb, vb = _ptr(d.ka), _ptr(d.va), _ptr(d.kb), _ptr(d.vb)
    F32, F64 = _ffi.F32, _ffi.F64
    assert lib.spamd_merge_partition(-1, ka, 1, kb, part.ptr(), s) == EINVAL
    assert lib.spamd_merge_partition(1, ka, -1, kb, part.ptr(), s) == EINVAL
    for fill in (0, 1, 2):
        def union(op, type_code, na=1, nb=1):
            return lib.spamd_merge_union(fill, op, type_code, na, ka, va, nb, kb, vb, 0, 0, 0, _ptr(d.part), counts.ptr(),
                                         counts.ptr(), gk.ptr(), gv.ptr(), s)
        assert union(0, F64, na=-1) == EINVAL and union(0, F64, nb=-1) == EINVAL
        assert union(6, F64) == ETYPE                              # power is not a function of the fused merge
        assert union(64, F64) == ETYPE and union(66, F32) == ETYPE  # bitwise functions of floating-point values
        assert union(0, _ffi.C128) == ETYPE

    def fused(op, type_code, na=1, nb=1):
        return lib.spamd_merge_union_fused(op, type_code, na, ka, va, nb, kb, vb, 0, 0, 0, ws.ptr(), total.ptr(), 0, gk.ptr(),
                                           gv.ptr(), s)
    assert fused(0, F64, na=-1) == EINVAL and fused(0, F64, na=0, nb=0) == EINVAL      # nothing to merge: no launch, EINVAL
    assert fused(6, F64) == ETYPE and fused(65, F32) == ETYPE and fused(0, _ffi.C64) == ETYPE
    z = np.zeros(1, dtype=np.complex128)
    zp = z.ctypes.data_as(ctypes.c_void_p)

    def cunion(op, type_code, na=1, nb=1):
        return lib.spamd_merge_union_complex(op, type_code, na, ka, va, nb, kb, vb, zp, zp, zp, _ptr(d.part), counts.ptr(), gk.ptr(),
                                             gv.ptr(), s)
    assert cunion(0, _ffi.C128, na=-1) == EINVAL and cunion(0, F64) == ETYPE and cunion(4, _ffi.C128) == EINVAL
    torch.cuda.synchronize()
    for g, what in ((part, "part"), (counts, "counts"), (total, "total"), (gk, "keys"), (gv, "values")):
        assert (g.check(what) == g.sentinel).all(), what
    assert (ws.check("workspace") == 0).all()
    assert lib.spamd_merge_num_blocks(0, 0) == 0 == lib.spamd_merge_fused_blocks(0, 0)
    assert lib.spamd_merge_num_blocks(mc.TILE, 0) == 1 and lib.spamd_merge_num_blocks(mc.TILE, 1) == 2


# ---- 3. the older union: lower_bound_match, invert_flags, union_positions ---------------------------------------------------
def _lower_bound_match(q, h, tq, th):
    pos, match = _Guarded(q.size, torch.int64), _Guarded(q.size, torch.int64)
    _call("spamd_lower_bound_match", q.size, _ptr(tq), h.size, _ptr(th), pos.ptr(), match.ptr(), _stream())
    want_pos, want_match = np.searchsorted(h, q, "left"), np.isin(q, h).astype(np.int64)
    assert np.array_equal(pos.check("pos"), want_pos) and np.array_equal(match.check("match"), want_match)
    return want_pos, want_match


@pytest.mark.parametrize("name", mc.UNION_MERGE_CASES)
def test_union_merge_and_its_primitives(U, name):
    ka, _, kb, _ = mc.case_operands(name)
    tka, _, tkb, _ = _dev_operands(name, "float64")
    na, nb = ka.size, kb.size
    pos_b, _ = _lower_bound_match(ka, kb, tka, tkb)
    pos_a, match_b = _lower_bound_match(kb, ka, tkb, tka)
    inv = _Guarded(nb, torch.int64)
    tpos_b, tpos_a, tmatch_b = dev(pos_b), dev(pos_a), dev(match_b)
    _call("spamd_invert_flags", nb, _ptr(tmatch_b), inv.ptr(), _stream())
    assert np.array_equal(inv.check("inverted flags"), 1 - match_b)
    union = np.union1d(ka, kb)
    want_a, want_b = np.searchsorted(union, ka), np.searchsorted(union, kb)
    ub = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(1 - match_b, out=ub[1:])
    assert union.size == na + ub[nb]
    # union_positions on the references' inputs, every output inside sentinels
    gkeys, ga, gb = _Guarded(union.size, torch.int64), _Guarded(na, torch.int64), _Guarded(nb, torch.int64)
    tub = dev(ub)
    _call("spamd_union_positions", na, _ptr(tka), _ptr(tpos_b), nb, _ptr(tkb), _ptr(tpos_a), _ptr(tmatch_b), _ptr(tub), ga.ptr(), gb.ptr(),
          gkeys.ptr(), _stream())
    assert np.array_equal(gkeys.check("keys"), union)
    assert np.array_equal(ga.check("slotA"), want_a) and np.array_equal(gb.check("slotB"), want_b)
    # the wrapper
    keys, slot_a, slot_b = (host(t) for t in U.union_merge(tka, tkb))
    assert np.array_equal(keys, union)
    assert np.array_equal(keys[slot_a], ka) and np.array_equal(keys[slot_b], kb)
    assert np.array_equal(slot_a, want_a) and np.array_equal(slot_b, want_b)
    matched = match_b.astype(bool)
    assert np.array_equal(slot_b[matched], slot_a[pos_a[matched]])             # a matched B element shares its partner's slot


def _coo(sp, keys, values, size):
    return sp.COO(keys[None, :].copy(), values.copy(), shape=(size,), has_duplicates=False, sorted=True)


def test_three_operands_and_where_use_the_older_union_twice(U, abi):
    """x, y from the pair that straddles tile edge 1 (the older union has no tiles: these are simply keys that interleave and
    match), z and the condition from its neighbours"""
    import sparse_amd as sp

    ka, va, kb, vb = mc.case_operands("tile edge 1: straddle")
    kc, vc, kd, _ = mc.case_operands("tile edge 1: before")
    kc, vc = kc[::2], vc[::2]                                        # other keys than x: the second union adds positions
    size = int(max(ka[-1], kb[-1], kc[-1], kd[-1])) + 1

    def dense(k, v, fill=0):
        out = np.full(size, fill, dtype=v.dtype)
        out[k] = v
        return out

    x, y, z = _coo(sp, ka, va, size), _coo(sp, kb, vb, size), _coo(sp, kc, vc, size)
    dx, dy, dz = dense(ka, va), dense(kb, vb), dense(kc, vc)
    got = sp.elemwise(lambda a, b, c: a + b * c, x, y, z)
    assert abi.count("spamd_union_positions") == 2
    assert np.array_equal(got.todense(), dx + dy * dz)
    want = dx + dy * dz
    assert got.nnz == np.count_nonzero(want) and np.array_equal(host(got.linear_loc()), np.flatnonzero(want))
    del abi[:]
    cond = _coo(sp, kd, np.ones(kd.size, dtype=bool), size)
    got = sp.where(cond, x, y)
    assert abi.count("spamd_union_positions") == 2
    want = np.where(dense(kd, np.ones(kd.size, dtype=bool), False), dx, dy)
    assert np.array_equal(got.todense(), want) and got.nnz == np.count_nonzero(want)

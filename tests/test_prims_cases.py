"""tests/prims_cases.py on its own, without a GPU: every reference against a second, differently written formulation, the
case tables against the boundary values they exist for, and the constants the cases are built around against the source
text of the kernels (a constant that moves fails here, next to the name of the cases that have to move with it)."""
import os

import numpy as np
import pytest

import prims_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- the thresholds, from the source -----------------------------------------------------------------------------------
def test_thresholds_in_the_source_are_the_ones_the_cases_straddle():
    prims, common, kern = _src("sparse_amd", "csrc", "prims.hip"), _src("sparse_amd", "csrc", "common.h"), _src("sparse_amd", "_kernels.py")

    def has(text, needle, cases):
        assert needle in text, f"`{needle}` is gone from the source: move {cases} in tests/prims_cases.py with it"

    has(prims, "DN_THREADS = 256, DN_ITEMS = 8, DN_TILE = DN_THREADS * DN_ITEMS", "DN_TILE / DENSE_N")
    assert pc.DN_TILE == 256 * 8
    has(prims, "rocprim::default_config, 128 * 1024>", "MERGE_NARROW / SORT_N / CSX_LARGE")
    has(prims, "rocprim::default_config, 256 * 1024>", "MERGE_WIDE / SORT_N / CSX_LARGE")
    assert (pc.MERGE_NARROW, pc.MERGE_WIDE) == (128 * 1024, 256 * 1024)
    has(prims, "if (end_bit <= 24) return rocprim::radix_sort_pairs<SortNarrowKeys>", "NARROW_BITS / *_MAX_KEYS")
    has(prims, "if (bits <= 24) return rocprim::radix_sort_pairs<SortNarrowKeys>", "NARROW_BITS / CSX_BITS_STEP")
    has(prims, "while (bits < 32 && ((int64_t)1 << bits) < n_minor) ++bits;", "CSX_BITS_STEP")
    assert pc.NARROW_BITS == 24 and pc.CSX_BITS_STEP == 2 ** 24
    has(prims, "if (nnz >= 8 * R) {", "ROWS_FACTOR / CSR_CASES")
    assert pc.ROWS_FACTOR == 8
    has(prims, "if (nnz > 0 && R <= 8 * nnz) {", "FILL_FACTOR / ROWS_CASES")
    assert pc.FILL_FACTOR == 8
    has(prims, "const bool wide = last - first >= 32;", "WIDE_STRETCH / STRETCHES")
    has(prims, "const bool twide = tlast - tfirst >= 32;", "WIDE_STRETCH / STRETCHES")
    assert pc.WIDE_STRETCH == 32
    has(prims, "if (b > 256 * 16) b = 256 * 16;", "GRID_CAP / N1")
    has(prims, "ceil_div(n, (int64_t)256 * per_thread)", "GRID_CAP / N1")
    assert pc.GRID_CAP == 256 * 16 and pc.N1 == 1_048_576
    has(prims, "dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, keys, n, flags2)", "CHECK_POSITIONS (the stride stays N1: 4096 x 256)")
    has(common, "constexpr int SMALL_SCAN_MAX = 16384;", "SMALL_SCAN_MAX / SCAN_LENGTHS")
    has(prims, "if (n + 1 <= SMALL_SCAN_MAX) {", "SCAN_LENGTHS")
    assert pc.SMALL_SCAN_MAX == 16384
    has(prims, "cells < ((unsigned __int128)1 << 32) ? 1 : (cells < ((unsigned __int128)1 << 52) ? 2 : 0)", "K2C_SHAPES")
    has(prims, "if (n < 0 || rows < 0 || rows > 65535) return SPAMD_EINVAL;", "TOO_MANY_ROWS")
    has(kern, "if count * 4 < n * 3:", "the densities of test_dense_nonfill")
    has(kern, "return max(1, int(max_key).bit_length())", "key_bits")


# ---- the references, a second way ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_key", [0, 1, 2, 3, 255, 256, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 40 + 3, 2 ** 62, 2 ** 63 - 1])
def test_key_bits(max_key):
    bits = pc.key_bits(max_key)
    assert bits == max(1, len(bin(max_key)) - 2)
    assert max_key < 2 ** bits and (bits == 1 or max_key >= 2 ** (bits - 1))
    if max_key >= 2 and max_key & (max_key - 1) == 0:
        assert bits == pc.key_bits(max_key - 1) + 1       # a power of two needs one more bit than its predecessor


def test_sort_reference_is_the_stable_order():
    keys = pc.sort_keys_case(5000, 37)
    sk, perm = pc.ref_sort(keys)
    want = sorted(range(keys.size), key=lambda i: (int(keys[i]), i))      # ties in their original order
    assert perm.tolist() == want and np.array_equal(sk, keys[want])
    assert np.array_equal(np.lexsort((np.arange(keys.size), keys)), perm)


def test_scan_reference():
    for length in (1, 2, 5, 1025):
        v = pc.scan_case(length)
        out, acc = pc.ref_scan(v), 0
        for i in range(length):
            assert int(out[i]) == acc
            acc += int(v[i])
        assert v[-1] == pc.SCAN_SENTINEL and int(out[-1]) < pc.SCAN_SENTINEL
    big = pc.scan_case(17408, big=True)
    assert int(pc.ref_scan(big)[-1]) == sum(big[:-1].tolist()) > 2 ** 53     # (Python integers: no wrap, no double)


@pytest.mark.parametrize("name", list(pc.ROWS_CASES))
def test_rows_reference_against_bincount(name):
    rows, R = pc.ROWS_CASES[name]
    want = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.clip(rows, 0, R), minlength=R + 1)[:R], out=want[1:])
    got = pc.ref_rows_to_indptr(rows, R)
    assert np.array_equal(got, want) and got.dtype == np.int64
    if rows.size <= 2000:
        assert got.tolist() == [sum(1 for r in rows.tolist() if min(max(r, 0), R) < i) for i in range(R + 1)]
    assert np.all(np.diff(rows) >= 0)
    # int32 ids are the same ids
    assert np.array_equal(pc.ref_rows_to_indptr(np.clip(rows, 0, 2 ** 31 - 1).astype(np.int32), R), got)


def test_csr_to_keys_reference_against_a_loop():
    for (R, nnz, C) in pc.CSR_CASES:
        for idt in (np.int32, np.int64):
            indptr, indices = pc.csr_case(R, nnz, C, idt)
            assert indptr.dtype == idt and indices.dtype == idt and indices.size == nnz == int(indptr[-1])
            want = [r * C + int(indices[e]) for r in range(R) for e in range(int(indptr[r]), int(indptr[r + 1]))]
            assert pc.ref_csr_to_keys(indptr, indices, C).tolist() == want


@pytest.mark.parametrize("shape", pc.K2C_SHAPES, ids=str)
def test_keys_to_csr_reference_against_python_integers(shape):
    R, C = shape
    keys = pc.k2c_keys(R, C)
    indptr, indices = pc.ref_keys_to_csr(keys, R, C)
    assert indptr.size == R + 1 and indices.size == keys.size and np.all(np.diff(keys) > 0)
    lst = keys.tolist()
    assert indices.tolist() == [k % C for k in lst]
    rows = [k // C for k in lst]
    probe = sorted(set([0, 1, 2, R // 2, R - 1, R] + rows[:50] + rows[-50:] + [r + 1 for r in rows[:50]]))
    for r in (p for p in probe if 0 <= p <= R):
        assert int(indptr[r]) == sum(1 for q in rows if q < r) if len(rows) < 200 else int(indptr[r]) == int(np.searchsorted(np.array(rows, dtype=object), r))
    if keys.size:     # the round trip through the other reference
        idx_rows = np.repeat(np.arange(R), np.diff(indptr))
        assert [int(a) * C + int(b) for a, b in zip(idx_rows[:100], indices[:100])] == lst[:100]
        assert int(indptr[0]) == 0 and int(indptr[-1]) == keys.size


def test_csx_swap_reference_against_a_dense_transpose():
    for (n_major, n_minor, nnz, mode) in [c for c in pc.CSX_SMALL if c[1] <= 300] + [(12, 1000, 700, "gaps")]:
        indices, indptr = pc.csx_case(n_major, n_minor, nnz, mode)
        data = np.arange(1, nnz + 1, dtype=np.float64)
        dense = np.zeros((n_major, n_minor))
        major = np.repeat(np.arange(n_major), np.diff(indptr))
        dense[major, indices] = data
        nd, ni, nptr = pc.ref_csx_swap(data, indices, indptr, n_minor)
        t = dense.T
        r, c = np.nonzero(t)                    # row-major over the transpose: (minor, major) order
        assert np.array_equal(ni, c) and np.array_equal(nd, t[r, c])
        assert np.array_equal(nptr, np.searchsorted(r, np.arange(n_minor + 1)))


def test_dense_nonfill_reference():
    sp = pc.float_specials("float32")
    bits = np.array([sp[k] for k in ("+0", "-0", "+nan", "-nan", "1", "+0", "denormal")], dtype=np.uint32)
    keys, vals = pc.ref_dense_nonfill(bits, 0)
    assert keys.tolist() == [1, 2, 3, 4, 6] and np.array_equal(vals, bits[[1, 2, 3, 4, 6]])
    keys, _ = pc.ref_dense_nonfill(bits, 0, float_numeric=True)           # both zeros go, NaNs of both signs stay
    as_float = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        assert keys.tolist() == np.flatnonzero(as_float != 0).tolist() == [2, 3, 4, 6]
    keys, _ = pc.ref_dense_nonfill(bits, sp["+nan"])                      # a NaN fill: only its own bit pattern is fill
    assert keys.tolist() == [0, 1, 3, 4, 5, 6]
    for name in pc.DENSE_TYPES:
        got = pc.float_specials(name) if pc.DENSE_TYPES[name][1] == "f" else None
        if got and name != "bfloat16":
            f = np.array(list(got.values()), dtype=f"u{pc.DENSE_TYPES[name][0]}").view(name)
            assert f[0] == 0 and f[1] == 0 and np.signbit(f[1]) and np.isnan(f[2:5]).all() and f[5] == 1 and f[6] == -1 and 0 < f[7] < np.finfo(name).tiny
    b = np.array(list(pc.float_specials("bfloat16").values()), dtype=np.uint32) << 16       # bfloat16: the top half of a float32
    f = b.view(np.float32)
    assert f[0] == 0 and np.signbit(f[1]) and np.isnan(f[2:5]).all() and f[5] == 1 and f[6] == -1 and 0 < f[7] < np.finfo(np.float32).tiny


def test_flag_references():
    keys = np.array([3, 3, 4, 9, 9, 9, 10])
    assert pc.ref_flag_heads(keys).tolist() == [1, 0, 1, 1, 0, 0, 1]
    assert pc.ref_flag_heads(keys[:1]).tolist() == [1] and pc.ref_flag_heads(keys[:0]).size == 0
    z = np.array([1 + 2j, 0j, complex(0.0, -0.0)], dtype=np.complex128)
    assert pc.ref_flag_ne_bits(pc.bits_of(z), pc.bits_of(np.zeros(1, np.complex128))[0]).tolist() == [1, 0, 1]
    f = np.array([0.0, -0.0, np.nan], dtype=np.float32)
    assert pc.ref_flag_ne_bits(pc.bits_of(f), pc.bits_of(np.float32([0.0]))[0]).tolist() == [0, 1, 1]


def test_linearize_reference_against_strides():
    for ndim, shape in pc.LINEARIZE_SHAPES.items():
        coords = pc.coords_case(shape, 200, np.int64)
        assert (coords[:, 0] == 0).all() and (coords[:, -1] == np.array(shape) - 1).all()
        orders = pc.axis_orders(ndim)
        assert len(set(orders)) == len(orders) and tuple(reversed(range(ndim))) in orders and tuple(range(ndim)) in orders
        assert len(orders) == (ndim + 1 if ndim > 2 else ndim)
        for order in orders:
            want = []
            for p in range(coords.shape[1]):
                k = 0
                for a in order:
                    k = k * shape[a] + int(coords[a, p])
                want.append(k)
            assert pc.ref_linearize(coords, shape, order).tolist() == want


# ---- the tables hold what they are for -------------------------------------------------------------------------------
def test_sort_cases_hold_every_size_and_width():
    assert set(pc.SORT_N) == {1, 2, 255, 131071, 131072, 131073, 262143, 262144, 262145}
    assert set(pc.NARROW_MAX_KEYS) | set(pc.WIDE_MAX_KEYS) == {0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 31, 2 ** 40 + 3, 2 ** 62}
    assert {m for _, m in pc.SORT_CASES} == set(pc.NARROW_MAX_KEYS) | set(pc.WIDE_MAX_KEYS)
    for n in pc.SORT_N:
        widths = sorted(pc.key_bits(m) for (k, m) in pc.SORT_CASES if k == n)
        assert len(widths) == 2 and widths[0] <= 24 < widths[1]
    for n in (131071, 131072, 131073):
        assert (n, 2 ** 24 - 1) in pc.SORT_CASES          # 24 bits: the last width of the 128 K configuration
    for n in (262143, 262144, 262145):
        assert (n, 2 ** 24) in pc.SORT_CASES              # 25 bits: the first width of the 256 K configuration
    for n, max_key in pc.SORT_CASES:
        keys = pc.sort_keys_case(n, max_key)
        assert keys.size == n and keys.min() >= 0 and keys.max() <= max_key
        if n >= 2:
            assert keys.min() == 0 and keys.max() == max_key
        if n >= 255:
            assert n / 32 <= np.unique(keys).size <= n / 16 + 2 or max_key < n / 16
    for nbytes, nans in ((4, pc.NAN32), (8, pc.NAN64)):
        bits = pc.payload_bits(1000, nbytes)
        f = bits.view(np.float32 if nbytes == 4 else np.float64)
        assert np.isnan(f[::8]).all() and set(bits[::8].tolist()) == set(nans) and len({b >> (8 * nbytes - 1) for b in nans}) == 2


def test_scan_cases():
    assert set(pc.SCAN_LENGTHS) == {1, 2, 1023, 1024, 1025, 16383, 16384, 16385, 17408}
    v = pc.scan_case(1025)
    assert set(v[:-1].tolist()) == {0, 1, 2, 3} and v[-1] == pc.SCAN_SENTINEL
    assert pc.scan_case(1025, big=True)[:-1].min() >= 2 ** 40 - 2


def test_rows_cases_hold_every_stretch_at_every_place():
    assert set(pc.STRETCHES) == {0, 1, 31, 32, 33, 63, 64, 65, 200}
    for g in pc.STRETCHES:
        rows, R = pc.ROWS_CASES[f"stretch {g}"]
        assert pc.takes_fill(rows.size, R)
        for e in (0,) + pc.STRETCH_POSITIONS + (rows.size,):
            assert pc.stretch_of(rows, R, e) == g, (g, e)
    assert {e % 64 for e in pc.STRETCH_POSITIONS} >= {0, 63} and any(e % 256 == 0 for e in pc.STRETCH_POSITIONS)
    rows, R = pc.ROWS_CASES["every stretch, lanes 0 and 63"]
    assert pc.takes_fill(rows.size, R)
    for lane in (0, 63):
        assert {pc.stretch_of(rows, R, e) for e in range(rows.size) if e % 64 == lane and e >= 64} >= set(pc.STRETCHES)
    rows, R = pc.ROWS_CASES["second trip"]
    assert rows.size > pc.N1 + 256 and pc.takes_fill(rows.size, R)
    assert [pc.stretch_of(rows, R, e) for e in (pc.N1, pc.N1 + 63, pc.N1 + 256, rows.size)] == [200, 32, 33, 65]
    rows, R = pc.ROWS_CASES["long runs"]
    assert pc.takes_fill(rows.size, R) and np.bincount(rows).max() >= 2000
    for name in ("hypersparse", "one element, hypersparse", "R = 8 nnz + 1", "ids beyond R", "no elements, R = 0", "no elements, R = 5"):
        rows, R = pc.ROWS_CASES[name]
        assert not pc.takes_fill(rows.size, R), name
    for name in ("one element", "R = 8 nnz", "ids beyond R, fill"):
        rows, R = pc.ROWS_CASES[name]
        assert pc.takes_fill(rows.size, R), name
    (a, Ra), (b, Rb) = pc.ROWS_CASES["R = 8 nnz"], pc.ROWS_CASES["R = 8 nnz + 1"]
    assert a is b and Ra == 8 * a.size and Rb == Ra + 1 and a.max() < Ra
    assert pc.stretch_of(a, Ra, a.size) >= 32          # (the rows behind the last element: the wave-wide tail)
    for name in ("ids beyond R", "ids beyond R, fill"):
        rows, R = pc.ROWS_CASES[name]
        assert rows.max() > R


def test_keys_to_csr_shapes_sit_on_both_sides_of_both_class_edges():
    cls = {s: pc.k2c_class(*s) for s in pc.K2C_SHAPES}
    assert 65537 * 65535 == 2 ** 32 - 1 and cls[(65537, 65535)] == 1 and cls[(65536, 65536)] == 2
    assert cls[(4, 2 ** 50 - 1)] == 2 and cls[(4, 2 ** 50)] == 0
    for s in ((1, 1), (7, 1), (1, 7), (2 ** 20, 4095), (2 ** 20, 2 ** 31 + 11), (1000, 2 ** 53 + 1), (0, 5), (5, 0)):
        assert s in cls
    assert cls[(2 ** 20, 4095)] == 1 and cls[(2 ** 20, 2 ** 31 + 11)] == 2 and cls[(1000, 2 ** 53 + 1)] == 0
    assert max(R for R, _ in pc.K2C_SHAPES) <= 2 ** 20
    # both reciprocal-division classes meet keys that are only right after the `++q` repair
    assert {pc.k2c_class(*s) for s in pc.K2C_REPAIR_SHAPES} == {1, 2}
    for R, C in pc.K2C_REPAIR_SHAPES:
        assert pc.needs_repair(pc.k2c_keys(R, C), C) >= 100, (R, C)
    assert pc.needs_repair(np.arange(0, 49 * 50, 49, dtype=np.int64), 49) > 0 == pc.needs_repair(np.arange(0, 48 * 50, 48, dtype=np.int64), 48)
    for R, C in pc.K2C_SHAPES:
        keys, cells = pc.k2c_keys(R, C), R * C
        if cells == 0:
            assert keys.size == 0
            continue
        have = set(keys.tolist())
        assert {0, cells - 1} <= have and cells < 2 ** 63
        for m in (1, R - 1):
            assert {k for k in (m * C - 1, m * C, m * C + 1) if 0 <= k < cells} <= have
        if cells > 10 ** 6:
            assert keys.size > 4900


def test_csr_cases_sit_on_both_sides_of_the_dispatch():
    assert {(nnz - pc.ROWS_FACTOR * R) for R, nnz, _ in pc.CSR_CASES} == {-1, 0} and 2 ** 40 in {C for _, _, C in pc.CSR_CASES}
    for R, nnz, C in pc.CSR_CASES:
        indptr, indices = pc.csr_case(R, nnz, C, np.int64)
        lengths = np.diff(indptr)
        assert set(pc.ROW_LENGTHS) <= set(lengths.tolist()) and lengths[0] == 0 and lengths[1] == 0 and lengths[-1] == 0 and lengths[-2] == 0
        assert indices.max() == C - 1 and indices.min() == 0


def test_csx_cases():
    minors = {c[1] for c in pc.CSX_SMALL + pc.CSX_LARGE}
    assert {1, 2, 255, 256, 257, 2 ** 24, 2 ** 24 + 1} <= minors
    assert {c[2] for c in pc.CSX_SMALL} >= {1, 70}
    assert {c[2] for c in pc.CSX_LARGE if c[1] == 2 ** 24} >= {1, 70, 131071, 131072, 131073}
    assert {c[2] for c in pc.CSX_LARGE if c[1] == 2 ** 24 + 1} >= {1, 70, 262143, 262144, 262145}
    assert {c[2] for c in pc.CSX_LARGE if c[1] < 2 ** 24} >= {131071, 131072, 131073}
    for cases in (pc.CSX_SMALL, pc.CSX_LARGE):
        assert {c[0] == 1 for c in cases} == {True, False} and {c[3] for c in cases} == {"ends", "gaps"}
    for (n_major, n_minor, nnz, mode) in pc.CSX_SMALL + tuple(c for c in pc.CSX_LARGE if c[2] <= 131072):
        indices, indptr = pc.csx_case(n_major, n_minor, nnz, mode)
        assert indices.size == nnz == indptr[-1] and indptr.size == n_major + 1 and indices.min() >= 0 and indices.max() < n_minor
        major = np.repeat(np.arange(n_major), np.diff(indptr))
        assert np.all(np.diff(major * n_minor + indices) > 0)            # ordered by (major, minor), no duplicates
        if mode == "gaps":
            h = n_minor // 2
            assert indices.min() >= 100 and indices.max() < n_minor - 100 and not np.any((indices >= h - 60) & (indices < h + 60))
        elif nnz >= 2:
            assert indices[0] == 0 and indices[-1] == n_minor - 1      # the last index needs the key's top bit
        if nnz >= 1000:
            assert np.diff(indptr).max() > 64


def test_dense_cases():
    assert set(pc.DENSE_N) == {1, 2047, 2048, 2049, 2048 * 257 + 5, pc.N1 + 257}
    assert set(pc.DENSE_TYPES) == {"float16", "bfloat16", "float32", "float64", "int8", "int64", "bool"}
    for name, (nbytes, kind) in pc.DENSE_TYPES.items():
        sp = pc.float_specials(name) if kind == "f" else None
        for fill in ((0, 1) if kind == "b" else (0, 0x3c if nbytes == 1 else 0x3c01)):
            for density in (0.0, 0.1, 0.9, 1.0):
                bits = pc.dense_case(name, 4099, fill, density)
                assert bits.dtype.itemsize == nbytes and bits.size == 4099
                count = int((bits != fill).sum())
                if density == 0.0:
                    assert count == 0
                elif density == 1.0:
                    assert count == bits.size
                else:
                    assert (count * 4 < bits.size * 3) == (density < 0.75) and count > 0     # either side of the clone / view choice
                if sp and density >= 0.9:
                    have = set(bits.tolist())
                    assert {sp["-0"], sp["+nan"], sp["-nan"], sp["nan2"]} <= have
                    assert sp["+0"] in have or (fill == 0 and density == 1.0)     # (+0 is the fill value itself or one of the others)


def test_the_remaining_tables():
    assert set(pc.MOVE_N) == {1, 256, 257, pc.N1 + 257} and set(pc.MOVE_ROWS) == {1, 3, 16} and set(pc.ELEM_BYTES) == {1, 2, 4, 8, 16}
    assert pc.TOO_MANY_ROWS == 65536
    assert pc.CHECK_N == 4_200_000 and set(pc.CHECK_POSITIONS) == {1, 63, 64, 255, 256, 257, 1023, 1024, 1025, pc.N1 - 1, pc.N1, pc.N1 + 1, pc.CHECK_N - 1}
    assert set(pc.COORD_NDIMS) == {1, 3, 16} and set(pc.LINEARIZE_SHAPES) == {1, 2, 5, 16}
    assert all(len(s) == n for n, s in pc.LINEARIZE_SHAPES.items())
    assert pc.LINEARIZE_INT32_SHAPE == (70000, 70000) and 70000 * 70000 > 2 ** 31 and 70000 < 2 ** 31
    assert set(pc.CONVERT_TYPES) == {"float32", "float64", "int32", "int64", "bool"} and set(pc.CONVERT_N) == {257, pc.N1 + 257}
    for src in pc.CONVERT_TYPES:
        v = pc.convert_values(src, 5000)
        assert v.dtype == np.dtype(src)
        for dst in pc.CONVERT_TYPES:       # in range: the conversion back returns the value (bool: its truth)
            w = v.astype(dst)
            if dst == "bool" or src == "bool":
                assert np.array_equal(w.astype(bool), v.astype(bool))
            elif dst.startswith("int") and src.startswith("float"):
                assert np.array_equal(w, np.trunc(v).astype(dst))
            else:
                assert np.array_equal(w.astype(src), v)
        if src.startswith("float"):
            assert np.signbit(v[v == 0]).any() and (v != np.trunc(v)).any()

"""Cases for the key and index primitives (csrc/prims.hip behind the `_kernels` wrappers): plain NumPy references of every
operation and the case tables, each built around a place where the code takes another path.  No GPU, no torch, no
package import.  Everything is integers and bit patterns: every comparison against these references is exact.

The switches the cases straddle (tests/test_prims_cases.py reads each from the source text, so a constant that moves
fails there and names the cases to move with it):

  GRID_CAP * 256 = N1   `grid_for` launches at most 4096 workgroups of 256: a grid-stride loop takes a second trip from
                        element 1,048,576 on
  MERGE_NARROW/_WIDE    rocPRIM's merge sort below 128 K pairs for keys of at most NARROW_BITS = 24 bits, below 256 K above
  FILL_FACTOR           rows_to_indptr: the element-side fill kernel while R <= 8 nnz, R + 1 binary searches above
  WIDE_STRETCH          ... whose wave fills an empty stretch cooperatively when `last - first >= 32`
  ROWS_FACTOR           csr_to_keys: a wave per row from nnz >= 8 R on, a search per element below
  DN_TILE               dense_nonfill: 256 threads x 8 elements per workgroup
  2^32 / 2^52 cells     keys_to_csr: 32-bit and 64-bit reciprocal division, the generic modulo above
"""
import bisect

import numpy as np

GRID_CAP = 4096
N1 = GRID_CAP * 256
MERGE_NARROW, MERGE_WIDE, NARROW_BITS = 128 * 1024, 256 * 1024, 24
FILL_FACTOR, WIDE_STRETCH = 8, 32
ROWS_FACTOR = 8
DN_TILE = 256 * 8
SMALL_SCAN_MAX = 16384


# ---- references ----------------------------------------------------------------------------------------------------
def key_bits(max_key):
    """bits a radix sort must look at for keys in [0, max_key] (at least one)"""
    bits = 1
    while (1 << bits) <= int(max_key):
        bits += 1
    return bits


def ref_sort(keys):
    perm = np.argsort(keys, kind="stable")
    return keys[perm], perm.astype(np.int64)


def ref_scan(values):
    """values[n + 1] -> out[n + 1], out[i] = values[0] + ... + values[i - 1]: the last entry never enters"""
    out = np.zeros(values.size, dtype=np.int64)
    np.cumsum(values[:-1], out=out[1:])
    return out


def ref_rows_to_indptr(rows, R):
    return np.searchsorted(np.clip(rows.astype(np.int64), 0, R), np.arange(R + 1), "left").astype(np.int64)


def ref_csr_to_keys(indptr, indices, C):
    R = indptr.size - 1
    return np.repeat(np.arange(R, dtype=np.int64), np.diff(indptr.astype(np.int64))) * np.int64(C) + indices.astype(np.int64)


def ref_keys_to_csr(keys, R, C):
    """(indptr[R + 1], indices[nnz]) as int64; Python integers where the row starts do not fit int64"""
    if keys.size == 0:
        return np.zeros(R + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if (R + 1) * C < 2 ** 63:
        indptr = np.searchsorted(keys, np.arange(R + 1, dtype=np.int64) * np.int64(C), "left")
    else:
        lst = keys.tolist()
        indptr = np.array([bisect.bisect_left(lst, r * C) for r in range(R + 1)])
    return indptr.astype(np.int64), keys % np.int64(C)


def k2c_class(R, C):
    """division class of keys_to_csr: 1 below 2^32 cells, 2 below 2^52, 0 (generic modulo) above"""
    cells = max(R, 1) * max(C, 1)
    return 1 if cells < 2 ** 32 else (2 if cells < 2 ** 52 else 0)


def ref_csx_swap(data, indices, indptr, n_minor):
    n_major = indptr.size - 1
    major = np.repeat(np.arange(n_major, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    perm = np.argsort(indices, kind="stable")
    new_indptr = np.zeros(n_minor + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices.astype(np.int64), minlength=n_minor), out=new_indptr[1:])
    return data[perm], major[perm], new_indptr


def bits_of(a):
    """the unsigned bit view of a value array (bool and complex included)"""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 16:
        return a.view(np.uint64).reshape(-1, 2)
    return a.view(f"u{a.dtype.itemsize}")


def ref_dense_nonfill(bits, fill_bits, float_numeric=False):
    """bits: unsigned patterns; the elements that differ from `fill_bits` (with float_numeric: apart from the sign bit)"""
    mask = bits.dtype.type((1 << (8 * bits.dtype.itemsize - (1 if float_numeric else 0))) - 1)
    keys = np.flatnonzero((bits ^ bits.dtype.type(fill_bits)) & mask)
    return keys.astype(np.int64), bits[keys]


def ref_flag_heads(keys):
    return np.concatenate([[1], (keys[1:] != keys[:-1]).astype(np.int64)]) if keys.size else np.zeros(0, dtype=np.int64)


def ref_flag_ne_bits(bits, fill):
    """bits: [n] unsigned words or [n, 2] for 16-byte elements; fill: one element of the same form"""
    ne = bits != fill
    return (ne.any(axis=1) if bits.ndim == 2 else ne).astype(np.int64)


def ref_linearize(coords, shape, order):
    return np.ravel_multi_index(tuple(coords[a].astype(np.int64) for a in order), tuple(int(shape[a]) for a in order)).astype(np.int64)


# ---- a. sorts ------------------------------------------------------------------------------------------------------
SORT_N = (1, 2, 255, MERGE_NARROW - 1, MERGE_NARROW, MERGE_NARROW + 1, MERGE_WIDE - 1, MERGE_WIDE, MERGE_WIDE + 1)
NARROW_MAX_KEYS = (0, 1, 2 ** NARROW_BITS - 1)
WIDE_MAX_KEYS = (2 ** NARROW_BITS, 2 ** 31, 2 ** 40 + 3, 2 ** 62)


def _sort_cases():
    """every n with one key width on each side of 24 bits; the sizes around a merge/radix switch get the widths next to
    the switch of the configuration (2^24 - 1: the last narrow one; 2^24: a power of two, one bit more than 2^24 - 1)"""
    out = []
    for i, n in enumerate(SORT_N):
        narrow = 2 ** NARROW_BITS - 1 if abs(n - MERGE_NARROW) <= 1 else NARROW_MAX_KEYS[i % 3]
        wide = 2 ** NARROW_BITS if abs(n - MERGE_WIDE) <= 1 else WIDE_MAX_KEYS[i % 4]
        out += [(n, narrow), (n, wide)]
    return out


SORT_CASES = _sort_cases()


def sort_keys_case(n, max_key, seed=0):
    """n keys from a pool of about n / 16 distinct values that always holds 0 and max_key (both drawn when n >= 2)"""
    rng = np.random.default_rng([seed, n, max_key % (2 ** 31)])
    pool = np.unique(np.concatenate([rng.integers(0, max_key + 1, size=max(n // 16, 1), dtype=np.int64),
                                     np.array([0, max_key], dtype=np.int64)]))
    keys = rng.choice(pool, size=n)
    if n >= 2:
        a, b = rng.choice(n, size=2, replace=False)
        keys[a], keys[b] = 0, max_key
    return keys.astype(np.int64)


NAN32 = (0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc12345)
NAN64 = (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xffffffffffffffff, 0x7ff8000000abcdef)


def payload_bits(n, nbytes, seed=0):
    """n random words of 4 or 8 bytes, every eighth one of the NaN patterns above (a payload moves bit-wise)"""
    rng = np.random.default_rng([seed, n, nbytes])
    dt = np.uint32 if nbytes == 4 else np.uint64
    bits = rng.integers(0, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)
    nans = np.array(NAN32 if nbytes == 4 else NAN64, dtype=dt)
    bits[::8] = nans[np.arange(bits[::8].size) % nans.size]
    return bits


# ---- b. scan -------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = (1, 2, 1023, 1024, 1025, SMALL_SCAN_MAX - 1, SMALL_SCAN_MAX, SMALL_SCAN_MAX + 1, 17408)   # n + 1
SCAN_SENTINEL = 2 ** 61 + 12345


def scan_case(length, big=False, seed=0):
    """length = n + 1 values: 0..3 (or near 2^40), the last one a large sentinel that must not enter the result"""
    rng = np.random.default_rng([seed, length, int(big)])
    v = rng.integers(0, 4, size=length, dtype=np.int64)
    if big:
        v += 2 ** 40 - 2
    v[-1] = SCAN_SENTINEL
    return v


# ---- c. rows_to_indptr -----------------------------------------------------------------------------------------------
STRETCHES = (0, 1, 31, 32, 33, 63, 64, 65, 200)


def takes_fill(nnz, R):
    return nnz > 0 and R <= FILL_FACTOR * nnz


def rows_with_stretches(nnz, gaps, tail, seed=0, runs=True):
    """Sorted row ids of nnz elements and R.  `gaps`: {element index e: g}: exactly g empty rows lie between element
    e - 1's row and element e's (e = 0: before the first element); `tail` empty rows follow the last element.  Every other
    element stays in its predecessor's row or opens the next one (`runs`: at random; otherwise always the next one)."""
    rng = np.random.default_rng([seed, nnz, tail])
    inc = rng.integers(0, 2, size=nnz, dtype=np.int64) if runs else np.ones(nnz, dtype=np.int64)
    inc[0] = 0
    for e, g in gaps.items():
        assert 0 <= e < nnz
        inc[e] = g + (1 if e else 0)
    rows = np.cumsum(inc)
    return rows, int(rows[-1]) + 1 + tail


def stretch_of(rows, R, e):
    """empty rows in front of element e's row (e = len(rows): after the last element)"""
    if e == len(rows):
        return R - 1 - int(rows[-1])
    return int(rows[e]) - (int(rows[e - 1]) + 1 if e else 0)


# element positions that open a stretch: lane 0 and lane 63 of a wave, 256 k (the first element of a workgroup), others
STRETCH_POSITIONS = (64, 127, 300, 512)


def _rows_cases():
    cases = {}
    for g in STRETCHES:      # the same stretch in front, between elements (at every position above) and behind
        gaps = {0: g}
        gaps.update({e: g for e in STRETCH_POSITIONS})
        cases[f"stretch {g}"] = rows_with_stretches(1000, gaps, g, seed=g)
    # all lengths at once, each at lane 0 and at lane 63 of some wave
    gaps = {}
    for i, g in enumerate(STRETCHES):
        gaps[64 * (2 * i + 1)] = g
        gaps[64 * (2 * i + 2) + 63] = g
    cases["every stretch, lanes 0 and 63"] = rows_with_stretches(64 * 20, gaps, 33, seed=1)
    # the second trip of the fill kernel's grid-stride loop: stretches opened by elements N1 (lane 0), N1 + 63, N1 + 256
    cases["second trip"] = rows_with_stretches(N1 + 300, {N1: 200, N1 + 63: 32, N1 + 256: 33, 5: 64}, 65, seed=2)
    # long runs of one row (a stretch in front of each)
    lengths = [1000, 1, 300, 64, 65, 2000]
    rows = np.repeat(np.cumsum([3, 1, 40, 32, 33, 1]), lengths)
    cases["long runs"] = (rows.astype(np.int64), int(rows[-1]) + 1)
    # hypersparse: the binary-search kernel (R > 8 nnz)
    cases["hypersparse"] = rows_with_stretches(100, {0: 5000, 10: 1, 50: 70000, 64: 31}, 3000, seed=3)
    one = rows_with_stretches(1, {0: 7}, 0)
    cases["one element"] = one
    cases["one element, hypersparse"] = (one[0], 40)
    # either side of the dispatch on the same ids
    rows, _ = rows_with_stretches(100, {0: 33, 30: 200, 64: 32, 99: 100}, 0, seed=4)
    assert rows[-1] < 8 * 100 - 40
    cases["R = 8 nnz"] = (rows, 800)
    cases["R = 8 nnz + 1"] = (rows, 801)
    # ids beyond R are clamped (a trusting constructor lets them through): both kernels
    cases["ids beyond R"] = (np.array([0, 0, 5, 999, 1500, 4000], dtype=np.int64), 1000)
    cases["ids beyond R, fill"] = (np.concatenate([np.arange(0, 400, 2), [450, 900, 4000]]).astype(np.int64), 500)
    cases["no elements, R = 0"] = (np.zeros(0, dtype=np.int64), 0)
    cases["no elements, R = 5"] = (np.zeros(0, dtype=np.int64), 5)
    return cases


ROWS_CASES = _rows_cases()


# ---- d. keys_to_csr --------------------------------------------------------------------------------------------------
K2C_SHAPES = ((65537, 65535), (65536, 65536),                   # 2^32 - 1 cells | 2^32 cells
              (4, 2 ** 50 - 1), (4, 2 ** 50),                    # below 2^52 cells | 2^52 cells
              (1, 1), (7, 1), (1, 7), (2 ** 20, 4095), (2 ** 20, 2 ** 31 + 11), (1000, 2 ** 53 + 1),
              (0, 5), (5, 0), (0, 0)) + tuple((2 ** 20, C) for C in (49, 4090, 49 * 2 ** 7, 65530, 49 * 2 ** 26))
# (the last five: row lengths C for which the truncated product k * (1 / C) falls short of the quotient at about half of all
# multiples of C, so the reciprocal division's `++q` repair is what makes the column right - few C do that: none of the others)
K2C_REPAIR_SHAPES = K2C_SHAPES[-5:]


def needs_repair(keys, C):
    """how many keys the reciprocal division (csrc/div_recip.h) gets wrong before its repair: floor(double(k) * (1.0 / C)) != k // C"""
    inv = 1.0 / np.float64(C)
    return int((np.floor(keys.astype(np.float64) * inv).astype(np.int64) != keys // np.int64(C)).sum())


def k2c_keys(R, C, seed=0):
    """a sorted unique sample of the keys of an R x C matrix: 0, cells - 1, m C + {-1, 0, 1} (m: the first and the last rows,
    the middle one and 1000 random ones) and 5000 random keys"""
    cells = R * C
    if cells == 0:
        return np.zeros(0, dtype=np.int64)
    rng = np.random.default_rng([seed, R % (2 ** 31), C % (2 ** 31)])
    special = [0, cells - 1]
    for m in [1, 2, 3, R // 2, R - 2, R - 1, R] + rng.integers(0, R, size=1000).tolist():
        special += [m * C + o for o in (-1, 0, 1)]
    special = [k for k in special if 0 <= k < cells]
    keys = np.concatenate([np.array(special, dtype=np.int64), rng.integers(0, cells, size=5000, dtype=np.int64)])
    return np.unique(keys)


# ---- e. csr_to_keys --------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)


def csr_case(R, nnz, C, idx_dtype, seed=0):
    """(indptr, indices) of R rows and nnz elements: empty rows in front and behind, rows of every length above, and one
    row that takes what is left"""
    rng = np.random.default_rng([seed, R, nnz])
    pattern = list(ROW_LENGTHS) * 3
    rest = nnz - sum(pattern)
    lead = (R - len(pattern) - 1) // 2
    assert rest > 64 and lead >= 2
    lengths = [0] * lead + pattern + [rest] + [0] * (R - lead - len(pattern) - 1)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(idx_dtype)
    top = min(C, np.iinfo(idx_dtype).max + 1)
    indices = rng.integers(0, top, size=nnz, dtype=np.int64)
    indices[0], indices[-1] = top - 1, 0
    return indptr, indices.astype(idx_dtype)


CSR_CASES = tuple((R, nnz, C) for R in (400,) for nnz in (ROWS_FACTOR * R - 1, ROWS_FACTOR * R) for C in (2 ** 40, 1000))


# ---- f. csx_swap_2d --------------------------------------------------------------------------------------------------
def _minor_values(n_minor, mode):
    """(count, map from 0..count-1 to a minor index): everything, or everything but >= 100 indices at the front, in the
    middle and at the end"""
    if mode == "ends":
        return n_minor, lambda j: j
    assert n_minor >= 1000
    h = n_minor // 2
    lo_count = h - 60 - 100                      # [100, h - 60)
    hi_count = n_minor - 100 - (h + 60)          # [h + 60, n_minor - 100)
    return lo_count + hi_count, lambda j: np.where(j < lo_count, j + 100, j - lo_count + h + 60)


def csx_case(n_major, n_minor, nnz, mode="ends", seed=0):
    """(indices, indptr) int64 of a compressed matrix ordered by (major, minor), minor indices ascending inside a major
    slice.  mode "ends": the first and the last minor index are stored (with n_major, n_minor > 1 in the first and the last
    slice); mode "gaps": no minor index below 100, within 60 of the middle, or in the last 100."""
    rng = np.random.default_rng([seed, n_major, n_minor % (2 ** 31), nnz])
    count, to_minor = _minor_values(n_minor, mode)
    cells = n_major * count
    assert nnz <= cells
    if cells <= 4 * nnz or cells <= 2 ** 22:
        ids = rng.choice(cells, size=nnz, replace=False).astype(np.int64)
    else:
        ids = np.unique(rng.integers(0, cells, size=nnz + nnz // 2 + 64, dtype=np.int64))
        ids = ids[rng.permutation(ids.size)[:nnz]]
        assert ids.size == nnz
    if mode == "ends" and nnz >= 2:
        ids = ids[(ids != 0) & (ids != cells - 1)]
        ids = np.concatenate([ids[:nnz - 2], [0, cells - 1]])
    ids = np.sort(ids)
    assert ids.size == nnz and np.all(np.diff(ids) > 0)
    major, minor = ids // count, to_minor(ids % count)
    indptr = np.searchsorted(major, np.arange(n_major + 1), "left").astype(np.int64)
    return minor.astype(np.int64), indptr


CSX_BITS_STEP = 2 ** NARROW_BITS      # n_minor = 2^24 sorts 24 key bits, 2^24 + 1 sorts 25: the other rocPRIM configuration
# (n_major, n_minor, nnz, mode)
CSX_SMALL = ((100, 1, 70, "ends"), (1, 1, 1, "ends"), (50, 2, 70, "ends"), (3, 2, 1, "ends"),
             (1, 255, 70, "ends"), (40, 255, 1, "ends"), (1, 256, 70, "ends"), (9, 256, 70, "ends"), (1, 257, 70, "ends"),
             (9, 257, 70, "ends"), (1, 257, 1, "ends"),
             (1, 5000, 3000, "gaps"), (12, 5000, 3000, "gaps"))
CSX_LARGE = tuple([(1, CSX_BITS_STEP, 1, "ends"), (1, CSX_BITS_STEP, 70, "ends"), (5, CSX_BITS_STEP + 1, 1, "ends"),
                   (1, CSX_BITS_STEP + 1, 70, "ends")]
                  + [(m, CSX_BITS_STEP, n, mode) for (m, n, mode) in ((1, MERGE_NARROW - 1, "ends"), (37, MERGE_NARROW, "gaps"),
                                                                     (37, MERGE_NARROW + 1, "ends"))]
                  + [(m, CSX_BITS_STEP + 1, n, mode) for (m, n, mode) in ((37, MERGE_WIDE - 1, "ends"), (1, MERGE_WIDE, "ends"),
                                                                         (37, MERGE_WIDE + 1, "gaps"))]
                  + [(37, 5000, MERGE_NARROW + d, "gaps") for d in (-1, 0, 1)])


# ---- g. dense_nonfill ------------------------------------------------------------------------------------------------
DENSE_N = (1, DN_TILE - 1, DN_TILE, DN_TILE + 1, DN_TILE * 257 + 5, N1 + 257)
# name -> (bytes, kind): patterns are generated as unsigned words, the GPU test views them as the type
DENSE_TYPES = {"float16": (2, "f"), "bfloat16": (2, "f"), "float32": (4, "f"), "float64": (8, "f"), "int8": (1, "i"),
               "int64": (8, "i"), "bool": (1, "b")}
# (exponent bits, mantissa bits)
_FLOAT_LAYOUT = {"float16": (5, 10), "bfloat16": (8, 7), "float32": (8, 23), "float64": (11, 52)}


def float_specials(name):
    """bit patterns {+0, -0, +NaN, -NaN, NaN with another payload, 1.0, -1.0, smallest denormal} of a floating type"""
    e, m = _FLOAT_LAYOUT[name]
    sign = 1 << (e + m)
    exp_all = ((1 << e) - 1) << m
    one = ((1 << (e - 1)) - 1) << m
    qnan = exp_all | (1 << (m - 1))
    return {"+0": 0, "-0": sign, "+nan": qnan, "-nan": sign | qnan, "nan2": qnan | 1, "1": one, "-1": sign | one, "denormal": 1}


def dense_case(name, n, fill_bits, density, seed=0):
    """n patterns of type `name`, a share `density` of them different from `fill_bits` (0.0: none, 1.0: all); floating
    types hold both zeros and NaNs of both signs among the others (where n allows), never an accidental fill value"""
    nbytes, kind = DENSE_TYPES[name]
    dt = np.dtype(f"u{nbytes}")
    rng = np.random.default_rng([seed, n, fill_bits % (2 ** 31), int(density * 100)])
    if kind == "b":
        other = np.full(n, 1 - fill_bits, dtype=dt)
    elif kind == "i":
        other = rng.integers(0, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)
    else:
        e, m = _FLOAT_LAYOUT[name]
        # finite values: any sign and mantissa, exponent field below all-ones
        other = (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(e + m)
                 | rng.integers(0, (1 << e) - 1, size=n, dtype=np.uint64) << np.uint64(m)
                 | rng.integers(0, 1 << m, size=n, dtype=np.uint64)).astype(dt)
        sp = float_specials(name)
        pats = np.array([sp[k] for k in ("+0", "-0", "+nan", "-nan", "nan2", "denormal")], dtype=dt)
        where = rng.choice(n, size=min(n, max(6, n // 16)), replace=False)
        other[where] = pats[np.arange(where.size) % pats.size]
    fill = dt.type(fill_bits)
    other[other == fill] = dt.type(fill_bits ^ 1) if kind != "b" else dt.type(1 - fill_bits)
    keep = rng.random(n) < density if 0.0 < density < 1.0 else np.full(n, density >= 1.0)
    return np.where(keep, other, fill).astype(dt)


# ---- h. flags and movement ---------------------------------------------------------------------------------------------
MOVE_N = (1, 256, 257, N1 + 257)
MOVE_ROWS = (1, 3, 16)
ELEM_BYTES = (1, 2, 4, 8, 16)
TOO_MANY_ROWS = 65536       # rows of a [k, n] input ride in the grid's y dimension (at most 65535)

# ---- i. checks -------------------------------------------------------------------------------------------------------
CHECK_N = 4_200_000
CHECK_POSITIONS = (1, 63, 64, 255, 256, 257, 1023, 1024, 1025, N1 - 1, N1, N1 + 1, CHECK_N - 1)
COORD_NDIMS = (1, 3, 16)

# ---- j. linearize ----------------------------------------------------------------------------------------------------
LINEARIZE_SHAPES = {1: (1_000_003,), 2: (1201, 977), 5: (7, 3, 11, 2, 13), 16: (2, 3) * 8}
LINEARIZE_INT32_SHAPE = (70000, 70000)     # int32 coordinates whose key passes 2^31


def axis_orders(ndim):
    """every rotation of the axes, and their reversal"""
    base = list(range(ndim))
    out = [tuple(base[r:] + base[:r]) for r in range(ndim)]
    rev = tuple(reversed(base))
    return out if rev in out else out + [rev]


def coords_case(shape, nnz, idx_dtype, seed=0):
    """coords[ndim, nnz] inside `shape`, with the first and the last cell among them"""
    rng = np.random.default_rng([seed, len(shape), nnz])
    c = np.stack([rng.integers(0, d, size=nnz, dtype=np.int64) for d in shape])
    c[:, 0] = 0
    c[:, -1] = np.array(shape) - 1
    return c.astype(idx_dtype)


# ---- k. convert ------------------------------------------------------------------------------------------------------
CONVERT_TYPES = ("float32", "float64", "int32", "int64", "bool")
CONVERT_N = (257, N1 + 257)


def convert_values(src, n, seed=0):
    """n values of type `src` that every one of the five types holds exactly enough to convert in range: integers of at
    most 21 bits and (floats) their halves and quarters, both zeros included"""
    rng = np.random.default_rng([seed, n, len(src)])
    k = rng.integers(-2 ** 21, 2 ** 21, size=n, dtype=np.int64)
    k[rng.random(n) < 0.2] = 0
    if src == "bool":
        return (k & 1).astype(np.bool_)
    if src.startswith("int"):
        return k.astype(src)
    v = (k / 4.0).astype(src)
    v[::7] = -0.0
    return v

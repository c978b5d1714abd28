"""tests/reduce_cases.py against plain Python loops: the layouts are what their names say, the keys have the stated
form, the references are right, and the exactness assertions fire when violated.  No GPU."""
import math
import operator
from fractions import Fraction

import numpy as np
import pytest

import reduce_cases as RC

LAYOUTS = RC.layouts()
LOOPED = ["thread", "edges"] + [k for k in LAYOUTS if k.startswith("tiny_")]


def _runs(heads, n):
    ends = list(heads[1:]) + [n]
    return [(int(a), int(b)) for a, b in zip(heads, ends)]


def test_layouts_are_what_their_names_say():
    T, L = RC.TILE, LAYOUTS
    for name, (heads, n) in L.items():
        assert heads.dtype == np.int64 and heads[0] == 0 and np.all(np.diff(heads) > 0) and heads[-1] < n, name
        assert n <= 150_000, name
    h, n = L["thread"]
    assert n == 3 * T + 3 and RC.run_lengths(h, n)[:18].tolist() == list(range(1, 10)) * 2
    assert {int(x) % 4 for x in h} == {0, 1, 2, 3}
    h, n = L["edges"]
    assert set(RC.EDGE_POSITIONS) <= set(h.tolist()) and RC.run_lengths(h, n).max() <= 9
    h, n = L["singles_at_edge"]
    lens = dict(zip(h.tolist(), RC.run_lengths(h, n).tolist()))
    assert lens[2047] == lens[2048] == lens[2049] == 1
    for n in (5 * T - 1, 5 * T, 5 * T + 1):
        h, m = L[f"tile_exact_{n}"]
        assert m == n and h.tolist() == list(range(0, n, T))
    h, n = L["all_heads"]
    assert n == 3 * T + 3 and h.tolist() == list(range(n))
    for w in (31, 32, 33):
        h, n = L[f"walk_{w}"]
        heads = set(h.tolist())
        assert T - 1 in heads and (w + 1) * T in heads and not any(T <= x < (w + 1) * T for x in heads)
        assert n == (w + 2) * T + 3 and max(x for x in heads if x < T - 1) >= T - 10
    h, n = L["walk_mixed"]
    heads = set(h.tolist())
    assert not any(T <= x < 34 * T for x in heads) and {35 * T + p for p in RC.EDGE_POSITIONS} <= heads
    rems = set()
    for name, (h, n) in L.items():
        if name.startswith("open_end_"):
            assert n - int(h[-1]) > 3 * T
            rems.add((n % T, n % 4))
    assert rems == {(0, 0), (1, 1), (2, 2), (2047, 3)}
    for n in range(1, 6):
        assert L[f"tiny_one_run_{n}"][0].tolist() == [0] and L[f"tiny_all_heads_{n}"][0].tolist() == list(range(n))


def test_layouts_are_the_same_on_every_call():
    again = RC.layouts()
    assert list(again) == list(LAYOUTS)
    for name in LAYOUTS:
        assert np.array_equal(again[name][0], LAYOUTS[name][0]) and again[name][1] == LAYOUTS[name][1]


@pytest.mark.parametrize("divisor", [1, 9, 141, 100_003, 2 ** 31])
@pytest.mark.parametrize("name", ["thread", "edges", "tiny_one_run_5", "tiny_all_heads_5"])
def test_keys_have_the_stated_form(name, divisor):
    heads, n = LAYOUTS[name]
    keys, gids = RC.make_keys(heads, n, divisor, np.random.default_rng(1))
    assert keys.dtype == np.int64 and len(keys) == n and len(gids) == len(heads)
    assert np.all(np.diff(gids) >= 1) and np.any(np.diff(gids) > 1) or len(gids) < 4
    k = [int(x) for x in keys]
    for r, (a, b) in enumerate(_runs(heads, n)):
        assert all(x // divisor == int(gids[r]) for x in k[a:b])
        js = [x % divisor for x in k[a:b]]
        assert all(y > x for x, y in zip(js, js[1:])) or divisor == 1


_PY = {"add": operator.add, "multiply": operator.mul, "logical_or": lambda a, b: int(bool(a) or bool(b)),
       "logical_and": lambda a, b: int(bool(a) and bool(b))}


def _loop_reference(op, data, a, b):
    """one run by a plain loop in exact Python arithmetic (integers wrapped to the dtype at the end)"""
    dt = data.dtype
    vals = data[a:b].tolist()
    if op in ("maximum", "minimum", "fmax", "fmin"):
        nan = [v for v in vals if v != v]
        rest = [v for v in vals if v == v]
        pick = max if op in ("maximum", "fmax") else min
        if nan and (op in ("maximum", "minimum") or not rest):
            return math.nan
        return pick(rest)
    if dt.kind == "f":
        vals = [Fraction(v) for v in vals]
    acc = vals[0]
    for v in vals[1:]:
        acc = _PY[op](acc, v)
    if dt.kind == "i":
        bits = 8 * dt.itemsize
        acc = (acc + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)
    return acc


@pytest.mark.parametrize("op,dtype", RC.TABLE, ids=[f"{o}-{np.dtype(d).name}" for o, d in RC.TABLE])
def test_exact_data_and_reference_against_a_python_loop(op, dtype):
    for name in LOOPED:
        heads, n = LAYOUTS[name]
        data = RC.make_data(op, dtype, heads, n, np.random.default_rng(7))
        assert data.dtype == np.dtype(dtype) and len(data) == n
        want = RC.reference(op, data, heads, n)
        assert want.dtype == data.dtype and len(want) == len(heads)
        for r, (a, b) in enumerate(_runs(heads, n)):
            loop = _loop_reference(op, data, a, b)
            if isinstance(loop, float) and loop != loop:
                assert np.isnan(want[r]), (name, r)
            else:
                assert Fraction(want[r].item()) == Fraction(loop), (name, r, want[r], loop)       # exact: no rounding happened
    if np.dtype(dtype).kind == "f" and op in ("maximum", "fmax"):
        heads, n = LAYOUTS["edges"]
        data = RC.make_data(op, dtype, heads, n, np.random.default_rng(7))
        lens = RC.run_lengths(heads, n)
        nan_runs = np.add.reduceat(np.isnan(data).astype(np.int64), heads)
        assert np.isnan(data[RC.TILE - 1]) and np.isnan(data[RC.TILE]) and np.any(nan_runs == lens) and np.any(nan_runs == 0)
        assert np.any(np.isnan(data[heads])) and np.any(np.isnan(data[heads + lens - 1]))
        vals = data[~np.isnan(data)]
        assert len(np.unique(vals)) == len(vals) and not np.any(vals == 0)
    if op.startswith("logical"):
        heads, n = LAYOUTS["thread"]
        want = RC.reference(op, RC.make_data(op, dtype, heads, n, np.random.default_rng(7)), heads, n)
        assert 0.2 < want.mean() < 0.8            # neither all true nor all false: a misplaced element shows


def test_the_exactness_assertions_fire():
    heads, n = LAYOUTS["tiny_one_run_5"]
    with pytest.raises(AssertionError, match="not exact"):
        RC.assert_exact_sums(np.full(5, 2.0 ** 22, dtype=np.float32), heads, n)
    RC.assert_exact_sums(np.full(5, 2.0 ** 21, dtype=np.float32), heads, n)
    RC.assert_exact_sums(np.full(5, 2.0 ** 22, dtype=np.float64), heads, n)
    with pytest.raises(AssertionError):
        RC.assert_exact_sums(np.array([1.5, 1, 1, 1, 1], dtype=np.float64), heads, n)
    big = np.zeros(1, dtype=np.int64), 300
    with pytest.raises(AssertionError, match="twos"):
        RC.assert_exact_products(np.full(300, 2.0), *big)
    with pytest.raises(AssertionError, match="halves"):
        RC.assert_exact_products(np.full(300, 0.5), *big)
    with pytest.raises(AssertionError):
        RC.assert_exact_products(np.full(300, 3.0), *big)
    RC.assert_exact_products(np.array([2.0, 0.5, -1.0] * 100), *big)
    with pytest.raises(AssertionError, match="gamma"):
        RC.gamma(2 ** 24, np.float32)
    with pytest.raises(AssertionError, match="divisor"):
        RC.make_keys(np.zeros(1, dtype=np.int64), 5, 3, np.random.default_rng(0))


@pytest.mark.parametrize("dtype", RC.FLOAT_DTYPES)
def test_rounding_references(dtype):
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    assert RC.unit_roundoff(dtype) == u and RC.gamma(3, dtype) == 3 * u / (1 - 3 * u)
    heads, n = LAYOUTS["thread"]
    data = RC.rounding_data(dtype, n, np.random.default_rng(3))
    assert data.dtype == np.dtype(dtype) and data.min() < -0.9 and data.max() > 0.9
    exact, bound = RC.fsum_reference(data, heads, n)
    seq = RC.sequential_reference(data, heads, n)
    for r, (a, b) in enumerate(_runs(heads, n)):
        true = sum(Fraction(float(v)) for v in data[a:b])
        assert abs(Fraction(exact[r]) - true) <= Fraction(2.0 ** -53) * abs(true)
        acc = data[a]
        for v in data[a + 1:b]:
            acc = acc + v                          # NumPy scalars of the value type: rounded at every step
        assert acc.dtype == np.dtype(dtype) and seq[r] == acc
        m = b - a
        want = 0.0 if m == 1 else RC.gamma(m - 1, dtype) * float(np.abs(data[a:b].astype(np.float64)).sum()) + u * abs(exact[r])
        assert bound[r] == pytest.approx(want, rel=1e-12) and (bound[r] > 0) == (m > 1)
        assert abs(Fraction(float(seq[r])) - true) <= Fraction(bound[r])      # left to right is one of "any order"


@pytest.mark.parametrize("top", [2 ** 53, 2 ** 62])
def test_keys_at_range(top):
    """the keys really sit at q d - 1, q d, q d + 1 at the top of the range, and the double-precision guess of the
    quotient is wrong for some of them: the corrections are needed"""
    heads, n = LAYOUTS["thread"]
    small = large = 0
    for d in RC.RANGE_DIVISORS:
        keys, lo, hi = RC.range_keys(heads, n, d, top, np.random.default_rng(d % 1000))
        k = [int(x) for x in keys]
        assert all(a <= b for a, b in zip(k, k[1:])) and 0 <= k[0] and top - d <= k[-1] < top
        g = [x // d for x in k]
        assert [i for i in range(n) if i == 0 or g[i] != g[i - 1]] == heads.tolist()       # the runs of k // d ARE the layout
        ks = set(k)
        triples = sum(1 for q in set(g) if q * d - 1 in ks and q * d in ks and (q * d + 1 in ks or d == 1))
        assert triples >= 100, (d, triples)
        assert max(g) == top // d - 1 and min(g) == 0
        small, large = small + lo, large + hi
    # below 2^53 the guess for q d - 1 is never one too large (that needs 1 / d < q 2^-53, i.e. q d > 2^53); the guess for
    # q d is one too small where 1 / d rounds down (10^12 + 39 of the six divisors): the `r >= d` correction decides there
    assert small > 0 and (large > 0 or top == 2 ** 53)


def test_pad_to_quotient():
    heads, n = LAYOUTS["walk_31"]
    for q in (23, 24):
        h, m = RC.pad_to_quotient(heads, n, q)
        assert m // len(h) == q and np.array_equal(h[:len(heads)], heads) and np.all(np.diff(h[len(heads):]) == 1)

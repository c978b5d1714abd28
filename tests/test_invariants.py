"""The checker of tests/invariants.py has to bite: every valid array set passes, every single mutation of one is rejected with
the name of the rule it breaks.  NumPy only - no device."""
import numpy as np
import pytest

import invariants as inv


def _coo(coords, data, shape, fill=0.0, idt=np.int64, pruned=False):
    data = np.asarray(data, dtype=np.float64)
    coords = np.asarray(coords, dtype=idt).reshape(len(shape), data.size)
    return dict(coords=coords, data=data, shape=tuple(shape), fill_value=np.float64(fill), index_dtype=idt, pruned=pruned,
                keys=inv.host_keys(coords, shape) if inv._prod(shape) < 2 ** 63 else None)


VALID_COO = {
    "empty shape": _coo([], [], (0,)),
    "no stored element, non-empty shape": _coo([[], []], [], (4, 5)),
    "0-d": _coo(np.zeros((0, 1)), [2.5], ()),
    "1-D": _coo([[1, 4, 8]], [1.0, -2.0, 3.0], (9,)),
    "3-D int32": _coo([[0, 0, 1, 2, 2], [0, 3, 1, 0, 3], [4, 0, 2, 2, 4]], [1.0, 2.0, 3.0, 4.0, 5.0], (3, 4, 5), idt=np.int32),
    "3-D int64, fill value": _coo([[0, 0, 1, 2, 2], [0, 3, 1, 0, 3], [4, 0, 2, 2, 4]], [1.0, 2.0, 3.0, 4.0, 0.0], (3, 4, 5), fill=1.5),
    "2-D first and last position": _coo([[0, 2, 6], [0, 3, 7]], [1.0, 2.0, 3.0], (7, 8), idt=np.int32),
    "stored -0.0, pruned": _coo([[0, 1, 1], [2, 0, 5]], [1.0, -0.0, 2.0], (2, 6), pruned=True),
    "keys beyond 2^63": _coo([[0, 1, 2 ** 40 - 1], [5, 0, 2 ** 40 - 1]], [1.0, 2.0, 3.0], (2 ** 40, 2 ** 40)),
}


def _gcxs(data, indices, indptr, shape, ca, fill=0.0, idt=np.int64, pruned=False):
    return dict(data=np.asarray(data, dtype=np.float64), indices=np.asarray(indices, dtype=idt), indptr=np.asarray(indptr, dtype=idt),
                shape=tuple(shape), compressed_axes=ca, fill_value=np.float64(fill), pruned=pruned)


VALID_GCXS = {
    "csr int32, leading and trailing empty rows": _gcxs([1.0, 2.0, 3.0, 4.0, 5.0], [0, 2, 5, 1, 5], [0, 0, 3, 3, 5, 5, 5], (6, 6), (0,), idt=np.int32),
    "csc int64": _gcxs([1.0, 2.0, 3.0, 4.0], [0, 3, 3, 1], [0, 2, 2, 3, 4], (4, 4), (1,)),
    "3-D compressed (0, 2)": _gcxs([1.0, 2.0, 3.0, 4.0, 5.0], [0, 2, 1, 0, 1], [0, 2, 2, 3, 3, 3, 5, 5, 5], (2, 3, 4), (0, 2)),
    "3-D compressed (1,), int32": _gcxs([1.0, 2.0, 3.0], [7, 0, 6], [0, 1, 1, 3], (2, 3, 4), (1,), idt=np.int32),
    "empty shape": _gcxs([], [], [0], (0, 5), (0,)),
    "no stored element, non-empty shape": _gcxs([], [], [0, 0, 0, 0], (3, 4), (0,), idt=np.int32),
    "1-D": _gcxs([1.0, 2.0, 3.0], [0, 3, 6], [], (7,), None),
    "stored -0.0, pruned": _gcxs([-0.0, 2.0, 3.0], [1, 0, 2], [0, 1, 3], (2, 3), (0,), pruned=True),
}


@pytest.mark.parametrize("name", VALID_COO)
def test_valid_coo_arrays_pass(name):
    inv.check_coo_arrays(**VALID_COO[name])


@pytest.mark.parametrize("name", VALID_GCXS)
def test_valid_gcxs_arrays_pass(name):
    inv.check_gcxs_arrays(**VALID_GCXS[name])


# ---- mutations: each returns the mutated keyword set, or None where the valid set has no room for it ------------------------
def _copy(v):
    return {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in v.items()}


def _swap_columns(v):
    if v["data"].size < 2 or not v["shape"]:
        return None
    v["coords"][:, [0, 1]] = v["coords"][:, [1, 0]]
    v["data"][[0, 1]] = v["data"][[1, 0]]
    if v["keys"] is not None:
        v["keys"][[0, 1]] = v["keys"][[1, 0]]
    return v


def _duplicate_column(v):
    if v["data"].size < 1:
        return None
    last = v["data"].size - 1
    v["coords"] = np.concatenate([v["coords"], v["coords"][:, last:]], axis=1)
    v["data"] = np.concatenate([v["data"], [0.25]])                     # (a partner that changes nothing much in a dense image)
    if v["keys"] is not None:
        v["keys"] = np.concatenate([v["keys"], v["keys"][last:]])
    return v


def _coordinate_at_extent(v):
    if v["data"].size < 1 or not v["shape"] or max(v["shape"]) >= 2 ** 31:
        return None
    d = len(v["shape"]) - 1
    v["coords"][d, -1] = v["shape"][d]
    v["keys"] = None
    return v


def _negative_coordinate(v):
    if v["data"].size < 1 or not v["shape"]:
        return None
    v["coords"][0, 0] = -1
    v["keys"] = None
    return v


def _keys_off_by_one(v):
    if v["keys"] is None or v["data"].size < 1:
        return None
    v["keys"][v["data"].size // 2] += 1
    return v


def _keys_int32(v):
    if v["keys"] is None:
        return None
    v["keys"] = v["keys"].astype(np.int32)
    return v


def _positive_zero_when_pruned(v):
    if v["data"].size < 1 or v["fill_value"] != 0:
        return None
    v["data"][-1] = 0.0
    v["pruned"] = True
    return v


COO_MUTATIONS = {
    "two columns swapped": (_swap_columns, inv.RULE_COO_ORDER),
    "a duplicated column": (_duplicate_column, inv.RULE_COO_ORDER),
    "a coordinate equal to the extent": (_coordinate_at_extent, inv.RULE_COO_BOUNDS),
    "a negative coordinate": (_negative_coordinate, inv.RULE_COO_BOUNDS),
    "keys off by one in one element": (_keys_off_by_one, inv.RULE_COO_KEYS),
    "keys as int32": (_keys_int32, inv.RULE_COO_KEYS_DTYPE),
    "a stored +0.0 under pruned=True": (_positive_zero_when_pruned, inv.RULE_PRUNED),
}


def _ptr_first(v):
    if v["compressed_axes"] is None:
        return None
    v["indptr"][0] = 3
    return v


def _ptr_decreasing(v):
    p = v["indptr"]
    if p.size < 3:
        return None
    p[p.size - 2] = p[p.size - 1] + 1          # an inner pointer above its successor; indptr[0] and indptr[-1] stay
    return v


def _ptr_last_short(v):
    p = v["indptr"]
    if v["compressed_axes"] is None or v["data"].size < 1:
        return None
    p[p == p[-1]] -= 1               # (every trailing empty row with it: the pointers stay non-decreasing)
    return v


def _row_with_two(v):
    p = v["indptr"] if v["compressed_axes"] is not None else np.array([0, v["data"].size])
    return next((int(p[r]) for r in range(p.size - 1) if p[r + 1] - p[r] >= 2), None)


def _swap_inside_row(v):
    k = _row_with_two(v)
    if k is None:
        return None
    v["indices"][[k, k + 1]] = v["indices"][[k + 1, k]]
    return v


def _index_at_row_length(v):
    if v["data"].size < 1:
        return None
    ca = v["compressed_axes"] or ()
    v["indices"][-1] = inv._prod(s for d, s in enumerate(v["shape"]) if d not in ca)
    return v


def _mixed_widths(v):
    if v["compressed_axes"] is None:
        return None
    v["indices"], v["indptr"] = v["indices"].astype(np.int32), v["indptr"].astype(np.int64)
    return v


def _duplicate_inside_row(v):
    k = _row_with_two(v)
    if k is None:
        return None
    v["indices"][k + 1] = v["indices"][k]
    return v


GCXS_MUTATIONS = {
    "indptr[0] = 3": (_ptr_first, inv.RULE_GCXS_PTR_FIRST),
    "one decreasing pointer pair": (_ptr_decreasing, inv.RULE_GCXS_PTR_MONOTONE),
    "indptr[-1] one short": (_ptr_last_short, inv.RULE_GCXS_PTR_LAST),
    "two indices swapped inside a row": (_swap_inside_row, inv.RULE_GCXS_ROW_ORDER),
    "an index twice inside a row": (_duplicate_inside_row, inv.RULE_GCXS_ROW_ORDER),
    "an index equal to the row length": (_index_at_row_length, inv.RULE_GCXS_BOUNDS),
    "indices int32 with indptr int64": (_mixed_widths, inv.RULE_GCXS_WIDTH),
    "a stored +0.0 under pruned=True": (_positive_zero_when_pruned, inv.RULE_PRUNED),
}


def _mutate_and_expect(check, valid, mutations, name, mutation):
    mutate, rule = mutations[mutation]
    v = mutate(_copy(valid[name]))
    if v is None:
        return                       # (no room for this mutation in this set; `test_every_mutation_was_applied` counts)
    with pytest.raises(AssertionError) as e:
        check(**v)
    assert str(e.value).startswith(rule + ":"), (name, mutation, str(e.value))
    assert "position" in str(e.value) or rule in (inv.RULE_COO_KEYS_DTYPE, inv.RULE_GCXS_WIDTH, inv.RULE_GCXS_PTR_LAST), str(e.value)


@pytest.mark.parametrize("mutation", COO_MUTATIONS)
@pytest.mark.parametrize("name", VALID_COO)
def test_mutated_coo_arrays_are_rejected(name, mutation):
    _mutate_and_expect(inv.check_coo_arrays, VALID_COO, COO_MUTATIONS, name, mutation)


@pytest.mark.parametrize("mutation", GCXS_MUTATIONS)
@pytest.mark.parametrize("name", VALID_GCXS)
def test_mutated_gcxs_arrays_are_rejected(name, mutation):
    _mutate_and_expect(inv.check_gcxs_arrays, VALID_GCXS, GCXS_MUTATIONS, name, mutation)


def test_every_mutation_was_applied():
    """a mutation that found no room in any valid set would prove nothing (the loops are repeated here: this test must not
    depend on the others having run)"""
    for check, valid, mutations in ((inv.check_coo_arrays, VALID_COO, COO_MUTATIONS), (inv.check_gcxs_arrays, VALID_GCXS, GCXS_MUTATIONS)):
        for mutation, (mutate, _) in mutations.items():
            rooms = [name for name in valid if mutate(_copy(valid[name])) is not None]
            assert len(rooms) >= 2, (check.__name__, mutation, rooms)


def test_layout_and_dtype_rules():
    v = _copy(VALID_COO["3-D int32"])
    with pytest.raises(AssertionError, match="^" + inv.RULE_COO_LAYOUT):
        inv.check_coo_arrays(**dict(v, data=v["data"][:-1], keys=None))
    with pytest.raises(AssertionError, match="^" + inv.RULE_COO_INDEX_DTYPE):
        inv.check_coo_arrays(**dict(v, coords=v["coords"].astype(np.int16)))
    with pytest.raises(AssertionError, match="^" + inv.RULE_COO_INDEX_DTYPE):
        inv.check_coo_arrays(**dict(v, index_dtype=np.int64))
    g = _copy(VALID_GCXS["csc int64"])
    with pytest.raises(AssertionError, match="^" + inv.RULE_GCXS_LAYOUT):
        inv.check_gcxs_arrays(**dict(g, indptr=g["indptr"][:-1]))
    with pytest.raises(AssertionError, match="^" + inv.RULE_GCXS_PTR_LAST.replace("[", r"\[").replace("]", r"\]")):
        inv.check_gcxs_arrays(**dict(g, data=g["data"][:-1]))
    with pytest.raises(AssertionError, match="^" + inv.RULE_GCXS_WIDTH):
        inv.check_gcxs_arrays(**dict(g, indices=g["indices"].astype(np.int16), indptr=g["indptr"].astype(np.int16)))


def test_bit_comparison_of_the_pruned_rule():
    """-0.0 is a stored element, +0.0 is not; a NaN fill value is found by its bits"""
    assert inv.eq_bits(np.array([0.0, -0.0, 1.0]), 0.0).tolist() == [True, False, False]
    assert inv.eq_bits(np.array([0.0, -0.0], dtype=np.float32), np.float32(-0.0)).tolist() == [False, True]
    assert inv.eq_bits(np.array([np.nan, 1.0]), np.nan).tolist() == [True, False]
    assert inv.eq_bits(np.array([0j, complex(0.0, -0.0), 1j]), 0).tolist() == [True, False, False]
    assert inv.eq_bits(np.array([0, 3, 0], dtype=np.int64), 0).tolist() == [True, False, True]
    assert inv.eq_bits(np.zeros(0), 0.0).shape == (0,)


def test_host_keys_use_python_integers_beyond_int64():
    k = inv.host_keys(np.array([[2 ** 40 - 1], [2 ** 40 - 1]]), (2 ** 40, 2 ** 40))
    assert k.dtype == object and k[0] == 2 ** 80 - 1
    assert inv.host_keys(np.array([[1], [2]], dtype=np.int32), (70_000, 70_000)).tolist() == [70_002]     # (no int32 overflow)


def test_single_nonzero_pointer_of_an_empty_compressed_range_is_rejected():
    """the defect of the compressed-axis slice `x[a:a]`, `a > 0`, on arrays alone: one pointer, `indptr[a]`, not zero"""
    for p, idt in ((7, np.int32), (1, np.int64)):
        bad = _gcxs([], [], [p], (0, 12), (0,), idt=idt)
        with pytest.raises(AssertionError) as e:
            inv.check_gcxs_arrays(**bad)
        assert str(e.value).startswith(inv.RULE_GCXS_PTR_FIRST + ":") and "indptr[0]" in str(e.value)
        inv.check_gcxs_arrays(**_gcxs([], [], [0], (0, 12), (0,), idt=idt))
    bad = _gcxs([], [], [7], (12, 0), (1,))
    with pytest.raises(AssertionError, match=r"^gcxs\.indptr\[0\]"):
        inv.check_gcxs_arrays(**bad)

"""CPU: the dictionary model of the coordinate kernels (coord_ref.py) agrees with oracle/sparse.py on the oracle's own ordinary
inputs, behaves as documented at the packing limit (where the oracle aliases), and the fixture sets of test_coord_limits_gpu.py
hold every event they are built for — the GPU tests import the same builders, so an edited fixture cannot pass by losing one."""
import numpy as np
import pytest

import coord_ref as R
from coord_ref import LIMIT
from oracle import sparse as OS
from test_oracle_sparse import random_coords


def _ordinary(seed, n=600, extent=9, batch=3, stride=1):
    rng = np.random.default_rng(seed)
    c = random_coords(rng, n, extent=extent, batch=batch, stride=stride)
    c = np.concatenate([c, c[rng.integers(0, len(c), n // 2)]])
    rng.shuffle(c)
    return c


@pytest.mark.parametrize("q", [1, 2, 4])
def test_unique_first_equals_the_oracle(q):
    c = _ordinary(q)
    uniq, inv, ids, status = R.unique_first(R.rows_of(c), q)
    ru, rinv = OS.unique_first(c, q)
    assert status == 0 and uniq == R.rows_of(ru) and inv == rinv.tolist()
    assert [ids[k] for k in uniq] == list(range(len(uniq)))
    queries = _ordinary(10 + q, extent=11, batch=4)
    assert R.lookup(ids, R.rows_of(queries), q) == OS.Index(ru).lookup(OS.quantise(queries, q)).tolist()
    assert R.first_rows(R.rows_of(c), q) == OS.Index(OS.quantise(c, q)).lookup(OS.quantise(c, q)).tolist()


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_maps_equal_the_oracle(stride):
    rng = np.random.default_rng(20 + stride)
    fine = random_coords(rng, 700, extent=7, batch=2, stride=stride)
    rows = R.rows_of(fine)
    ids = R.unique_first(rows, 1)[2]
    assert R.kernel_map(ids, rows, 3, stride) == OS.kernel_map(fine, fine, 3, stride).tolist()
    coarse, parent, _, _ = R.unique_first(rows, 2 * stride)
    rc, rparent = OS.unique_first(fine, 2 * stride)
    assert coarse == R.rows_of(rc) and parent == rparent.tolist()
    assert R.kernel_map(ids, coarse, 2, stride) == OS.kernel_map(fine, rc, 2, stride).tolist()
    assert R.transpose_map(rows, parent, stride) == OS.transpose_map(fine, rparent, stride).tolist()


def test_hierarchy_is_the_chain_of_unique_calls():
    c = _ordinary(30, n=900)
    levels = R.hierarchy(R.rows_of(c), 3)
    src = c
    for l, (uniq, inv, _, status) in enumerate(levels):
        ru, rinv = OS.unique_first(src, 1 << l)
        assert status == 0 and uniq == R.rows_of(ru) and inv == rinv.tolist()
        src = ru
    assert [len(lv[0]) for lv in levels] == sorted((len(lv[0]) for lv in levels), reverse=True)


def test_a_prefix_of_the_list_numbers_as_a_prefix():
    """first-occurrence numbering is stable under truncation, level by level: the device-count tests compute the model once per
    capacity and cut it at every live count"""
    rows = R.rows_of(_ordinary(31, n=500))
    full = R.hierarchy(rows, 3)
    for live in (0, 1, 77, 500, len(rows)):
        part = R.hierarchy(rows[:live], 3)
        n = live
        for (fu, fi, _, _), (pu, pi, _, _) in zip(full, part):
            assert pi == fi[:n] and pu == fu[:len(pu)] and len(pu) == max(fi[:n], default=-1) + 1
            n = len(pu)


def test_grid_rank_model():
    dims = (2, 3, 4)
    rows = [(0, 0, 0, 0), (0, 2, 4, 6), (0, 1, 0, 0), (0, -2, 0, 0), (0, 4, 0, 0), (0, 0, 6, 0), (0, 0, 0, 8), (0, 2, 0, 2)]
    vol, off = R.grid_rank(rows, 2, dims)
    want = [-1] * 24
    want[0], want[(1 * 3 + 2) * 4 + 3], want[(1 * 3 + 0) * 4 + 1] = 0, 1, 7
    assert vol == want and off == 5
    assert R.grid_rank([], 1, dims) == ([-1] * 24, 0)
    with pytest.raises(ValueError):
        R.grid_rank([(0, 0, 0, 0), (1, 0, 0, 0)], 1, dims)


def test_the_model_does_not_alias_where_packing_does():
    a, b = (0, 2 ** 19, 5, -7), (1, -(2 ** 19), 5, -7)
    assert OS.pack(np.array([a]))[0] == OS.pack(np.array([b]))[0]            # the oracle cannot tell these apart
    ids = R.unique_first([(1, -(2 ** 19) + 2, 5, -7)], 1)[2]
    assert R.lookup(ids, [a, b]) == [-1, -1] and not R.in_range(*a) and not R.in_range(*b)
    assert R.in_range(14, LIMIT, -LIMIT, LIMIT) and not R.in_range(15, 0, 0, 0) and not R.in_range(-1, 0, 0, 0)
    assert not R.in_range(0, LIMIT + 1, 0, 0) and not R.in_range(0, 0, -LIMIT - 1, 0) and not R.in_range(0, 0, 0, LIMIT + 1)
    # quantise first, then test the range
    assert R.quantise((0, -524286, 0, 0), 4) == (0, -524288, 0, 0)
    assert R.unique_first([(0, -524286, 0, 0)], 1)[3] == 0 and R.unique_first([(0, -524286, 0, 0)], 4)[1:] == ([-1], {}, 1)
    assert R.unique_first([(0, 524287, 0, 0)], 1)[3] == 1 and R.unique_first([(0, 524287, 0, 0)], 2)[:2] == ([(0, 524286, 0, 0)], [0])
    # a neighbour over the edge is absent even when the place it would alias to is occupied
    ids = {(0, LIMIT, 0, 0): 0, (1, -(2 ** 19), 0, 0): 1}
    assert R.kernel_map(ids, [(0, LIMIT, 0, 0)], 3, 2)[14] == [-1]


# ---- the fixture sets hold their events ------------------------------------------------------------------------------------

def _refused(rows, q):
    return [r for r, i in zip(rows, R.unique_first(rows, q)[1]) if i < 0]


def _accepted(rows, q):
    return [r for r, i in zip(rows, R.unique_first(rows, q)[1]) if i >= 0]


def test_limit_set_holds_every_event():
    rows = R.rows_of(R.limit_set())
    assert 200 <= len(rows) <= 900 and len(set(rows)) < len(rows)            # a few hundred, duplicated
    assert rows != sorted(rows)
    acc1, ref1 = set(_accepted(rows, 1)), set(_refused(rows, 1))
    for axis in (1, 2, 3):
        for sign in (1, -1):
            assert any(r[axis] == sign * LIMIT for r in acc1), (axis, sign)
            assert any(r[axis] == sign * (LIMIT + 1) and R.in_range(*(r[:axis] + (0,) + r[axis + 1:])) for r in ref1), (axis, sign)
    assert any(r[0] == 14 for r in acc1) and any(r[0] == 15 and R.in_range(14, *r[1:]) for r in ref1)
    assert acc1 & set(_refused(rows, 4))                                     # legal at q = 1, refused at q = 4
    assert ref1 & set(_accepted(rows, 2))                                    # refused at q = 1, accepted at q = 2
    for q in (1, 2, 4):
        assert R.unique_first(rows, q)[3] == 1 and len(_accepted(rows, q)) > 200
    spatial = {}
    for r in acc1:
        spatial.setdefault(r[1:], set()).add(r[0])
    assert any(len(b) > 1 for b in spatial.values())                         # one place in two batches
    assert any(all(c < 0 and c % 2 for c in r[1:]) for r in acc1)            # negative odd
    # the refused and accepted rows are interleaved: accepted rows are numbered behind refused ones
    inv = R.unique_first(rows, 1)[1]
    assert -1 in inv[:len(inv) // 2] and -1 in inv[len(inv) // 2:]


def test_clean_set_has_no_refused_row():
    rows = R.rows_of(R.clean_set())
    for q in (1, 2, 4):
        assert R.unique_first(rows, q)[3] == 0
    assert any(max(abs(c) for c in r[1:]) > LIMIT - 8 for r in rows) and any(r[0] == 14 for r in rows)


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_accepted_set_has_neighbours_over_the_edge(stride):
    rows = R.rows_of(R.accepted_set(stride))
    assert len(set(rows)) == len(rows) and all(R.in_range(*r) and all(c % stride == 0 for c in r[1:]) for r in rows)
    ids = {r: i for i, r in enumerate(rows)}
    for axis in (1, 2, 3):       # a +stride (axes at +LIMIT) or -stride (the axis at -LIMIT) neighbour out of range
        assert any(abs(r[axis]) + stride > LIMIT for r in rows), axis
    assert any(r[1] + stride > LIMIT for r in rows)
    k3 = R.kernel_map(ids, rows, 3, stride)
    corner = [i for i, r in enumerate(rows) if r[1] + stride > LIMIT]
    assert all(k3[14][i] == -1 for i in corner) and any(k3[12][i] >= 0 for i in corner)   # +x over the edge, -x inside
    assert k3[13] == list(range(len(rows)))
    # at least one fine voxel per child slot, negative ones among them, for the transposed map
    parent = R.unique_first(rows, 2 * stride)[1]
    up = R.transpose_map(rows, parent, stride)
    assert all(any(v >= 0 for v in line) for line in up)
    assert any(c < 0 and (c // stride) % 2 for r in rows for c in r[1:])


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_map_rows_have_the_asked_length_and_touch_the_limit(n, stride):
    rows = R.rows_of(R.map_rows(n, stride))
    assert len(rows) == n == len(set(rows)) and all(R.in_range(*r) and all(c % stride == 0 for c in r[1:]) for r in rows)
    assert any(max(abs(c) for c in r[1:]) + stride > LIMIT for r in rows)
    if n > 1:
        assert any(max(abs(c) for c in r[1:]) < 100 for r in rows)


def test_alias_rows_alias_under_packing():
    c, pairs = R.alias_rows()
    rows = R.rows_of(c)
    assert len(set(rows)) == len(rows) and all(R.in_range(*r) for r in rows)
    ids = {r: i for i, r in enumerate(rows)}
    want = R.kernel_map(ids, rows, 3, R.ALIAS_STRIDE)
    packed = OS.kernel_map(c, c, 3, R.ALIAS_STRIDE)
    for i, k, j in pairs:
        dx, dy, dz = R.offsets(3)[k]
        b, x, y, z = rows[i]
        nb = (b, x + dx * R.ALIAS_STRIDE, y + dy * R.ALIAS_STRIDE, z + dz * R.ALIAS_STRIDE)
        assert not R.in_range(*nb) and OS.pack(np.array([nb]))[0] == OS.pack(c[j:j + 1])[0]
        assert want[k][i] == -1 and packed[k, i] == j            # the packing oracle walks into the alias, the model does not
    assert any(v >= 0 for k in range(27) if k != 13 for v in want[k])


def test_query_set_asks_inside_at_and_past_the_limit():
    rows = R.rows_of(R.query_set())
    ids = R.unique_first(R.rows_of(R.limit_set()), 1)[2]
    got = R.lookup(ids, rows)
    assert any(g >= 0 for g in got) and any(g < 0 and R.in_range(*r) for g, r in zip(got, rows))
    assert any(not R.in_range(*r) for r in rows) and any(r[0] > 15 for r in rows) and any(r[0] < 0 for r in rows)
    assert any(abs(r[1]) >= 2 ** 19 for r in rows)


@pytest.mark.parametrize("stride", [1, 2])
def test_rank_rows_cover_every_way_off_the_grid(stride):
    dims = (5, 7, 11)
    rows = R.rows_of(R.rank_rows(stride, dims))
    vol, off = R.grid_rank(rows, stride, dims)
    assert sum(v >= 0 for v in vol) + off == len(rows) and sum(v >= 0 for v in vol) > 150
    assert vol[0] >= 0 and vol[-1] >= 0
    bad = [r for r in rows if not R.on_grid(r, stride, dims)]
    for axis in (1, 2, 3):
        assert any(r[axis] < 0 for r in bad)
        assert any(r[axis] == dims[axis - 1] * stride for r in bad) and any(r[axis] > dims[axis - 1] * stride for r in bad)
    if stride > 1:
        assert any(all(c >= 0 for c in r[1:]) and any(c % stride for c in r[1:]) for r in bad)
    # rows that a swap of two extents would let in, and cells it would move
    assert any(r[1] // stride < dims[1] and r[1] // stride >= dims[0] and r[2] == r[3] == 0 for r in bad)
    assert any(r[2] // stride < dims[2] and r[2] // stride >= dims[1] and r[1] == r[3] == 0 for r in bad)


@pytest.mark.parametrize("cap", [257, 8193, 16385, 32769, 69637])
def test_count_rows_are_ordinary_with_repeats(cap):
    rows = R.rows_of(R.count_rows(cap))
    assert len(rows) == cap and 0.35 * cap < cap - len(set(rows)) < 0.45 * cap
    assert any(c < 0 and c % 2 for r in rows for c in r[1:]) and len({r[0] for r in rows}) == 3
    for q in (1, 2, 4):
        assert R.unique_first(rows, q)[3] == 0
    assert rows[:50] != sorted(rows[:50])


def test_hash_load_rows_fill_a_table_but_for_one_slot():
    keys, absent = R.hash_load_rows()
    keys, absent = R.rows_of(keys), R.rows_of(absent)
    assert len(keys) == 1023 == len(set(keys)) and all(R.in_range(*r) for r in keys)
    assert any(max(abs(c) for c in r[1:]) == LIMIT for r in keys)
    assert len(absent) == 2000 and not set(absent) & set(keys)
    assert sum(R.in_range(*r) for r in absent) == 1900


def test_three_key_rows_race_onto_three_keys():
    rows = R.rows_of(R.three_key_rows())
    first = R.first_rows(rows)
    assert len(rows) == 20000 and len(set(rows)) == 3 and sorted(set(first)) == sorted({rows.index(r) for r in set(rows)})
    assert max(first) >= 5000 and min(rows.count(r) for r in set(rows)) > 3000

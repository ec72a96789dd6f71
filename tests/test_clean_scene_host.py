"""CPU-only: the host restatement of the clean-up rule (tests/clean_scene_ref.py) on cases whose answers are written out by
hand, so that the GPU tests compare the kernels against something checked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clean_scene_ref import REPORT_KEYS, adjacent, clean_rows_ref, components_ref  # noqa: E402


def test_adjacency_counts():
    cells = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    for connectivity in (6, 18, 26):
        assert sum(adjacent(c, (0, 0, 0), connectivity) for c in cells) == connectivity
    assert not adjacent((0, 0, 0), (0, 0, 0), 26) and not adjacent((2, 0, 0), (0, 0, 0), 26)


def test_bar_with_a_negative_key_in_the_middle():
    coords = [(x, 0, 0) for x in range(9)]
    keys = [0, 0, 0, 0, -1, 0, 0, 0, 0]
    for connectivity in (6, 18, 26):
        assert components_ref(coords, keys, connectivity).tolist() == [0, 0, 0, 0, -1, 5, 5, 5, 5]
    assert components_ref(coords, None, 6).tolist() == [0] * 9


def test_corner_contact_needs_26():
    coords = [(0, 0, 0), (1, 1, 1)]
    assert components_ref(coords, None, 26).tolist() == [0, 0]
    assert components_ref(coords, None, 18).tolist() == [0, 1]
    assert components_ref(coords, None, 6).tolist() == [0, 1]


def test_edge_contact_needs_18():
    coords = [(0, 0, 0), (0, 1, -1)]
    assert components_ref(coords, None, 26).tolist() == [0, 0]
    assert components_ref(coords, None, 18).tolist() == [0, 0]
    assert components_ref(coords, None, 6).tolist() == [0, 1]


def test_keys_separate_touching_rows_and_labels_follow_row_order():
    coords = [(2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0)]
    assert components_ref(coords, [1, 1, 2, 1], 6).tolist() == [0, 0, 2, 3]       # row 3 touches only row 2, of another key
    assert components_ref(coords, [1, 1, 1, 1], 6).tolist() == [0, 0, 0, 0]


def test_duplicate_rows_raise():
    with pytest.raises(ValueError):
        components_ref([(0, 0, 0), (1, 0, 0), (0, 0, 0)])


SIX = dict(coords=[(0, 0, 0), (1, 0, 0), (5, 0, 0), (6, 0, 0), (10, 0, 0), (12, 0, 0)], tsdf=[0.0] * 6, semantic=[3] * 6,
           instance=[5, 5, 5, 5, 5, 7])


def test_six_rows_split_ties_and_fresh_ids():
    """instance 5 in pieces of 2, 2 and 1 rows: the first piece of 2 keeps the id (tie: smaller label), the others get
    max + 1 = 8 and 9 in ascending label order; instance 7 is in one piece and stays"""
    c, t, s, i, report = clean_rows_ref(**SIX, split_instances=True)
    assert i.tolist() == [5, 5, 8, 8, 9, 7] and s.tolist() == [3] * 6 and len(c) == 6
    assert report == dict(zip(REPORT_KEYS, (6, 0, 4, 0, 0, 0, 2)))


def test_six_rows_clear_then_split():
    """min_segment_voxels=2 clears the two single rows first; the fresh id then counts from the largest id left, 5"""
    c, t, s, i, report = clean_rows_ref(**SIX, min_segment_voxels=2, split_instances=True)
    assert s.tolist() == [3, 3, 3, 3, 0, 0] and i.tolist() == [5, 5, 6, 6, 0, 0] and t.tolist() == [0.0] * 6
    assert report == dict(zip(REPORT_KEYS, (6, 0, 4, 0, 2, 2, 1)))


def test_six_rows_geometry_rules():
    """min_voxels=2 removes the single rows and keeps a component of exactly 2; keep_largest=1 keeps the first of the two
    largest (tie: smaller label); a row with tsdf 1 is no geometry and is kept as it is"""
    c, t, s, i, report = clean_rows_ref(**SIX, min_voxels=2)
    assert [tuple(r) for r in c.tolist()] == SIX["coords"][:4] and report["rows_removed"] == 2 and report["components_removed"] == 2
    c, _, _, _, report = clean_rows_ref(**SIX, keep_largest=1)
    assert [tuple(r) for r in c.tolist()] == SIX["coords"][:2] and report["components"] == 4 and report["components_removed"] == 3
    six = dict(SIX, tsdf=[0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    c, t, _, _, report = clean_rows_ref(**six, min_voxels=2)
    assert [tuple(r) for r in c.tolist()] == SIX["coords"][:5] and t.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert report["components"] == 3 and report["rows_removed"] == 1


def test_inputs_are_left_alone():
    sem, ins = np.array(SIX["semantic"]), np.array(SIX["instance"])
    clean_rows_ref(SIX["coords"], SIX["tsdf"], sem, ins, min_segment_voxels=2, split_instances=True)
    assert sem.tolist() == SIX["semantic"] and ins.tolist() == SIX["instance"]

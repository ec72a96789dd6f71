"""CPU: the numpy statement of the distance-field rule (tests/distance_field_ref.py) against answers written by hand, against
scipy's Euclidean distance transform, under a mirror, and against the accuracy the module's docstring states."""
import numpy as np
import pytest

import distance_field_ref as D
import raycast_fixtures as FX

FAR = D.FAR


def rows(cells, values):
    return np.array(cells, np.int32).reshape(-1, 3), np.array(values, np.float32)


def test_one_site_pair():
    coords, tsdf = rows([(0, 0, 0), (1, 0, 0)], [-0.5, 0.5])
    assert D.site_rows(coords, tsdf).tolist() == [0, 1]         # the inside row borders empty space, the outside row borders it
    dist2, site, state = D.distance_field(coords, tsdf, (-2, 0, 0), (5, 3, 1))
    assert dist2[:, 0, 0].tolist() == [4, 1, 0, 0, 1, 4, 9]
    assert site[:, 0, 0].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert dist2[:, 2, 0].tolist() == [8, 5, 4, 4, 5, 8, 13]
    assert site[:, 2, 0].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert state[:, 0, 0].tolist() == [0, 0, 2, 1, 0, 0, 0] and not state[:, 1:].any()
    cut2, cut_site, _ = D.distance_field(coords, tsdf, (-2, 0, 0), (5, 3, 1), radius=2)
    assert cut2[:, 0, 0].tolist() == [4, 1, 0, 0, 1, 4, FAR] and cut_site[:, 0, 0].tolist() == [0, 0, 0, 1, 1, 1, -1]
    assert cut2[:, 2, 0].tolist() == [FAR, FAR, 4, 4, FAR, FAR, FAR]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_equidistant_sites_give_the_smaller_row_whatever_its_coordinate(order):
    cells = [(0, 0, 0), (4, 0, 0)]
    coords, tsdf = rows([cells[k] for k in order], [-1.0, -1.0])
    dist2, site, _ = D.distance_field(coords, tsdf, (0, 0, 0), (5, 1, 1))
    assert dist2[:, 0, 0].tolist() == [0, 1, 4, 1, 0]
    first, second = order.index(0), order.index(1)              # the rows at x = 0 and at x = 4
    assert site[:, 0, 0].tolist() == [first, first, 0, second, second]


def test_a_repeated_coordinate_counts_once_with_its_first_row():
    coords, tsdf = rows([(0, 0, 0), (0, 0, 0), (1, 0, 0)], [0.5, -0.5, 0.5])
    assert D.site_rows(coords, tsdf).tolist() == []             # the first row at (0,0,0) is outside: nothing is inside
    coords, tsdf = rows([(0, 0, 0), (0, 0, 0), (1, 0, 0)], [-0.5, 0.5, 0.5])
    assert D.site_rows(coords, tsdf).tolist() == [0, 2]


def test_inside_rows_at_the_edge_of_the_rows_are_sites_and_a_buried_one_is_not():
    cells = [(x, y, z) for x in range(3) for y in range(3) for z in range(3)]
    coords, tsdf = rows(cells, [0.0] * 27)                      # tsdf == 0 is inside
    centre = cells.index((1, 1, 1))
    assert D.site_rows(coords, tsdf).tolist() == [r for r in range(27) if r != centre]
    dist2, site, state = D.distance_field(coords, tsdf, (0, 0, 0), (3, 3, 3))
    assert dist2[1, 1, 1] == 1 and site[1, 1, 1] == cells.index((0, 1, 1))      # six at distance 1: the smallest row
    assert (np.delete(dist2.reshape(-1), centre) == 0).all() and (state == 2).all()
    assert np.array_equal(np.delete(site.reshape(-1), centre), np.delete(np.arange(27), centre))


def test_a_scene_without_an_inside_row_has_no_site():
    cells = [(x, y, 0) for x in range(3) for y in range(3)]
    coords, tsdf = rows(cells, [0.25] * 9)
    assert len(D.site_rows(coords, tsdf)) == 0
    dist2, site, state = D.distance_field(coords, tsdf, (-1, -1, -1), (4, 4, 2))
    assert (dist2 == FAR).all() and (site == -1).all()
    assert (state[1:4, 1:4, 1] == 1).all() and state.sum() == 9


def _sphere_box():
    s = FX.sphere()
    return s, (-3, -2, -4), (27, 26, 28)


def test_unbounded_dist2_is_scipys_transform_of_the_site_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    s, lo, hi = _sphere_box()
    dist2, _, _ = D.distance_field(s["coords"], s["tsdf"], lo, hi)
    mask = np.ones(dist2.shape, bool)
    at = s["coords"][D.site_rows(s["coords"], s["tsdf"])] - np.array(lo)
    mask[at[:, 0], at[:, 1], at[:, 2]] = False
    want = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)
    assert np.array_equal(dist2, want)


def test_mirroring_the_coordinates_mirrors_dist2():
    s, lo, hi = _sphere_box()
    dist2, _, state = D.distance_field(s["coords"], s["tsdf"], lo, hi, radius=6)
    mirrored = s["coords"] * np.array([-1, 1, 1], np.int32)
    m2, _, mstate = D.distance_field(mirrored, s["tsdf"], (1 - hi[0], lo[1], lo[2]), (1 - lo[0], hi[1], hi[2]), radius=6)
    assert np.array_equal(m2[::-1], dist2) and np.array_equal(mstate[::-1], state)
    assert (dist2 == FAR).any() and (dist2 != FAR).any()


@pytest.mark.parametrize("scene", ["sphere", "slab_box"])
def test_the_distance_is_within_one_cell_of_the_nearest_crossed_edge(scene):
    """a site is an end of a crossed edge and every crossed edge has a site at an end, half a cell from its midpoint: the
    distance to the nearest site is within half a cell of the distance to the nearest midpoint, and a midpoint is within half a
    cell of its edge's nearest point — one cell in all, as eprecon_amd/distance_field.py states"""
    s = FX.SCENES[scene]()
    lo, hi = (-2, -2, -2), tuple(d + 2 for d in s["dims"])
    dist2, _, _ = D.distance_field(s["coords"], s["tsdf"], lo, hi)
    mids = D.crossed_edge_midpoints(s["coords"], s["tsdf"])
    assert len(mids) > 100
    cells = D.box_cells(lo, hi).astype(np.float64)
    nearest = np.full(len(cells), np.inf)
    for k in range(0, len(cells), 2048):
        part = cells[k:k + 2048]
        nearest[k:k + 2048] = np.sqrt(sum((part[:, None, a] - mids[None, :, a]) ** 2 for a in range(3)).min(1))
    gap = np.abs(np.sqrt(dist2.reshape(-1).astype(np.float64)) - nearest)
    assert gap.max() <= 0.5 + 1e-12, gap.max()

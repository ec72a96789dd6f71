"""CPU: the restatement of the simplification rule (tests/simplify_ref.py) held to cases written out by hand.
The GPU tests hold eprecon_amd/simplify.py to the restatement; these hold the restatement to the rule."""
import math

import numpy as np
import pytest

import simplify_cases as C
import simplify_ref as R

F32 = lambda rows: np.array(rows, np.float32)


def test_one_triangle_in_three_cells_is_unchanged():
    verts = F32([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1]])
    out = R.simplify(verts, [[0, 1, 2]], 1.0)
    # ranks of the cells (0,0,0) < (0,1,0) < (1,0,0)
    assert out["cluster"].tolist() == [0, 2, 1] and out["cells"].tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert out["faces"].tolist() == [[0, 2, 1]] and out["kept"].tolist() == [0] and out["written"].all()
    # one plane through each vertex: the minimiser is the vertex
    assert np.abs(out["positions"][out["cluster"]] - verts.astype(np.float64)).max() < 1e-12
    assert np.abs(out["normals"] - [0, 0, 1]).max() == 0
    rep = out["report"]
    assert [rep[k] for k in ("vertices_in", "faces_in", "clusters", "vertices_out", "faces_out", "faces_degenerate", "faces_duplicate")] == \
        [3, 1, 3, 3, 1, 0, 0]
    assert rep["max_shift"] < 1e-12


def test_one_triangle_in_one_cell_gives_an_empty_mesh():
    out = R.simplify(F32([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1]]), [[0, 1, 2]], 1.0)
    assert out["cluster"].tolist() == [0, 0, 0]
    assert out["faces"].shape == (0, 3) and out["vertices"].shape == (0, 3) and not out["written"].any()
    rep = out["report"]
    assert (rep["clusters"], rep["vertices_out"], rep["faces_out"], rep["faces_degenerate"], rep["faces_duplicate"]) == (1, 0, 0, 1, 0)
    assert 0 < rep["max_shift"] <= math.sqrt(3)


def test_two_triangles_sharing_an_edge_across_a_cell_face():
    """a-b crosses the face x = 1; c and d lie in the one cell (0, 1, 0): both faces map to the triple {a, b, cd}, the second
    is a duplicate of the first, and the merged vertex is the mean of c and d (all four points lie in the plane z = 0.5)"""
    verts = F32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.875, 1.5, 0.5], [0.625, 1.25, 0.5]])
    out = R.simplify(verts, [[0, 1, 2], [0, 1, 3]], 1.0)
    assert out["cluster"].tolist() == [0, 2, 1, 1]
    assert out["kept"].tolist() == [0] and out["faces"].tolist() == [[0, 2, 1]]
    assert (out["report"]["faces_degenerate"], out["report"]["faces_duplicate"], out["report"]["vertices_out"]) == (0, 1, 3)
    assert np.abs(out["positions"][1] - [0.75, 1.375, 0.5]).max() < 1e-12
    assert np.abs(out["positions"][0] - [0.5, 0.5, 0.5]).max() < 1e-12


def test_dyadic_lattice_faces_go_to_the_upper_cell():
    values = np.array([-0.5, -0.3125, -0.25, -0.0625, 0.0, 0.0625, 0.1875, 0.25, 0.4375, 0.5])
    want = [-2, -2, -1, -1, 0, 0, 0, 1, 1, 2]
    verts = np.stack([values, values[::-1], np.zeros_like(values)], 1).astype(np.float32)
    cells = R.cells_of(verts, 0.25)
    assert cells[:, 0].tolist() == want and cells[:, 1].tolist() == want[::-1] and cells[:, 2].tolist() == [0] * 10
    # ... and from an origin that is itself dyadic
    assert R.cells_of(verts, 0.25, origin=[0.0625, 0, 0])[:, 0].tolist() == [-3, -2, -2, -1, -1, 0, 0, 0, 1, 1]
    verts, faces = C.dyadic_lattice()
    out = R.simplify(verts, faces, 0.25)
    assert out["cells"][:, :2].min() == -2 and out["cells"][:, :2].max() == 2
    on_face = np.flatnonzero(verts[:, 0] == 0.25)
    assert len(on_face) == 17 and (out["cells"][out["cluster"][on_face], 0] == 1).all()
    assert not out["fragile"].any()


def test_a_flat_patch_is_represented_by_its_mean():
    s = 0.0625 + 0.3125 * np.arange(10)      # (dyadic: the float32 vertices lie in the plane exactly)
    verts, faces = C.grid(s, s, lambda x, y: 0.25 + 0.25 * x - 0.125 * y)
    out = R.simplify(verts, faces, 1.0)
    assert out["report"]["clusters"] > 9
    assert np.abs(out["positions"] - out["means"]).max() < 1e-12
    n = np.array([-0.25, 0.125, 1.0]) / np.linalg.norm([-0.25, 0.125, 1.0])
    assert np.abs(out["normals"] - n.astype(np.float32)).max() < 1e-6


def test_a_cluster_on_a_ridge_moves_towards_both_planes():
    verts, faces = C.dihedral()
    out = R.simplify(verts, faces, 1.0, origin=[-0.5, -0.5, -0.5])
    k = int(np.flatnonzero((out["cells"] == 0).all(1))[0])
    assert (out["cluster"] == k).sum() == 9 and np.abs(out["means"][k] - [0, 0, 0.3 - 0.4 / 3]).max() < 1e-6
    dist = lambda p, sign: abs(p[2] - 0.3 + sign * 0.5 * p[0]) / math.sqrt(1.25)
    for sign in (-1.0, 1.0):
        assert dist(out["positions"][k], sign) < 0.05 * dist(out["means"][k], sign)
    assert np.abs(out["positions"][k] - [0, 0, 0.3]).max() < 2e-3      # on the ridge; y = 0 by symmetry


def test_energy_at_the_output_is_at_most_the_energy_at_the_mean():
    rng = np.random.default_rng(7)
    half, clipped = 0.5, 0
    for _ in range(200):
        a, b, c0 = np.zeros((3, 3)), np.zeros(3), 0.0
        for _ in range(int(rng.integers(1, 7))):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            w, d = rng.uniform(0.01, 1.0), rng.uniform(-1.0, 1.0)
            a, b, c0 = a + w * np.outer(u, u), b - w * d * u, c0 + w * d * d
        m = rng.uniform(-half, half, 3)
        p, x, lam, _ = R.represent(a, b, m, half, 1e-3)
        q = (a, b, c0, lam, m)
        assert np.abs(p).max() <= half
        assert R.energy(q, p) <= R.energy(q, m) + 1e-12 * (1.0 + abs(R.energy(q, m)))
        assert R.energy(q, x) <= R.energy(q, p) + 1e-9 * (1.0 + abs(R.energy(q, p)))
        clipped += bool(np.abs(x).max() > half)
    assert 20 < clipped < 200      # both branches of the clip are exercised


def test_a_duplicate_pair_and_a_flipped_pair():
    verts = F32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]])
    faces = [[0, 1, 2], [1, 2, 0], [0, 1, 3], [3, 1, 0], [2, 1, 0]]
    out = R.simplify(verts, faces, 1.0)
    # cells (0,0,0) (0,0,1) (0,1,0) (1,0,0): vertex 3 -> 1, vertex 2 -> 2, vertex 1 -> 3
    assert out["cluster"].tolist() == [0, 3, 2, 1]
    assert out["kept"].tolist() == [0, 2] and out["faces"].tolist() == [[0, 3, 2], [0, 3, 1]]      # each keeps its own orientation
    assert (out["report"]["faces_degenerate"], out["report"]["faces_duplicate"]) == (0, 3)


def test_colour_rounding_at_one_half():
    verts = F32([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    colors = np.array([[1, 0, 255], [2, 1, 254], [7, 8, 9], [10, 11, 12]], np.uint8)
    out = R.simplify(verts, [[0, 2, 3], [1, 2, 3]], 1.0, colors=colors)
    # sums 3, 1, 509 over 2 members: 1.5 -> 2, 0.5 -> 1, 254.5 -> 255
    assert out["rgb"][0].tolist() == [2, 1, 255] and out["rgb"][1].tolist() == [10, 11, 12] and out["rgb"][2].tolist() == [7, 8, 9]
    three = R.simplify(np.concatenate([verts, F32([[0.25, 0.75, 0.25]])]), [[0, 2, 3], [1, 2, 3], [4, 2, 3]], 1.0,
                       colors=np.concatenate([colors, np.array([[1, 1, 1]], np.uint8)]))
    assert three["rgb"][0].tolist() == [1, 1, 170]      # 4/3 -> 1, 2/3 -> 1, 510/3 = 170


def test_labels_split_a_cell_and_are_never_mixed():
    verts = F32([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    out = R.simplify(verts, [[0, 2, 3], [1, 2, 3]], 1.0, semantic=[3, 1, 0, 0], instance=[0, 0, -2, 5])
    assert out["report"]["clusters"] == 4 and out["cluster"].tolist() == [1, 0, 3, 2]
    assert out["cluster_semantic"].tolist() == [1, 3, 0, 0] and out["cluster_instance"].tolist() == [0, 0, 5, -2]
    assert out["report"]["faces_out"] == 2


@pytest.mark.parametrize("triangles", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_the_fans_need_no_mask(triangles):
    """the share of clusters a GPU comparison of positions may leave out (at most 1 %) is 0 on the numpy-built fixtures"""
    for collapse in (False, True):
        verts, faces = C.fan(triangles, collapse)
        out = R.simplify(verts, faces, 1.0)
        assert not out["fragile"].any()
        assert (out["cluster"] == out["cluster"][0]).sum() == 1      # the hub is alone
        if collapse:
            assert out["report"]["faces_out"] == 0 and out["report"]["faces_degenerate"] == triangles

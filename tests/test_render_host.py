"""CPU-only: the float64 restatement of view rendering (tests/render_ref.py) on a case worked by hand, the cap on the pixels
it leaves out of a comparison on every fixture view, the argument parsing of both command-line tools, write_png."""
import math

import numpy as np
import pytest

import render_ref as RR

import eprecon_amd.render as RD

LEFT_OUT_CAP = 0.01          # at most 1 % of a view's pixels may be left out: a condition of the tests, not a measurement


def test_restatement_on_a_hand_computed_4x4_case():
    """K = [[2,0,2],[0,2,2],[0,0,1]], camera at the origin: pixel (r, c) looks along ((c - 1.5) / 2, (r - 1.5) / 2, 1) and
    meets the plane z = 2 at (x, y) = (c - 1.5, r - 1.5).  The triangle a (-2,-2), b (2.2,-2), c (-2,2.2) in that plane
    covers x + y < 0.2: ten of the sixteen points.  Barycentric weights there: w_b = (x + 2) / 4.2, w_c = (y + 2) / 4.2."""
    k = np.array([[2.0, 0, 2.0], [0, 2.0, 2.0], [0, 0, 1]])
    verts = np.array([[-2, -2, 2], [2.2, -2, 2], [-2, 2.2, 2]], np.float32)
    front = np.array([[0, 2, 1]], np.int32)          # ((v1 - v0) x (v2 - v0)) . v0 < 0: faces the camera
    lab = np.array([70, 80, 90])
    out = RR.render_view(verts, front, k, np.eye(4), 4, 4, labels=(lab,), backgrounds=(-5,))
    want_corner = np.array([[0, 0, 1, 1],          # row 0: y = -1.5
                            [0, 0, 1, -1],         # row 1: y = -0.5; (x, y) = (-0.5, -0.5) has w_b = w_c (left out)
                            [2, 2, -1, -1],
                            [2, -1, -1, -1]])
    assert np.array_equal(out["face"], np.where(want_corner >= 0, 0, -1))
    tie = np.zeros((4, 4), bool)
    tie[1, 1] = True
    assert np.array_equal(out["left_out"], tie)
    ok = ~tie
    assert np.array_equal(out["corner"][ok], want_corner[ok])
    assert np.array_equal(out["labels"][0][ok], np.where(want_corner >= 0, lab[np.maximum(want_corner, 0)], -5)[ok])
    assert np.array_equal(out["depth"], np.where(want_corner >= 0, 2.0, 0.0))
    for r in range(4):
        for c in range(4):
            x, y = c - 1.5, r - 1.5
            if want_corner[r, c] < 0:
                assert tuple(out["rgb"][r, c]) == (255, 255, 255)
                continue
            value = 153.0 * (0.3 + 0.7 / math.sqrt(1.0 + (x * x + y * y) / 4.0))       # n = (0, 0, +-1): |n . d| / |d| = 1 / |d|
            assert abs(out["shade"][r, c, 0] - value) < 1e-12
            assert tuple(out["rgb"][r, c]) == (int(math.floor(value + 0.5)),) * 3
    # wound the other way it is a back face: culled, or drawn identically without culling
    back = front[:, [0, 2, 1]]
    assert (RR.render_view(verts, back, k, np.eye(4), 4, 4)["face"] == -1).all()
    again = RR.render_view(verts, back, k, np.eye(4), 4, 4, cull_back=False)
    assert np.array_equal(again["face"], out["face"]) and np.array_equal(again["rgb"], out["rgb"])
    # with back = [0, 1, 2] slot 1 is vertex 1 and slot 2 vertex 2 again: the same corners by vertex index
    assert np.array_equal(again["corner"][ok], want_corner[ok])
    # an x.5 before rounding is left out: colour 5, ambient 0.5, cosine 1 / 1.25 = 0.8 -> 5 * (0.5 + 0.5 * 0.8) = 4.5
    tri = np.array([[-50, -50, 4], [150, -50, 4], [-50, 150, 4]], np.float32)
    col = np.full((3, 3), 5, np.uint8)
    k1 = np.array([[1.0, 0, -0.25], [0, 1.0, 0.5], [0, 0, 1]])              # pixel (0, 0): d = (0.75, 0, 1), |d| = 1.25
    half = RR.render_view(tri, np.array([[0, 2, 1]], np.int32), k1, np.eye(4), 1, 1, colors=col, ambient=0.5)
    assert abs(half["shade"][0, 0, 0] - 4.5) < 1e-12 and half["left_out"][0, 0]


@pytest.mark.parametrize("cull", [True, False])
def test_left_out_cap_on_every_fixture_view(cull):
    verts, faces, poses = RR.fixture()
    sem, ins, col = RR.fixture_labels(len(verts))
    n_hit = []
    for v in range(len(poses)):
        for colors in (None, col):
            out = RR.render_view(verts, faces, RR.K_SMALL, poses[v], RR.H, RR.W, labels=(sem, ins), colors=colors, cull_back=cull)
            assert out["left_out"].mean() <= LEFT_OUT_CAP, (v, cull, int(out["left_out"].sum()))
        n_hit.append(int((out["face"] >= 0).sum()))
    # the fixture shows what it is meant to: surfaces over most of both outside views, and from inside the closed cube
    # every pixel once back faces are drawn
    assert n_hit[0] > 1500 and n_hit[1] > 1500
    if not cull:
        assert n_hit[2] == RR.H * RR.W


def test_left_out_cap_on_the_tessellated_patch():
    verts, faces = RR.patch()
    assert len(faces) == 128
    out = RR.render_view(verts, faces, RR.K_SMALL, np.eye(4), RR.H, RR.W)
    assert out["left_out"].mean() <= LEFT_OUT_CAP
    assert len(np.unique(out["face"][out["face"] >= 0])) > 100          # nearly every small face owns a pixel


def test_small_scene_has_views_without_left_out_pixels():
    """the pixel-domain test scores the views the restatement leaves nothing out of: there are such views (the mesh of the
    CPU marching cubes here is the device's, vertex for vertex: tests/test_marching_cubes.py)"""
    from oracle import marching_cubes as OM
    tsdf, _, _, poses = RR.scene24()
    verts, faces = OM.marching_cubes(tsdf, 0.0)
    verts = verts.astype(np.float32) * np.float32(RR.VOXEL) + RR.ORIGIN
    assert len(faces) > 1000
    left = [RR.render_view(verts, faces, RR.K_SMALL, pose, RR.H, RR.W)["left_out"] for pose in poses]
    assert all(m.mean() <= LEFT_OUT_CAP for m in left)
    assert sum(not m.any() for m in left) >= 2
    gt_verts, gt_faces, _, _ = RR.disagreeing_ground_truth(verts, faces, np.zeros(len(verts), np.int64), np.zeros(len(verts), np.int64))
    left_gt = [RR.render_view(gt_verts, gt_faces, RR.K_SMALL, pose, RR.H, RR.W)["left_out"] for pose in poses]
    assert all(m.mean() <= LEFT_OUT_CAP for m in left_gt)
    assert sum(not a.any() and not b.any() for a, b in zip(left, left_gt)) >= 2


def test_render_cli_arguments():
    a = RD.parse_args(["--pred", "p", "--data_path", "d", "--scenes", "s.txt", "--out", "o"])
    assert (a.pred, a.data_path, a.scenes, a.out, a.every, a.size, a.mode) == ("p", "d", "s.txt", "o", 10, [640, 480], "all")
    a = RD.parse_args(["--pred", "p", "--data_path", "d", "--scenes", "s", "--out", "o", "--every", "3", "--size", "64", "48",
                       "--mode", "instance"])
    assert (a.every, a.size, a.mode) == (3, [64, 48], "instance")
    for bad in (["--pred", "p", "--data_path", "d", "--scenes", "s"], ["--pred", "p", "--data_path", "d", "--scenes", "s", "--out", "o",
                                                                       "--mode", "depth"]):
        with pytest.raises(SystemExit):
            RD.parse_args(bad)
    k = RD.scaled_intrinsics([[577.0, 0, 319.5], [0, 578.0, 239.5], [0, 0, 1]], (64, 48))
    assert np.allclose(k, [[57.7, 0, 31.95], [0, 57.8, 23.95], [0, 0, 1]], rtol=1e-15, atol=0)


def test_panoptic_score_cli_takes_views_next_to_info():
    from eprecon_amd import panoptic_score as PS
    base = ["--pred", "p", "--scenes", "s.txt"]
    a = PS.parse_args(base + ["--views", "d", "--info", "i", "--gt_mesh", "m", "--every", "4", "--size", "64", "48"])
    assert (a.views, a.info, a.gt_mesh, a.gt, a.every, a.size) == ("d", "i", "m", None, 4, [64, 48])
    a = PS.parse_args(base + ["--views", "d", "--info", "i", "--gt_mesh", "m"])
    assert (a.every, a.size) == (10, [640, 480])
    # what --gt alone and --info alone do is unchanged
    a = PS.parse_args(base + ["--gt", "g"])
    assert (a.gt, a.info, a.views) == ("g", None, None)
    a = PS.parse_args(base + ["--info", "i"])
    assert (a.gt, a.info, a.views) == (None, "i", None)
    for bad in (base, base + ["--gt", "g", "--info", "i"], base + ["--views", "d"], base + ["--views", "d", "--info", "i"],
                base + ["--views", "d", "--gt_mesh", "m"], base + ["--views", "d", "--gt", "g", "--info", "i", "--gt_mesh", "m"],
                base + ["--info", "i", "--gt_mesh", "m"]):
        with pytest.raises(SystemExit):
            PS.parse_args(bad)


def test_write_png_round_trip(tmp_path):
    image_mod = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    path = RD.write_png(str(tmp_path / "sub" / "a.png"), rgb)
    assert np.array_equal(np.asarray(image_mod.open(path)), rgb)
    grey = rng.integers(0, 256, (5, 7)).astype(np.uint8)
    assert np.array_equal(np.asarray(image_mod.open(RD.write_png(str(tmp_path / "g.png"), grey))), grey)
    with pytest.raises(ValueError):
        RD.write_png(str(tmp_path / "bad.png"), rgb.astype(np.float32))

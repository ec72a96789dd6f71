"""CPU-only: the float64 restatement of vertex colouring (tests/colorize_ref.py) on cases worked by hand, the cap on the
vertices it leaves out of a comparison on every fixture of the GPU tests, the share of the analytic room it colours, the
command-line arguments and scene_frames on a directory written here."""
import os

import numpy as np
import pytest

import colorize_cases as CC
import colorize_ref as CR
import render_ref as RR

UNDECIDED_CAP = 0.01          # at most 1 % of a fixture's vertices may be left out: a condition of the tests, not a measurement

K4 = np.array([[2.0, 0, 2.0], [0, 2.0, 2.0], [0, 0, 1]])          # a 4 x 4 image: pixel (r, c) has its centre at (c + 0.5, r + 0.5)
TRI_V = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)   # a face in the plane z = 1 whose first corner is on the axis
TRI_F = np.array([[0, 1, 2]], np.int32)


def words(depth, face=0, shape=(4, 4)):
    return CR.pack_visibility(np.full(shape, depth), np.full(shape, face))


def behind(distance):
    pose = np.eye(4)
    pose[2, 3] = -distance
    return pose


def test_a_vertex_on_a_pixel_centre_takes_that_pixel():
    """K4, camera at the origin: the vertex (-0.5, 0.5, 2) projects to (1.5, 2.5), the centre of pixel (row 2, column 1)"""
    verts = np.array([[-0.5, 0.5, 2], [1, 0.5, 2], [-0.5, 2, 2]], np.float32)
    frames = CC.seeded_frames(1, seed=1, h=4, w=4)
    out = CR.colorize(verts, TRI_F, K4, K4, np.eye(4)[None], frames, words(2.0)[None])
    assert out["seen"][0] == 1 and tuple(out["rgb"][0]) == tuple(frames[0, 2, 1])
    cosine = 2.0 / np.sqrt(0.25 + 0.25 + 4.0)                 # n = (0, 0, 2.25), q = (-0.5, 0.5, 2)
    assert abs(out["acc"][0, 3] - cosine / 4.0) < 1e-15
    assert np.allclose(out["acc"][0, :3], frames[0, 2, 1] * cosine / 4.0, rtol=1e-15, atol=0)
    assert out["undecided"][0]                                # (x and y are integers: the floor's argument is on a boundary)


def test_two_facing_views_mix_four_to_one():
    """the vertex (0, 0, 1) seen along the axis from z = 1 and from z = 2: cos = 1 in both, weights 1 and 1/4; constant frames
    (200, 100, 50) and (100, 50, 250) mix to ((4 * 200 + 100) / 5, (4 * 100 + 50) / 5, (4 * 50 + 250) / 5) = (180, 90, 90)"""
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    frames[0], frames[1] = (200, 100, 50), (100, 50, 250)
    poses = np.stack([np.eye(4), behind(1.0)])
    vis = np.stack([words(1.0), words(2.0)])
    out = CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, vis)
    assert out["seen"][0] == 2 and tuple(out["rgb"][0]) == (180, 90, 90)
    assert np.array_equal(out["acc"][0], [200 + 25.0, 100 + 12.5, 50 + 62.5, 1.25])
    # min_views = 3 is not reached: the fallback colour
    again = CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, vis, min_views=3, fallback=(1, 2, 3))
    assert tuple(again["rgb"][0]) == (1, 2, 3) and again["seen"][0] == 2


def test_a_nearer_surface_in_the_buffer_hides_the_vertex():
    """as above, but the second view's buffer holds 1.9 where the vertex is at z = 2: nearer by more than the 0.04 tolerance"""
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    frames[0], frames[1] = (200, 100, 50), (100, 50, 250)
    poses = np.stack([np.eye(4), behind(1.0)])
    out = CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, np.stack([words(1.0), words(1.9)]))
    assert out["seen"][0] == 1 and tuple(out["rgb"][0]) == (200, 100, 50)
    # within the tolerance it counts; no hit, a face index past the mesh and a degenerate face do not
    assert CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, np.stack([words(1.0), words(1.97)]))["seen"][0] == 2
    assert CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, np.stack([words(1.0), words(2.0, face=-1)]))["seen"][0] == 1
    assert CR.colorize(TRI_V, TRI_F, K4, K4, poses, frames, np.stack([words(1.0), words(2.0, face=1)]))["seen"][0] == 1
    flat = np.array([[0, 0, 1]], np.int32)
    assert CR.colorize(TRI_V, flat, K4, K4, poses, frames, np.stack([words(1.0), words(2.0)]))["seen"][0] == 0


@pytest.mark.parametrize("size", CC.VIS_SIZES)
def test_undecided_cap_on_the_small_fixtures(size):
    k_vis = CC.vis_intrinsics(RR.K_SMALL, size, (CC.FRAME_W, CC.FRAME_H))
    coloured = 0
    for name, verts, faces, poses in CC.small_cases():
        vis = CC.cpu_visibility(verts, faces, k_vis, poses, size[1], size[0])
        out = CR.colorize(verts, faces, RR.K_SMALL, k_vis, poses, CC.seeded_frames(len(poses)), vis)
        assert out["undecided"].mean() <= UNDECIDED_CAP, (name, int(out["undecided"].sum()))
        coloured += int((out["seen"] > 0).sum())
    assert coloured > 400          # the fixtures show what they are meant to: most patch vertices take a colour


def test_the_restatement_colours_the_analytic_room():
    """the end-to-end scene of the GPU test on the CPU: marching cubes of the oracle (the device's mesh, vertex for vertex:
    tests/test_marching_cubes.py) and render_ref's visibility.  At least half the vertices are seen; the worst error of a
    vertex against the colour function at the vertex is what the GPU test takes its bound from (144.1 levels
    here, a vertex at a silhouette that samples the black outside; the median is 0.3 levels)."""
    from oracle import marching_cubes as OM
    scene = CC.analytic_scene()
    verts, faces = OM.marching_cubes(scene["tsdf"], 0.0)
    verts = verts.astype(np.float32) * np.float32(scene["voxel"]) + scene["origin"]
    w, h = CC.SCENE_VIS_SIZE
    k_vis = CC.vis_intrinsics(scene["k"], (w, h), (320, 240))
    vis = CC.cpu_visibility(verts, faces, k_vis, scene["poses"], h, w, pixel_center=0.0)
    out = CR.colorize(verts, faces, scene["k"], k_vis, scene["poses"], scene["frames"], vis, pixel_center=0.0,
                      tolerance=scene["voxel"])
    worst, share = CC.scene_error(verts, out)
    print(f"analytic room: {len(verts)} vertices, {100 * share:.1f} % seen, worst error {worst:.2f} levels")
    assert out["undecided"].mean() <= UNDECIDED_CAP
    assert share >= 0.5
    seen = out["seen"] >= 1
    err = np.abs(out["value"][seen] - CC.colour_of(verts.astype(np.float64)[seen])).max(1)
    assert np.median(err) < 1.0          # the colours are the scene's: the worst cases are silhouettes, not the rule


def test_colorize_cli_arguments():
    from eprecon_amd import colorize as CZ
    a = CZ.parse_args(["--pred", "p", "--data_path", "d", "--scenes", "s.txt"])
    assert (a.pred, a.data_path, a.scenes, a.out, a.every, a.vis_size, a.min_views) == ("p", "d", "s.txt", None, 10, [640, 480], 1)
    a = CZ.parse_args(["--pred", "p", "--data_path", "d", "--scenes", "s", "--out", "o", "--every", "3", "--vis_size", "64", "48",
                       "--min_views", "2"])
    assert (a.out, a.every, a.vis_size, a.min_views) == ("o", 3, [64, 48], 2)
    for bad in (["--pred", "p", "--data_path", "d"], ["--pred", "p", "--data_path", "d", "--scenes", "s", "--vis_size", "64"]):
        with pytest.raises(SystemExit):
            CZ.parse_args(bad)
    from eprecon_amd import reconstruct
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o"]).color is False
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o", "--color"]).color is True


def test_scene_frames_reads_a_scene_directory(tmp_path):
    image_mod = pytest.importorskip("PIL.Image")
    from eprecon_amd import colorize as CZ
    pred, data = CC.write_disk_scene(str(tmp_path))
    root = os.path.join(data, CC.DISK_SCENE)
    bad = np.eye(4)
    bad[0, 3] = -np.inf
    np.savetxt(os.path.join(root, "pose", "pose_2.txt"), bad)          # ScanNet marks a lost frame this way
    frames, k, poses, kept = CZ.scene_frames(data, CC.DISK_SCENE, [0, 1, 2, 3])
    assert kept == [0, 1, 3] and frames.shape == (3, CC.FRAME_H, CC.FRAME_W, 3) and frames.dtype == np.uint8
    assert np.array_equal(k, RR.K_SMALL) and poses.shape == (3, 4, 4)
    assert np.allclose(poses, RR.scene24()[3][[0, 1, 3]], rtol=0, atol=1e-15)
    with image_mod.open(os.path.join(root, "color", "color_3.jpg")) as im:
        assert np.array_equal(frames[2], np.asarray(im.convert("RGB")))
    assert CZ.pose_frame_ids(root, 2) == [0, 2]
    none = CZ.scene_frames(data, CC.DISK_SCENE, [2])
    assert none[3] == [] and none[0].shape[0] == 0

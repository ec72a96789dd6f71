"""GPU: vertex colouring (eprecon_amd/colorize.py, csrc/mesh_colorize.hip) against the float64 restatement
tests/colorize_ref.py outside the vertices that leaves out, on hand-built visibility words and vertex placements, bit for
bit across runs and splits of the views, at its edges and errors, end to end on the analytic room and on disk."""
import os

import numpy as np
import pytest

import colorize_cases as CC
import colorize_ref as CR
import render_ref as RR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

UNDECIDED_CAP = 0.01
ACC_RTOL = 1e-12


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def words_to_device(vis):
    return dev(np.asarray(vis, np.uint64).view(np.int64))


def words_to_host(vis):
    return vis.view(torch.int64).cpu().numpy().view(np.uint64)


def check_against_restatement(col, ref, min_views=1, fallback=(153, 153, 153)):
    rgb, seen = col.colors(min_views=min_views, fallback=fallback)
    assert ref["undecided"].mean() <= UNDECIDED_CAP
    ok = ~ref["undecided"]
    assert np.array_equal(seen.cpu().numpy()[ok], ref["seen"][ok])
    acc = col.acc.cpu().numpy()
    assert np.all(np.abs(acc[ok] - ref["acc"][ok]) <= ACC_RTOL * np.abs(ref["acc"][ok]))
    assert np.array_equal(rgb.cpu().numpy()[ok], ref["rgb"][ok])


@pytest.fixture(scope="module")
def small_cases():
    return CC.small_cases()


@pytest.mark.parametrize("size", CC.VIS_SIZES)
def test_small_fixtures_against_the_restatement(small_cases, size):
    from eprecon_amd import colorize as CZ
    from eprecon_amd import render as RD
    coloured = 0
    for name, verts, faces, poses in small_cases:
        frames = CC.seeded_frames(len(poses))
        col = CZ.MeshColorizer(dev(verts), dev(faces), vis_size=size)
        col.integrate(frames, RR.K_SMALL, poses)
        k_vis = RD.scaled_intrinsics(RR.K_SMALL, size, native=(CC.FRAME_W, CC.FRAME_H))
        assert np.array_equal(k_vis, CC.vis_intrinsics(RR.K_SMALL, size, (CC.FRAME_W, CC.FRAME_H)))
        vis = words_to_host(RD.visibility(col.verts, col.faces, k_vis, poses, size[1], size[0]))
        ref = CR.colorize(verts, faces, RR.K_SMALL, k_vis, poses, frames, vis)
        check_against_restatement(col, ref)
        coloured += int((ref["seen"] > 0).sum())
    assert coloured > 400


def hand_mesh():
    """vertices 0-2: a large face in the plane z = 2 that faces a camera at the origin; face 1 has a corner out of range,
    face 2 two equal corners; the other vertices belong to no face"""
    verts = [[-4, -3, 2], [4, -3, 2], [-4, 5, 2]]
    faces = np.array([[0, 2, 1], [0, 1, 99], [0, 0, 1]], np.int32)
    return verts, faces


def test_hand_built_visibility_words():
    """seven loose vertices in the plane z = 2, each on a pixel of its own whose word is built by hand"""
    from eprecon_amd import colorize as CZ
    verts, faces = hand_mesh()
    xs = [-0.8, -0.55, -0.3, -0.05, 0.2, 0.45, 0.7]
    verts = np.array(verts + [[x, 0.13, 2] for x in xs], np.float32)
    frames = CC.seeded_frames(1)
    k = RR.K_SMALL
    inf = 0xFFFFFFFFFFFFFFFF
    word = lambda depth, face: int(CR.pack_visibility(np.array([depth]), np.array([face]))[0])
    cases = [(inf, 0),                 # no hit
             (word(2.0, 7), 0),        # a face index past the mesh
             (word(2.0, 1), 0),        # a face with a corner out of range
             (word(2.0, 2), 0),        # a degenerate face
             (word(2.0, 0), 1),        # the face, at the vertex's depth
             (word(1.5, 0), 0),        # a surface half a metre nearer: hidden
             (word(5.0, 0), 1)]        # a surface behind the vertex
    vis = np.full((1, CC.FRAME_H, CC.FRAME_W), np.uint64(inf))
    for x, (w, _) in zip(xs, cases):
        c, r = int(np.floor(k[0, 0] * x / 2 + k[0, 2])), int(np.floor(k[1, 1] * 0.13 / 2 + k[1, 2]))
        assert vis[0, r, c] == np.uint64(inf)          # a pixel of its own
        vis[0, r, c] = np.uint64(w)
    col = CZ.MeshColorizer(dev(verts), dev(faces))
    col.accumulate(dev(frames), words_to_device(vis), k, k, np.eye(4)[None])
    ref = CR.colorize(verts, faces, k, k, np.eye(4)[None], frames, vis)
    assert not ref["undecided"].any()
    assert list(ref["seen"][3:]) == [want for _, want in cases] and not ref["seen"][:3].any()
    check_against_restatement(col, ref)
    rgb = col.colors()[0].cpu().numpy()
    assert (rgb[ref["seen"] == 0] == 153).all() and (col.acc.cpu().numpy()[ref["seen"] == 0] == 0).all()


def test_vertex_placement_and_the_last_column_and_row():
    """dyadic intrinsics for this case only: the vertex (63/32, 47/32, 2) projects to (63.5, 47.5) exactly, x = 63 and
    y = 47 are the last column and row, x0 and y0 are clamped to 62 and 46 with fx = fy = 1: the bytes of pixel (47, 63)"""
    from eprecon_amd import colorize as CZ
    k = np.array([[32.0, 0, 32.0], [0, 32.0, 24.0], [0, 0, 1]])
    base, faces = hand_mesh()
    loose = [[63 / 32, 47 / 32, 2],       # exactly on the last column and row
             [0.3, 0.2, -1.0],            # behind the camera
             [0.3, 0.2, 12.0],            # beyond zfar = 10
             [-6.0, 0.2, 2.0],            # left of the frame by a clear margin
             [0.3, 4.5, 2.0],             # below it
             [0.3, 0.2, 2.0]]             # inside
    verts = np.array(base + loose, np.float32)
    frames = CC.seeded_frames(1, seed=9)
    vis = CR.pack_visibility(np.full((1, CC.FRAME_H, CC.FRAME_W), 50.0), np.zeros((1, CC.FRAME_H, CC.FRAME_W), np.int64))
    col = CZ.MeshColorizer(dev(verts), dev(faces), zfar=10.0)
    col.accumulate(dev(frames), words_to_device(vis), k, k, np.eye(4)[None])
    rgb, seen = (t.cpu().numpy() for t in col.colors())
    assert list(seen[3:]) == [1, 0, 0, 0, 0, 1]
    assert tuple(rgb[3]) == tuple(frames[0, 47, 63])
    ref = CR.colorize(verts, faces, k, k, np.eye(4)[None], frames, vis, zfar=10.0)
    assert np.array_equal(seen, ref["seen"]) and np.array_equal(rgb, ref["rgb"])
    assert np.all(np.abs(col.acc.cpu().numpy() - ref["acc"]) <= ACC_RTOL * np.abs(ref["acc"]))


def test_bit_identical_across_runs_and_splits(small_cases):
    from eprecon_amd import colorize as CZ
    _, verts, faces, poses = small_cases[-1]          # the patch of one vertex more than a workgroup, four views
    frames = CC.seeded_frames(len(poses))
    run = lambda: CZ.MeshColorizer(dev(verts), dev(faces), vis_size=(64, 48))
    whole, again, split = run().integrate(frames, RR.K_SMALL, poses), run().integrate(dev(frames), RR.K_SMALL, poses), run()
    split.integrate(frames[:2], RR.K_SMALL, poses[:2])
    split.integrate(frames[2:], RR.K_SMALL, poses[2:])
    assert int((whole.seen > 1).sum()) > 100          # sums of several views, so that their order could show
    for other in (again, split):
        assert torch.equal(whole.acc, other.acc) and torch.equal(whole.seen, other.seen)
    # 70 views in one call run as two launches (64 + 6): the same chain as one view at a time
    many_f, many_p = np.concatenate([frames] * 18)[:70], np.concatenate([poses] * 18)[:70]
    one, each = run().integrate(many_f, RR.K_SMALL, many_p), run()
    for i in range(70):
        each.integrate(many_f[i:i + 1], RR.K_SMALL, many_p[i:i + 1])
    assert torch.equal(one.acc, each.acc) and torch.equal(one.seen, each.seen) and int(one.seen.max()) > 40


def test_empty_meshes_and_chunks_that_see_nothing(small_cases):
    from eprecon_amd import colorize as CZ
    _, verts, faces, poses = small_cases[3]
    frames = CC.seeded_frames(len(poses))
    # N = 0
    col = CZ.MeshColorizer(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    col.integrate(frames, RR.K_SMALL, poses)
    rgb, seen = col.colors()
    assert tuple(rgb.shape) == (0, 3) and seen.numel() == 0 and col.acc.numel() == 0
    # M = 0: vertices without a face see nothing; the state keeps the bits it had
    for f, p in ((np.zeros((0, 3), np.int32), poses), (faces, poses[3:])):          # (poses[3]: the patch is behind the camera)
        col = CZ.MeshColorizer(dev(verts), dev(f), vis_size=(32, 24))
        col.acc.fill_(7.25)
        col.seen.fill_(3)
        col.integrate(frames[:len(p)], RR.K_SMALL, p)
        assert bool((col.acc == 7.25).all()) and bool((col.seen == 3).all())
    # no view: nothing runs
    col.integrate(frames[:0], RR.K_SMALL, poses[:0])
    assert bool((col.acc == 7.25).all())


def test_min_views_and_fallback(small_cases):
    from eprecon_amd import colorize as CZ
    _, verts, faces, poses = small_cases[-1]
    col = CZ.MeshColorizer(dev(verts), dev(faces), vis_size=(64, 48)).integrate(CC.seeded_frames(len(poses)), RR.K_SMALL, poses)
    rgb1, seen = (t.cpu().numpy() for t in col.colors())
    rgb3 = col.colors(min_views=3, fallback=(1, 2, 3))[0].cpu().numpy()
    assert (seen >= 3).any() and (seen == 0).any() and ((seen > 0) & (seen < 3)).any()
    assert np.array_equal(rgb3[seen >= 3], rgb1[seen >= 3]) and (rgb3[seen < 3] == [1, 2, 3]).all()
    assert (rgb1[seen == 0] == 153).all()
    acc = col.acc.cpu().numpy()
    want = np.minimum(255.0, np.floor(acc[:, :3] / np.where(acc[:, 3:] > 0, acc[:, 3:], 1.0) + 0.5))
    assert np.array_equal(rgb1[seen > 0], want[seen > 0].astype(np.uint8))


def test_errors(small_cases):
    import ctypes
    from eprecon_amd import _lib
    from eprecon_amd import colorize as CZ
    _, verts, faces, poses = small_cases[2]
    frames = CC.seeded_frames(len(poses))
    with pytest.raises(_lib.EpreconError):
        CZ.MeshColorizer(torch.from_numpy(verts), torch.from_numpy(faces))
    col = CZ.MeshColorizer(dev(verts), dev(faces), vis_size=(32, 24))
    with pytest.raises(ValueError):
        col.integrate(frames, RR.K_SMALL, poses[:2])
    with pytest.raises(ValueError):
        col.integrate(frames.astype(np.float32), RR.K_SMALL, poses)
    with pytest.raises(ValueError):
        col.integrate(frames[..., :2], RR.K_SMALL, poses)
    # the entries: argument rules are a status, never a fault; no vertex or no view is a no-op even without buffers
    lib = _lib.load()
    st = _lib.current_stream()
    acc = lambda nv, nviews, hc, wc, tol=0.04, cos=0.1: lib.eprecon_colorize_accumulate_async(
        None, nv, None, 0, None, nviews, None, hc, wc, None, 24, 32, 0.5, 0.05, 100.0, tol, cos, None, None, st)
    assert acc(0, 3, 48, 64) == 0 and acc(5, 0, 48, 64) == 0
    for bad in (acc(5, 3, 48, 64), acc(5, 3, 1, 64), acc(5, 3, 48, 1), acc(-1, 3, 48, 64), acc(5, 3, 48, 64, tol=-1.0),
                acc(5, 3, 48, 64, cos=1.5)):
        assert bad != 0
    assert lib.eprecon_colorize_finish_async(None, None, 0, 1, 0, 0, 0, None, st) == 0
    assert lib.eprecon_colorize_finish_async(None, None, 4, 1, 0, 0, 0, None, st) != 0
    assert lib.eprecon_colorize_finish_async(ctypes.c_void_p(256), ctypes.c_void_p(256), 4, 1, 0, 256, 0, ctypes.c_void_p(256), st) != 0
    assert not col.acc.any()


def test_analytic_room_end_to_end():
    """the mesh of the analytic room coloured from its own painted views: every vertex seen is within the restatement's
    worst error (on the same frames and buffers) plus one level for the final rounding of the colour function there"""
    from eprecon_amd import colorize as CZ
    from eprecon_amd import render as RD
    from eprecon_amd.save_scene import tsdf2mesh
    scene = CC.analytic_scene()
    mesh = tsdf2mesh(scene["voxel"], scene["origin"], dev(scene["tsdf"]))
    rule = dict(vis_size=CC.SCENE_VIS_SIZE, tolerance=scene["voxel"], pixel_center=0.0)
    out = CZ.colorize_mesh(mesh, scene["frames"], scene["k"], scene["poses"], chunk=2, **rule)
    verts, faces = mesh["vertices"], mesh["faces"]
    assert out["vertex_colors"].shape == (len(verts), 3) and out["vertex_normals"] is mesh["vertex_normals"]
    w, h = CC.SCENE_VIS_SIZE
    k_vis = RD.scaled_intrinsics(scene["k"], (w, h), native=(320, 240))
    vis = words_to_host(RD.visibility(dev(verts), dev(faces), k_vis, scene["poses"], h, w, pixel_center=0.0))
    ref = CR.colorize(verts, faces, scene["k"], k_vis, scene["poses"], scene["frames"], vis, pixel_center=0.0,
                      tolerance=scene["voxel"])
    worst, share = CC.scene_error(verts, ref)
    bound = worst + 1.0
    seen = out["vertex_seen"] >= 1
    err = np.abs(out["vertex_colors"][seen].astype(np.float64) - CC.colour_of(verts.astype(np.float64)[seen]))
    print(f"analytic room: {len(verts)} vertices, {100 * seen.mean():.1f} % seen, bound {bound:.2f}, worst {err.max():.2f}, "
          f"median {np.median(err.max(1)):.2f} levels")
    assert share >= 0.5 and seen.mean() >= 0.5
    assert err.max() <= bound
    assert np.median(err.max(1)) < 1.5
    ok = ~ref["undecided"]
    assert ref["undecided"].mean() <= UNDECIDED_CAP
    assert np.array_equal(out["vertex_seen"][ok], ref["seen"][ok]) and np.array_equal(out["vertex_colors"][ok], ref["rgb"][ok])


def read_export_ply(path):
    """the binary layout save_scene.export_ply writes -> (header lines, vertex records, faces int32[M,3])"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in head if l.startswith("property") and "list" not in l]
    dtype = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[t]) for t, name in props])
    vert = np.frombuffer(data, dtype, nv, end)
    face = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, end + nv * dtype.itemsize)
    assert end + nv * dtype.itemsize + nf * 13 == len(data) and (face["n"] == 3).all()
    return head, vert, face["v"]


def test_cli_writes_the_coloured_scene(tmp_path, capsys):
    pytest.importorskip("PIL")
    from eprecon_amd import colorize as CZ
    from eprecon_amd import render as RD
    pred, data = CC.write_disk_scene(str(tmp_path))
    scenes = tmp_path / "scenes.txt"
    scenes.write_text(CC.DISK_SCENE + "\n")
    out = str(tmp_path / "out")
    assert CZ.main(["--pred", pred, "--data_path", data, "--scenes", str(scenes), "--out", out, "--every", "1", "--vis_size", "64",
                    "48"]) == 0
    assert "% seen" in capsys.readouterr().out
    head, vert, face = read_export_ply(os.path.join(out, f"mesh_color_{CC.DISK_SCENE}.ply"))
    assert [l.split()[-1] for l in head if l.startswith("property") and "list" not in l] == [
        "x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    npz = os.path.join(pred, CC.DISK_SCENE + ".npz")
    verts, faces, _, _ = (t.cpu().numpy() for t in RD.scene_mesh(npz))
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), verts) and np.array_equal(face, faces)
    mesh = CZ.colorize_scene(npz, data, CC.DISK_SCENE, every=1, vis_size=(64, 48))
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), mesh["vertex_colors"])
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), mesh["vertex_normals"])
    assert (mesh["vertex_seen"] > 0).mean() > 0.5 and len(np.unique(mesh["vertex_colors"], axis=0)) > 100
    # chunks of one frame and chunks of all give the same mesh; the tolerance is the file's voxel size
    again = CZ.colorize_scene(npz, data, CC.DISK_SCENE, ids=[0, 1, 2, 3], chunk=1, vis_size=(64, 48), tolerance=RR.VOXEL)
    assert np.array_equal(again["vertex_colors"], mesh["vertex_colors"]) and np.array_equal(again["vertex_seen"], mesh["vertex_seen"])


def test_reconstruct_color_adds_one_file_and_changes_none(tmp_path, capsys):
    pytest.importorskip("PIL")
    from test_reconstruct_gpu import HEIGHT, SCENE, WIDTH, write_scene
    from eprecon_amd import reconstruct
    root = str(tmp_path / "data")
    write_scene(root)
    files = {}
    for name, extra in (("plain", []), ("color", ["--color"])):
        out = str(tmp_path / name)
        assert reconstruct.main(["--data_path", root, "--out", out, "--size", str(WIDTH), str(HEIGHT)] + extra) == 0
        d = os.path.join(out, "scene_scannet_fusion_eval_0")
        files[name] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    coloured = f"mesh_color_{SCENE}.ply"
    assert sorted(files["color"]) == sorted(list(files["plain"]) + [coloured])
    assert {SCENE + ".npz", SCENE + ".ply", f"mesh_semantic_{SCENE}.ply", f"mesh_instance_{SCENE}.ply"} == set(files["plain"])
    for f, data in files["plain"].items():
        assert files["color"][f] == data, f
    d = os.path.join(str(tmp_path / "color"), "scene_scannet_fusion_eval_0")
    _, vert, face = read_export_ply(os.path.join(d, coloured))
    _, plain_vert, plain_face = read_export_ply(os.path.join(d, SCENE + ".ply"))
    assert len(vert) == len(plain_vert) > 0 and np.array_equal(face, plain_face)
    assert np.array_equal(vert["x"], plain_vert["x"]) and "red" in vert.dtype.names
    assert "of the vertices coloured" in capsys.readouterr().out

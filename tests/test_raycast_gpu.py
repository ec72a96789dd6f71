"""GPU: eprecon_amd.raycast (csrc/tsdf_raycast.hip) against tests/raycast_ref.py on the views of tests/raycast_fixtures.py — hit,
row, depth, normal, labels and shading — at the image, scene and build edges, bit-identical across runs and splits, on saved
files and through the command line, and against marching cubes + the rasteriser as a second witness of the same surface.

Tolerances: 4 x the distance of the reference's own float32 twin from float64 (raycast_fixtures.TWIN_*, measured and bounded by
tests/test_raycast_host.py), below the ceilings of 1e-3 cell and 1e-3 per normal component."""
import os

import numpy as np
import pytest

import raycast_fixtures as FX
import raycast_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEPTH_TOL_CELLS, NORMAL_TOL = 4 * FX.TWIN_DEPTH, 4 * FX.TWIN_NORMAL
assert DEPTH_TOL_CELLS <= FX.DEPTH_CEILING and NORMAL_TOL <= FX.NORMAL_CEILING


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def grid_of(scene):
    from eprecon_amd.raycast import SceneGrid
    s = scene if isinstance(scene, dict) else FX.SCENES[scene]()
    return SceneGrid(dev(s["coords"]), dev(s["tsdf"]), s["origin"], s["voxel_size"]), s


def bits(out):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v) for k, v in out.items()}


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def compare(out, refs, voxel, what, extra_mask=None):
    """a cast's images against the reference's, view by view, outside left_out -> the number of hit pixels compared"""
    n = 0
    for v, ref in enumerate(refs):
        ok = ~ref["left_out"] if extra_mask is None else ~(ref["left_out"] | extra_mask[v])
        row, depth, normal = host(out["row"][v]), host(out["depth"][v]), host(out["normal"][v])
        assert np.array_equal((row >= 0)[ok], (ref["row"] >= 0)[ok]), (what, v, "hit")
        assert np.array_equal(row[ok], ref["row"][ok]), (what, v, "row")
        err_d = np.abs(depth.astype(np.float64) - ref["depth"])[ok].max(initial=0.0) / voxel
        err_n = np.abs(normal.astype(np.float64) - ref["normal"])[ok].max(initial=0.0)
        print(f"[raycast] {what} view {v}: depth {err_d:.3e} cells, normal {err_n:.3e}")
        assert err_d <= DEPTH_TOL_CELLS, (what, v, err_d)
        assert err_n <= NORMAL_TOL, (what, v, err_n)
        assert (depth[row < 0] == 0).all() and (normal[row < 0] == 0).all()
        n += int((ok & (ref["row"] >= 0)).sum())
    return n


@pytest.mark.parametrize("case", list(FX.CASES))
def test_matches_the_reference(case):
    from eprecon_amd import raycast as RC
    scene, k, poses, h, w = FX.CASES[case]
    grid, s = grid_of(scene)
    refs = FX.reference(case)
    out = RC.raycast(grid, k, np.stack(poses), h, w)
    assert out["depth"].shape == (len(poses), h, w) and out["normal"].shape == (len(poses), h, w, 3) and out["row"].dtype == torch.int32
    assert compare(out, refs, s["voxel_size"], case) >= 1
    # labels: sem[row], ins[row] of the reference, backgrounds where nothing is hit
    sem, ins = RC.raycast_labels(grid, out, dev(s["semantic"]), dev(s["instance"]), backgrounds=(0, 255))
    colors = np.stack([40 + 20 * s["semantic"] % 200, 250 - 9 * s["instance"] % 230, np.full(len(s["semantic"]), 181)], 1).astype(np.uint8)
    rgb = RC.raycast_shaded(grid, out, k, np.stack(poses), colors=dev(colors))
    grey = RC.raycast_shaded(grid, out, k, np.stack(poses), ambient=0.45, background_rgb=(3, 2, 1))
    for v, ref in enumerate(refs):
        ok, hit = ~ref["left_out"], ref["row"] >= 0
        assert np.array_equal(host(sem[v])[ok], np.where(hit, s["semantic"][np.maximum(ref["row"], 0)], 0)[ok])
        assert np.array_equal(host(ins[v])[ok], np.where(hit, s["instance"][np.maximum(ref["row"], 0)], 255)[ok])
        for image, kwargs in ((rgb, {"colors": colors}), (grey, {"ambient": 0.45, "background": (3, 2, 1)})):
            want, near = R.flat_shade(ref["normal"], ref["row"], k, poses[v], **kwargs)
            assert (ref["left_out"] | near).mean() <= FX.LEFT_OUT_CAP
            keep = ok & ~near
            assert np.array_equal(host(image[v])[keep], want[keep]), (case, v)


def test_views_in_one_call_in_three_and_twice():
    from eprecon_amd import raycast as RC
    _, k, poses, h, w = FX.CASES["sphere"]
    grid, _ = grid_of("sphere")
    poses = np.stack(poses)
    whole = RC.raycast(grid, k, poses, h, w)
    again = RC.raycast(grid, k, poses, h, w)
    assert same_bits(whole, again)
    parts = [RC.raycast(grid, k, poses[v:v + 1], h, w) for v in range(3)]
    assert same_bits(whole, {key: torch.cat([p[key] for p in parts]) for key in whole})
    other, _ = grid_of("sphere")                       # a second build of the same rows
    assert same_bits(whole, RC.raycast(other, k, poses, h, w))
    # refine = 0 is the first interpolation alone; more steps only move the depth inside the hit segment
    r0, r4 = RC.raycast(grid, k, poses[:1], h, w, refine=0), RC.raycast(grid, k, poses[:1], h, w, refine=4)
    assert torch.equal(r0["row"] >= 0, r4["row"] >= 0) and (r0["depth"] - r4["depth"]).abs().max() < FX.VOXEL


def test_scene_edges_without_a_surface():
    from eprecon_amd import raycast as RC
    _, k, poses, h, w = FX.CASES["sphere"]
    empty = RC.SceneGrid(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), torch.zeros(0, device="cuda"), FX.ORIGIN, FX.VOXEL)
    s = FX.sphere()
    positive = RC.SceneGrid(dev(s["coords"]), dev(np.abs(s["tsdf"]) + 0.01), s["origin"], s["voxel_size"])
    assert not empty.active and not positive.active
    for grid in (empty, positive):
        out = RC.raycast(grid, k, np.stack(poses), h, w)
        assert out["depth"].shape == (3, h, w) and not out["depth"].any() and not out["normal"].any() and (out["row"] == -1).all()
    sem, ins = RC.raycast_labels(empty, out, torch.zeros(0, dtype=torch.int32, device="cuda"),
                                 torch.zeros(0, dtype=torch.int32, device="cuda"), backgrounds=(4, 5))
    assert (sem == 4).all() and (ins == 5).all()
    assert (RC.raycast_shaded(empty, out, k, np.stack(poses)) == 255).all()


def test_a_single_non_positive_row():
    from eprecon_amd import raycast as RC
    scene = {"coords": np.array([[5, 6, 7], [20, 3, 1]], np.int32), "tsdf": np.array([-0.3, 0.4], np.float32),
             "origin": FX.ORIGIN, "voxel_size": FX.VOXEL}
    grid, _ = grid_of(scene)
    assert grid.box == ((4, 5, 6), (5, 6, 7))
    k, pose, h, w = FX.intrinsics(32, 24, 601.3), FX.look_at(FX.world([-6.7, 1.4, 12.2]), FX.world([5.1, 6.05, 6.9])), 24, 32
    ref = R.cast_view(R.row_dict(scene["coords"], scene["tsdf"]), k, pose, h, w, FX.ORIGIN, FX.VOXEL)
    assert ref["left_out"].mean() <= FX.LEFT_OUT_CAP and (ref["row"] == 0).sum() > 50 and (ref["row"] == -1).any()
    assert compare(RC.raycast(grid, k, pose[None], h, w), [ref], FX.VOXEL, "single row") > 50


def test_shifted_sphere_gives_the_same_pictures():
    from eprecon_amd import raycast as RC
    _, k, poses, h, w = FX.CASES["sphere_shifted"]
    a = RC.raycast(grid_of("sphere")[0], k, np.stack(poses), h, w)
    b = RC.raycast(grid_of("sphere_shifted")[0], k, np.stack(poses), h, w)
    ok = ~(FX.reference("sphere")[0]["left_out"] | FX.reference("sphere_shifted")[0]["left_out"])
    ra, rb = host(a["row"][0]), host(b["row"][0])
    assert np.array_equal(ra[ok], rb[ok]) and (ra[ok] >= 0).sum() > 500
    assert np.abs(host(a["depth"][0]) - host(b["depth"][0]))[ok].max() / FX.VOXEL <= DEPTH_TOL_CELLS
    assert np.abs(host(a["normal"][0]) - host(b["normal"][0]))[ok].max() <= NORMAL_TOL


@pytest.mark.parametrize("axis,sign", [(0, 1), (1, -1), (2, 1)])
def test_cameras_along_an_axis_return(axis, sign):
    """the centre ray has two direction components that are exactly zero, the centre row and column one: ties everywhere
    (nothing is compared with the reference), but the walk ends inside its bounds and sees the sphere"""
    from eprecon_amd import raycast as RC
    grid, _ = grid_of("sphere")
    z = np.zeros(3)
    z[axis] = sign
    x = np.zeros(3)
    x[(axis + 1) % 3] = 1.0
    pose = np.eye(4)
    pose[:3, :3] = np.stack([x, np.cross(z, x), z], 1)
    eye, voxel = np.array([11.0, 12.0, 11.0]), 0.25
    eye[axis] -= sign * 30.0
    pose[:3, 3] = eye * voxel                               # integer lattice coordinates (origin 0, a binary voxel size)
    flat = RC.SceneGrid(grid.coords, grid.tsdf, np.zeros(3), voxel)
    k = np.array([[50.0, 0.0, 4.0], [0.0, 50.0, 4.0], [0.0, 0.0, 1.0]])
    out = RC.raycast(flat, k, pose[None], 8, 8, pixel_center=0.0)         # raises on a status word
    depth = host(out["depth"][0])
    assert np.isfinite(depth).all() and (host(out["row"][0]) >= 0).sum() >= 32
    hit = depth[depth > 0]
    assert hit.min() > 15 * voxel and hit.max() < 45 * voxel


def test_errors():
    from eprecon_amd import raycast as RC
    from eprecon_amd._lib import EpreconError
    s = FX.sphere()
    with pytest.raises(EpreconError):
        RC.SceneGrid(torch.from_numpy(s["coords"]), torch.from_numpy(s["tsdf"]), s["origin"], s["voxel_size"])
    with pytest.raises(ValueError):
        RC.SceneGrid(dev(s["coords"]), dev(s["tsdf"][:-1]), s["origin"], s["voxel_size"])
    grid, _ = grid_of("sphere")
    _, k, poses, h, w = FX.CASES["sphere"]
    bad = np.array(k)
    bad[2] = [0.0, 1e-3, 1.0]
    with pytest.raises(EpreconError):
        RC.raycast(grid, bad, np.stack(poses), h, w)
    with pytest.raises(EpreconError):           # a coordinate the hash key cannot hold
        RC.SceneGrid(dev(np.array([[1 << 19, 0, 0]], np.int32)), dev(np.array([-0.5], np.float32)), s["origin"], s["voxel_size"])
    with pytest.raises(EpreconError):           # ... nor its neighbour, which a cast would look up
        RC.SceneGrid(dev(np.array([[0, (1 << 19) - 2, 0]], np.int32)), dev(np.array([0.5], np.float32)), s["origin"], s["voxel_size"])


def test_second_witness_marching_cubes_and_the_rasteriser():
    """two surface finders that share no kernel, on the same volume: both cut the same cells, so along a ray they differ by at
    most the ray's path through one cell — asserted as 2 voxel sizes, on the pixels that hit in both with all 8 neighbours"""
    from eprecon_amd import raycast as RC, render as RD
    from eprecon_amd.save_scene import marching_cubes
    from eprecon_amd.scene_io import scatter_volumes
    grid, s = grid_of("sphere")
    h, w = 96, 128
    k, poses = FX.intrinsics(w, h, 231.7), np.stack(FX.SPHERE_POSES[:1])
    cast = host(RC.raycast(grid, k, poses, h, w)["depth"][0])
    vol = scatter_volumes(s["dims"], s["coords"], {"tsdf": s["tsdf"]}, "cuda")["tsdf"]
    verts, faces = marching_cubes(vol, 0.0)[:2]
    verts = verts * s["voxel_size"] + dev(s["origin"], torch.float32).reshape(1, 3)
    vis = RD.visibility(verts, faces, k, poses, h, w, cull_back=False)
    mesh = host(RD.resolve(vis, verts, faces, k, poses, outputs=("depth",))["depth"][0])
    both = (cast > 0) & (mesh > 0)
    interior = both.copy()
    interior[0] = interior[-1] = interior[:, 0] = interior[:, -1] = False
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior[1:-1, 1:-1] &= both[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    assert both.sum() > 3000 and interior.sum() >= 0.9 * both.sum(), (both.sum(), interior.sum())
    worst = np.abs(cast - mesh)[interior].max()
    print(f"[raycast] second witness: {interior.sum()} of {both.sum()} pixels, largest depth difference {worst / s['voxel_size']:.3f} cells")
    assert worst <= 2 * s["voxel_size"]


def _volumes(s):
    vols = []
    for key, fill, dtype in (("tsdf", 1.0, np.float32), ("semantic", 0, np.int32), ("instance", 0, np.int32)):
        vol = np.full(s["dims"], fill, dtype)
        vol[tuple(s["coords"].T)] = s[key]
        vols.append(vol)
    return vols


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    from eprecon_amd.scene_io import write_scene
    root = tmp_path_factory.mktemp("raycast_scene")
    s = FX.slab_box()
    dense, sparse = str(root / "dense" / "scene_a.npz"), str(root / "sparse" / "scene_a.npz")
    os.makedirs(os.path.dirname(dense)), os.makedirs(os.path.dirname(sparse))
    head = {"origin": s["origin"].astype(np.float32), "voxel_size": s["voxel_size"]}
    write_scene(dense, *_volumes(s), **head)
    order = np.random.default_rng(5).permutation(len(s["coords"]))           # the file order of rows does not matter
    write_scene(sparse, s["tsdf"][order], s["semantic"][order], s["instance"][order], coords=s["coords"][order],
                dims=np.array(s["dims"]), **head)
    return {"dense": dense, "sparse": sparse, "root": root}


def test_dense_and_sparse_files_give_the_same_pictures(saved):
    from eprecon_amd import raycast as RC
    _, k, poses, h, w = FX.CASES["slab_box"]
    a = RC.raycast_scene(saved["dense"], k, np.stack(poses), h, w, modes=("semantic", "instance", "shaded", "normal"))
    b = RC.raycast_scene(saved["sparse"], k, np.stack(poses), h, w, modes=("semantic", "instance", "shaded", "normal"))
    assert sorted(a) == ["depth", "instance", "instance_rgb", "normal", "normal_rgb", "row", "semantic", "semantic_rgb", "shaded_rgb"]
    assert same_bits(a, b)
    # (the file's origin is float32: the pictures are those of the fixture up to that rounding, the ids exactly off the ties)
    s, refs = FX.slab_box(), FX.reference("slab_box")
    for v, ref in enumerate(refs):
        agree = (host(a["semantic"][v]) == np.where(ref["row"] >= 0, s["semantic"][np.maximum(ref["row"], 0)], 0))
        assert agree.mean() > 0.99
    assert set(np.unique(host(a["semantic"]))) == {0, 1, 5} and set(np.unique(host(a["instance"]))) == {0, 2, 7}


def test_command_line(saved, tmp_path, capsys):
    from PIL import Image
    from eprecon_amd import raycast as RC
    data = tmp_path / "data" / "scene_a"
    os.makedirs(data / "pose"), os.makedirs(data / "intrinsic")
    k_small = FX.intrinsics(64, 48, 47.9)
    k4 = np.eye(4)
    k4[:3, :3] = k_small * [[10.0], [10.0], [1.0]]                          # of the 640 x 480 sensor
    np.savetxt(data / "intrinsic" / "intrinsic_depth.txt", k4, delimiter=" ")
    for i, pose in enumerate(FX.SLAB_POSES):
        np.savetxt(data / "pose" / f"pose_{i}.txt", pose, delimiter=" ")
    (tmp_path / "scenes.txt").write_text("scene_a\n")
    common = ["--pred", os.path.dirname(saved["sparse"]), "--data_path", str(tmp_path / "data"), "--scenes", str(tmp_path / "scenes.txt"),
              "--every", "1", "--size", "64", "48"]
    out = tmp_path / "out"
    assert RC.main(common + ["--out", str(out)]) == 0
    assert "scene_a: 2 frames" in capsys.readouterr().out
    assert sorted(os.listdir(out / "scene_a")) == sorted(f"{m}_{i}.png" for m in RC.MODES for i in (0, 1))
    ids, k, poses = RC.scene_views(str(tmp_path / "data"), "scene_a", 1, (64, 48))
    want = RC.raycast_scene(saved["sparse"], k, poses, 48, 64, modes=RC.MODES)
    for j in (0, 1):
        depth_png = np.asarray(Image.open(out / "scene_a" / f"depth_{j}.png"))
        assert depth_png.dtype == np.uint16 and depth_png.shape == (48, 64)
        metres = host(want["depth"][j]).astype(np.float64)
        assert np.array_equal(depth_png, np.floor(metres * 1000.0 + 0.5).astype(np.uint16)) and depth_png.max() > 500
        for mode in ("normal", "semantic", "instance", "shaded"):
            assert np.array_equal(np.asarray(Image.open(out / "scene_a" / f"{mode}_{j}.png")), host(want[mode + "_rgb"][j])), mode
    assert RC.main(common + ["--out", str(tmp_path / "one"), "--mode", "depth"]) == 0
    assert sorted(os.listdir(tmp_path / "one" / "scene_a")) == ["depth_0.png", "depth_1.png"]

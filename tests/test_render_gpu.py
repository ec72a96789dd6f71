"""View rendering on the GPU (csrc/mesh_render.hip through eprecon_amd/render.py) against the depth render it shares its
rasteriser with (bit for bit) and against the float64 restatement tests/render_ref.py outside the pixels that leaves out;
the pixel domain of panoptic_score against tests/panoptic_score_ref.py on the restatement's images."""
import json
import os

import numpy as np
import pytest

import panoptic_score_ref as PR
import render_ref as RR

import eprecon_amd.render as RD

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LEFT_OUT_CAP = 0.01
INF_BITS = 0x7F800000


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def gpu_render(verts, faces, poses, k=RR.K_SMALL, h=RR.H, w=RR.W, labels=(), backgrounds=(), colors=None, **raster):
    v, f = dev(verts, torch.float32), dev(faces, torch.int32)
    vis = RD.visibility(v, f, k, poses, h, w, **raster)
    out = RD.resolve(vis, v, f, k, poses, labels=[dev(a, torch.int32) for a in labels], backgrounds=backgrounds,
                     colors=None if colors is None else dev(colors), pixel_center=raster.get("pixel_center", 0.5))
    return vis, {key: ([host(x) for x in val] if key == "labels" else host(val)) for key, val in out.items()}


def compare_with_restatement(verts, faces, poses, k=RR.K_SMALL, h=RR.H, w=RR.W, labels=(), backgrounds=(), colors=None, **raster):
    """every output of resolve against the restatement outside its left-out mask, with and without vertex colours
    -> (the GPU outputs, pixels hit and compared)"""
    n_hit = 0
    for col in ([None] if colors is None else [colors, None]):
        _, got = gpu_render(verts, faces, poses, k, h, w, labels, backgrounds, col, **raster)
        for v in range(len(poses)):
            ref = RR.render_view(verts, faces, k, poses[v], h, w, labels=labels, backgrounds=backgrounds, colors=col, **raster)
            assert ref["left_out"].mean() <= LEFT_OUT_CAP
            ok = ~ref["left_out"]
            assert np.array_equal(got["face"][v][ok], ref["face"][ok]), np.argwhere(ok & (got["face"][v] != ref["face"]))[:5]
            assert np.array_equal(got["depth"][v][ok] > 0, ref["face"][ok] >= 0)                 # hit and no-hit agree
            assert np.array_equal(got["corner"][v][ok], ref["corner"][ok])
            for a, b, bg in zip(got["labels"], ref["labels"], backgrounds):
                assert np.array_equal(a[v][ok], b[ok])
                assert (a[v][ok & (ref["face"] < 0)] == bg).all()
            assert np.array_equal(got["rgb"][v][ok], ref["rgb"][ok]), np.argwhere(ok & (got["rgb"][v] != ref["rgb"]).any(-1))[:5]
            hit = ok & (ref["face"] >= 0)
            assert np.all(np.abs(got["depth"][v][hit] - ref["depth"][hit]) <= 1e-6 * ref["depth"][hit])     # fp32 rounding
            n_hit += int(hit.sum())
    return got, n_hit


@pytest.fixture(scope="module")
def fixture():
    verts, faces, poses = RR.fixture()
    sem, ins, col = RR.fixture_labels(len(verts))
    return verts, faces, poses, sem, ins, col


@pytest.mark.parametrize("cull", [True, False])
def test_depth_half_equals_render_depth_bit_for_bit(fixture, cull):
    from eprecon_amd import evaluation as E
    verts, faces, poses = fixture[:3]
    v, f = dev(verts), dev(faces)
    vis = RD.visibility(v, f, RR.K_SMALL, poses, RR.H, RR.W, cull_back=cull)
    again = RD.visibility(v, f, RR.K_SMALL, poses, RR.H, RR.W, cull_back=cull)
    assert vis.dtype == torch.uint64 and tuple(vis.shape) == (3, RR.H, RR.W)
    assert torch.equal(vis.view(torch.int64), again.view(torch.int64))                 # run-to-run bit-identical
    depth = RD.resolve(vis, v, f, RR.K_SMALL, poses, outputs=("depth",))["depth"]
    want = E.render_depth(v, f, RR.K_SMALL, poses, RR.H, RR.W, cull_back=cull)
    assert torch.equal(depth.view(torch.int32), want.view(torch.int32))
    # the raw words: upper half = the z-buffer (at or above the +inf bits where nothing is hit), lower half a face index
    words = host(vis.view(torch.int64))
    upper, lower = (words >> 32) & 0xffffffff, words & 0xffffffff
    hit = host(want) > 0
    assert np.array_equal(upper[hit], host(want.view(torch.int32))[hit].astype(np.int64))
    assert (upper[~hit] >= INF_BITS).all() and (lower[hit] < len(faces)).all()
    assert hit.any() and (~hit).any()


@pytest.mark.parametrize("cull", [True, False])
def test_fixture_matches_restatement(fixture, cull):
    verts, faces, poses, sem, ins, col = fixture
    got, n = compare_with_restatement(verts, faces, poses, labels=(sem, ins), backgrounds=(-7, 123456), colors=col, cull_back=cull)
    assert n > 2 * 4000
    assert (got["face"][2] >= 0).all() == (not cull)          # inside the closed cube: every pixel once back faces are drawn
    # other shading parameters go through as well
    v, f = dev(verts), dev(faces)
    vis = RD.visibility(v, f, RR.K_SMALL, poses[:1], RR.H, RR.W, cull_back=cull)
    rgb = host(RD.resolve(vis, v, f, RR.K_SMALL, poses[:1], colors=dev(col), ambient=0.55, background_rgb=(1, 2, 3), outputs=("rgb",))["rgb"])
    ref = RR.render_view(verts, faces, RR.K_SMALL, poses[0], RR.H, RR.W, colors=col, ambient=0.55, background_rgb=(1, 2, 3), cull_back=cull)
    assert np.array_equal(rgb[0][~ref["left_out"]], ref["rgb"][~ref["left_out"]])


def test_small_boxes_tessellated_patch():
    verts, faces = RR.patch()
    sem, ins, col = RR.fixture_labels(len(verts))
    got, n = compare_with_restatement(verts, faces, np.eye(4)[None], labels=(sem, ins), backgrounds=(0, -1), colors=col)
    assert n > 2 * 300 and len(np.unique(got["face"][got["face"] >= 0])) > 100


def test_equal_depth_goes_to_the_smallest_face_index(fixture):
    verts, faces, poses = fixture[:3]
    keep = faces[[12, 13, 4]]                               # floor (large boxes: the queue path) and a cube face
    _, base = gpu_render(verts, keep, poses[:2])
    assert all((base["face"] == i).any() for i in range(3))
    _, dup = gpu_render(verts, np.concatenate([keep, keep[:1]]), poses[:2])           # face 3 duplicates face 0
    assert np.array_equal(dup["face"], base["face"]) and not (dup["face"] == 3).any()
    # listed in another order, the smaller index of each pair still wins: faces 1 and 3, faces 0 and 4 are twins
    order = np.array([1, 0, 2, 0, 1])
    _, mixed = gpu_render(verts, keep[order], poses[:2])
    want = np.where(base["face"] < 0, -1, np.array([1, 0, 2])[np.maximum(base["face"], 0)])
    assert np.array_equal(mixed["face"], want)
    assert np.array_equal(mixed["depth"].view(np.int32), base["depth"].view(np.int32))


def test_shared_diagonal_leaves_no_gap():
    """the square of test_render_shared_edge_leaves_no_gap: two triangles whose diagonal runs through pixel centres"""
    k = np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1]])
    z = 2.0
    c0, c1, r0, r1 = 12, 52, 4, 44
    P = lambda c, r: [(c + 0.5 - 32.0) / 50.0 * z, (r + 0.5 - 24.0) / 50.0 * z, z]
    v = np.array([P(c0, r0), P(c1, r0), P(c1, r1), P(c0, r1)], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    _, got = gpu_render(v, f, np.eye(4)[None], k=k, cull_back=False)
    inner = got["face"][0][r0 + 1:r1, c0 + 1:c1]
    assert ((inner == 0) | (inner == 1)).all()
    assert (inner == 0).any() and (inner == 1).any()
    assert (got["corner"][0][r0 + 1:r1, c0 + 1:c1] >= 0).all()


def test_queue_overflow_gives_the_same_buffer(fixture):
    from eprecon_amd import _lib
    verts, faces, poses = fixture[:3]
    lib = _lib.load()
    v, f = dev(verts), dev(faces)
    want = RD.visibility(v, f, RR.K_SMALL, poses, RR.H, RR.W, cull_back=False)
    k = np.asarray(RR.K_SMALL, np.float64)
    w2c = np.linalg.inv(poses)[:, :3, :4]
    cams = dev(np.concatenate([k.ravel(), np.linalg.inv(k).ravel(), w2c.ravel()]))
    for cap in (1, 0):
        out = torch.zeros((3, RR.H, RR.W), dtype=torch.int64, device="cuda")
        n_ws = int(lib.eprecon_render_visibility_workspace_bytes(cap))
        assert n_ws == 256 + (256 if cap else 0)
        ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
        rc = lib.eprecon_render_visibility_async(_lib.ptr(v), len(verts), _lib.ptr(f), len(faces), _lib.ptr(cams), 3, RR.H, RR.W,
                                                 0.5, 0.05, 100.0, 0, _lib.ptr(out), cap, _lib.ptr(ws), ws.numel(),
                                                 _lib.current_stream())
        assert rc == 0
        assert torch.equal(out, want.view(torch.int64)), cap
    # argument checks of the entry: a workspace too small, no output buffer
    args = (_lib.ptr(v), len(verts), _lib.ptr(f), len(faces), _lib.ptr(cams), 3, RR.H, RR.W, 0.5, 0.05, 100.0, 0)
    assert lib.eprecon_render_visibility_async(*args, _lib.ptr(out), 64, _lib.ptr(ws), ws.numel(), _lib.current_stream()) == -2
    assert lib.eprecon_render_visibility_async(*args, None, 1, _lib.ptr(ws), ws.numel(), _lib.current_stream()) == -1


def test_edges_of_the_interface(fixture):
    from eprecon_amd import _lib
    verts, faces, poses, sem, ins, col = fixture
    # zero faces and zero vertices: all background; outputs that are not asked for are not produced
    v0, f0 = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    vis = RD.visibility(v0, f0, RR.K_SMALL, poses[:2], 5, 7)
    assert (vis.view(torch.int64) == -1).all()
    out = RD.resolve(vis, v0, f0, RR.K_SMALL, poses[:2], labels=(empty, empty), backgrounds=(-3, 9), background_rgb=(10, 20, 30))
    assert (out["depth"] == 0).all() and (out["face"] == -1).all() and (out["corner"] == -1).all()
    assert (out["labels"][0] == -3).all() and (out["labels"][1] == 9).all()
    assert (host(out["rgb"]) == np.array([10, 20, 30], np.uint8)).all() and out["rgb"].shape == (2, 5, 7, 3)
    only = RD.resolve(vis, v0, f0, RR.K_SMALL, poses[:2], outputs=("face",))
    assert sorted(only) == ["face", "labels"] and only["labels"] == []
    assert sorted(RD.resolve(vis, v0, f0, RR.K_SMALL, poses[:2], outputs=())) == ["labels"]
    # faces with an index out of range are not drawn, wherever they stand in the list of a face's corners
    _, want = gpu_render(verts, faces, poses, labels=(sem,), colors=col)
    bad = np.concatenate([faces, [[0, 1, len(verts)], [-1, 2, 3], [4, 2 ** 31 - 1, 5]]]).astype(np.int32)
    _, got = gpu_render(verts, bad, poses, labels=(sem,), colors=col)
    for key in ("depth", "face", "corner", "rgb"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["labels"][0], want["labels"][0])
    # a triangle crossing the near plane and reaching behind the camera keeps exact coverage, either winding
    cross = np.array([[-1.0, -0.2, -1.0], [1.0, -0.3, 3.0], [-0.5, 0.6, 2.0]], np.float32)
    for order in ([0, 1, 2], [0, 2, 1]):
        _, n = compare_with_restatement(cross, np.array([order], np.int32), np.eye(4)[None], labels=(np.array([5, 6, 7]),),
                                        backgrounds=(-1,), cull_back=False)
        assert n > 50
    # CPU tensors are refused; K must end in (0, 0, 1); a buffer of the wrong kind, labels of the wrong length
    cv, cf = torch.from_numpy(verts), torch.from_numpy(faces)
    with pytest.raises(_lib.EpreconError):
        RD.visibility(cv, cf, RR.K_SMALL, poses, RR.H, RR.W)
    v, f = dev(verts), dev(faces)
    vis = RD.visibility(v, f, RR.K_SMALL, poses, RR.H, RR.W)
    for args in ((vis.cpu(), v, f), (vis, cv, cf), (vis, v, cf)):
        with pytest.raises(_lib.EpreconError):
            RD.resolve(*args, RR.K_SMALL, poses)
    with pytest.raises(_lib.EpreconError):
        RD.resolve(vis, v, f, RR.K_SMALL, poses, labels=(torch.from_numpy(sem),))
    with pytest.raises(_lib.EpreconError):
        RD.resolve(vis, v, f, RR.K_SMALL, poses, colors=torch.from_numpy(col))
    skew = RR.K_SMALL.copy()
    skew[2, 0] = 1e-3
    with pytest.raises(_lib.EpreconError):
        RD.visibility(v, f, skew, poses, RR.H, RR.W)
    with pytest.raises(ValueError):
        RD.resolve(vis.view(torch.int64).to(torch.int32), v, f, RR.K_SMALL, poses)
    with pytest.raises(ValueError):
        RD.resolve(vis, v, f, RR.K_SMALL, poses, labels=(dev(sem[:5]),))
    with pytest.raises(ValueError):
        RD.resolve(vis, v, f, RR.K_SMALL, poses[:2])


def test_conveniences_on_mesh_dicts_and_ply_files(fixture, tmp_path):
    from eprecon_amd.save_scene import export_ply
    verts, faces, poses, sem, ins, col = fixture
    _, want = gpu_render(verts, faces, poses, labels=(sem, ins), colors=col)
    mesh = {"vertices": verts, "faces": faces, "vertex_normals": np.zeros_like(verts)}
    got = RD.render_labels(dict(mesh, vertex_semantic=sem, vertex_instance=ins), RR.K_SMALL, poses, RR.H, RR.W)
    assert sorted(got) == ["corner", "depth", "face", "labels"] and len(got["labels"]) == 2
    for key in ("depth", "face", "corner"):
        assert np.array_equal(host(got[key]), want[key]), key
    assert all(np.array_equal(host(a), b) for a, b in zip(got["labels"], want["labels"]))
    only = RD.render_labels(dict(mesh, vertex_instance=ins), RR.K_SMALL, poses, RR.H, RR.W, backgrounds=(-1,))
    assert len(only["labels"]) == 1
    assert np.array_equal(host(only["labels"][0]), np.where(want["face"] < 0, -1, want["labels"][1]))
    assert np.array_equal(host(RD.render_shaded(dict(mesh, vertex_colors=col), RR.K_SMALL, poses, RR.H, RR.W)), want["rgb"])
    # from a file: the geometry only; labels and colours are given
    path = str(tmp_path / "mesh.ply")
    export_ply(mesh, path)
    from_file = RD.render_labels(path, RR.K_SMALL, poses, RR.H, RR.W, labels=(sem,))
    assert np.array_equal(host(from_file["face"]), want["face"]) and np.array_equal(host(from_file["labels"][0]), want["labels"][0])
    assert np.array_equal(host(RD.render_shaded(path, RR.K_SMALL, poses, RR.H, RR.W, colors=col)), want["rgb"])
    _, grey = gpu_render(verts, faces, poses, cull_back=False)
    assert np.array_equal(host(RD.render_shaded(path, RR.K_SMALL, poses, RR.H, RR.W, cull_back=False)), grey["rgb"])


# ------------------------------------------------------------------------------------------------------- the small scene

@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the analytic 24^3 scene saved in both forms, its device mesh on the host, and the restatement of all four views"""
    root = tmp_path_factory.mktemp("render_scene")
    tsdf, sem, ins, poses = RR.scene24()
    dense, sparse = str(root / "dense" / "scene_a.npz"), str(root / "sparse" / "scene_a.npz")
    os.makedirs(os.path.dirname(dense)), os.makedirs(os.path.dirname(sparse))
    np.savez_compressed(dense, origin=RR.ORIGIN, voxel_size=RR.VOXEL, tsdf=tsdf, semantic=sem, instance=ins)
    rows = np.argwhere(tsdf != 1.0)
    pick = lambda vol: vol[rows[:, 0], rows[:, 1], rows[:, 2]]
    np.savez_compressed(sparse, origin=RR.ORIGIN, voxel_size=RR.VOXEL, dims=np.array(tsdf.shape), sparse_coords=rows.astype(np.int32),
                        sparse_tsdf=pick(tsdf), sparse_semantic=pick(sem), sparse_instance=pick(ins))
    verts, faces, vsem, vins = (host(t) for t in RD.scene_mesh(dense))
    assert len(faces) > 1000 and set(np.unique(vsem)) >= {1, 5, 13}
    return {"root": root, "dense": dense, "sparse": sparse, "poses": poses, "verts": verts, "faces": faces, "vsem": vsem, "vins": vins}


def test_render_scene_on_both_saved_forms(scene):
    from eprecon_amd.save_scene import COLOR_PALETTE
    a = RD.render_scene(scene["dense"], RR.K_SMALL, scene["poses"], RR.H, RR.W)
    b = RD.render_scene(scene["sparse"], RR.K_SMALL, scene["poses"], RR.H, RR.W)
    assert sorted(a) == sorted(b) == ["depth", "face", "instance", "instance_rgb", "semantic", "semantic_rgb", "shaded_rgb"]
    for key in a:
        assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                           b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), key
    verts, faces, vsem, vins = (scene[k] for k in ("verts", "faces", "vsem", "vins"))
    palettes = {"semantic_rgb": COLOR_PALETTE[vsem.astype(np.int64) % len(COLOR_PALETTE)],
                "instance_rgb": COLOR_PALETTE[vins.astype(np.int64) % len(COLOR_PALETTE)], "shaded_rgb": None}
    n_hit = 0
    for v in range(len(scene["poses"])):
        for key, colors in palettes.items():
            ref = RR.render_view(verts, faces, RR.K_SMALL, scene["poses"][v], RR.H, RR.W, labels=(vsem, vins), colors=colors)
            assert ref["left_out"].mean() <= LEFT_OUT_CAP
            ok = ~ref["left_out"]
            assert np.array_equal(host(a[key])[v][ok], ref["rgb"][ok]), (v, key)
        assert np.array_equal(host(a["face"])[v][ok], ref["face"][ok])
        assert np.array_equal(host(a["semantic"])[v][ok], ref["labels"][0][ok])
        assert np.array_equal(host(a["instance"])[v][ok], ref["labels"][1][ok])
        n_hit += int((ok & (ref["face"] >= 0)).sum())
    assert n_hit > 3000
    only = RD.render_scene(scene["dense"], RR.K_SMALL, scene["poses"][:1], RR.H, RR.W, modes=("instance",))
    assert sorted(only) == ["depth", "face", "instance", "instance_rgb", "semantic"]
    assert torch.equal(only["instance_rgb"], a["instance_rgb"][:1])


def _ground_truth(scene, name, verts, faces, sem_ids, ins_ids):
    """a mesh as <name>_vh_clean_2.ply with ScanNet ids at its vertices in the three label files"""
    from eprecon_amd.save_scene import export_ply
    root = scene["root"]
    os.makedirs(root / "gt_mesh", exist_ok=True), os.makedirs(root / "info", exist_ok=True)
    export_ply({"vertices": verts, "faces": faces, "vertex_normals": np.zeros_like(verts)}, str(root / "gt_mesh" / f"{name}_vh_clean_2.ply"))
    np.save(root / "info" / f"{name}_vert.npy", verts)
    np.save(root / "info" / f"{name}_sem_label.npy", sem_ids)
    np.save(root / "info" / f"{name}_ins_label.npy", ins_ids)
    return str(root / "gt_mesh" / f"{name}_vh_clean_2.ply"), str(root / "info")


def _pixel_sites(scene, gt_verts, gt_faces, sem_ids, ins_ids, views):
    """the restatement's label images of both meshes -> (predicted, ground-truth) site labels of panoptic_score_ref"""
    pred, gt = [], []
    for v in views:
        p = RR.render_view(scene["verts"], scene["faces"], RR.K_SMALL, scene["poses"][v], RR.H, RR.W, labels=(scene["vsem"], scene["vins"]))
        g = RR.render_view(gt_verts, gt_faces, RR.K_SMALL, scene["poses"][v], RR.H, RR.W, labels=(sem_ids, ins_ids))
        assert not p["left_out"].any() and not g["left_out"].any()
        seen_p, seen_g = (p["face"] >= 0).reshape(-1), (g["face"] >= 0).reshape(-1)
        lp = PR.pred_labels(p["labels"][0], p["labels"][1])
        lg = PR.gt_labels(g["labels"][0], g["labels"][1])
        pred += [x if s else None for x, s in zip(lp, seen_p)]
        gt += [x if s else None for x, s in zip(lg, seen_g)]
    return pred, gt


def _clean_views(scene, gt_verts, gt_faces):
    views = [v for v in range(len(scene["poses"]))
             if not any(RR.render_view(x, f, RR.K_SMALL, scene["poses"][v], RR.H, RR.W)["left_out"].any()
                        for x, f in ((scene["verts"], scene["faces"]), (gt_verts, gt_faces)))]
    assert len(views) >= 2, views
    return views


def test_score_pixels_matches_the_restatement(scene):
    from eprecon_amd import panoptic_score as PS
    mapping = np.array(PR.MAPPING)
    verts, vsem, vins = scene["verts"], scene["vsem"], scene["vins"]
    gt_verts, gt_faces, sem_ids, ins_ids = RR.disagreeing_ground_truth(verts, scene["faces"], mapping[vsem], vins)
    ply, info = _ground_truth(scene, "scene_a", gt_verts, gt_faces, sem_ids, ins_ids)
    views = _clean_views(scene, gt_verts, gt_faces)
    tables = PS.score_pixels(scene["dense"], ply, info, "scene_a", RR.K_SMALL, scene["poses"][views], RR.H, RR.W, chunk=3)
    pred, gt = _pixel_sites(scene, gt_verts, gt_faces, sem_ids, ins_ids, views)
    want = PR.score(pred, gt)
    assert want["M"].sum() == len(views) * RR.H * RR.W                    # the sites are all pixels of the frames
    assert want["M"][-1, :-1].sum() > 0 and want["M"][:-1, -1].sum() > 0 and want["M"][:-1, -2].sum() > 0
    PR.assert_tables_equal(tables, want, tol=1e-12)
    PR.assert_summaries_equal(PS.PanopticScore().add(tables).summary(), PR.summary([want]), tol=1e-12)
    one = PS.score_pixels(scene["sparse"], ply, info, "scene_a", RR.K_SMALL, scene["poses"][views], RR.H, RR.W, chunk=1)
    assert np.array_equal(one.counts, tables.counts)
    # label files that do not belong to the mesh
    np.save(os.path.join(info, "scene_a_sem_label.npy"), sem_ids[:-1])
    with pytest.raises(ValueError):
        PS.score_pixels(scene["dense"], ply, info, "scene_a", RR.K_SMALL, scene["poses"][views], RR.H, RR.W)


def test_score_pixels_of_the_ground_truth_itself_is_perfect(scene):
    from eprecon_amd import panoptic_score as PS
    mapping = np.array(PR.MAPPING)
    sem_ids, ins_ids = mapping[scene["vsem"]].astype(np.int64), scene["vins"].astype(np.int64)
    ply, info = _ground_truth(scene, "scene_b", scene["verts"], scene["faces"], sem_ids, ins_ids)
    tables = PS.score_pixels(scene["dense"], ply, info, "scene_b", RR.K_SMALL, scene["poses"], RR.H, RR.W)
    summary = PS.PanopticScore().add(tables).summary()
    present = [r for r in summary["classes"].values() if r["pq"] is not None]
    assert len(present) == 3 and all(r["pq"] == 1.0 and r["fp"] == 0 and r["fn"] == 0 for r in present)
    assert summary["all"]["pq"] == 1.0 and summary["miou"] == 1.0


def test_command_line_tools(scene, tmp_path, capsys):
    from PIL import Image as image_mod
    from eprecon_amd import panoptic_score as PS
    mapping = np.array(PR.MAPPING)
    sem_ids = np.where(scene["verts"][:, 2] > 0.55, 7, mapping[scene["vsem"]]).astype(np.int64)
    ply, info = _ground_truth(scene, "scene_a", scene["verts"], scene["faces"], sem_ids, scene["vins"].astype(np.int64))
    data = tmp_path / "data" / "scene_a"
    os.makedirs(data / "pose"), os.makedirs(data / "intrinsic")
    k4 = np.eye(4)
    k4[:3, :3] = RR.K_SMALL * [[10.0], [10.0], [1.0]]                     # of the 640 x 480 sensor
    np.savetxt(data / "intrinsic" / "intrinsic_depth.txt", k4, delimiter=" ")
    frames = [scene["poses"][0], scene["poses"][1], np.full((4, 4), -np.inf), scene["poses"][2], scene["poses"][3]]
    for i, pose in enumerate(frames):
        np.savetxt(data / "pose" / f"pose_{i}.txt", pose, delimiter=" ")
    (tmp_path / "scenes.txt").write_text("scene_a\n")
    pred_dir = os.path.dirname(scene["dense"])
    ids, k, poses = RD.scene_views(str(tmp_path / "data"), "scene_a", every=1, size=(64, 48))
    assert ids == [0, 1, 3, 4] and np.allclose(k, RR.K_SMALL, rtol=1e-14, atol=0)             # the frame without a pose is skipped
    common = ["--pred", pred_dir, "--scenes", str(tmp_path / "scenes.txt")]
    out = tmp_path / "out"
    assert RD.main(common + ["--data_path", str(tmp_path / "data"), "--out", str(out), "--every", "1", "--size", "64", "48"]) == 0
    assert sorted(os.listdir(out / "scene_a")) == sorted(f"{m}_{i}.png" for m in ("semantic", "instance", "shaded") for i in ids)
    want = RD.render_scene(scene["dense"], k, poses, 48, 64)
    for j, i in enumerate(ids):
        for mode in ("semantic", "instance", "shaded"):
            assert np.array_equal(np.asarray(image_mod.open(out / "scene_a" / f"{mode}_{i}.png")), host(want[mode + "_rgb"][j]))
    assert RD.main(common + ["--data_path", str(tmp_path / "data"), "--out", str(tmp_path / "two"), "--every", "3", "--size", "64", "48",
                             "--mode", "instance"]) == 0
    assert sorted(os.listdir(tmp_path / "two" / "scene_a")) == ["instance_0.png", "instance_3.png"]
    capsys.readouterr()
    assert PS.main(common + ["--views", str(tmp_path / "data"), "--info", info, "--gt_mesh", os.path.dirname(ply), "--every", "1",
                             "--size", "64", "48", "--out", str(tmp_path / "pixels.json")]) == 0
    text = capsys.readouterr().out
    assert text.splitlines()[0].split()[:4] == ["class", "PQ", "SQ", "RQ"] and "mIoU" in text
    tables = PS.score_pixels(scene["dense"], ply, info, "scene_a", k, poses, 48, 64)
    with open(tmp_path / "pixels.json") as fh:
        assert json.load(fh) == json.loads(json.dumps(PS.PanopticScore().add(tables).summary()))

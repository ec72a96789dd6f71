"""Scene evaluation on the GPU (csrc/mesh_eval.hip + the masked marching cubes through eprecon_amd/evaluation.py) against
float64 numpy restatements (tests/evaluation_ref.py) and, end to end, on a synthetic scene in the ScanNet layout."""
import json
import math
import os

import numpy as np
import pytest

import evaluation_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def look_at(eye, target):
    from eprecon_amd import synthetic as S
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    return S._look_at_pose(np.asarray(eye, np.float64), f / np.linalg.norm(f))


K_SMALL = np.array([[60.0, 0, 31.7], [0, 60.0, 23.3], [0, 0, 1]])
CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
# outward-wound faces (v1 - v0) x (v2 - v0) points out of the cube
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                   [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def compare_render(verts, faces, poses, k=K_SMALL, h=48, w=64, **kw):
    from eprecon_amd import evaluation as E
    got = E.render_depth(dev(verts), dev(faces), k, poses, h, w, **kw)
    again = E.render_depth(dev(verts), dev(faces), k, poses, h, w, **kw)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))            # run-to-run bit-identical
    got = got.cpu().numpy()
    n_hit = 0
    for v in range(len(poses)):
        ref, amb = R.render_depth(verts, faces, k, poses[v], h, w, **kw)
        ok = ~amb
        assert np.array_equal(got[v][ok] > 0, ref[ok] > 0), np.argwhere(ok & ((got[v] > 0) != (ref > 0)))[:5]
        both = ok & (ref > 0)
        assert np.all(np.abs(got[v][both] - ref[both]) <= 1e-5 * ref[both])
        n_hit += int(both.sum())
    return got, n_hit


def test_render_single_triangle_and_near_plane_crossing():
    tri = np.array([[-0.4, -0.3, 2.0], [0.5, -0.2, 2.5], [0.1, 0.4, 1.5]], np.float32)
    pose = np.eye(4)[None]
    f = np.array([[0, 2, 1]], np.int32)            # faces the camera: ((v1-v0) x (v2-v0)) . v0 < 0
    _, n = compare_render(tri, f, pose)
    assert n > 100
    got, n_back = compare_render(tri, f[:, [0, 2, 1]], pose)        # the back face is culled
    assert n_back == 0 and (got == 0).all()
    _, n2 = compare_render(tri, f[:, [0, 2, 1]], pose, cull_back=False)
    assert n2 == n
    # a triangle crossing the near plane and reaching behind the camera: exact coverage with no clipping
    cross = np.array([[-1.0, -0.2, -1.0], [1.0, -0.3, 3.0], [-0.5, 0.6, 2.0]], np.float32)
    for order in ([0, 1, 2], [0, 2, 1]):
        _, n3 = compare_render(cross, np.array([order], np.int32), pose, cull_back=False, znear=0.05)
        assert n3 > 50


def test_render_shared_edge_leaves_no_gap():
    """a square of two triangles whose diagonal runs through pixel centres: every pixel inside the square is hit"""
    from eprecon_amd import evaluation as E
    k = np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1]])
    # corners project onto pixel centres (c + 0.5): x = (c + 0.5 - 32) / 50 * z
    z = 2.0
    c0, c1, r0, r1 = 12, 52, 4, 44
    P = lambda c, r: [(c + 0.5 - 32.0) / 50.0 * z, (r + 0.5 - 24.0) / 50.0 * z, z]
    v = np.array([P(c0, r0), P(c1, r0), P(c1, r1), P(c0, r1)], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    got = E.render_depth(dev(v), dev(f), k, np.eye(4)[None], 48, 64, cull_back=False).cpu().numpy()[0]
    assert (got[r0 + 1:r1, c0 + 1:c1] > 0).all()
    assert all(got[r0 + i, c0 + i] > 0 for i in range(1, r1 - r0))       # the diagonal itself (corners: fp32 vertices)
    compare_render(v, f, np.eye(4)[None], k=k, cull_back=False)


@pytest.mark.parametrize("cull", [True, False])
def test_render_closed_cube_outside_and_inside(cull):
    outside = np.stack([look_at([1.6, -2.1, 1.2], [0.05, 0.0, -0.1]), look_at([-2.5, 0.3, -0.7], [0, 0.1, 0])])
    got, n = compare_render(CUBE_V, CUBE_F, outside, cull_back=cull)
    assert n > 500
    inside = np.stack([look_at([0.1, -0.05, 0.12], [1.0, 0.3, 0.2]), look_at([-0.2, 0.1, 0.0], [-0.4, -1.0, -0.3])])
    got, n = compare_render(CUBE_V, CUBE_F, inside, cull_back=cull)
    if cull:
        assert n == 0 and (got == 0).all()          # from inside every face is a back face
    else:
        assert (got > 0).all()                      # the closed cube surrounds the camera


def test_render_marching_cubes_mesh_matches_sphere_traced_depth():
    from eprecon_amd import evaluation as E
    from eprecon_amd import save_scene as SS
    from eprecon_amd import synthetic as S
    w = S.make_window(seed=0, width=160, height=120)
    tsdf = S.analytic_tsdf(w, 0)
    verts, faces, _ = SS.marching_cubes(dev(tsdf), 0.0)
    verts = verts * 0.04 + dev(w["vol_origin_partial"])
    got = E.render_depth(verts, faces, w["intrinsics"], w["poses"], 120, 160, pixel_center=0.0).cpu().numpy()
    agree = total = 0
    for v in range(len(w["poses"])):
        ref = S.render_depth(w, v)
        both = (ref > 0) & (got[v] > 0)
        total += int(both.sum())
        agree += int((np.abs(got[v][both] - ref[both]) < 0.02).sum())
    assert total > 0.3 * got.size and agree >= 0.99 * total, (agree, total)


def test_eval_depth_matches_restatement():
    from eprecon_amd import evaluation as E
    rng = np.random.default_rng(3)
    pred = rng.uniform(0.2, 12.0, (5, 37, 53)).astype(np.float32)
    trgt = (pred * rng.uniform(0.6, 1.5, pred.shape)).astype(np.float32)
    pred[rng.random(pred.shape) < 0.2] = 0
    trgt[rng.random(pred.shape) < 0.2] = 0
    trgt[1, :5] = 11.0
    pred[2] = 0                       # an all-invalid frame
    trgt[3, :3, :3] = pred[3, :3, :3]
    got = E.eval_depth(dev(pred), dev(trgt))
    assert len(got) == 5
    for v in range(5):
        want = R.eval_depth(pred[v], trgt[v])
        for k in E.DEPTH_KEYS:
            if math.isnan(want[k]):
                assert math.isnan(got[v][k]), (v, k)
            else:
                assert got[v][k] == pytest.approx(want[k], rel=1e-9, abs=0), (v, k)
    again = E.depth_sums(dev(pred), dev(trgt))
    assert torch.equal(again, E.depth_sums(dev(pred), dev(trgt)))
    single = E.eval_depth(dev(pred[0]), dev(trgt[0]))
    assert single["AbsRel"] == got[0]["AbsRel"]


def _blob(n=18, seed=0):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).astype(np.float32)
    vol = np.full((n, n, n), 1e9, np.float32)
    for _ in range(4):
        c, r = rng.uniform(5, n - 6, 3), rng.uniform(2.0, 3.4)
        vol = np.minimum(vol, np.linalg.norm(g - c, axis=-1) - r)
    return np.clip(vol / 3.0, -1, 1).astype(np.float32)


def test_masked_marching_cubes():
    from oracle import marching_cubes as OM
    from eprecon_amd import save_scene as SS
    vol = _blob(18, 1)
    plain = SS.marching_cubes(dev(vol), 0.0)
    full = SS.marching_cubes(dev(vol), 0.0, weight=dev(np.full(vol.shape, 0.5, np.float32)))
    for a, b in zip(plain, full):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # every weight > 0: today's output, bit for bit
    with pytest.raises(ValueError):
        SS.marching_cubes(dev(vol), 0.0, weight=dev(np.ones((18, 18, 17), np.float32)))
    rng = np.random.default_rng(4)
    weight = (rng.random(vol.shape) > 0.03).astype(np.float32) * rng.uniform(0.5, 3, vol.shape).astype(np.float32)
    weight[:, :, 11:] = 0                                                   # a whole unobserved slab, as after re-fusion
    table = OM.build_table()[0]
    ov, of = OM.marching_cubes(vol, 0.0, table)
    mv, mf, keep = R.masked_mesh(vol, weight, ov, of, table)
    assert 0 < len(mf) < len(of)
    gv, gf, gn = SS.marching_cubes(dev(vol), 0.0, weight=dev(weight))
    assert np.array_equal(gv.cpu().numpy(), mv) and np.array_equal(gf.cpu().numpy(), mf)
    # no face lies in a cell with a zero-weight corner
    cell = np.floor(gv.cpu().numpy()[gf.cpu().numpy().reshape(-1)].reshape(-1, 3, 3).min(1)).astype(int)
    for x, y, z in cell:
        assert (weight[x:x + 2, y:y + 2, z:z + 2] > 0).all()


@pytest.mark.parametrize("voxel", [0.02, 0.03125])
def test_voxel_down_sample_matches_restatement(voxel):
    from eprecon_amd import evaluation as E
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.0, 2.0, (40000, 3)).astype(np.float32)
    pts[0] = -1.0                                        # the minimum on every axis: min_bound = -1 - voxel / 2
    pts[-1] = [7.0, 1.0, 6.0]                            # a far outlier (above the minimum)
    mb = -1.0 - voxel * 0.5                              # (fp64, as the down-sample forms it)
    # points on voxel boundaries min_bound + k * voxel (k >= 1), and others one fp32 step below a boundary
    k = np.maximum(np.floor((pts[1:3001].astype(np.float64) - mb) / voxel), 1.0)
    on = (mb + k * voxel).astype(np.float32)
    pts[1:3001] = on
    pts[3001:5001] = np.nextafter(on[:2000], np.float32(-np.inf))
    pts[5001:11001] = pts[5001:5007].repeat(1000, 0)     # crowded voxels
    q = pts.astype(np.float64)
    assert (q.min(0) == -1.0).all()
    f = (q[1:3001] - mb) / voxel
    exact = f == np.floor(f)
    if voxel == 0.03125:
        assert exact.all()                               # binary voxel: every one of them lies exactly on a boundary
    assert exact.sum() > 0
    got = E.voxel_down_sample(dev(pts), voxel)
    again = E.voxel_down_sample(dev(pts), voxel)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    want, keys = R.voxel_down_sample(pts, voxel)
    g = got.cpu().numpy()
    assert g.shape == want.shape
    w32 = want.astype(np.float32)
    # equal to fp32 rounding: one ulp, or the 2^-36 voxel step of the fixed-point sums where the mean is close to 0
    tol = np.maximum(np.spacing(np.abs(w32)), voxel * 2.0 ** -36)
    assert np.all(np.abs(g.astype(np.float64) - w32) <= tol), np.abs(g - w32).max()
    # the same voxel set: every output lies in its voxel of the restatement's key order
    assert np.array_equal(np.floor((g.astype(np.float64) - mb) / voxel).astype(np.int64), keys)
    # a point exactly on a boundary belongs to the voxel above it, one a step below to the voxel below
    ib = 1 + np.flatnonzero(exact.any(1))[:200]
    assert len(ib) > 0
    for i in ib:
        kk = np.floor((q[i] - mb) / voxel).astype(np.int64)
        kb = np.floor((q[3000 + i] - mb) / voxel).astype(np.int64) if 3000 + i < 5001 else None
        assert (keys == kk).all(1).any()
        if kb is not None:
            assert (kb <= kk).all() and (kb < kk).any()
    one = E.voxel_down_sample(dev(pts[:1]), voxel).cpu().numpy()
    assert np.array_equal(one, pts[:1])


def _clouds(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.uniform(-2, 3, (n, 3)).astype(np.float32)
    if kind == "clustered":
        c = rng.uniform(-5, 5, (6, 3))
        return (c[rng.integers(0, 6, n)] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    if kind == "plane":
        p = rng.uniform(-2, 2, (n, 3))
        p[:, 2] = 0.5
        return p.astype(np.float32)
    if kind == "same":
        return np.tile(np.array([[0.3, -0.1, 2.0]], np.float32), (n, 1))
    if kind == "far":                                   # queries far outside the reference box, on every side
        p = rng.uniform(-2, 3, (n, 3))
        p[np.arange(n), rng.integers(0, 3, n)] += rng.choice([-60.0, 60.0], n)
        return p.astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind1,kind2,n1,n2", [("uniform", "uniform", 20000, 20000), ("clustered", "clustered", 20000, 15000),
                                               ("clustered", "uniform", 3000, 5000), ("plane", "uniform", 8000, 4000),
                                               ("same", "uniform", 500, 2000), ("uniform", "same", 4000, 100),
                                               ("uniform", "uniform", 1, 3000), ("uniform", "uniform", 3000, 1),
                                               ("uniform", "far", 20000, 3000), ("clustered", "far", 20000, 3000)])
def test_nn_correspondance_exact(kind1, kind2, n1, n2):
    from eprecon_amd import evaluation as E
    a, b = _clouds(kind1, n1, 6), _clouds(kind2, n2, 7)
    b[: min(50, n2)] = a[np.arange(min(50, n2)) % n1]                   # exact hits
    idx, dist = E.nn_correspondance(dev(a), dev(b))
    ri, rd, second = R.nn_brute(a, b)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    # 1e-6 m, or one fp32 step of the returned distance where that is coarser (queries tens of metres away)
    assert np.all(np.abs(dist - rd) <= np.maximum(1e-6, np.spacing(rd.astype(np.float32)))), np.abs(dist - rd).max()
    # (at an fp64 tie both take the smallest index: the indices agree everywhere)
    assert np.array_equal(idx, ri), np.argwhere(idx != ri)[:5]


def test_nn_correspondance_empty_inputs():
    from eprecon_amd import evaluation as E
    a = dev(np.zeros((0, 3), np.float32))
    b = dev(np.ones((4, 3), np.float32))
    for x, y in ((a, b), (b, a), (a, a)):
        i, d = E.nn_correspondance(x, y)
        assert i.numel() == 0 and d.numel() == 0


def test_nn_correspondance_large_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    from eprecon_amd import evaluation as E
    rng = np.random.default_rng(8)
    a = rng.uniform(-3, 3, (200000, 3)).astype(np.float32)
    b = rng.uniform(-3.2, 3.2, (200000, 3)).astype(np.float32)
    idx, dist = E.nn_correspondance(dev(a), dev(b))
    rd, ri = spatial.cKDTree(a.astype(np.float64)).query(b.astype(np.float64), k=1)
    assert np.abs(dist.cpu().numpy() - rd).max() < 1e-6
    assert (idx.cpu().numpy() == ri).mean() > 0.9999


# ------------------------------------------------------------------------------------------------------ end to end

def _room_poses():
    poses = []
    for eye in ([-0.4, 0.9, 1.4], [0.5, 1.6, 1.6], [0.0, 2.7, 1.5]):
        for yaw in range(0, 360, 30):
            t = np.deg2rad(yaw)
            poses.append(look_at(eye, np.array(eye) + [np.sin(t), np.cos(t), -0.45]))
    return np.stack(poses).astype(np.float32)


def _analytic_mesh(voxel, origin, dims):
    from eprecon_amd import save_scene as SS
    from eprecon_amd import synthetic as S
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    return SS.tsdf2mesh(voxel, dev(np.asarray(origin, np.float32)), dev(tsdf))


@pytest.fixture(scope="module")
def scannet_scene(tmp_path_factory):
    """a synthetic scene in the ScanNet layout: depth/depth_<i>.png (sphere-traced, mm), pose/pose_<i>.txt,
    intrinsic/intrinsic_depth.txt; model/<scene>.ply = the analytic scene meshed at 4 cm, gt/<scene>_vh_clean_2.ply = at 2 cm,
    both up to z = 1.8 m (what the cameras see of the walls).  Frame 3 has an invalid (inf) pose."""
    from PIL import Image
    from eprecon_amd import synthetic as S
    from eprecon_amd.save_scene import export_ply
    root = tmp_path_factory.mktemp("scannet")
    scene = "scene0707_00"
    h, w = 120, 160
    window = S.make_window(seed=0, width=w, height=h)
    window = dict(window, poses=_room_poses(), image_hw=(h, w))
    sdir = root / "data" / scene
    for d in ("depth", "pose", "intrinsic"):
        os.makedirs(sdir / d)
    k4 = np.eye(4)
    k4[:3, :3] = window["intrinsics"]
    np.savetxt(sdir / "intrinsic" / "intrinsic_depth.txt", k4, delimiter=" ")
    n = len(window["poses"])
    for i in range(n):
        depth = S.render_depth(window, i)
        Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(sdir / "depth" / f"depth_{i}.png")
        pose = np.full((4, 4), np.inf) if i == 3 else window["poses"][i]
        np.savetxt(sdir / "pose" / f"pose_{i}.txt", pose, delimiter=" ")
    origin = np.array([-1.92, 0.2, -0.4])
    os.makedirs(root / "model")
    os.makedirs(root / "gt")
    export_ply(_analytic_mesh(0.04, origin, (96, 96, 55)), root / "model" / f"{scene}.ply")
    export_ply(_analytic_mesh(0.02, origin, (192, 192, 110)), root / "gt" / f"{scene}_vh_clean_2.ply")
    return {"root": root, "scene": scene, "n": n, "K": window["intrinsics"]}


def test_evaluate_scene_end_to_end(scannet_scene, tmp_path):
    from eprecon_amd import evaluation as E
    s, root = scannet_scene, scannet_scene["root"]
    sdir = root / "data" / s["scene"]
    frames = list(E.scannet_frames(str(sdir)))
    assert len(frames) == s["n"] and np.isinf(frames[3][0][0, 0])
    mesh = str(root / "model" / f"{s['scene']}.ply")
    gt = str(root / "gt" / f"{s['scene']}_vh_clean_2.ply")
    out = tmp_path / "out"
    m = E.evaluate_scene(mesh, frames, s["K"], gt, out_dir=str(out), scene=s["scene"], chunk=7)
    assert list(m) == E.METRIC_KEYS and all(isinstance(v, float) for v in m.values())
    assert sorted(os.listdir(out)) == [f"{s['scene']}_metrics.json", f"{s['scene']}_trim_single.ply"]
    assert json.load(open(out / f"{s['scene']}_metrics.json")) == pytest.approx(m)
    tv, tf = E.read_ply(str(out / f"{s['scene']}_trim_single.ply"))
    assert len(tv) > 1000 and len(tf) > 1000
    print({k: round(v, 4) for k, v in m.items()})
    assert m["fscore"] > 0.9 and m["complete"] > 0.5 and m["AbsRel"] < 0.05 and m["r1"] > 0.95
    # the same prediction shifted by 10 cm scores clearly lower
    v, f = E.read_ply(mesh)
    shifted = E.evaluate_scene((v + np.array([0.1, 0.0, 0.0], np.float32), f), frames, s["K"], gt, scene="shifted")
    print({k: round(v, 4) for k, v in shifted.items()})
    assert shifted["fscore"] < m["fscore"] - 0.2


def test_cli_reproduces_metrics_json(scannet_scene, capsys):
    from eprecon_amd import evaluation as E
    s, root = scannet_scene, scannet_scene["root"]
    frames = list(E.scannet_frames(str(root / "data" / s["scene"])))
    direct = E.evaluate_scene(str(root / "model" / f"{s['scene']}.ply"), frames, s["K"],
                              str(root / "gt" / f"{s['scene']}_vh_clean_2.ply"))
    E.main(["--model", str(root / "model"), "--data_path", str(root / "data"), "--gt_path", str(root / "gt")])
    got = json.load(open(root / "model" / "metrics.json"))
    assert list(got) == [s["scene"]] and got[s["scene"]] == pytest.approx(direct, nan_ok=True)
    assert os.path.exists(root / "model" / f"{s['scene']}_trim_single.ply")
    table = capsys.readouterr().out
    assert all(k in table for k in E.METRIC_KEYS) and "fscore" in table.splitlines()[-1]

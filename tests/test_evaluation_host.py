"""Scene evaluation, host side (no GPU): the PLY reader, the numpy restatements the GPU tests compare against, and the
metric assembly of eprecon_amd/evaluation.py (tools/evaluation.py + tools/evaluation_utils.py of the reference)."""
import math

import numpy as np
import pytest

import evaluation_ref as R
from eprecon_amd import evaluation as E
from eprecon_amd.save_scene import export_ply


def test_read_ply_round_trips_export_ply(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((57, 3)).astype(np.float32) * 3
    f = rng.integers(0, 57, (91, 3)).astype(np.int32)
    n = rng.standard_normal((57, 3)).astype(np.float32)
    for col in (None, rng.integers(0, 255, (57, 3)).astype(np.uint8)):
        mesh = {"vertices": v, "faces": f, "vertex_normals": n}
        if col is not None:
            mesh["vertex_colors"] = col
        export_ply(mesh, tmp_path / "m.ply")
        gv, gf = E.read_ply(str(tmp_path / "m.ply"))
        assert gv.dtype == np.float32 and gf.dtype == np.int32
        assert np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gf, f)
    export_ply({"vertices": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32),
                "vertex_normals": np.zeros((0, 3), np.float32)}, tmp_path / "e.ply")
    gv, gf = E.read_ply(str(tmp_path / "e.ply"))
    assert gv.shape == (0, 3) and gf.shape == (0, 3)


SCANNET_HEADER = """ply
format {fmt} 1.0
comment VCGLIB generated
element vertex {nv}
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property uchar alpha
element face {nf}
property list uchar int vertex_indices
end_header
"""


def _scannet_mesh():
    v = np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 2.25, 0], [0, 2.25, -0.125], [0.5, 0.5, 3.0]], np.float32)
    rgba = np.array([[10, 20, 30, 255]] * 5, np.uint8)
    polys = [[0, 1, 2], [0, 2, 3], [1, 2, 4, 3]]        # the quad is fanned into two triangles
    want = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 4], [1, 4, 3]], np.int32)
    return v, rgba, polys, want


def test_read_ply_scannet_layout_binary(tmp_path):
    v, rgba, polys, want = _scannet_mesh()
    rec = np.zeros(len(v), [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])
    rec["x"], rec["y"], rec["z"] = v.T
    rec["r"], rec["g"], rec["b"], rec["a"] = rgba.T
    body = rec.tobytes()
    for p in polys:
        body += np.uint8(len(p)).tobytes() + np.array(p, "<i4").tobytes()
    path = tmp_path / "scene0000_00_vh_clean_2.ply"
    path.write_bytes(SCANNET_HEADER.format(fmt="binary_little_endian", nv=len(v), nf=len(polys)).encode() + body)
    gv, gf = E.read_ply(str(path))
    assert np.array_equal(gv, v) and np.array_equal(gf, want)
    # every face a triangle: the structured fast path
    body = rec.tobytes() + b"".join(np.uint8(3).tobytes() + np.array(p, "<i4").tobytes() for p in polys[:2])
    path.write_bytes(SCANNET_HEADER.format(fmt="binary_little_endian", nv=len(v), nf=2).encode() + body)
    gv, gf = E.read_ply(str(path))
    assert np.array_equal(gv, v) and np.array_equal(gf, want[:2])


def test_read_ply_scannet_layout_ascii(tmp_path):
    v, rgba, polys, want = _scannet_mesh()
    lines = [" ".join([repr(float(x)) for x in v[i]] + [str(c) for c in rgba[i]]) for i in range(len(v))]
    lines += [" ".join([str(len(p))] + [str(i) for i in p]) for p in polys]
    path = tmp_path / "a.ply"
    path.write_text(SCANNET_HEADER.format(fmt="ascii", nv=len(v), nf=len(polys)) + "\n".join(lines) + "\n")
    gv, gf = E.read_ply(str(path))
    assert np.array_equal(gv, v) and np.array_equal(gf, want)


def test_read_ply_rejects_other_files(tmp_path):
    p = tmp_path / "x.ply"
    p.write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        E.read_ply(str(p))


def test_down_sample_restatement_matches_brute_force():
    rng = np.random.default_rng(1)
    voxel = 0.25
    pts = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    pts[0] = -1.0                                         # the minimum: min_bound = -1.125
    mb = np.full(3, -1.0 - voxel / 2)
    pts[1:41] = mb + np.maximum(np.floor((pts[1:41] - mb) / voxel), 1) * voxel     # on voxel boundaries
    pts[41:61] = np.nextafter(pts[1:21], np.float32(-np.inf))                      # one step below a boundary
    p = pts.astype(np.float64)
    assert (p.min(0) == -1.0).all()
    f = (p[1:41] - mb) / voxel
    assert (f == np.floor(f)).all()
    means, keys = R.voxel_down_sample(pts, voxel)
    groups = {}
    for i, q in enumerate(p):
        groups.setdefault(tuple(int(math.floor((q[a] - mb[a]) / voxel)) for a in range(3)), []).append(q)
    assert [tuple(k) for k in keys] == sorted(groups)
    for k, m in zip(keys, means):
        assert np.allclose(m, np.mean(groups[tuple(k)], 0), rtol=0, atol=1e-15)


def test_nn_restatement_matches_brute_force():
    rng = np.random.default_rng(2)
    a = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    b = np.concatenate([rng.uniform(0, 1, (150, 3)), a[:5]]).astype(np.float32)
    idx, dist, _ = R.nn_brute(a, b, chunk=37)
    for j, q in enumerate(b.astype(np.float64)):
        d = np.sqrt(((a.astype(np.float64) - q) ** 2).sum(1))
        assert idx[j] == int(np.argmin(d)) and abs(dist[j] - d.min()) < 1e-12
    assert (dist[-5:] == 0).all() and list(idx[-5:]) == [0, 1, 2, 3, 4]
    e, d, _ = R.nn_brute(a[:0], b)
    assert len(e) == 0 and len(d) == 0


def test_mesh_metric_assembly_hand_computed():
    dist1 = np.array([0.01, 0.02, 0.2, 0.06])     # target points -> prediction
    dist2 = np.array([0.0, 0.04, 0.049, 0.1, 0.5])    # predicted points -> target
    m = E.mesh_metrics(dist1, dist2, threshold=0.05)
    prec, recal = 3 / 5, 2 / 4
    assert m["prec"] == pytest.approx(prec) and m["recal"] == pytest.approx(recal)
    assert m["fscore"] == pytest.approx(2 * prec * recal / (prec + recal))
    assert m["dist1"] == pytest.approx(dist2.mean()) and m["dist2"] == pytest.approx(dist1.mean())   # the reference's naming
    z = E.mesh_metrics(np.array([1.0]), np.array([1.0, 2.0]))
    assert z["prec"] == 0 and z["recal"] == 0 and math.isnan(z["fscore"])
    e = E.mesh_metrics(np.zeros(0), np.zeros(0))
    assert all(math.isnan(e[k]) for k in E.MESH_KEYS)


def test_depth_metrics_from_sums_and_scene_average():
    pred = np.array([[0.0, 1.0, 2.0], [4.0, 1.0, 12.0]], np.float32)
    trgt = np.array([[1.0, 1.25, 2.0], [0.0, 2.0, 11.0]], np.float32)
    m = (pred > 0) & (trgt > 0) & (trgt < 10)
    p, t = pred[m].astype(np.float64), trgt[m].astype(np.float64)
    d = np.abs(p - t)
    th = np.maximum(p / t, t / p)
    sums = np.array([[m.sum(), (pred > 0).sum(), (d / t).sum(), d.sum(), (d * d / t).sum(), (d * d).sum(),
                      ((np.log(p) - np.log(t)) ** 2).sum(), (th < 1.25).sum(), (th < 1.5625).sum(), (th < 1.953125).sum()],
                     [0, 2, 0, 0, 0, 0, 0, 0, 0, 0]])
    got = E.depth_metrics_from_sums(sums, pred.size)
    want = R.eval_depth(pred, trgt)
    for k in E.DEPTH_KEYS:
        assert got[0][k] == pytest.approx(want[k], rel=1e-12)
    assert all(math.isnan(got[1][k]) for k in E.DEPTH_KEYS if k != "complete") and got[1]["complete"] == 2 / 6
    # two frames evaluated, one skipped: the denominator is three (tools/evaluation.py:150-151)
    frames = [{k: 1.0 for k in E.DEPTH_KEYS}, {k: 2.0 for k in E.DEPTH_KEYS}]
    avg = E.average_depth_metrics(frames, 3)
    assert all(avg[k] == pytest.approx(1.0) for k in E.DEPTH_KEYS)
    assert math.isnan(E.average_depth_metrics(frames + [got[1]], 4)["AbsRel"])       # a NaN frame makes the scene NaN
    assert E.average_depth_metrics(frames + [got[1]], 4)["complete"] == pytest.approx((1 + 2 + 1 / 3) / 4)


def test_visualize_prints_the_nanmean_table(tmp_path, capsys):
    import json
    m1 = {k: 1.0 for k in E.METRIC_KEYS}
    m2 = dict(m1, fscore=float("nan"), prec=3.0)
    (tmp_path / "metrics.json").write_text(json.dumps({"b": m2, "a": m1}))
    text = E.visualize(str(tmp_path / "metrics.json"))
    rows = dict(l.split() for l in text.splitlines())
    assert list(rows) == E.METRIC_KEYS and rows["fscore"] == "1.000" and rows["prec"] == "2.000"
    assert capsys.readouterr().out.strip() == text.strip()


def test_nn_grid_sizes():
    cell, dims = E.nn_grid(np.zeros(3), np.array([4.0, 2.0, 0.0]), 1000)
    assert dims[2] == 1 and 1000 <= np.prod(dims.astype(np.int64)) <= 4000 * 1.5
    assert (np.floor(np.array([4.0, 2.0, 0.0]) / cell) + 1 == dims).all()
    cell, dims = E.nn_grid(np.ones(3), np.ones(3), 7)
    assert list(dims) == [1, 1, 1] and cell > 0


def test_operators_refuse_host_tensors():
    import torch
    from eprecon_amd import _lib
    with pytest.raises(_lib.EpreconError):
        E.nn_correspondance(torch.zeros(3, 3), torch.zeros(3, 3))
    with pytest.raises(_lib.EpreconError):
        E.voxel_down_sample(torch.zeros(3, 3), 0.02)
    with pytest.raises(_lib.EpreconError):
        E.render_depth(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), np.eye(3), np.eye(4)[None], 4, 4)

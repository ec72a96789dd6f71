"""CPU: the sparse / point-voxel oracle (oracle/sparse.py, oracle/pointvoxel.py) against the float64 dense formulations of
tests/dense_ref.py — a second witness that goes through no kernel map and no hash — on the edge inputs the GPU module
(test_pointvoxel_dense_gpu.py) feeds the HIP kernels: negative and odd-negative coordinates on every axis, interleaved
batches, the 1 -> 2 -> 4 -> 8 hierarchy, points on voxel faces / edges / corners and one ulp below them, absent corners,
a crowded voxel and empty target voxels."""
import numpy as np
import torch

import dense_ref as DR
from oracle import pointvoxel as PV
from oracle import sparse as OS

# SPVCNN's layers at cr = 1, 1/2, 1/4 (models/modules.py:75-175: cs = 32, 64, 128, 96, 96 scaled) and ConvGRU's
# (hidden = input = 24 / 48 / 96: C_in = 2 hidden), plus a ragged shape.  (kind, tensor stride of the input, C_in, C_out)
LAYERS = [("k3", 1, 81, 32), ("down", 1, 32, 32), ("k3", 2, 32, 64), ("down", 2, 64, 64), ("k3", 4, 64, 128),
          ("up", 2, 128, 96), ("k3", 2, 160, 96), ("up", 1, 96, 96), ("k3", 1, 128, 96),
          ("k3", 1, 39, 16), ("down", 1, 16, 16), ("k3", 2, 16, 32), ("up", 2, 64, 48), ("k3", 1, 72, 48),
          ("k3", 4, 16, 32), ("down", 2, 16, 16), ("up", 1, 24, 24), ("k3", 1, 48, 24), ("k3", 1, 96, 48),
          ("k3", 1, 192, 96), ("k3", 2, 13, 7), ("down", 4, 13, 7), ("up", 4, 7, 13)]


# the oracle's side of the comparison is a per-offset loop: a subset keeps the CPU suite short (the GPU module runs LAYERS)
CPU_LAYERS = [("k3", 1, 39, 16), ("down", 1, 16, 16), ("k3", 2, 32, 64), ("down", 2, 13, 7), ("k3", 4, 64, 128),
              ("up", 2, 128, 96), ("up", 1, 24, 24), ("down", 4, 13, 7), ("up", 4, 7, 13), ("k3", 4, 13, 7)]


def edge_coords(seed, n=600, extent=6, batch=3):
    """(b, x, y, z) rows, unique: random ones in [-extent, extent) interleaved over `batch` batches, plus every point of the
    cube {-4..1}^3 (odd negatives -1 / -3 on every axis, which floor to -2 / -4 at stride 2) in every batch — the same xyz
    in different batches — shuffled so that the batches interleave"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(-4, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    fixed = np.concatenate([np.concatenate([np.full((len(g), 1), b), g], 1) for b in range(batch)])
    rnd = np.concatenate([rng.integers(0, batch, (n, 1)), rng.integers(-extent, extent, (n, 3))], 1)
    rows = np.concatenate([fixed, rnd])
    _, first = np.unique(rows, axis=0, return_index=True)
    rows = rows[np.sort(first)]
    rng.shuffle(rows)
    return rows.astype(np.int32)


def hierarchy(coords, levels=4):
    """[(coords at stride 2^l, parent row of each finer row in it)] for l = 0 .. levels - 1 (parent None at l = 0),
    numbered by the dense reference"""
    out = [(np.asarray(coords, np.int64), None)]
    for lvl in range(1, levels):
        u, inv = DR.number_first(DR.quantise_coords(out[-1][0], 2 ** lvl))
        out.append((u, inv))
    return out


def ulp_below(a):
    return np.nextafter(np.float32(a), np.float32(-np.inf), dtype=np.float32)


def face_points(seed, n_random=400, batch=3, lo=-6, hi=6):
    """scaled-frame points (x, y, z, b) f32: on the voxel faces / edges / corners of every stride up to 8 (integer and
    multiple-of-s planes), one ulp below them, -0.0, and random ones — the trilinear corner tables at strides 1 .. 8"""
    rng = np.random.default_rng(seed)
    planes = np.arange(lo, hi + 1, dtype=np.float32)
    vals = np.concatenate([planes, ulp_below(planes), np.array([-0.0, ulp_below(0.0), 0.5, -0.5], np.float32)])
    pts = []
    for _ in range(3 * len(vals)):      # faces (one coordinate on a plane), edges (two), corners (three)
        k = rng.integers(1, 4)
        p = rng.uniform(lo, hi, 3).astype(np.float32)
        axes = rng.choice(3, k, replace=False)
        p[axes] = rng.choice(vals, k)
        pts.append(p)
    pts = np.concatenate([np.array(pts, np.float32), rng.uniform(lo, hi, (n_random, 3)).astype(np.float32),
                          np.array([[-0.0, -0.0, -0.0], [-1, -3, -1], [ulp_below(-1), ulp_below(-3), ulp_below(-4)]],
                                   np.float32)])
    b = rng.integers(0, batch, (len(pts), 1)).astype(np.float32)
    return np.concatenate([pts, b], 1)


def with_far_points(pts, seed, n=40):
    """pts plus n points at x in [40, 44): their voxels are left out of sparse_voxel_set, all eight corners absent"""
    rng = np.random.default_rng(seed)
    far = rng.uniform(-4, 4, (n, 4)).astype(np.float32)
    far[:, 0] += 44
    far[:, 3] = rng.integers(0, 3, n)
    return np.concatenate([pts, far])


def sparse_voxel_set(pts, s, rng):
    """the voxels of pts at stride s (first-occurrence order), 40 % of them dropped (absent corners) and none at x >= 32"""
    vox = np.concatenate([pts[:, 3:4], np.floor(pts[:, :3])], 1).astype(np.int64)
    full = DR.number_first(DR.quantise_coords(vox, s))[0]
    keep = (rng.random(len(full)) < 0.6) & (full[:, 1] < 32)
    return full[keep]


def metric_points(seed, res=0.37, crowd=1200):
    """metric points (x, y, z, b) f32 for a voxelisation at `res`: random ones around the origin (negative coordinates),
    exact multiples k * res formed in float32 (voxel faces of the quotient up to rounding) and one ulp below them, and
    `crowd` points inside one voxel (a list of >= 1,000 points for the scatter-mean)"""
    rng = np.random.default_rng(seed)
    r = np.float32(res)
    k = rng.integers(-9, 9, (300, 3)).astype(np.float32)
    on = k * r
    below = ulp_below(on)
    rnd = rng.uniform(-9 * res, 9 * res, (700, 3)).astype(np.float32)
    crowded = (np.float32(-3.0) + rng.uniform(0.05, 0.95, (crowd, 3)).astype(np.float32)) * r
    pts = np.concatenate([on, below, rnd, crowded, np.array([[-0.0, -0.0, -0.0]], np.float32)])
    b = rng.integers(0, 3, (len(pts), 1)).astype(np.float32)
    b[-crowd - 1:-1] = 1
    order = rng.permutation(len(pts))
    return np.concatenate([pts, b], 1)[order]


def test_frame_shift_keeps_the_parents():
    f = DR.Frame([np.array([[0, -3, -1, 5], [0, 7, 0, -8]])], 8)
    assert f.shift % 8 == 0 and f.side % 8 == 0
    c = np.array([[0, -1, -3, -4]])
    vol = f.embed(c, np.ones((1, 1)), 1)
    down = torch.nn.functional.avg_pool3d(vol, 2) * 8        # the 2^3 block that holds (-1, -3, -4) at stride 2
    assert float(f.read(down, DR.quantise_coords(c, 2), 2)[0, 0]) == 1.0
    assert np.array_equal(DR.quantise_coords(c, 2), [[0, -2, -4, -4]])


def test_voxel_numbering_and_parents():
    """unique_first at quanta 2 / 4 / 8 and the coarse parents of every hierarchy step == the dict numbering of floor(c / q)"""
    c = edge_coords(0)
    for q in (2, 4, 8):
        u, inv = OS.unique_first(c, q)
        ru, rinv = DR.number_first(DR.quantise_coords(c, q))
        assert np.array_equal(u, ru) and np.array_equal(inv, rinv)
    lv = hierarchy(c)
    for lvl in range(1, 4):
        u, parent = OS.unique_first(lv[lvl - 1][0], 2 ** lvl)
        assert np.array_equal(u, lv[lvl][0]) and np.array_equal(parent, lv[lvl][1])


def _oracle_layer(kind, fine, coarse, parent, x, w, stride):
    if kind == "k3":
        return OS.sparse_conv(x, OS.kernel_map(fine, fine, 3, stride), w)
    if kind == "down":
        return OS.sparse_conv(x, OS.kernel_map(fine, coarse, 2, stride), w)
    return OS.sparse_conv(x, OS.transpose_map(fine, parent, stride), w)


def dense_layer(frame, kind, fine, coarse, x, w, stride):
    if kind == "k3":
        return DR.subm_conv3(frame, fine, x, w, stride)
    if kind == "down":
        return DR.down_conv(frame, fine, x, coarse, w, stride)
    return DR.up_conv(frame, coarse, x, fine, w, stride)


def layer_case(kind, stride, cin, cout, seed, coords=None):
    """-> (frame, fine coords at `stride`, coarse coords at 2 stride, parent, x, w): x lives on the input side of the layer"""
    rng = np.random.default_rng(seed)
    lv = hierarchy(edge_coords(seed) if coords is None else coords)
    lvl = int(np.log2(stride))
    fine = lv[lvl][0]
    coarse, parent = lv[lvl + 1] if lvl + 1 < len(lv) else (None, None)
    n_in = len(coarse) if kind == "up" else len(fine)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((27 if kind == "k3" else 8, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    return DR.Frame([lv[0][0]], 8), fine, coarse, parent, x, w


def test_convolutions_match_dense_formulation():
    for i, (kind, stride, cin, cout) in enumerate(CPU_LAYERS):
        frame, fine, coarse, parent, x, w = layer_case(kind, stride, cin, cout, seed=10 + i)
        got = _oracle_layer(kind, fine, coarse, parent, x, w, stride)
        ref = dense_layer(frame, kind, fine, coarse, x, w, stride).numpy()
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, atol=1e-4, err_msg=f"{kind} s{stride} {cin}->{cout}")


def test_voxelize_and_scatter_mean():
    """floor of the float32 quotient, first-occurrence numbering, float64 scatter-mean (a 1,200-point voxel included), and
    point_to_voxel into a set with voxels that hold no point (0) at strides 1 / 2 / 4 / 8"""
    rng = np.random.default_rng(5)
    pts = metric_points(5)
    scaled, vox = PV.point_quantize(pts, 0.37)
    r_scaled, r_vox = DR.quantise_points(pts, 0.37)
    assert np.array_equal(scaled, r_scaled) and np.array_equal(vox, r_vox)
    u, inv = OS.unique_first(vox, 1)
    ru, rinv = DR.number_first(r_vox)
    assert np.array_equal(u, ru) and np.array_equal(inv, rinv)
    assert np.bincount(rinv).max() >= 1000
    feat = rng.standard_normal((len(pts), 13)).astype(np.float32)
    np.testing.assert_allclose(PV.segment_mean(feat, inv, len(u)), DR.scatter_mean(feat, rinv, len(ru)).numpy(), atol=1e-5)
    z = PV.Points(feat, pts)
    z.vox = vox
    for s in (1, 2, 4, 8):
        target = DR.number_first(DR.quantise_coords(vox, s))[0]
        extra = target[:40].copy()
        extra[:, 1] += 1000                                       # voxels no point falls into
        target = np.concatenate([extra[:20], target, extra[20:]])
        got = PV.point_to_voxel(target, s, z, feat)
        ref = DR.scatter_mean(feat, DR.lookup(target, DR.quantise_coords(vox, s)), len(target)).numpy()
        np.testing.assert_allclose(got, ref, atol=1e-5)
        assert not got[:20].any() and not got[-20:].any()


def test_trilinear_tables_and_devoxelize():
    """corner indices exactly, weights within 1e-6, at strides 1 .. 8, on face / edge / corner points and one ulp below them,
    with some corners absent and some points whose eight corners are all absent (weights 0, output exactly 0)"""
    rng = np.random.default_rng(6)
    pts = with_far_points(face_points(6), 6)
    for s in (1, 2, 4, 8):
        vset = sparse_voxel_set(pts, s, rng)
        idx, w = PV.trilinear(vset, s, pts)
        ridx, rw = DR.corner_tables(vset, s, pts)
        assert np.array_equal(idx, ridx)
        np.testing.assert_allclose(w, rw, atol=1e-6)
        none = (ridx < 0).all(1)
        assert none.sum() > 10 and (ridx >= 0).any(1).sum() > 10
        feat = rng.standard_normal((len(vset), 6)).astype(np.float32)
        got = PV.devoxelize(feat, idx, w)
        np.testing.assert_allclose(got, DR.devoxelize(feat, ridx, rw).numpy(), atol=1e-5)
        assert not got[none].any()


def test_gate_formulas():
    """the ConvGRU arithmetic the oracle composes (oracle/spvcnn.py convgru) == the float64 gates"""
    from oracle.spvcnn import _sigmoid
    rng = np.random.default_rng(7)
    v, h, zg = (rng.standard_normal((50, 9)).astype(np.float32) * 4 for _ in range(3))
    zg = _sigmoid(zg)
    np.testing.assert_allclose(_sigmoid(v), DR.gate(v, 1).numpy(), atol=1e-6)
    np.testing.assert_allclose(_sigmoid(v) * h, DR.gate(v, 2, h).numpy(), atol=1e-5)
    q = np.tanh(v.astype(np.float64)).astype(np.float32)
    np.testing.assert_allclose((1 - zg) * h + zg * q, DR.gate(v, 3, h, zg).numpy(), atol=1e-5)

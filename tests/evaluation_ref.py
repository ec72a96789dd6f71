"""numpy restatements for the scene-evaluation tests (eprecon_amd/evaluation.py, csrc/mesh_eval.hip) — test helpers,
written from the reference's formulas (tools/evaluation_utils.py) and open3d's documented VoxelDownSample rule, in fp64."""
import numpy as np


def eval_depth(pred, trgt):
    """eval_depth of tools/evaluation_utils.py on one frame, every element in fp64 (NaN for an empty mask)"""
    pred, trgt = np.asarray(pred, np.float32), np.asarray(trgt, np.float32)
    mask1 = pred > 0
    mask = (trgt < 10) & (trgt > 0) & mask1
    p, t = pred[mask].astype(np.float64), trgt[mask].astype(np.float64)
    with np.errstate(all="ignore"):
        abs_diff = np.abs(p - t)
        thresh = np.maximum(t / p, p / t)
        mean = lambda a: float(np.mean(a)) if len(a) else float("nan")
        return {"AbsRel": mean(abs_diff / t), "AbsDiff": mean(abs_diff), "SqRel": mean(abs_diff ** 2 / t),
                "RMSE": float(np.sqrt(mean(abs_diff ** 2))), "LogRMSE": float(np.sqrt(mean((np.log(p) - np.log(t)) ** 2))),
                "r1": mean(thresh < 1.25), "r2": mean(thresh < 1.25 ** 2), "r3": mean(thresh < 1.25 ** 3),
                "complete": float(np.mean(mask1))}


def voxel_down_sample(points, voxel):
    """open3d VoxelDownSample: min_bound = min - voxel / 2, idx = floor((p - min_bound) / voxel) in fp64, fp64 mean per
    voxel, voxels in (x, y, z) key order -> (means f64[m,3], idx int64[m,3])"""
    p = np.asarray(points, np.float32).astype(np.float64)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    mb = p.min(0) - voxel * 0.5
    idx = np.floor((p - mb) / voxel).astype(np.int64)
    keys, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(keys), 3))
    np.add.at(sums, inv, p)
    cnt = np.bincount(inv, minlength=len(keys)).astype(np.float64)
    return sums / cnt[:, None], keys


def nn_brute(verts1, verts2, chunk=256):
    """for every point of verts2 the nearest of verts1 (fp64 squared distances, first index on ties) -> (idx, dist, d2)"""
    a = np.asarray(verts1, np.float32).astype(np.float64)
    b = np.asarray(verts2, np.float32).astype(np.float64)
    if len(a) == 0 or len(b) == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 0))
    idx, d2min, second = np.zeros(len(b), np.int64), np.zeros(len(b)), np.zeros(len(b))
    for s in range(0, len(b), chunk):
        q = b[s:s + chunk]
        d = q[:, None, :] - a[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = np.argmin(d2, 1)
        idx[s:s + chunk] = i
        d2min[s:s + chunk] = d2[np.arange(len(q)), i]
        # the runner-up distance at another index (ties are allowed to differ in index)
        d2[np.arange(len(q)), i] = np.inf
        second[s:s + chunk] = d2.min(1) if d2.shape[1] else np.inf
    return idx, np.sqrt(d2min), second


def render_depth(verts, faces, K, pose, height, width, pixel_center=0.5, znear=0.05, zfar=100.0, cull_back=True, rel_edge=1e-6):
    """float64 ray / triangle oracle of one view -> (depth f64[H,W] (0 = no hit), ambiguous bool[H,W]: the ray lies within
    rel_edge (relative) of an edge plane of a triangle that could be drawn there)"""
    v = np.asarray(verts, np.float64)
    w2c = np.linalg.inv(np.asarray(pose, np.float64))
    vc = v @ w2c[:3, :3].T + w2c[:3, 3]
    kinv = np.linalg.inv(np.asarray(K, np.float64))
    uu, vv = np.meshgrid(np.arange(width) + pixel_center, np.arange(height) + pixel_center)
    d = np.stack([uu, vv, np.ones_like(uu)], -1) @ kinv.T
    dn = np.linalg.norm(d, axis=-1)
    depth = np.full((height, width), np.inf)
    amb = np.zeros((height, width), bool)
    for f in np.asarray(faces, np.int64):
        a, b, c = vc[f[0]], vc[f[1]], vc[f[2]]
        n = np.cross(b - a, c - a)
        nd = n @ a
        if nd == 0 or (cull_back and not nd < 0):
            continue
        s = []
        for e in (np.cross(a, b), np.cross(b, c), np.cross(c, a)):
            sk = d @ e
            s.append(sk)
            amb |= np.abs(sk) <= rel_edge * np.linalg.norm(e) * dn
        s = np.stack(s)
        cov = (s >= 0).all(0) | (s <= 0).all(0)
        with np.errstate(all="ignore"):
            z = nd / (d @ n) * d[..., 2]
        hit = cov & (z >= znear) & (z <= zfar)
        depth = np.where(hit & (z < depth), z, depth)
    depth[np.isinf(depth)] = 0.0
    return depth, amb


def masked_mesh(vol, weight, verts, faces, table):
    """oracle.marching_cubes output (verts, faces in cell raster order) restricted to the cells whose eight corners have
    weight > 0: the faces of the other cells dropped, the vertices no remaining face uses dropped, order kept"""
    dx, dy, dz = vol.shape
    inside = vol < 0.0
    live = weight > 0
    keep = []
    for x in range(dx - 1):
        for y in range(dy - 1):
            for z in range(dz - 1):
                cs = sum(int(inside[x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2)]) << k for k in range(8))
                nt = int((table[cs][::3][:5] >= 0).sum())
                ok = bool(live[x:x + 2, y:y + 2, z:z + 2].all())
                keep += [ok] * nt
    keep = np.array(keep, bool)
    assert len(keep) == len(faces)
    f = faces[keep]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[f].astype(np.int32), keep

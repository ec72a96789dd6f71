"""Per-stage times of the scene evaluation (eprecon_amd/evaluation.py) on a synthetic scene of ~1,000 frames, next to a CPU
comparison (scipy cKDTree for the nearest neighbours, numpy restatements of the down-sample and of eval_depth).

    python tools/eval_scene_timing.py [--frames 1000] [--height 480] [--width 640] [--chunk 32] [--out FILE.json]

The scene is the analytic room of eprecon_amd/synthetic.py: the prediction is its mesh at 4 cm, the ground truth at 2 cm, and
the "sensor" depth is the ground-truth mesh rendered at every pose.  Also reports how the rasteriser scales: the same frames
against the 8 cm mesh (about a quarter of the triangles), a quarter of the frames, and cameras close to a wall (a few large
screen-space triangles).  Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def room_poses(n, seed=0, near_wall=False):
    from eprecon_amd import synthetic as S
    rng = np.random.default_rng(seed)
    poses = []
    for i in range(n):
        t = 2 * np.pi * i / max(n, 1) * 3
        if near_wall:
            eye = np.array([rng.uniform(-1.0, 1.0), 3.25, rng.uniform(0.8, 1.8)])
            fwd = np.array([rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2)])
        else:
            eye = np.array([0.6 * np.cos(t / 3), 1.2 + 0.5 * np.sin(t / 3), 1.4 + rng.uniform(-0.1, 0.1)])
            fwd = np.array([np.sin(t), np.cos(t), -0.6 + rng.uniform(-0.1, 0.1)])
        poses.append(S._look_at_pose(eye, fwd / np.linalg.norm(fwd)))
    return np.stack(poses).astype(np.float32)


def analytic_mesh(voxel, torch):
    from eprecon_amd import save_scene as SS
    from eprecon_amd import synthetic as S
    origin = np.array([-1.92, 0.2, -0.4])
    dims = [int(round(3.84 / voxel))] * 3
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    verts, faces, _ = SS.marching_cubes(torch.from_numpy(tsdf).cuda(), 0.0)
    return verts * voxel + torch.tensor(origin, dtype=torch.float32, device="cuda"), faces


def timed(torch, fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / reps * 1e3


def down_sample_np(p, voxel):
    p = p.astype(np.float64)
    mb = p.min(0) - voxel * 0.5
    keys, inv = np.unique(np.floor((p - mb) / voxel).astype(np.int64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(keys), 3))
    np.add.at(sums, inv, p)
    return (sums / np.bincount(inv)[:, None]).astype(np.float32)


def eval_depth_np(pred, trgt):
    m1 = pred > 0
    m = (trgt < 10) & (trgt > 0) & m1
    p, t = pred[m].astype(np.float64), trgt[m].astype(np.float64)
    d = np.abs(p - t)
    th = np.maximum(t / p, p / t)
    return [np.mean(d / t), np.mean(d), np.mean(d * d / t), np.sqrt(np.mean(d * d)),
            np.sqrt(np.mean((np.log(p) - np.log(t)) ** 2)), np.mean(th < 1.25), np.mean(th < 1.5625), np.mean(th < 1.953125),
            np.mean(m1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--cpu_frames", type=int, default=50, help="frames of the numpy eval_depth comparison (scaled up)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from eprecon_amd import evaluation as E
    from eprecon_amd import synthetic as S

    h, w, n, ch = args.height, args.width, args.frames, args.chunk
    k = S.intrinsics_for(w, h)
    poses = room_poses(n)
    pv, pf = analytic_mesh(0.04, torch)
    gv, gf = analytic_mesh(0.02, torch)
    coarse_v, coarse_f = analytic_mesh(0.08, torch)
    res = {"frames": n, "image": [h, w], "chunk": ch, "pred_triangles": int(pf.shape[0]), "gt_triangles": int(gf.shape[0]),
           "gpu_ms": {}, "cpu_ms": {}, "raster_scaling_ms": {}}
    # the "sensor": the ground-truth mesh rendered at every pose (kept on the host, like frames read from disk)
    trgt = [E.render_depth(gv, gf, k, poses[i:i + ch], h, w).cpu() for i in range(0, n, ch)]
    E.render_depth(pv, pf, k, poses[:ch], h, w)                                    # warm-up (library load, first launches)

    def render_all(verts, faces, pp):
        return [E.render_depth(verts, faces, k, pp[i:i + ch], h, w) for i in range(0, len(pp), ch)]

    preds, res["gpu_ms"]["render"] = timed(torch, lambda: render_all(pv, pf, poses))
    trgt_dev = [t.cuda() for t in trgt]
    _, res["gpu_ms"]["depth_metrics"] = timed(torch, lambda: [E.depth_sums(p, t) for p, t in zip(preds, trgt_dev)])
    fusion = E.Refusion(pv)

    def fuse():
        for i, p in enumerate(preds):
            fusion.integrate(p, k, poses[i * ch:(i + 1) * ch])
    _, res["gpu_ms"]["fusion"] = timed(torch, fuse)
    res["fusion_dims"] = [int(d) for d in fusion.dims]
    mesh, res["gpu_ms"]["extraction"] = timed(torch, fusion.extract)
    tv = torch.from_numpy(mesh["vertices"]).cuda()
    (dp, dg), res["gpu_ms"]["down_sample"] = timed(torch, lambda: (E.voxel_down_sample(tv, 0.02), E.voxel_down_sample(gv, 0.02)))
    res["points"] = {"trim_vertices": int(tv.shape[0]), "pred_down": int(dp.shape[0]), "gt_down": int(dg.shape[0])}
    _, res["gpu_ms"]["nn"] = timed(torch, lambda: (E.nn_correspondance(dp, dg), E.nn_correspondance(dg, dp)))
    res["metrics"] = E.eval_mesh(tv, gv)

    # CPU comparison
    tv_np, gv_np = mesh["vertices"], gv.cpu().numpy()
    (cp, cg), res["cpu_ms"]["down_sample_numpy"] = timed(torch, lambda: (down_sample_np(tv_np, 0.02), down_sample_np(gv_np, 0.02)))
    try:
        from scipy.spatial import cKDTree
        _, res["cpu_ms"]["nn_ckdtree"] = timed(torch, lambda: (cKDTree(cp).query(cg, k=1), cKDTree(cg).query(cp, k=1)))
    except ImportError:
        res["cpu_ms"]["nn_ckdtree"] = None
    nc = min(args.cpu_frames, n)
    pred_np = torch.cat(preds)[:nc].cpu().numpy()
    trgt_np = torch.cat(trgt)[:nc].numpy()
    _, t_cpu = timed(torch, lambda: [eval_depth_np(pred_np[i], trgt_np[i]) for i in range(nc)])
    res["cpu_ms"]["depth_metrics_numpy_scaled"] = t_cpu * n / nc

    # rasteriser scaling: triangles, frames, large screen-space triangles
    sc = res["raster_scaling_ms"]
    _, sc["mesh_4cm_all_frames"] = timed(torch, lambda: render_all(pv, pf, poses))
    _, sc["mesh_8cm_all_frames"] = timed(torch, lambda: render_all(coarse_v, coarse_f, poses))
    _, sc["mesh_4cm_quarter_frames"] = timed(torch, lambda: render_all(pv, pf, poses[: n // 4]))
    near = room_poses(n, seed=1, near_wall=True)
    _, sc["mesh_4cm_near_wall_frames"] = timed(torch, lambda: render_all(pv, pf, near))
    sc["triangles_8cm"] = int(coarse_f.shape[0])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

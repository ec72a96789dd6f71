"""Time of the scene ground-truth stages at the real size: a scene of 270 x 265 x 120 cells at 4 cm with its two coarser
levels, the size the reference's own comment names.

    python tools/time_generate_gt.py [--frames 300] [--points 200000] [--reps 5] [--out FILE.json]

Reports, warmed up, the median of --reps:
    tsdf_levels_ms        fuse_scene_tsdf: --frames synthetic 480 x 640 depth frames into the three levels (wall clock,
                          uploads included; the frames sit in host memory as a loader leaves them)
    voxelize_ms[l]        voxelize_labels of a --points cloud on the room's surfaces at level l (wall clock, uploads and the
                          three volumes' way back included), and the device time of the C call alone
    fill_ms               interpolate_labels of the level-0 semantic volume (wall clock), and the device time of the three passes
The sample comes from a seed: a box room with a few blocks in it, cameras on a circle looking outward, depths from the
analytic room clipped at 3 m.  Nothing here is asserted by a test.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS, VOXEL_SIZE, ORIGIN = (270, 265, 120), 0.04, np.array([-5.4, -5.3, -0.4])
H, W = 480, 640


def cameras(n):
    k = np.array([[577.87 * W / 1296.0, 0, (W - 1) / 2], [0, 577.87 * W / 1296.0, (H - 1) / 2], [0, 0, 1.0]])
    poses = []
    for v in range(n):
        yaw = 2 * np.pi * v / n
        fwd = np.array([np.sin(yaw), np.cos(yaw), -0.2])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        p = np.eye(4)
        p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = right, np.cross(fwd, right), fwd, [0.8 * np.sin(yaw), 0.8 * np.cos(yaw), 1.4]
        poses.append(p)
    return k, np.stack(poses)


def depth_frames(n, seed=0):
    """planar depth of a wall 2.4 m ahead with seeded relief and holes: the integration's cost does not depend on the content"""
    rng = np.random.default_rng(seed)
    base = (2.4 + 0.3 * rng.standard_normal((8, H // 8, W // 8))).astype(np.float32)
    base = np.clip(np.repeat(np.repeat(base, 8, 1), 8, 2), 0.3, 3.0)
    frames = [base[v % 8] for v in range(n)]
    return frames


def cloud(n, seed=1):
    """points on the floor, the four walls and three blocks of the scene box, labelled per surface"""
    rng = np.random.default_rng(seed)
    ext = np.array(DIMS) * VOXEL_SIZE
    lo, hi = ORIGIN + 0.3, ORIGIN + ext - 0.3
    u = rng.random((n, 3))
    p = lo + u * (hi - lo)
    kind = rng.integers(0, 8, n)
    p[kind == 0, 2] = lo[2]
    p[kind == 1, 0], p[kind == 2, 0] = lo[0], hi[0]
    p[kind == 3, 1], p[kind == 4, 1] = lo[1], hi[1]
    for b, c in ((5, (-2.0, 1.0)), (6, (1.5, -2.5)), (7, (3.0, 2.0))):
        m = kind == b
        p[m, 0], p[m, 1] = c[0] + 0.6 * u[m, 0], c[1] + 0.6 * u[m, 1]
        p[m, 2] = lo[2] + 0.8 * u[m, 2]
    p += rng.normal(0, 0.005, p.shape)
    semantic = np.array([2, 1, 1, 1, 1, 5, 6, 7])[kind]
    return p, rng.uniform(0, 255, (n, 3)), semantic.astype(np.int64), (kind + 1).astype(np.int64)


def wall(fn, reps, sync):
    fn()
    out = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return {"ms_median": float(np.median(out)), "ms_min": float(np.min(out)), "ms_max": float(np.max(out))}


def events(fn, reps, torch):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(out)), "ms_min": float(np.min(out)), "ms_max": float(np.max(out))}


def main(args):
    import torch
    from eprecon_amd import _lib
    from eprecon_amd import generate_gt as GG
    lib = _lib.load()
    sync = torch.cuda.synchronize
    bnds = np.stack([ORIGIN, ORIGIN + np.array(DIMS) * VOXEL_SIZE], 1)
    levels = GG.level_volumes(bnds, VOXEL_SIZE, 3, 3)
    res = {"dims": [lv["vol_dim"].tolist() for lv in levels], "frames": args.frames, "points": args.points, "reps": args.reps}

    intr, poses = cameras(args.frames)
    depths = depth_frames(args.frames)
    res["tsdf_levels"] = wall(lambda: GG.fuse_scene_tsdf(depths, intr, poses, levels), max(args.reps // 2, 1), sync)
    vols = GG.fuse_scene_tsdf(depths, intr, poses, levels)
    res["tsdf_observed_share"] = [float((v.get_volume()[1] > 0).float().mean()) for v in vols]
    del vols

    xyz, rgb, sem, ins = cloud(args.points)
    res["voxelize"] = []
    for l, lv in enumerate(levels):
        vs, dims = VOXEL_SIZE * 2 ** l, [int(d) for d in lv["vol_dim"]]
        entry = wall(lambda: GG.voxelize_labels(xyz, rgb, sem, ins, bnds[:, 0], vs, dims), args.reps, sync)
        dev = [torch.from_numpy(a).cuda() for a in (xyz, rgb, sem, ins)]
        cells = int(np.prod(dims))
        outs = [torch.empty(cells * 3, dtype=torch.float64, device="cuda"), torch.empty(cells, dtype=torch.int64, device="cuda"),
                torch.empty(cells, dtype=torch.int64, device="cuda")]
        ws = torch.empty(int(lib.eprecon_label_volumes_workspace_bytes(len(xyz), cells)), dtype=torch.uint8, device="cuda")
        vmin = np.ascontiguousarray(bnds[:, 0])
        dims_c = (ctypes.c_int32 * 3)(*dims)
        call = lambda: _lib.check(lib.eprecon_label_volumes(
            *[_lib.ptr(t) for t in dev], len(xyz), vmin.ctypes.data_as(ctypes.c_void_p), vs, ctypes.cast(dims_c, ctypes.c_void_p),
            *[_lib.ptr(t) for t in outs], _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_label_volumes")
        entry["device"] = events(call, args.reps, torch)
        counts = torch.bincount(torch.from_numpy(np.ravel_multi_index(
            np.clip(np.rint((xyz - bnds[:, 0]) / vs).astype(np.int64), 0, np.array(dims) - 1).T, dims)))
        entry["occupied_cells"], entry["longest_list"] = int((counts > 0).sum()), int(counts.max())
        res["voxelize"].append(entry)
        if l == 0:
            sem_vol = outs[1].reshape(dims).cpu().numpy()

    res["fill_sites"] = int((sem_vol != 0).sum())
    res["fill"] = wall(lambda: GG.interpolate_labels(sem_vol), args.reps, sync)
    v = torch.from_numpy(sem_vol.astype(np.int32)).cuda()
    out = torch.empty_like(v)
    ws = torch.empty(int(lib.eprecon_label_fill_workspace_bytes(*v.shape)), dtype=torch.uint8, device="cuda")
    res["fill"]["device"] = events(lambda: GG._label_fill(lib, v, tuple(v.shape), out, workspace=ws), args.reps, torch)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    main(ap.parse_args())

"""One timing of the ray caster (eprecon_amd/raycast.py, csrc/tsdf_raycast.hip) next to the existing route to the same
pictures, on the same rows in the same process.  Print-only: it asserts nothing.

    python tools/time_raycast.py [--voxel 0.04] [--views 32] [--width 640] [--height 480] [--reps 10] [--out FILE.json]

The rows: the cells with |tsdf| < 1 of the analytic room of eprecon_amd/synthetic.py at --voxel (96^3 voxels at 4 cm, a 3-voxel
truncation).  The cameras: synthetic.make_window's arcs, --views of them.  HIP events around each call, [median, min, max] ms of
--reps after warm-up, the calls alternating rep by rep:

    build        SceneGrid: clear + build launches and the one read of the header
    cast         raycast on a built grid: the launch and the one read of the status word
    labels       raycast_labels + raycast_shaded on its result (torch, element-wise)
    mesh_route   what render.py does for the same pictures: scatter the rows into a dense volume, marching_cubes, visibility,
                 resolve (depth, two label images, shaded)
    mesh_views   visibility + resolve alone, on a mesh extracted once

`hit_share` is the share of pixels the cast hits; `agree_2_voxels` the share of the pixels hit by both routes whose depths lie
within two voxel sizes of each other.  Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def room(np, voxel):
    from eprecon_amd import synthetic as S
    origin = np.array([-1.92, 0.2, -0.4])
    dims = [int(round(3.84 / voxel))] * 3
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    coords = np.argwhere(np.abs(tsdf) < 1)
    b = coords // 16
    return coords.astype(np.int32), tsdf[tuple(coords.T)], (1 + (b[:, 0] + 3 * b[:, 1]) % 5).astype(np.int32), \
        (1 + b[:, 2] % 6).astype(np.int32), origin, dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from time_render import event_ms
    from eprecon_amd import raycast as RC, render as RD, synthetic as S
    from eprecon_amd.save_scene import marching_cubes
    from eprecon_amd.scene_io import scatter_volumes

    coords, tsdf, sem, ins, origin, dims = room(np, args.voxel)
    h, w = args.height, args.width
    k = S.intrinsics_for(w, h)
    poses = np.concatenate([S.make_window(seed=s, width=w, height=h, advance=0.1 * s)["poses"].astype(np.float64)
                            for s in range((args.views + 8) // 9)])[:args.views]
    to = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    c_dev, t_dev, sem_dev, ins_dev = to(coords, torch.int32), to(tsdf, torch.float32), to(sem, torch.int32), to(ins, torch.int32)
    origin_dev = to(origin, torch.float32).reshape(1, 3)
    grid = RC.SceneGrid(c_dev, t_dev, origin, args.voxel)
    out = RC.raycast(grid, k, poses, h, w)

    def mesh():
        vols = scatter_volumes(dims, coords, {"tsdf": tsdf, "semantic": sem, "instance": ins}, "cuda")
        verts, faces, _, vsem, vins = marching_cubes(vols["tsdf"], 0.0, labels=(vols["semantic"], vols["instance"]))
        return verts * args.voxel + origin_dev, faces, vsem, vins

    def views(m):
        verts, faces, vsem, vins = m
        vis = RD.visibility(verts, faces, k, poses, h, w, cull_back=False)
        return RD.resolve(vis, verts, faces, k, poses, labels=(vsem, vins), colors=RD.palette_colors(vins), outputs=("depth", "rgb"))

    def pictures():
        RC.raycast_labels(grid, out, sem_dev, ins_dev)
        return RC.raycast_shaded(grid, out, k, poses, RD.palette_colors(ins_dev))

    once = mesh()
    ms = event_ms(torch, {
        "build": lambda: RC.SceneGrid(c_dev, t_dev, origin, args.voxel),
        "cast": lambda: RC.raycast(grid, k, poses, h, w),
        "labels": pictures,
        "mesh_route": lambda: views(mesh()),
        "mesh_views": lambda: views(once),
    }, args.reps)
    theirs = views(once)["depth"]
    both = (out["depth"] > 0) & (theirs > 0)
    close = ((out["depth"] - theirs).abs() <= 2 * args.voxel) & both
    res = {"voxel": args.voxel, "dims": dims, "rows": int(len(coords)), "non_positive_rows": int((tsdf <= 0).sum()),
           "grid_bytes": int(grid.mem.numel()), "views": int(len(poses)), "height": h, "width": w, "reps": args.reps, "ms": ms,
           "faces": int(once[1].shape[0]), "hit_share": float((out["row"] >= 0).float().mean()),
           "mesh_hit_share": float((theirs > 0).float().mean()),
           "agree_2_voxels": float(close.sum()) / max(float(both.sum()), 1.0),
           "ns_per_pixel_cast": 1e6 * ms["cast"][0] / (len(poses) * h * w),
           "mesh_route_over_build_cast_labels": ms["mesh_route"][0] / (ms["build"][0] + ms["cast"][0] + ms["labels"][0])}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

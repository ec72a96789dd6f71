"""One timing of vertex colouring (eprecon_amd/colorize.py, csrc/mesh_colorize.hip) next to a torch composition of the same
rule on the same inputs in the same process.

    python tools/time_colorize.py [--views 32] [--height 968] [--width 1296] [--voxel 0.04] [--reps 20] [--out FILE.json]

One chunk: --views frames of --width x --height (ScanNet's colour size) over marching cubes of the analytic room of
eprecon_amd/synthetic.py at --voxel (tools/eval_scene_timing.py's mesh, 96^3 voxels at 4 cm), seen from its walk through
the room; seeded random bytes as frames, on the device.  HIP events around each call, [median, min, max] ms of --reps after
warm-up, the calls alternating rep by rep:

    accumulate        the C entry alone on a camera block and a visibility buffer made once (with the two memsets of its state)
    accumulate_away   the same with every camera a kilometre back: all waves skip all views (what the projection alone costs)
    integrate         MeshColorizer.integrate: the camera block, render.visibility at 640 x 480, the entry
    torch             projection, visibility lookup and facing in fp64 tensors, grid_sample (fp32, align_corners) for the
                      bilinear sample, masked weighted sums: the same rule as tensor expressions

`pairs_kept` counts the (vertex, view) pairs that contribute; `ns_per_pair` and `ns_per_candidate` (all vertices x views)
divide the accumulate time by them.  `torch_max_level_diff` is the largest difference of a final channel between the two
(grid_sample interpolates in fp32).  Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def torch_rule(torch, verts, faces, frames_f32, vis, k, k_vis, w2c, pc, znear, zfar, tolerance, min_cos):
    """acc f64[N,4], seen int64[N] of one chunk as tensor expressions (frames_f32: [V,3,H,W] float32)"""
    v64 = verts.double()
    n_views, _, hc, wc = frames_f32.shape
    hd, wd = vis.shape[1:]
    acc = torch.zeros((verts.shape[0], 4), dtype=torch.float64, device=verts.device)
    seen = torch.zeros(verts.shape[0], dtype=torch.int64, device=verts.device)
    words = vis.view(torch.int64)
    for v in range(n_views):
        q = v64 @ w2c[v, :, :3].T + w2c[v, :, 3]
        z = q[:, 2]
        keep = (z >= znear) & (z <= zfar)
        zs = torch.where(keep, z, torch.ones_like(z))
        ud, vd = (q @ k_vis[0]) / zs, (q @ k_vis[1]) / zs
        cd, rd = torch.floor(ud - pc + 0.5), torch.floor(vd - pc + 0.5)
        keep &= (cd >= 0) & (cd <= wd - 1) & (rd >= 0) & (rd <= hd - 1)
        word = words[v, rd.clamp(0, hd - 1).long(), cd.clamp(0, wd - 1).long()]
        bits, tri = (word >> 32) & 0xFFFFFFFF, word & 0xFFFFFFFF
        keep &= (bits < 0x7F800000) & (tri < faces.shape[0])
        depth = bits.to(torch.int32).view(torch.float32).double()
        keep &= z <= depth + tolerance
        corners = v64[faces[tri.clamp(0, faces.shape[0] - 1)].long()] @ w2c[v, :, :3].T + w2c[v, :, 3]      # [N,3,3]
        n = torch.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], dim=1)
        nlen = n.norm(dim=1)
        cosine = (n * q).sum(1).abs() / (nlen * q.norm(dim=1)).clamp_min(1e-300)
        keep &= (nlen > 0) & (cosine >= min_cos)
        x, y = (q @ k[0]) / zs - pc, (q @ k[1]) / zs - pc
        keep &= (x >= 0) & (x <= wc - 1) & (y >= 0) & (y <= hc - 1)
        grid = torch.stack([x / (wc - 1) * 2 - 1, y / (hc - 1) * 2 - 1], -1).float().reshape(1, 1, -1, 2)
        sample = torch.nn.functional.grid_sample(frames_f32[v:v + 1], grid, mode="bilinear", align_corners=True)[0, :, 0].T.double()
        w = torch.where(keep, cosine / (zs * zs), torch.zeros_like(z))
        acc[:, :3] += w[:, None] * sample
        acc[:, 3] += w
        seen += keep
    return acc, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--height", type=int, default=968)
    ap.add_argument("--width", type=int, default=1296)
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from eval_scene_timing import analytic_mesh, room_poses
    from time_render import event_ms
    from eprecon_amd import _lib
    from eprecon_amd import colorize as CZ
    from eprecon_amd import render as RD
    from eprecon_amd import synthetic as S

    h, w, n = args.height, args.width, args.views
    k = S.intrinsics_for(w, h)
    poses = room_poses(n).astype(np.float64)
    away = poses.copy()
    away[:, :3, 3] = poses[:, :3, 3] - 1000.0 * poses[:, :3, 2]                   # a kilometre back: everything beyond zfar
    verts, faces = analytic_mesh(args.voxel, torch)
    nv = verts.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    col = CZ.MeshColorizer(verts, faces, tolerance=args.voxel)
    wd, hd = RD.NATIVE_SIZE
    k_vis = RD.scaled_intrinsics(k, (wd, hd), native=(w, h))
    vis = RD.visibility(col.verts, col.faces, k_vis, poses, hd, wd)
    vis_away = RD.visibility(col.verts, col.faces, k_vis, away, hd, wd)

    def fresh(fn):
        col.acc.zero_()
        col.seen.zero_()
        fn()

    frames_f32 = frames.permute(0, 3, 1, 2).float().contiguous()
    dev64 = lambda a: torch.from_numpy(np.asarray(a, np.float64)).cuda()
    w2c = dev64(np.linalg.inv(poses)[:, :3, :4])
    rule = (0.5, float(np.float32(0.05)), 100.0, args.voxel, 0.1)
    torch_call = lambda: torch_rule(torch, col.verts, col.faces, frames_f32, vis, dev64(k), dev64(k_vis), w2c, *rule)
    lib = _lib.load()

    def entry(buffer, cameras):
        cams = dev64(np.concatenate([np.asarray(k, np.float64).ravel(), k_vis.ravel(), np.linalg.inv(cameras)[:, :3, :4].ravel()]))
        call = lambda: lib.eprecon_colorize_accumulate_async(
            _lib.ptr(col.verts), nv, _lib.ptr(col.faces), faces.shape[0], _lib.ptr(cams), n, _lib.ptr(frames), h, w, _lib.ptr(buffer),
            hd, wd, 0.5, 0.05, 100.0, args.voxel, 0.1, _lib.ptr(col.acc), _lib.ptr(col.seen), _lib.current_stream())
        return lambda: fresh(call)

    ms = event_ms(torch, {
        "accumulate": entry(vis, poses),
        "accumulate_away": entry(vis_away, away),
        "integrate": lambda: fresh(lambda: col.integrate(frames, k, poses)),
        "torch": torch_call,
    }, args.reps)
    fresh(lambda: col.accumulate(frames, vis, k, k_vis, poses))
    first = col.acc.clone()
    fresh(lambda: col.integrate(frames, k, poses))
    same = torch.equal(first, col.acc)
    rgb, seen = col.colors()
    t_acc, t_seen = torch_call()
    t_rgb = torch.where(t_acc[:, 3:] > 0, torch.floor(t_acc[:, :3] / t_acc[:, 3:].clamp_min(1e-300) + 0.5).clamp(max=255.0),
                        torch.full_like(t_acc[:, :3], 153.0))
    both = (seen > 0) & (t_seen > 0)
    pairs = int(seen.sum())
    acc_ms = ms["accumulate"][0]
    res = {"views": n, "frame": [h, w], "visibility": [hd, wd], "voxel": args.voxel, "vertices": int(nv), "triangles": int(faces.shape[0]),
           "reps": args.reps, "ms": ms, "torch_over_integrate": ms["torch"][0] / ms["integrate"][0],
           "torch_over_accumulate": ms["torch"][0] / acc_ms, "pairs_kept": pairs, "candidates": int(nv) * n,
           "ns_per_pair": 1e6 * acc_ms / max(pairs, 1), "ns_per_candidate": 1e6 * acc_ms / max(int(nv) * n, 1),
           "seen_fraction": float((seen > 0).float().mean()), "integrate_bit_equal_accumulate": bool(same),
           "torch_seen_mismatch": int((seen.long() != t_seen).sum()),
           "torch_max_level_diff": float((rgb.double() - t_rgb)[both].abs().max()) if bool(both.any()) else 0.0}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

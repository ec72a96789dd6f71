"""One timing of the mesh simplification (eprecon_amd/simplify.py, csrc/mesh_simplify.hip) next to a torch composition of the
same rule on the same mesh in the same process.

    python tools/time_simplify.py [--voxel 0.04] [--cells 0.08 0.16] [--reps 20] [--out FILE.json]

The mesh: marching cubes of tools/time_clean_scene.py's room (the analytic room of eprecon_amd/synthetic.py at --voxel, a
3-voxel truncation) with labels in 16^3-cell blocks and seeded colours, in world metres.  Per cell size, HIP events around
each call, [median, min, max] ms of --reps after warm-up, the calls alternating rep by rep:

    keys             eprecon_simplify_keys_async alone
    faces            eprecon_simplify_faces_async alone, on the cluster ids computed once
    lists            the two eprecon_segment_lists_async calls (corner entries, member vertices)
    quadrics         eprecon_simplify_quadrics_async alone, one lane per cluster, on lists built once
    simplify_device  the whole call: keys, ranks, faces, first faces, lists, quadrics, compaction, report, three host reads
    torch_quadrics   the yardstick for `quadrics`: the same per-cluster outputs from per-corner quadrics summed with index_add_
                     in float64, torch.linalg.solve and the same clip

`largest_difference_cells` is the largest distance between the kernel's and the yardstick's positions, in cells (index_add_
sums in no fixed order: the two agree to rounding, not to the bit).  Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def room_mesh(torch, np, voxel):
    """-> (verts f32[N,3] world metres, faces int32[M,3], semantic, instance int32[N], colors u8[N,3]) on the device, dims"""
    from eprecon_amd import synthetic as S
    from eprecon_amd.save_scene import marching_cubes
    origin = np.array([-1.92, 0.2, -0.4])
    dims = [int(round(3.84 / voxel))] * 3
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    i, j, k = np.meshgrid(*[np.arange(d) // 16 for d in dims], indexing="ij")
    sem, ins = (1 + (i + 3 * j) % 5).astype(np.int32), (1 + k % 6).astype(np.int32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    verts, faces, _, vs, vi = marching_cubes(to(tsdf), 0.0, labels=(to(sem), to(ins)))
    verts = (verts * float(voxel) + to(origin.astype(np.float32)).reshape(1, 3)).contiguous()
    colors = to(np.random.default_rng(0).integers(0, 256, (verts.shape[0], 3)).astype(np.uint8))
    return (verts, faces, vs, vi, colors), dims


def torch_quadrics(torch, verts, faces, colors, cluster, tri, k, cell, regularize):
    """positions f64[k,3], normals f32[k,3], rgb u8[k,3] of the rule from torch calls (origin zero)"""
    v = verts.double()
    cl = cluster.long()
    centre_v = (torch.floor(v / cell) + 0.5) * cell
    centre = torch.zeros((k, 3), dtype=torch.float64, device=v.device)
    centre[cl] = centre_v
    count = torch.bincount(cl, minlength=k)
    mean = torch.zeros((k, 3), dtype=torch.float64, device=v.device).index_add_(0, cl, v - centre_v) / count.clamp(min=1)[:, None]
    f = faces.long()
    pa, pb, pc = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.linalg.cross(pb - pa, pc - pa)
    length = n.square().sum(1).sqrt()
    u = n / length.clamp(min=1e-300)[:, None]
    w = torch.where(length > 0, length / 2, torch.zeros_like(length))
    outer = w[:, None, None] * u[:, :, None] * u[:, None, :]
    a = torch.zeros((k, 3, 3), dtype=torch.float64, device=v.device)
    b = torch.zeros((k, 3), dtype=torch.float64, device=v.device)
    ns = torch.zeros((k, 3), dtype=torch.float64, device=v.device)
    for c in range(3):
        t = tri[:, c].long()
        d = -(u * (pa - centre[t])).sum(1)
        a.index_add_(0, t, outer)
        b.index_add_(0, t, (-w * d)[:, None] * u)
        ns.index_add_(0, t, n)
    trace = a.diagonal(dim1=1, dim2=2).sum(1)
    lam = regularize * trace / 3.0
    solvable = trace > 0
    eye = torch.eye(3, dtype=torch.float64, device=v.device)
    lhs = a + torch.where(solvable, lam, torch.ones_like(lam))[:, None, None] * eye
    x = torch.linalg.solve(lhs, b + lam[:, None] * mean)
    x = torch.where(solvable[:, None], x, mean)
    step = x - mean
    half = 0.5 * cell
    bound = torch.where(step > 0, (half - mean) / step, torch.where(step < 0, (-half - mean) / step, torch.full_like(step, 1.0)))
    t = bound.min(1).values.clamp(0.0, 1.0)
    pos = centre + (mean + t[:, None] * step).clamp(-half, half)
    nl = ns.square().sum(1).sqrt()
    normal = torch.where(nl[:, None] > 0, ns / nl.clamp(min=1e-300)[:, None], torch.zeros_like(ns)).float()
    total = torch.zeros((k, 3), dtype=torch.int64, device=v.device).index_add_(0, cl, colors.long())
    rgb = ((2 * total + count[:, None]) // (2 * count.clamp(min=1)[:, None])).to(torch.uint8)
    return pos, normal, rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--cells", type=float, nargs="+", default=[0.08, 0.16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from time_render import event_ms
    from eprecon_amd import _lib
    from eprecon_amd import simplify as SM

    (verts, faces, sem, ins, colors), dims = room_mesh(torch, np, args.voxel)
    n, m = verts.shape[0], faces.shape[0]
    lib = _lib.load()
    origin = np.zeros(3, np.float64)
    res = {"voxel": args.voxel, "dims": dims, "vertices": int(n), "faces": int(m), "reps": args.reps, "cells": {}}
    for cell in args.cells:
        out = SM.simplify_device(verts, faces, cell, sem, ins, colors)
        cluster, tri, k = out["cluster"], out["tri"], out["report"]["clusters"]
        key = torch.empty(n, dtype=torch.int64, device="cuda")
        status = torch.empty(1, dtype=torch.int32, device="cuda")
        tri2, face_key = torch.empty_like(tri), torch.empty(m, dtype=torch.int64, device="cuda")
        marks = torch.empty(k, dtype=torch.uint8, device="cuda")
        pos = torch.empty((k, 3), dtype=torch.float64, device="cuda")
        normal = torch.empty((k, 3), dtype=torch.float32, device="cuda")
        rgb = torch.empty((k, 3), dtype=torch.uint8, device="cuda")
        p = _lib.ptr

        def keys():
            return lib.eprecon_simplify_keys_async(p(verts), n, origin.ctypes.data, cell, p(key), p(status), _lib.current_stream())

        def face_pass():
            return lib.eprecon_simplify_faces_async(p(faces), m, p(cluster), n, k, p(tri2), p(face_key), p(marks), p(status),
                                                    _lib.current_stream())

        def lists():
            return SM._segment_lists(tri.reshape(-1), k), SM._segment_lists(cluster, k)

        keys()
        (c_off, c_ord), (m_off, m_ord) = lists()

        def quadrics():
            return lib.eprecon_simplify_quadrics_async(p(verts), n, p(faces), m, p(colors), p(key), p(c_off), p(c_ord), p(m_off), p(m_ord), k,
                                                       origin.ctypes.data, cell, 1e-3, p(pos), p(normal), p(rgb), _lib.current_stream())

        ms = event_ms(torch, {
            "keys": keys,
            "faces": face_pass,
            "lists": lists,
            "quadrics": quadrics,
            "simplify_device": lambda: SM.simplify_device(verts, faces, cell, sem, ins, colors),
            "torch_quadrics": lambda: torch_quadrics(torch, verts, faces, colors, cluster, tri, k, cell, 1e-3),
        }, args.reps)
        quadrics()
        want = torch_quadrics(torch, verts, faces, colors, cluster, tri, k, cell, 1e-3)
        corner_counts = (c_off[1:] - c_off[:-1])
        res["cells"][str(cell)] = {
            "report": out["report"], "ms": ms,
            "corner_entries_per_cluster": [float(corner_counts.float().mean()), int(corner_counts.max())],
            "largest_difference_cells": float((pos - want[0]).abs().max()) / cell,
            "bits_equal_to_whole_call": bool(torch.equal(pos.view(torch.int64), out["positions"].view(torch.int64))),
            "rgb_equal": bool(torch.equal(rgb, want[2])),
            "torch_over_quadrics": ms["torch_quadrics"][0] / ms["quadrics"][0]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

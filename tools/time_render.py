"""One timing of view rendering (eprecon_amd/render.py: visibility + resolve) next to the depth render it shares its rasteriser
with, on the same mesh and views in the same process.

    python tools/time_render.py [--views 32] [--height 480] [--width 640] [--reps 20] [--out FILE.json]

The mesh is the analytic room of eprecon_amd/synthetic.py at 4 cm (tools/eval_scene_timing.py's), the views its walk
through the room.  HIP events around each call, [median, min, max] of --reps after warm-up, the calls of
a block alternating rep by rep.  `ms` times the Python calls, which
include what the wrappers do per call (the camera block with its inverses on the host and its copy, the buffers);
`entry_ms` times the C entries alone on buffers made once.  `resolve_labels` writes two label images, `resolve_rgb` the
shaded image, `resolve_all` depth, face, corner, two label images and the shaded image.  Writes nothing into the
repository unless --out is given.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def event_ms(torch, calls, reps, warmup=3):
    """{name: call} -> {name: [median, min, max] ms}: the calls alternate rep by rep, so that whatever else the machine does
    during the measurement falls on all of them alike"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: [statistics.median(t), min(t), max(t)] for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from eval_scene_timing import analytic_mesh, room_poses
    from eprecon_amd import evaluation as E
    from eprecon_amd import render as RD
    from eprecon_amd import synthetic as S

    h, w, n = args.height, args.width, args.views
    k = S.intrinsics_for(w, h)
    poses = room_poses(n)
    verts, faces = analytic_mesh(0.04, torch)
    nv = verts.shape[0]
    sem = (torch.arange(nv, device="cuda") % 21).to(torch.int32)
    ins = (torch.arange(nv, device="cuda") % 97).to(torch.int32)
    col = RD.palette_colors(sem)
    vis = RD.visibility(verts, faces, k, poses, h, w)
    ms = event_ms(torch, {
        "render_depth": lambda: E.render_depth(verts, faces, k, poses, h, w),
        "visibility": lambda: RD.visibility(verts, faces, k, poses, h, w),
        "resolve_labels": lambda: RD.resolve(vis, verts, faces, k, poses, labels=(sem, ins), outputs=()),
        "resolve_all": lambda: RD.resolve(vis, verts, faces, k, poses, labels=(sem, ins), colors=col),
    }, args.reps)
    # the C entries alone: the camera block, the buffers and the workspace made once (the wrappers rebuild them per call)
    import numpy as np
    from eprecon_amd import _lib
    lib = _lib.load()
    k64, p64 = np.asarray(k, np.float64).reshape(3, 3), np.asarray(poses, np.float64).reshape(-1, 4, 4)
    cams = torch.from_numpy(np.concatenate([k64.ravel(), np.linalg.inv(k64).ravel(), np.linalg.inv(p64)[:, :3, :4].ravel()])).cuda()
    f32, i32 = verts.to(torch.float32).contiguous(), faces.to(torch.int32).contiguous()
    cap = int(min(n * faces.shape[0], 1 << 22))
    ws = torch.empty(int(lib.eprecon_render_visibility_workspace_bytes(cap)), dtype=torch.uint8, device="cuda")
    zbuf = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    vbuf = torch.empty((n, h, w), dtype=torch.int64, device="cuda")
    la, lb = (torch.empty((n, h, w), dtype=torch.int32, device="cuda") for _ in range(2))
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    mesh = (_lib.ptr(f32), nv, _lib.ptr(i32), faces.shape[0], _lib.ptr(cams), n, h, w)
    raster = mesh + (0.5, 0.05, 100.0, 1)
    tail = (cap, _lib.ptr(ws), ws.numel(), _lib.current_stream())

    def entry(fn, *a):
        assert fn(*a) == 0

    dev_ms = event_ms(torch, {
        "render_depth": lambda: entry(lib.eprecon_render_depth_async, *raster, _lib.ptr(zbuf), *tail),
        "visibility": lambda: entry(lib.eprecon_render_visibility_async, *raster, _lib.ptr(vbuf), *tail),
        "resolve_labels": lambda: entry(
            lib.eprecon_render_resolve_async, _lib.ptr(vbuf), *mesh, 0.5, None, None, None, _lib.ptr(sem), 0, _lib.ptr(la),
            _lib.ptr(ins), 0, _lib.ptr(lb), None, 0.3, 255, 255, 255, None, _lib.current_stream()),
        "resolve_rgb": lambda: entry(
            lib.eprecon_render_resolve_async, _lib.ptr(vbuf), *mesh, 0.5, None, None, None, None, 0, None, None, 0, None,
            _lib.ptr(col), 0.3, 255, 255, 255, _lib.ptr(rgb), _lib.current_stream()),
    }, args.reps)
    assert torch.equal(vbuf, vis.view(torch.int64))
    depth = E.render_depth(verts, faces, k, poses, h, w)
    same = torch.equal(RD.resolve(vis, verts, faces, k, poses, outputs=("depth",))["depth"].view(torch.int32), depth.view(torch.int32))
    res = {"views": n, "image": [h, w], "triangles": int(faces.shape[0]), "vertices": int(nv), "reps": args.reps, "ms": ms,
           "visibility_over_render_depth": ms["visibility"][0] / ms["render_depth"][0], "entry_ms": dev_ms,
           "entry_visibility_over_render_depth": dev_ms["visibility"][0] / dev_ms["render_depth"][0],
           "covered_fraction": float((depth > 0).float().mean()), "depth_bit_equal": bool(same)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

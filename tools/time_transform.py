"""Time of one sample of the fragment ground-truth transform at the real size: a 96^3 fragment, nine 480 x 640 views,
a scene of 270 x 265 x 120 cells with its two coarser levels.

    python tools/time_transform.py [--reps 20] [--out FILE.json]     eprecon_amd.transforms on the GPU: device events around
                                                                     RandomTransformSpace.__call__, warmed up, median of --reps
    python tools/time_transform.py --once                            one warm call and one more (the run to put under
                                                                     rocprofv3 --kernel-trace --stats)
    python tools/time_transform.py --reference                       the reference's transform on the CPU for the same seeded
                                                                     sample (build container only: tests/golden/ref_shim.py)

The sample comes from a seed: scene TSDF clip(N(0,1), -1, 1), integer colours and labels, depths uniform in 0.3-2.5 m, cameras
on a short arc — the layout of tests/transform_ref.py at the real size.  The seeded inputs are that module's (make_inputs,
camera_poses, sample_dict): the tool imports them from the test tree so that the timed sample and the tested one cannot drift apart.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_VOX, VOXEL_SIZE, VIEWS, H, W = (96, 96, 96), 0.04, 9, 480, 640
SCENE_DIMS = [(270, 265, 120), (135, 133, 60), (68, 67, 30)]
SCENE_ORIGIN = (-4.1, -2.3, -0.35)


def sample():
    import transform_ref as R
    inp = R.make_inputs(0, True, SCENE_ORIGIN, SCENE_DIMS, VIEWS, H, W)
    f = 577.87 * W / 1296.0
    inp["intrinsics"] = np.stack([np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], np.float32)] * VIEWS)
    inp["extrinsics"] = R.camera_poses(VIEWS)
    inp["extrinsics"][:, 2, 3] = 1.4
    return inp


def time_hip(args):
    import torch
    import transform_ref as R
    from eprecon_amd import transforms as T
    inp = sample()
    t0 = time.perf_counter()
    scene = T.SceneVolumes(*[inp[k] for k in ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full")])
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    torch.manual_seed(0)
    rts = T.RandomTransformSpace(list(N_VOX), VOXEL_SIZE, True, True, 1.5, 0.25, max_epoch=4)
    depth_dev = torch.from_numpy(inp["depth"]).cuda()

    def one(resident_depth):
        data = R.sample_dict(inp, torch, scene=scene)
        if resident_depth:
            data["depth"] = depth_dev
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        a.record()
        out = rts(data)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t) * 1e3, out

    for _ in range(3):
        one(False)
    if args.once:
        one(False)
        return
    res = {"fragment": list(N_VOX), "views": [VIEWS, H, W], "scene_dims": SCENE_DIMS, "reps": args.reps,
           "scene_upload_ms_once": upload_ms}
    for name, resident in (("depth_from_host", False), ("depth_on_device", True)):
        ev, wall = zip(*[one(resident)[:2] for _ in range(args.reps)])
        res[name] = {"event_ms_median": float(np.median(ev)), "event_ms_min": float(np.min(ev)), "event_ms_max": float(np.max(ev)),
                     "wall_ms_median": float(np.median(wall))}
    out = one(False)[2]
    res["in_band_share"] = [float((t.abs() < 1).float().mean()) for t in out["tsdf_list"]]
    cells = sum(int(np.prod(t.shape)) for t in out["tsdf_list"])
    res["crop_output_bytes"] = cells * 4 * 6          # tsdf + 3 colour + 2 labels, f32
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


def time_reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_shim
    torch = ref_shim.install()
    import transform_ref as R
    from datasets import transforms as RT
    inp = sample()
    torch.manual_seed(0)
    rts = RT.RandomTransformSpace(list(N_VOX), VOXEL_SIZE, True, True, 1.5, 0.25, max_epoch=4)
    times, convert = [], []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        data = R.sample_dict(inp, torch)       # (the copies stand in for ToTensor's torch.Tensor(volume) of every sample)
        t1 = time.perf_counter()
        rts(data)
        times.append((time.perf_counter() - t1) * 1e3)
        convert.append((t1 - t0) * 1e3)
    res = {"reference_transform_cpu_ms_median": float(np.median(times[1:])), "min": float(np.min(times[1:])),
           "max": float(np.max(times[1:])), "volume_copy_ms_median": float(np.median(convert[1:])), "reps": args.reps,
           "threads": torch.get_num_threads()}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    (time_reference if a.reference else time_hip)(a)

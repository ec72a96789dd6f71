"""What preparing a fragment's views costs, on the host (the reference's way) and on the device, in one process.

    python tools/time_views.py [--views 9] [--reps 50] [--out FILE.json]

Inputs: --views decoded 1296 x 968 colour frames (seeded noise over a smooth field) and as many 640 x 480 uint16 depth
frames, the sizes of a ScanNet fragment; decoding is not part of any figure.  After warm-up, --reps repetitions, the two
wall-clock paths alternating rep by rep, each ending in a device synchronise:
  host_ms      ResizeImage + ToTensor + .to(device) of imgs and depth (needs PIL; "not measurable here" without it)
  device_ms    PrepareViews: staging into the pinned buffer, the one copy, both launches
  kernel_ms    eprecon_prepare_views_async alone between device events on resident frames, with the bytes it must move
               (frames in, floats out) over that time against the HBM peak; depth_kernel_ms likewise
Every entry is [median, min, max] in ms.  The two paths' outputs are compared bit for bit before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, the datasheet's
HBM_COPY = 6.29e12         # what a float4 copy reaches on this part


def spread(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from eprecon_amd import transforms as T
    assert torch.cuda.is_available(), "time_views needs a GPU"
    dev = torch.device("cuda")
    v, (h, w), size = args.views, (968, 1296), (640, 480)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w]
    field = np.stack([x % 256, (y * 2) % 256, (x + y) // 5 % 256], -1).astype(np.uint8)
    frames = [field ^ rng.integers(0, 64, field.shape, dtype=np.uint8) for _ in range(v)]
    depth_mm = [rng.integers(0, 6000, (size[1], size[0])).astype(np.uint16) for _ in range(v)]
    k = np.stack([np.array([[1170.2, 0, 647.7], [0, 1170.2, 483.8], [0, 0, 1]], np.float32)] * v)
    poses = np.stack([np.eye(4)] * v)

    def sample(imgs, depth):
        return {"imgs": list(imgs), "depth": list(depth), "intrinsics": k.copy(), "extrinsics": poses.copy()}

    stage = T.PrepareViews(size, device=dev)

    def device_path():
        out = stage(sample(frames, depth_mm))
        torch.cuda.synchronize()
        return out

    try:
        from PIL import Image
        pil = [Image.fromarray(f) for f in frames]
        depth_m = []
        for d in depth_mm:
            m = d.astype(np.float32)
            m /= 1000.
            m[m > 3.0] = 0
            depth_m.append(m)
        resize, to_tensor = T.ResizeImage(size), T.ToTensor()

        def host_path():
            out = to_tensor(resize(sample(pil, depth_m)))
            out["imgs"], out["depth"] = out["imgs"].to(dev), out["depth"].to(dev)
            torch.cuda.synchronize()
            return out
    except ImportError:
        host_path = None

    got = device_path()
    res = {"views": v, "frame": [h, w], "size": list(size), "reps": args.reps}
    if host_path is not None:
        want = host_path()
        res["bit_equal"] = bool(torch.equal(got["imgs"], want["imgs"]) and torch.equal(got["depth"], want["depth"])
                                and torch.equal(got["intrinsics"], want["intrinsics"]))
        assert res["bit_equal"]
    paths = {"device_ms": device_path}
    if host_path is not None:
        paths["host_ms"] = host_path
    else:
        res["host_ms"] = "not measurable here"
    for fn in paths.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in paths}
    for _ in range(args.reps):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t0))
    res.update({name: spread(ts) for name, ts in times.items()})

    # the kernels alone, on resident inputs
    resident = torch.from_numpy(np.stack(frames)).to(dev)
    mm = torch.from_numpy(np.stack(depth_mm).view(np.int16)).to(dev)
    out = torch.empty((v, 3, size[1], size[0]), dtype=torch.float32, device=dev)
    calls = {"kernel_ms": lambda: T.prepare_views(resident, size, 2, 2, out=out), "depth_kernel_ms": lambda: T.depth_to_metres(mm)}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        res[name] = spread(ts)
    moved = resident.numel() + out.numel() * 4
    rate = moved / (res["kernel_ms"][0] * 1e-3)
    res.update(kernel_bytes=moved, kernel_bytes_per_s=rate, kernel_fraction_of_hbm_peak=rate / HBM_PEAK,
               kernel_fraction_of_hbm_copy=rate / HBM_COPY)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""One timing of the distance field (eprecon_amd/distance_field.py, csrc/distance_field.hip) next to a torch composition of the
same banded rule on the same rows in the same process.

    python tools/time_distance_field.py [--voxel 0.04] [--reps 10] [--torch_reps 3] [--out FILE.json]

The rows: the cells with |tsdf| < 1 of the analytic room of eprecon_amd/synthetic.py sampled on tools/time_generate_gt.py's
270 x 265 x 120 lattice at --voxel, in a seeded random order.  The box is the lattice itself.  Per max_distance (0.5 m, 2 m and
None, which is unbounded):

    call        distance_field() whole: the bounding-box read, the allocations, the six launches, the crop; HIP events,
                [median, min, max] ms of --reps after warm-up
    launches    the device time of every launch of one call, by kernel, from torch.profiler's device records: [median, min,
                max] us over --reps calls
    bytes       what the three passes must move at the least (each reads and writes one 8-byte key per cell; the last writes two
                int32 instead), and the HBM rate that is at the passes' summed time, against the 8.0 TB/s of the datasheet
    torch       the yardstick: per axis, the far-padded key volume unfolded into windows of 2 R + 1, the squared offsets added
                where a key is not far, and amin — the same minimum over the same packed keys, seeded with the kernel's own
                sites.  Run where the unfolded windows (cells x (2 R + 1) x 8 bytes, twice) fit in --torch_bytes; `equal` says
                that its dist2 and site are the kernel's

Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12          # bytes/s, the datasheet's
FAR_KEY = 0x7fffffff7fffffff
PASSES = ("df_pass_z_kernel", "df_pass_kernel<false>", "df_pass_kernel<true>")


def spread(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def room_rows(torch, np, dims, voxel, origin):
    from eprecon_amd import synthetic as S
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    coords = np.argwhere(np.abs(tsdf) < 1)
    coords = coords[np.random.default_rng(0).permutation(len(coords))]
    to = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    return to(coords, torch.int32), to(tsdf[tuple(coords.T)], torch.float32)


def launch_times(torch, fn, reps):
    """{kernel: [median, min, max] us} over `reps` calls of fn, and the calls' launch counts"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    per, counts = {}, []
    for _ in range(reps):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        device = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
        counts.append(len(device))
        once = {}
        for e in device:
            once[e.name] = once.get(e.name, 0.0) + e.time_range.elapsed_us()
        for name, us in once.items():
            per.setdefault(name, []).append(us)
    return {name: spread(ts) for name, ts in per.items()}, counts


def torch_banded(torch, seed, radius):
    """seed: int64 [X,Y,Z] keys (d2 << 32) | row, FAR_KEY where nothing is -> (dist2, site) int32 by unfold + amin per axis"""
    vol = seed
    for axis in (2, 1, 0):
        n = vol.shape[axis]
        reach = min(radius, n - 1)
        shape = list(vol.shape)
        shape[axis] = n + 2 * reach
        padded = torch.full(shape, FAR_KEY, dtype=torch.int64, device=vol.device)       # (F.pad would take the key through a double)
        padded.narrow(axis, reach, n).copy_(vol)
        windows = padded.unfold(axis, 2 * reach + 1, 1)
        k = torch.arange(-reach, reach + 1, device=vol.device, dtype=torch.int64)
        vol = torch.where(windows == FAR_KEY, windows, windows + ((k * k) << 32)).amin(-1)
    d2, row = vol >> 32, vol & 0xffffffff
    far = (vol == FAR_KEY) | (d2 > radius * radius)
    return torch.where(far, 0x7fffffff, d2).to(torch.int32), torch.where(far, -1, row).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch_reps", type=int, default=3)
    ap.add_argument("--torch_bytes", type=float, default=64e9, help="run the torch composition where its windows fit in this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from time_generate_gt import DIMS, ORIGIN
    from time_render import event_ms
    from eprecon_amd import _lib
    from eprecon_amd.distance_field import FAR, distance_field

    coords, tsdf = room_rows(torch, np, DIMS, args.voxel, ORIGIN)
    rows = (coords, tsdf, ORIGIN, args.voxel)
    lo, hi = (0, 0, 0), tuple(DIMS)
    cells = DIMS[0] * DIMS[1] * DIMS[2]
    sites = distance_field(rows, lo, hi, 0.0)
    _lib.drain_deferred()
    seed = torch.where(sites.dist2 == 0, sites.site.to(torch.int64), torch.full_like(sites.site, FAR_KEY, dtype=torch.int64))
    res = {"voxel": args.voxel, "dims": list(DIMS), "cells": cells, "rows": int(coords.shape[0]), "sites": int((sites.dist2 == 0).sum()),
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": {}}
    for max_distance in (0.5, 2.0, None):
        def call():
            return distance_field(rows, lo, hi, max_distance)
        field = call()
        _lib.drain_deferred()
        case = {"radius": field.radius, "near": int((field.dist2 != FAR).sum()), "call_ms": event_ms(torch, {"call": call}, args.reps)["call"]}
        case["launches_us"], counts = launch_times(torch, call, args.reps)
        case["device_records_per_call"] = spread(counts)
        passes = [case["launches_us"][n][0] for n in case["launches_us"] if any(p in n for p in PASSES)]
        case["pass_bytes"] = cells * (16 + 16 + 16)
        case["pass_us"] = sum(passes)
        case["pass_bytes_per_s"] = case["pass_bytes"] / (sum(passes) * 1e-6) if passes else None
        case["pass_fraction_of_hbm_peak"] = case["pass_bytes_per_s"] / HBM_PEAK if passes else None
        window_bytes = 2 * cells * (2 * min(field.radius, max(DIMS) - 1) + 1) * 8
        if window_bytes <= args.torch_bytes:
            run = lambda: torch_banded(torch, seed, field.radius)
            d2, site = run()
            case["torch_equal"] = bool(torch.equal(d2, field.dist2) and torch.equal(site, field.site))
            del d2, site
            case["torch_ms"] = event_ms(torch, {"torch": run}, args.torch_reps, warmup=1)["torch"]
            case["torch_over_call"] = case["torch_ms"][0] / case["call_ms"][0]
        else:
            case["torch_ms"] = None
            case["torch_window_bytes"] = window_bytes
        _lib.take_deferred()
        torch.cuda.empty_cache()
        res["cases"]["unbounded" if max_distance is None else f"{max_distance} m"] = case
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

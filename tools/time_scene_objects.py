"""One timing of the object inventory (eprecon_amd/scene_objects.py, csrc/segment_stats.hip) next to a torch composition of the
same moments table on the same rows in the same process.

    python tools/time_scene_objects.py [--voxel 0.04] [--floaters 400] [--reps 20] [--out FILE.json]

The rows: tools/time_clean_scene.py's room (the cells with |tsdf| < 1 of the analytic room of eprecon_amd/synthetic.py at
--voxel, labelled in 16^3-cell blocks, a seeded 1 % of rows with a spurious id, in a seeded random order) and the same rows
in raster order, which is how a dense file hands them over.  The segments are panoptic_score.segment_table's.  HIP events
around each call, [median, min, max] ms of --reps after warm-up, the calls alternating rep by rep:

    moments           eprecon_segment_moments_async alone (its initialisation launch included), table combined in LDS
    moments_memory    the same with EPRECON_SS_LDS=0: every update straight to memory
    extents           eprecon_segment_extents_async alone, with the directions of the table
    moments_raster, moments_memory_raster, extents_raster: the same on the rows in raster order
    scene_objects     the whole call: the activity rule, segment_table, both kernels, both reads, finish
    torch_moments     the yardstick: the same table from index_add_ on int64 and scatter_reduce amin / amax

`equal` says that the kernel's table, on both paths and in both orders, and the yardstick's are the same integers.  Writes
nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def torch_moments(torch, coords, rank, n):
    """the moments table int64[n,16] composed from torch calls; rows with a rank outside [0, n) are left out"""
    keep = (rank >= 0) & (rank < n)
    r, c = rank[keep].long(), coords[keep].long()
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    cols = torch.stack([torch.ones_like(x), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], 1)
    table = torch.zeros((n, 16), dtype=torch.int64, device=coords.device)
    table[:, :10].index_add_(0, r, cols)
    idx = r[:, None].expand(-1, 3)
    table[:, 10:13] = torch.full((n, 3), 2 ** 31 - 1, dtype=torch.int64, device=coords.device).scatter_reduce(0, idx, c, "amin")
    table[:, 13:16] = torch.full((n, 3), -2 ** 31, dtype=torch.int64, device=coords.device).scatter_reduce(0, idx, c, "amax")
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--floaters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from time_clean_scene import room_rows
    from time_render import event_ms
    from eprecon_amd import _lib
    from eprecon_amd import scene_objects as SO
    from eprecon_amd.panoptic_score import segment_table

    (coords, tsdf, sem, ins), dims = room_rows(torch, np, args.voxel, args.floaters)
    m = coords.shape[0]
    rank, _, keys = segment_table(sem, ins, mapping=SO.SCANNET20_MAPPING)
    n = keys.numel()
    c_host = coords.cpu().numpy()
    raster = torch.from_numpy(np.lexsort((c_host[:, 2], c_host[:, 1], c_host[:, 0]))).cuda()
    coords_r, rank_r = coords[raster].contiguous(), rank[raster].contiguous()
    lib = _lib.load()
    table = torch.empty((n, 16), dtype=torch.int64, device="cuda")
    ext = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    dirs = torch.from_numpy(SO.directions(SO.segment_moments(coords, rank, n).cpu().numpy())).cuda()

    def moments(c, r, lds):
        def call():
            os.environ["EPRECON_SS_LDS"] = lds
            return lib.eprecon_segment_moments_async(_lib.ptr(c), _lib.ptr(r), m, n, _lib.ptr(table), _lib.ptr(status), _lib.current_stream())
        return call

    def extents(c, r):
        def call():
            os.environ["EPRECON_SS_LDS"] = "1"
            return lib.eprecon_segment_extents_async(_lib.ptr(c), _lib.ptr(r), m, n, _lib.ptr(dirs), _lib.ptr(ext), _lib.ptr(status),
                                                     _lib.current_stream())
        return call

    def whole():
        os.environ["EPRECON_SS_LDS"] = "1"
        return SO.scene_objects(coords, tsdf, sem, ins, np.zeros(3, np.float32), args.voxel)

    ms = event_ms(torch, {
        "moments": moments(coords, rank, "1"),
        "moments_memory": moments(coords, rank, "0"),
        "extents": extents(coords, rank),
        "moments_raster": moments(coords_r, rank_r, "1"),
        "moments_memory_raster": moments(coords_r, rank_r, "0"),
        "extents_raster": extents(coords_r, rank_r),
        "scene_objects": whole,
        "torch_moments": lambda: torch_moments(torch, coords, rank, n),
    }, args.reps)
    want = torch_moments(torch, coords, rank, n)
    equal = True
    for c, r in ((coords, rank), (coords_r, rank_r)):
        for lds in ("1", "0"):
            moments(c, r, lds)()
            equal = equal and bool(torch.equal(table, want)) and int(status.item()) == 0
    os.environ["EPRECON_SS_LDS"] = "1"
    objs = whole()
    res = {"voxel": args.voxel, "dims": dims, "rows": int(m), "segments": int(n), "lds_segments": int(lib.eprecon_segment_stats_lds_segments()),
           "largest_segment": int(want[:, 0].max()) if n else 0, "objects": len(objs), "reps": args.reps, "ms": ms, "equal": equal,
           "ns_per_row_moments": 1e6 * ms["moments"][0] / max(m, 1),
           "torch_over_moments": ms["torch_moments"][0] / ms["moments"][0],
           "torch_over_moments_memory": ms["torch_moments"][0] / ms["moments_memory"][0]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""Time of the panoptic export's label transfer at the real size: one synthetic room of 270 x 265 x 120 cells at 4 cm whose
labelled voxels form a two-cell shell along the floor, the four walls and three boxes.

    python tools/time_label_transfer.py [--verts 150000] [--far 0.1] [--reps 9] [--out FILE.json]

--verts vertices lie on the labelled surfaces (jittered by half a cell); --far times as many more lie 1.0 - 1.2 m above the
floor and at least 1 m from every wall and box, i.e. about 25 - 30 cells from the nearest labelled voxel, where a predicted
scene has a hole under the ground-truth mesh.

Reports, warmed up, median / min / max of --reps (device events around the calls; wall clock where a host read is inside):
    bricks        eprecon_label_bricks_async alone (the occupancy words, the error flag, the site count)
    query[p]      the search with EPRECON_LT_PATH = p (0: threads for two shells, then waves; 1: waves only; 2: threads only),
                  and for p = 0 the share of the vertices that went through the wave kernel
    vote          eprecon_instance_vote_async alone;  instance_table: with torch.unique, the ranks and its host reads
    lattice       transfer_labels as a user calls it (masks + the one host read + query), wall clock
    cloud         the route without this kernel: the labelled voxels' fp32 centres built on the device, then
                  evaluation.nn_correspondance over them and a gather of the labels, wall clock; interleaved with `lattice`
and how many vertices the two routes give a different voxel (the cloud route rounds the site coordinates to fp32).
Nothing here is asserted by a test.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS, VOXEL_SIZE, ORIGIN = (270, 265, 120), 0.04, np.array([-5.4, -5.3, -0.4], np.float32)
WALL = 7                                                  # cells between the volume's faces and the room's surfaces
BOXES = ((60, 150, 20, 25), (170, 40, 30, 15), (200, 190, 15, 35))     # x0, y0, footprint edge, height (cells)


def scene():
    """-> semantic, instance int32[X,Y,Z]: class / instance per surface, 0 elsewhere"""
    sem, ins = np.zeros(DIMS, np.int32), np.zeros(DIMS, np.int32)
    x1, y1 = DIMS[0] - WALL, DIMS[1] - WALL
    room = (slice(WALL, x1), slice(WALL, y1), slice(WALL, DIMS[2]))
    for k, (sl, cls) in enumerate((((slice(WALL, WALL + 2),) + room[1:], 1), ((slice(x1 - 2, x1),) + room[1:], 1),
                                   ((room[0], slice(WALL, WALL + 2), room[2]), 1), ((room[0], slice(y1 - 2, y1), room[2]), 1),
                                   (room[:2] + (slice(WALL, WALL + 2),), 2))):
        sem[sl], ins[sl] = cls, k + 1
    for k, (x0, y0, e, h) in enumerate(BOXES):
        box = (slice(x0, x0 + e), slice(y0, y0 + e), slice(WALL + 2, WALL + 2 + h))
        inner = (slice(x0 + 2, x0 + e - 2), slice(y0 + 2, y0 + e - 2), slice(WALL + 2, WALL + h))
        sem[box], ins[box] = 5 + k, 10 + 7 * k
        sem[inner], ins[inner] = 0, 0
    return sem, ins


def vertices(sem, n_near, far_share, seed=0):
    rng = np.random.default_rng(seed)
    cells = np.argwhere(sem != 0)
    near = cells[rng.integers(0, len(cells), n_near)] * VOXEL_SIZE + ORIGIN + rng.uniform(-0.02, 0.02, (n_near, 3))
    n_far, far = int(n_near * far_share), []
    lo = ORIGIN + (WALL + 2) * VOXEL_SIZE + 1.0
    hi = ORIGIN + (np.array(DIMS) - WALL - 2) * VOXEL_SIZE - 1.0
    while sum(len(f) for f in far) < n_far:
        p = lo + rng.random((n_far, 3)) * (hi - lo)
        p[:, 2] = lo[2] + 0.2 * rng.random(n_far)
        keep = np.ones(n_far, bool)
        for x0, y0, e, _ in BOXES:                        # at least 1 m from every box's footprint
            b_lo = ORIGIN[:2] + np.array([x0, y0]) * VOXEL_SIZE - 1.0
            b_hi = ORIGIN[:2] + np.array([x0 + e, y0 + e]) * VOXEL_SIZE + 1.0
            keep &= ~((p[:, :2] > b_lo) & (p[:, :2] < b_hi)).all(1)
        far.append(p[keep])
    return np.concatenate([near] + far)[:n_near + n_far].astype(np.float32), n_far


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


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
    return stats(out)


def main(args):
    import torch
    from eprecon_amd import _lib
    from eprecon_amd import evaluation as EV
    from eprecon_amd import generate_semantic_instance as GSI
    lib = _lib.load()
    dev = torch.device("cuda")
    sync = torch.cuda.synchronize
    sem_h, ins_h = scene()
    verts_h, n_far = vertices(sem_h, args.verts, args.far)
    sem, ins, verts = (torch.from_numpy(a).to(dev) for a in (sem_h, ins_h, verts_h))
    mapping = torch.tensor(GSI.SCANNET20_MAPPING, dtype=torch.int32, device=dev)
    n = verts.shape[0]
    res = {"dims": list(DIMS), "sites": int((sem_h != 0).sum()), "verts": n, "far_verts": n_far, "reps": args.reps}

    # the pieces, device time
    (_d, dims_p), (_m, map_p) = GSI.c_i32(DIMS), GSI.c_i32(GSI.SCANNET20_MAPPING)
    masks, n_sites = GSI.brick_masks(sem, GSI.SCANNET20_MAPPING)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    res["bricks"] = events(lambda: _lib.check(lib.eprecon_label_bricks_async(
        _lib.ptr(sem), dims_p, map_p, len(GSI.SCANNET20_MAPPING), _lib.ptr(masks), _lib.ptr(status), _lib.current_stream()),
        "eprecon_label_bricks_async"), args.reps, torch)
    assert n_sites == res["sites"]
    res["query"] = {}
    outs = {}
    for path in ("0", "1", "2"):
        os.environ["EPRECON_LT_PATH"] = path
        query = lambda: GSI.query_labels(masks, sem, ins, ORIGIN, VOXEL_SIZE, verts, GSI.SCANNET20_MAPPING, 2)
        res["query"][path] = events(query, args.reps, torch)
        outs[path] = query()
        if path == "0":
            queued = int(_lib.workspace(256, sem.device)[:4].view(torch.int32).item())
            res["query"][path]["wave_share"] = queued / n
    os.environ["EPRECON_LT_PATH"] = "0"
    res["paths_identical"] = all(torch.equal(outs["0"][k], outs[p][k]) for p in ("1", "2") for k in outs["0"])
    out = outs["0"]
    res["dist_cells"] = {"near_max": float(out["dist"][:args.verts].max()) / VOXEL_SIZE,
                         "far_min": float(out["dist"][args.verts:].min()) / VOXEL_SIZE if n_far else None,
                         "far_max": float(out["dist"][args.verts:].max()) / VOXEL_SIZE if n_far else None}

    ids = torch.unique(out["instance"])
    rank = torch.searchsorted(ids, out["instance"]).to(torch.int32)
    n_class = int(out["semantic"].max()) + 1
    cls, cnt = (torch.empty(ids.numel(), dtype=torch.int32, device=dev) for _ in range(2))
    ws = torch.empty(ids.numel() * n_class * 8 + 256, dtype=torch.uint8, device=dev)
    res["vote"] = events(lambda: _lib.check(lib.eprecon_instance_vote_async(
        _lib.ptr(out["semantic"]), _lib.ptr(rank), n, ids.numel(), n_class, _lib.ptr(cls), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(),
        _lib.current_stream()), "eprecon_instance_vote_async"), args.reps, torch)
    res["instances"] = int(ids.numel())

    # the two routes as a user calls them, interleaved, wall clock
    def lattice():
        return GSI.transfer_labels(sem, ins, ORIGIN, VOXEL_SIZE, verts)

    def cloud():
        mapped = mapping[sem.reshape(-1).long()]
        lin = torch.nonzero(mapped != 0).reshape(-1)
        idx = torch.stack([lin // (DIMS[1] * DIMS[2]), lin // DIMS[2] % DIMS[1], lin % DIMS[2]], 1)
        centres = (idx.to(torch.float64) * VOXEL_SIZE + torch.from_numpy(ORIGIN).to(dev).to(torch.float64)).to(torch.float32)
        nn, dist = EV.nn_correspondance(centres, verts)
        win = lin[nn]
        return {"index": win.to(torch.int32), "dist": dist, "semantic": mapped[win], "instance": ins.reshape(-1)[win]}

    def table():
        return GSI.instance_table(out["semantic"], out["instance"])

    routes = {"lattice": lattice, "cloud": cloud, "instance_table": table}
    times = {k: [] for k in routes}
    last = {}
    for rep in range(args.reps + 1):                      # (the first round warms up)
        for name, fn in routes.items():
            sync()
            t = time.perf_counter()
            last[name] = fn()
            sync()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
    for name in routes:
        res[name] = stats(times[name])
    differ = last["lattice"]["index"] != last["cloud"]["index"]
    res["routes_differ"] = {"near": int(differ[:args.verts].sum()), "far": int(differ[args.verts:].sum())}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--verts", type=int, default=150000)
    ap.add_argument("--far", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    main(ap.parse_args())

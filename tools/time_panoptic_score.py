"""Time of the panoptic scoring at the real size: the seeded synthetic room of tools/time_label_transfer.py (270 x 265 x 120
cells at 4 cm) as the prediction, and as ground truth the same room moved by one cell along x on a grid shifted by a
fraction of a cell, with other instance ids, a seeded share of relabelled cells and a void rim.

    python tools/time_panoptic_score.py [--verts 150000] [--reps 9] [--out FILE.json]

Reports, warmed up, median / min / max of --reps:
    voxel_kernel    eprecon_voxel_pair_count_async alone (device events; arguments prepared beforehand)
    voxel_kernel_memory    the same with EPRECON_PC_LDS=0: every add goes straight to memory, no per-workgroup LDS table
    voxel_torch     the route without it, on the device: float64 cell arithmetic per axis, broadcast gathers of the
                    ground truth, torch.bincount of a combined key; interleaved with voxel_kernel, rep by rep
    pair_kernel     eprecon_pair_count_async alone on the vertices' ranks (device events); pair_kernel_memory likewise
    pair_torch      torch.bincount of the combined key of the same ranks; interleaved with pair_kernel
    score_volumes   segment tables + kernel + the one host read + finish on device volumes, wall clock
    score_voxels    the same from the files (np.load of six compressed arrays included), wall clock
    score_sites / score_vertices    the vertex domain likewise (score_vertices includes the label transfer and np.load)
and whether the two routes give the same table.  Nothing here is asserted by a test.
"""
import argparse
import ctypes
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_label_transfer import DIMS, ORIGIN, VOXEL_SIZE, scene, stats, vertices      # noqa: E402

GT_ORIGIN = (ORIGIN.astype(np.float64) + np.array([0.025, -0.027, 0.013])).astype(np.float32)      # 0.625, -0.675, 0.325 of a cell
MOVE = (1, 0, 0)


def ground_truth(sem, ins, mapping, seed=0):
    """-> tsdf f32, semantic int64 (ScanNet ids), instance int64 [X,Y,Z]: |tsdf| < 1 on the moved room's labelled cells and on
    a rim of one cell around them, whose class is 0 (void); 3 % of the labelled cells carry another class"""
    rng = np.random.default_rng(seed)
    g_sem = np.roll(np.asarray(mapping)[sem], MOVE, (0, 1, 2)).astype(np.int64)
    g_ins = np.roll(ins, MOVE, (0, 1, 2)).astype(np.int64) + 100
    labelled = g_sem != 0
    swap = labelled & (rng.random(DIMS) < 0.03)
    g_sem[swap] = rng.choice([3, 5, 8, 40], int(swap.sum()))
    rim = labelled.copy()
    for a in range(3):
        rim |= np.roll(labelled, 1, a) | np.roll(labelled, -1, a)
    tsdf = np.where(labelled, 0.2, np.where(rim, 0.8, 1.0)).astype(np.float32)
    return tsdf, g_sem, g_ins


def events_pair(fns, reps, torch):
    """the functions in turn, rep by rep (the first round warms up) -> {name: stats}"""
    out = {k: [] for k in fns}
    for rep in range(reps + 1):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep:
                out[name].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in out.items()}


def wall(fns, reps, torch):
    out = {k: [] for k in fns}
    for rep in range(reps + 1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                out[name].append((time.perf_counter() - t) * 1e3)
    return {k: stats(v) for k, v in out.items()}


def main(args):
    import torch
    from eprecon_amd import _lib
    from eprecon_amd import generate_semantic_instance as GSI
    from eprecon_amd import panoptic_score as PS
    lib = _lib.load()
    dev = torch.device("cuda")
    sem_h, ins_h = scene()
    tsdf_h, g_sem_h, g_ins_h = ground_truth(sem_h, ins_h, GSI.SCANNET20_MAPPING)
    verts_h, _ = vertices(sem_h, args.verts, 0.1)
    sem, ins, tsdf, g_sem, g_ins, verts = (torch.from_numpy(a).to(dev) for a in (sem_h, ins_h, tsdf_h, g_sem_h, g_ins_h, verts_h))
    res = {"dims": list(DIMS), "verts": int(verts.shape[0]), "reps": args.reps, "present_gt_cells": int((np.abs(tsdf_h) < 1).sum()),
           "labelled_pred_cells": int((sem_h != 0).sum())}

    # ---- the voxel domain: ranks and arguments once, then the kernel against the torch route
    p_rank, p_keys, _ = PS._pred_table(sem, ins, GSI.SCANNET20_MAPPING, PS.STUFF_IDS, PS.VALID_CLASSES)
    present = tsdf.abs() < 1.0
    g_rank, _, g_keys, _ = PS._segment_table(torch.where(present, g_sem, 0), g_ins, None, PS.STUFF_IDS, PS.VALID_CLASSES, False)
    P, G = p_keys.numel(), g_keys.numel()
    lo, dims = PS._lattice(DIMS, ORIGIN, VOXEL_SIZE, DIMS, GT_ORIGIN, VOXEL_SIZE)
    res.update(pred_segments=P, gt_segments=G, lattice=dims)
    counts, status = PS._table_buffers(P, G, dev)
    keep = [GSI.c_i32(v) for v in (DIMS, DIMS, lo, dims)]
    o_p, o_g = (ctypes.c_float * 3)(*ORIGIN.tolist()), (ctypes.c_float * 3)(*GT_ORIGIN.tolist())

    def voxel_kernel():
        _lib.check(lib.eprecon_voxel_pair_count_async(
            _lib.ptr(p_rank), _lib.ptr(g_rank), _lib.ptr(tsdf), keep[0][1], keep[1][1], ctypes.cast(o_p, ctypes.c_void_p),
            ctypes.cast(o_g, ctypes.c_void_p), VOXEL_SIZE, VOXEL_SIZE, 1.0, keep[2][1], keep[3][1], P, G, _lib.ptr(counts),
            _lib.ptr(status), _lib.current_stream()), "eprecon_voxel_pair_count_async")

    op64, og64 = (torch.from_numpy(o.astype(np.float64)).to(dev) for o in (ORIGIN, GT_ORIGIN))
    torch_table = {}

    def voxel_torch():
        ks = [torch.arange(lo[a], lo[a] + dims[a], device=dev) for a in range(3)]
        js = [torch.floor((op64[a] + ks[a].to(torch.float64) * VOXEL_SIZE - og64[a]) / VOXEL_SIZE + 0.5).long() for a in range(3)]
        in_p = [(ks[a] >= 0) & (ks[a] < DIMS[a]) for a in range(3)]
        in_g = [(js[a] >= 0) & (js[a] < DIMS[a]) for a in range(3)]
        kc = [ks[a].clamp(0, DIMS[a] - 1) for a in range(3)]
        jc = [js[a].clamp(0, DIMS[a] - 1) for a in range(3)]
        both_p = in_p[0][:, None, None] & in_p[1][None, :, None] & in_p[2][None, None, :]
        both_g = in_g[0][:, None, None] & in_g[1][None, :, None] & in_g[2][None, None, :]
        pr = torch.where(both_p, p_rank[kc[0][:, None, None], kc[1][None, :, None], kc[2][None, None, :]].long(), -1)
        at = (jc[0][:, None, None], jc[1][None, :, None], jc[2][None, None, :])
        gr = torch.where(both_g & (tsdf[at].abs() < 1.0), g_rank[at].long(), -1)
        key = torch.where(pr < 0, P, pr) * (G + 2) + torch.where(gr < 0, G + 1, gr)
        torch_table["voxel"] = torch.bincount(key.reshape(-1), minlength=(P + 1) * (G + 2)).reshape(P + 1, G + 2)

    def without_lds(fn):
        def run():
            os.environ["EPRECON_PC_LDS"] = "0"      # (read by the library at every call)
            try:
                fn()
            finally:
                del os.environ["EPRECON_PC_LDS"]
        return run

    res.update(events_pair({"voxel_kernel": voxel_kernel, "voxel_kernel_memory": without_lds(voxel_kernel), "voxel_torch": voxel_torch},
                           args.reps, torch))
    res["voxel_tables_equal"] = bool(torch.equal(counts, torch_table["voxel"])) and int(status[0]) == 0
    res["voxel_sites"] = int(counts.sum())

    # ---- the vertex domain
    out = GSI.transfer_labels(sem, ins, ORIGIN, VOXEL_SIZE, verts)
    rng = np.random.default_rng(1)
    n = verts.shape[0]
    noise = torch.from_numpy(rng.random(n) < 0.05).to(dev)
    v_sem = torch.where(noise, torch.from_numpy(rng.choice([0, 3, 5, 40], n)).to(dev), out["semantic"].long())
    v_ins = out["instance"].long() + 100
    vp_rank, vp_keys, _ = PS._pred_table(out["semantic"], out["instance"], None, PS.STUFF_IDS, PS.VALID_CLASSES)
    vg_rank, _, vg_keys, _ = PS._segment_table(v_sem, v_ins, None, PS.STUFF_IDS, PS.VALID_CLASSES, False)
    VP, VG = vp_keys.numel(), vg_keys.numel()
    v_counts, v_status = PS._table_buffers(VP, VG, dev)

    def pair_kernel():
        _lib.check(lib.eprecon_pair_count_async(_lib.ptr(vp_rank), _lib.ptr(vg_rank), n, VP, VG, _lib.ptr(v_counts), _lib.ptr(v_status),
                                                _lib.current_stream()), "eprecon_pair_count_async")

    def pair_torch():
        pr, gr = vp_rank.long(), vg_rank.long()
        key = torch.where(pr < 0, VP, pr) * (VG + 2) + torch.where(gr < 0, VG + 1, gr)
        torch_table["pair"] = torch.bincount(key, minlength=(VP + 1) * (VG + 2)).reshape(VP + 1, VG + 2)

    res.update(events_pair({"pair_kernel": pair_kernel, "pair_kernel_memory": without_lds(pair_kernel), "pair_torch": pair_torch},
                           args.reps, torch))
    res["pair_tables_equal"] = bool(torch.equal(v_counts, torch_table["pair"])) and int(v_status[0]) == 0

    # ---- what a user calls, wall clock
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "room.npz")
        np.savez_compressed(npz, origin=ORIGIN, voxel_size=VOXEL_SIZE, tsdf=np.ones(DIMS, np.float32), semantic=sem_h, instance=ins_h)
        gt_dir = os.path.join(tmp, "room")
        os.makedirs(gt_dir)
        with open(os.path.join(gt_dir, "tsdf_info.pkl"), "wb") as fh:
            pickle.dump({"vol_origin": GT_ORIGIN, "voxel_size": VOXEL_SIZE}, fh)
        for name, a in (("full_tsdf_layer0", tsdf_h), ("full_semantic_layer_interpolate0", g_sem_h), ("full_instance_layer_interpolate0", g_ins_h)):
            np.savez_compressed(os.path.join(gt_dir, name), a)
        for name, a in (("vert", verts_h), ("sem_label", v_sem.cpu().numpy()), ("ins_label", v_ins.cpu().numpy())):
            np.save(os.path.join(tmp, f"room_{name}.npy"), a)
        last = {}
        routes = {
            "score_volumes": lambda: last.update(volumes=PS.score_volumes(sem, ins, ORIGIN, VOXEL_SIZE, tsdf, g_sem, g_ins, GT_ORIGIN, VOXEL_SIZE)),
            "score_voxels": lambda: last.update(voxels=PS.score_voxels(npz, gt_dir)),
            "score_sites": lambda: last.update(sites=PS.score_sites(out["semantic"], out["instance"], v_sem, v_ins, None)),
            "score_vertices": lambda: last.update(vertices=PS.score_vertices(npz, tmp, "room")),
        }
        res.update(wall(routes, args.reps, torch))
    res["files_equal_volumes"] = bool((last["volumes"].counts == last["voxels"].counts).all() and (last["sites"].counts == last["vertices"].counts).all())
    res["volumes_equal_kernel"] = bool((last["volumes"].counts == counts.cpu().numpy()).all())
    for name in ("volumes", "sites"):
        s = PS.PanopticScore().add(last[name]).summary()
        res[name + "_summary"] = {"pq": s["all"]["pq"], "sq": s["all"]["sq"], "rq": s["all"]["rq"], "miou": s["miou"],
                                  "tp": int(last[name].tp.sum()), "fp": int(last[name].fp.sum()), "fn": int(last[name].fn.sum())}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--verts", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    main(ap.parse_args())

"""Panoptic benchmark export — mirror of tools/generate_semantic_instance.py of the reference.

A saved scene (origin, voxel_size, semantic and instance volumes: the .npz SaveScene writes, any layout) gives every
vertex of the scene's ScanNet mesh the labels of the nearest labelled voxel, and the files the ScanNet semantic and
instance benchmarks accept are written:

    python -m eprecon_amd.generate_semantic_instance --pred DIR --ply DIR --scenes FILE [--out DIR]

The reference builds the float64 world coordinates of all X*Y*Z cells and a cKDTree over the labelled ones.  Here the
volumes stay on the device and the search runs on them directly (csrc/label_transfer.hip): a 64-bit occupancy word
per 4x4x4 brick, shells of bricks around each vertex, site coordinates recomputed in float64 from the cell index
exactly as numpy computes `idx * voxel_size + origin`.  Equidistant voxels: the smallest linear cell index wins (the
reference's choice there is the KD-tree's traversal order).  DESIGN.md §1 f8, §5b.

EPRECON_LT_PATH (tests / timing): 0 (default) one thread per vertex for `near_shells` shells, the rest one wave each;
1 every vertex through the wave kernel; 2 none (the thread kernel walks to the end).  The results are bit-identical.
"""
import argparse
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import need_device
from .scene_io import LABEL_KEYS, read_ply, read_scene_list, scene_volumes

# tools/generate_semantic_instance.py:32 (class index of the network -> ScanNet label id; 0 = unlabelled, no site)
SCANNET20_MAPPING = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
CONFIDENCE = "1.0000"      # :79-80, f'{1.0:.4f}'
MAX_MAPPING = 256
_ALL_SHELLS = (1 << 31) - 1


def c_i32(values):
    arr = (ctypes.c_int32 * len(values))(*[int(v) for v in values])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def mapping_list(mapping):
    m = [int(v) for v in np.asarray(mapping).reshape(-1)]
    if not 1 <= len(m) <= MAX_MAPPING:
        raise ValueError(f"mapping: 1 .. {MAX_MAPPING} entries, got {len(m)}")
    return m


def _label_volume(vol):
    """the reference's `.astype(int)`: any integer or float dtype -> int32 (floats truncate toward zero)"""
    if vol.dim() != 3:
        raise ValueError(f"label volume: expected [X,Y,Z], got {tuple(vol.shape)}")
    return vol.to(torch.int32).contiguous()


def brick_masks(semantic_i32, mapping):
    """semantic int32[X,Y,Z] on the device -> (masks int64[bricks] holding the 64-bit occupancy words, number of sites).
    The one host read of a transfer: the error flag and the site count.  ValueError on a class id outside the mapping."""
    lib = _lib.load()
    m = mapping_list(mapping)
    dims = tuple(semantic_i32.shape)
    n_bricks = int(np.prod([(d + 3) // 4 for d in dims]))
    dev = semantic_i32.device
    masks = torch.empty(n_bricks, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    (_d, dims_p), (_m, map_p) = c_i32(dims), c_i32(m)
    _lib.check(lib.eprecon_label_bricks_async(_lib.ptr(semantic_i32), dims_p, map_p, len(m), _lib.ptr(masks), _lib.ptr(status),
                                              _lib.current_stream()), "eprecon_label_bricks_async")
    bad, n_sites = _lib.read_counts(status)
    if bad:
        raise ValueError(f"semantic volume holds a class id outside [0, {len(m)}) (the reference raises IndexError there)")
    return masks, int(n_sites)


def _near_shells(near_shells):
    path = os.environ.get("EPRECON_LT_PATH", "0")
    if path not in ("0", "1", "2"):
        raise ValueError(f"EPRECON_LT_PATH={path!r}: 0, 1 or 2")
    return {"0": max(int(near_shells), 0), "1": -1, "2": _ALL_SHELLS}[path]


def query_labels(masks, sem, ins, origin, voxel_size, vertices, mapping, near_shells):
    lib = _lib.load()
    m = mapping_list(mapping)
    dev = sem.device
    q = vertices.to(torch.float32).contiguous()
    if q.dim() != 2 or q.shape[1] != 3:
        raise ValueError(f"vertices: expected [N,3], got {tuple(q.shape)}")
    n = q.shape[0]
    out = {"semantic": torch.empty(n, dtype=torch.int32, device=dev), "instance": torch.empty(n, dtype=torch.int32, device=dev),
           "index": torch.empty(n, dtype=torch.int32, device=dev), "dist": torch.empty(n, dtype=torch.float32, device=dev)}
    if n == 0:
        return out
    origin = np.asarray(origin.detach().cpu().numpy() if isinstance(origin, torch.Tensor) else origin, np.float32).reshape(3)
    voxel_size = float(np.asarray(voxel_size, np.float64))
    if not voxel_size > 0.0:
        raise ValueError(f"voxel_size must be positive, got {voxel_size}")
    (_d, dims_p), (_m, map_p) = c_i32(tuple(sem.shape)), c_i32(m)
    origin_c = (ctypes.c_float * 3)(*origin.tolist())
    ws = _lib.workspace(int(lib.eprecon_label_transfer_workspace_bytes(dims_p, n)), dev)
    _lib.check(lib.eprecon_label_transfer_async(
        _lib.ptr(masks), _lib.ptr(sem), _lib.ptr(ins), dims_p, ctypes.cast(origin_c, ctypes.c_void_p), voxel_size, map_p, len(m),
        _lib.ptr(q), n, _near_shells(near_shells), _lib.ptr(out["index"]), _lib.ptr(out["dist"]), _lib.ptr(out["semantic"]),
        _lib.ptr(out["instance"]), _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_label_transfer_async")
    return out


def transfer_labels(semantic_vol, instance_vol, origin, voxel_size, vertices, mapping=SCANNET20_MAPPING, near_shells=2):
    """tools/generate_semantic_instance.py:22-52.  semantic_vol, instance_vol [X,Y,Z] (any integer or float dtype) and
    vertices [N,3] on the device; origin (3 values, taken as float32 like the file's) and voxel_size (float64) on the
    host.  -> {semantic int32[N] (mapped id of the nearest labelled voxel), instance int32[N], index int32[N] (its linear
    cell index (x * Y + y) * Z + z), dist f32[N]} on the device; with no labelled voxel: 0, 0, -1, +inf."""
    need_device(semantic_vol, instance_vol, vertices)
    sem, ins = _label_volume(semantic_vol), _label_volume(instance_vol)
    if sem.shape != ins.shape:
        raise ValueError(f"semantic {tuple(sem.shape)} and instance {tuple(ins.shape)} volumes differ in shape")
    masks, _ = brick_masks(sem, mapping)
    return query_labels(masks, sem, ins, origin, voxel_size, vertices, mapping, near_shells)


def instance_table(mapped_semantic, mapped_instance):
    """:62-77 -> (ids ascending, class id per id, vertex count per id), int32 device tensors.  The class of an instance is
    the most frequent mapped class among its vertices; among equally frequent ones the class of the earliest vertex
    (Counter(...).most_common(1) in CPython)."""
    need_device(mapped_semantic, mapped_instance)
    lib = _lib.load()
    sem = mapped_semantic.to(torch.int32).contiguous().reshape(-1)
    ins = mapped_instance.to(torch.int32).contiguous().reshape(-1)
    dev = sem.device
    if sem.numel() == 0:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return empty, empty.clone(), empty.clone()
    ids = torch.unique(ins)
    rank = torch.searchsorted(ids, ins).to(torch.int32)
    lo, hi = _lib.read_counts(torch.stack([sem.min(), sem.max()]))
    if lo < 0:
        raise ValueError(f"mapped semantic ids must not be negative, got {lo}")
    n_inst, n_class = ids.numel(), int(hi) + 1
    class_ids = torch.empty(n_inst, dtype=torch.int32, device=dev)
    counts = torch.empty(n_inst, dtype=torch.int32, device=dev)
    ws = _lib.workspace(n_inst * n_class * 8 + 256, dev)
    _lib.check(lib.eprecon_instance_vote_async(_lib.ptr(sem), _lib.ptr(rank), sem.numel(), n_inst, n_class, _lib.ptr(class_ids),
                                               _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
               "eprecon_instance_vote_async")
    return ids, class_ids, counts


def _host_ints(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).reshape(-1).astype(np.int64)


def _decimal_lines(values):
    """np.savetxt(fmt='%d') of a 1-D integer array, as bytes"""
    return ("\n".join(map(str, values.tolist())) + "\n").encode("ascii") if values.size else b""


def write_submission(out_dir, scene, mapped_semantic, mapped_instance, ids, class_ids):
    """:54-80: semantic/<scene>.txt (one label id per vertex), instance/predicted_masks/<scene>_NNN.txt (one 0 / 1 per
    vertex) and instance/<scene>.txt (mask file, class id, confidence per instance), byte for byte what np.savetxt(fmt='%d')
    and the reference's f.write produce.  -> the list of paths written"""
    sem, ins, ids, cls = (_host_ints(a) for a in (mapped_semantic, mapped_instance, ids, class_ids))
    os.makedirs(os.path.join(out_dir, "semantic"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "instance", "predicted_masks"), exist_ok=True)
    written = [os.path.join(out_dir, "semantic", scene + ".txt")]
    with open(written[0], "wb") as fh:
        fh.write(_decimal_lines(sem))
    lines = []
    rows = np.empty((ins.size, 2), np.uint8)       # one mask file: b'0\n' / b'1\n' per vertex
    rows[:, 1] = ord("\n")
    for i, (instance_id, class_id) in enumerate(zip(ids.tolist(), cls.tolist())):
        name = f"predicted_masks/{scene}_{i:03d}.txt"
        rows[:, 0] = ord("0") + (ins == instance_id)
        written.append(os.path.join(out_dir, "instance", name))
        with open(written[-1], "wb") as fh:
            fh.write(rows.tobytes())
        lines.append(f"{name} {class_id} {CONFIDENCE}\n")
    written.append(os.path.join(out_dir, "instance", scene + ".txt"))
    with open(written[-1], "w") as fh:
        fh.write("".join(lines))
    return written


def generate_semantic_instance(scene_name, pred_dir, ply_dir, out_dir=".", device=None, mapping=SCANNET20_MAPPING):
    """the reference's function of the same name with its two hard-wired directories as arguments: <pred_dir>/<scene>.npz,
    <ply_dir>/<scene>_vh_clean_2.ply -> the three kinds of file under out_dir.  -> {n_vertices, n_instances, files}, or
    None (nothing written, a warning printed) when the scene has no labelled voxel (the reference crashes there)."""
    device = torch.device(device if device is not None else "cuda")
    sem, ins, origin, voxel_size = scene_volumes(os.path.join(pred_dir, scene_name + ".npz"), device, LABEL_KEYS)
    masks, n_sites = brick_masks(sem, mapping)
    if n_sites == 0:
        print(f"[eprecon_amd] warning: No labelled voxel for scene {scene_name}")
        return None
    verts, _ = read_ply(os.path.join(ply_dir, scene_name + "_vh_clean_2.ply"))
    out = query_labels(masks, sem, ins, origin, voxel_size, torch.from_numpy(verts).to(device), mapping, 2)
    ids, class_ids, _ = instance_table(out["semantic"], out["instance"])
    files = write_submission(out_dir, scene_name, out["semantic"], out["instance"], ids, class_ids)
    return {"n_vertices": int(verts.shape[0]), "n_instances": int(ids.numel()), "files": files}


def main(argv=None):
    ap = argparse.ArgumentParser(description="ScanNet semantic / instance benchmark files from saved scenes")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--ply", required=True, help="directory of the <scene>_vh_clean_2.ply meshes")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", default=".", help="where semantic/ and instance/ are written (default: here)")
    args = ap.parse_args(argv)
    for scene in read_scene_list(args.scenes):
        print(scene)
        generate_semantic_instance(scene, args.pred, args.ply, args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

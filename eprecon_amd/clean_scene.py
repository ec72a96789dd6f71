"""Clean-up of a saved scene: connected components of its voxel rows on libeprecon_hip.so (csrc/components.hip), and the
rule that removes floaters and segment debris with them.  The reference has no such stage (its users cluster the finished
mesh in open3d afterwards); the rule is this project's own:

    label = components(coords, keys=None, connectivity=26)     # coords int32[M,3] on the device -> int32[M]
    coords, tsdf, semantic, instance, report = clean_rows(coords, tsdf, semantic, instance, min_voxels=50,
                                                          min_segment_voxels=10, split_instances=True)
    report = clean_scene("scene0000_00.npz", "clean/scene0000_00.npz", min_voxels=50, mesh=True)

    python -m eprecon_amd.clean_scene --pred DIR --scenes FILE --out DIR [--min_voxels N] [--keep_largest K]
                                      [--min_segment_voxels N] [--split_instances] [--connectivity 6|18|26] [--mesh]

components: two rows are adjacent when their coordinate difference d has d != 0, max |d_i| <= 1 and sum |d_i| <= 1 / 2 / 3
(connectivity 6 / 18 / 26); they are linked iff they are adjacent, carry the same key and that key is >= 0.  label[i] is
the smallest row index of row i's component, -1 for a row with a negative key: the same values on every run.  The hash
grid and the symmetric self map are the library's existing calls; the labelling is three launches whatever the set looks
like.  Device tensors are required (no CPU fallback).

clean_rows: a geometry pass over the rows with tsdf < 1 (components below min_voxels rows leave the list, or all but the
keep_largest largest), then a segment pass over the survivors keyed by their (semantic, instance) pair (components below
min_segment_voxels rows lose their ids; with split_instances the smaller pieces of an instance in several pieces get
fresh ids).  Sizes and the relabelling are torch calls on the device: this is a tool, their host reads are fine.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib
from ._lib import need_device, to_device
from .scene_io import VOLUME_KEYS, raster_rows, read_scene, read_scene_list, scatter_volumes, write_scene
from .sparse import HashGrid, check_hash_status

CONNECTIVITIES = (6, 18, 26)
RULE_KEYS = ("min_voxels", "keep_largest", "min_segment_voxels", "split_instances", "connectivity")
REPORT_KEYS = ("rows_in", "rows_removed", "components", "components_removed", "segment_components_cleared", "rows_cleared",
               "instances_split")


def components(coords, keys=None, connectivity=26):
    """coords int32[M,3] (pairwise distinct, |c| < 2^19 - 1), keys int32[M] or None -> label int32[M], all on the device.
    ValueError for duplicate rows, EpreconError for a CPU tensor, a coordinate out of the hash grid's range or a status
    word the kernels left set.  One host read (the three checks together); none, and no launch, for M == 0."""
    need_device(coords, *(() if keys is None else (keys,)))
    if coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int32:
        raise ValueError(f"components: expected int32 coords [M,3], got {coords.dtype} {tuple(coords.shape)}")
    if int(connectivity) not in CONNECTIVITIES:
        raise ValueError(f"components: connectivity must be 6, 18 or 26, got {connectivity}")
    m, dev = coords.shape[0], coords.device
    if keys is not None:
        if keys.shape != (m,):
            raise ValueError(f"components: {m} rows, keys of shape {tuple(keys.shape)}")
        keys = keys.to(torch.int32).contiguous()
    label = torch.empty(m, dtype=torch.int32, device=dev)
    if m == 0:
        return label
    lib = _lib.load()
    rows = torch.zeros((m, 4), dtype=torch.int32, device=dev)          # (batch 0, x, y, z)
    rows[:, 1:] = coords
    grid = HashGrid(m, dev).build(rows)
    nbr = torch.empty((27, m), dtype=torch.int32, device=dev)
    _lib.check(lib.eprecon_kernel_map_self_async(_lib.ptr(grid.mem), grid.capacity, _lib.ptr(rows), m, 1, _lib.ptr(nbr),
                                                 _lib.current_stream()), "eprecon_kernel_map_self_async")
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.eprecon_components_workspace_bytes(m), dev)
    _lib.check(lib.eprecon_components_async(_lib.ptr(nbr), m, _lib.ptr(keys), int(connectivity), _lib.ptr(label), _lib.ptr(status),
                                            _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_components_async")
    # the table keeps the FIRST row of a key: a row whose centre entry is not itself has an earlier twin
    twins = (nbr[13] != torch.arange(m, dtype=torch.int32, device=dev)).sum().to(torch.int32)
    table_status, n_twins, cc_status = _lib.read_counts(torch.stack([grid.header[0], twins, status[0]]))
    check_hash_status(table_status)
    if n_twins:
        raise ValueError(f"components: {n_twins} rows repeat the coordinates of an earlier row")
    if cc_status:
        raise _lib.EpreconError(f"eprecon_components_async: a bounded loop gave up (status {cc_status})")
    return label


def _sizes(label, member):
    """-> (counts int64[M]: rows of the component whose label is the index, 0 elsewhere; roots int64[C] ascending)"""
    counts = torch.bincount(label[member].long(), minlength=label.shape[0])
    return counts, torch.nonzero(counts).reshape(-1)


def _clean(coords, tsdf, semantic, instance, min_voxels, keep_largest, min_segment_voxels, split_instances, connectivity):
    """the rule on device rows -> (keep bool[M], semantic, instance of the kept rows, report of device / host scalars)"""
    m, dev = coords.shape[0], coords.device
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    report = {k: zero for k in REPORT_KEYS}
    report["rows_in"] = m
    # ---- geometry
    geo = tsdf < 1
    label = components(coords, torch.where(geo, 0, -1).to(torch.int32), connectivity).long()
    counts, roots = _sizes(label, geo)
    if int(keep_largest) > 0:
        order = torch.sort(counts[roots], descending=True, stable=True).indices          # ties: the smaller label first
        keep_root = torch.zeros(m, dtype=torch.bool, device=dev)
        keep_root[roots[order[:int(keep_largest)]]] = True
    else:
        keep_root = counts >= int(min_voxels)
    keep = ~geo | keep_root[label.clamp(min=0)]
    report["components"] = roots.numel()
    report["components_removed"] = (~keep_root[roots]).sum()
    report["rows_removed"] = (~keep).sum()
    coords, semantic, instance = coords[keep], semantic[keep].clone(), instance[keep].clone()
    # ---- segments
    n = coords.shape[0]
    seg = semantic > 0
    # rank of the (semantic, instance) pair: ids as int32, so class << 32 | (instance + 2^31) is one int64 per pair
    _, rank = torch.unique((semantic[seg].long() << 32) + (instance[seg].to(torch.int32).long() + (1 << 31)), return_inverse=True)
    keys = torch.full((n,), -1, dtype=torch.int32, device=dev)
    keys[seg] = rank.to(torch.int32)
    label = components(coords, keys, connectivity).long()
    counts, roots = _sizes(label, seg)
    small = (counts < int(min_segment_voxels)) & (counts > 0)
    clear = seg & small[label.clamp(min=0)]
    semantic[clear] = 0
    instance[clear] = 0
    report["segment_components_cleared"] = small.sum()
    report["rows_cleared"] = clear.sum()
    if split_instances and n:
        r = roots[~small[roots]]
        r = r[instance[r] > 0]
        by_size = torch.sort(counts[r], descending=True, stable=True).indices             # (size desc, label asc) ...
        r = r[by_size]
        by_pair = torch.sort(keys[r], stable=True).indices                                # ... within each pair
        r = r[by_pair]
        k = keys[r]
        first = torch.ones_like(k, dtype=torch.bool)
        first[1:] = k[1:] != k[:-1]
        losers = torch.sort(r[~first]).values                                             # ascending label over the scene
        base = instance.max().clamp(min=0).long()
        fresh = torch.zeros(n, dtype=torch.int64, device=dev)
        fresh[losers] = base + 1 + torch.arange(losers.numel(), dtype=torch.int64, device=dev)
        moved = seg & ~clear & (fresh[label.clamp(min=0)] > 0)
        instance[moved] = fresh[label[moved]].to(instance.dtype)
        report["instances_split"] = losers.numel()
    return keep, semantic, instance, report


def _host_report(report):
    dev_items = [(k, v) for k, v in report.items() if isinstance(v, torch.Tensor)]
    if dev_items:
        host = _lib.read_counts(torch.stack([v.to(torch.int64).reshape(()) for _, v in dev_items]))
        report = dict(report, **{k: h for (k, _), h in zip(dev_items, host)})
    return {k: int(report[k]) for k in REPORT_KEYS}


def clean_rows(coords, tsdf, semantic, instance, min_voxels=0, keep_largest=0, min_segment_voxels=0, split_instances=False,
               connectivity=26):
    """coords int32[M,3], tsdf f32[M], semantic, instance int[M] on the device -> (coords, tsdf, semantic, instance, report):
    the kept rows in their order, their ids after the segment pass, and the counts of REPORT_KEYS as host ints"""
    need_device(coords, tsdf, semantic, instance)
    m = coords.shape[0]
    if tsdf.shape != (m,) or semantic.shape != (m,) or instance.shape != (m,):
        raise ValueError(f"clean_rows: {m} rows, values of shapes {tuple(tsdf.shape)}, {tuple(semantic.shape)}, {tuple(instance.shape)}")
    keep, sem, ins, report = _clean(coords, tsdf, semantic, instance, min_voxels, keep_largest, min_segment_voxels,
                                    split_instances, connectivity)
    return coords[keep], tsdf[keep], sem, ins, _host_report(report)


# ---------------------------------------------------------------------------------------------------------------- files

def clean_scene(npz_in, npz_out, mesh=False, device=None, **rule):
    """A scene file in either form SaveScene writes -> the cleaned file in the same form (dense: the same keys and dtypes,
    removed cells back at TSDF 1 and ids 0; sparse: the kept rows in the file's order) -> the report (+ "path").  The rows of
    a dense file are its cells with tsdf != 1, semantic != 0 or instance != 0; whichever the form, the rule sees the rows in
    raster order, so both forms of one scene clean to the same volumes.  mesh: also <scene>.ply, mesh_semantic_<scene>.ply
    and mesh_instance_<scene>.ply beside npz_out (tsdf_panoptic2mesh + export_ply, as SaveScene writes them).
    **rule: clean_rows' keywords."""
    unknown = set(rule) - set(RULE_KEYS)
    if unknown:
        raise TypeError(f"clean_scene: unknown keywords {sorted(unknown)}")
    dev = torch.device(device if device is not None else "cuda")
    scene = read_scene(npz_in, rest=True)
    if scene.layout == "legacy":
        raise ValueError(f"{npz_in}: neither the dense nor the sparse form of a saved scene")
    rows, tsdf, semantic, instance, order = raster_rows(scene)
    keep, sem, ins, report = _clean(to_device(rows, torch.int32, dev), to_device(tsdf, torch.float32, dev), to_device(semantic, torch.int64, dev),
                                    to_device(instance, torch.int64, dev), *(rule.get(k, d) for k, d in zip(RULE_KEYS, (0, 0, 0, False, 26))))
    report = _host_report(report)
    keep, sem, ins = keep.cpu().numpy(), sem.cpu().numpy(), ins.cpu().numpy()
    if order is not None:
        kept = order[keep]                      # file positions of the kept rows, in raster order
        back = np.argsort(kept, kind="stable")  # ... and in the file's order
        idx = kept[back]
        out = {"coords": scene.coords[idx], "tsdf": scene.arrays["tsdf"][idx], "semantic": sem[back].astype(scene.arrays["semantic"].dtype),
               "instance": ins[back].astype(scene.arrays["instance"].dtype)}
        mesh_rows = dict(out)
    else:
        gone, stay = rows[~keep], rows[keep]
        out = {k: scene.arrays[k].copy() for k in VOLUME_KEYS}
        out["tsdf"][gone[:, 0], gone[:, 1], gone[:, 2]] = 1
        for key, values in (("semantic", sem), ("instance", ins)):
            out[key][gone[:, 0], gone[:, 1], gone[:, 2]] = 0
            out[key][stay[:, 0], stay[:, 1], stay[:, 2]] = values.astype(out[key].dtype)
        mesh_rows = {"coords": stay, "tsdf": out["tsdf"][stay[:, 0], stay[:, 1], stay[:, 2]], "semantic": sem, "instance": ins}
    out_dir = os.path.dirname(os.path.abspath(npz_out))
    os.makedirs(out_dir, exist_ok=True)
    write_scene(npz_out, **out, **scene.rest)
    report["path"] = npz_out
    if mesh:
        from .save_scene import export_ply, tsdf_panoptic2mesh
        scene_name = os.path.splitext(os.path.basename(npz_out))[0]
        vols = scatter_volumes(scene.dims, mesh_rows.pop("coords"), mesh_rows, dev)
        if bool((vols["tsdf"] == 1).all()):
            print(f"[eprecon_amd] warning: No valid data for scene {scene_name}")
        else:
            meshes = tsdf_panoptic2mesh(scene.voxel_size, torch.from_numpy(scene.origin).to(dev), *(vols[k] for k in VOLUME_KEYS))
            for m, name in zip(meshes, ("{}.ply", "mesh_semantic_{}.ply", "mesh_instance_{}.ply")):
                export_ply(m, os.path.join(out_dir, name.format(scene_name)))
    return report


def format_report(scene, report):
    return (f"{scene}: {report['rows_in']} rows, {report['rows_removed']} removed with {report['components_removed']} of "
            f"{report['components']} components; {report['rows_cleared']} rows cleared in {report['segment_components_cleared']} "
            f"segment components; {report['instances_split']} instances split -> {report['path']}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="remove floaters and segment debris from saved scenes")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="the cleaned <scene>.npz (and meshes) go here")
    ap.add_argument("--min_voxels", default=0, type=int, help="components of fewer TSDF rows are removed")
    ap.add_argument("--keep_largest", default=0, type=int, help="keep only the K largest components instead")
    ap.add_argument("--min_segment_voxels", default=0, type=int, help="segment components of fewer rows lose their ids")
    ap.add_argument("--split_instances", action="store_true", help="the smaller pieces of an instance in several pieces get fresh ids")
    ap.add_argument("--connectivity", default=26, type=int, choices=list(CONNECTIVITIES))
    ap.add_argument("--mesh", action="store_true", help="also write <scene>.ply, mesh_semantic_<scene>.ply, mesh_instance_<scene>.ply")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    for scene in read_scene_list(args.scenes):
        report = clean_scene(os.path.join(args.pred, scene + ".npz"), os.path.join(args.out, scene + ".npz"), mesh=args.mesh,
                             **{k: getattr(args, k) for k in RULE_KEYS})
        print(format_report(scene, report))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

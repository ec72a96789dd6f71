"""Object inventory of a saved scene: one record per segment with its voxel count, centroid, axis-aligned box and upright
oriented box.  The reference has no such stage (its users fit boxes in open3d afterwards); the rule is this project's own
(DESIGN.md §5b):

    table = segment_moments(coords, rank, n_segments)            # device int64[n,16]
    ext   = segment_extents(coords, rank, n_segments, dirs)      # device float64[n,4]
    objs  = finish(table, ext_or_None, keys, origin, voxel_size) # host: numpy in, list of dict out
    objs  = scene_objects(coords, tsdf, semantic, instance, origin, voxel_size, mapping=SCANNET20_MAPPING, surface=1.0,
                          min_voxels=1, oriented=True)
    objs  = describe_scene("scene0000_00.npz", out_json="scene0000_00_objects.json", boxes_ply=None, min_voxels=50)

    python -m eprecon_amd.scene_objects --pred DIR --scenes FILE --out DIR [--gt DIR] [--min_voxels N] [--surface 1.0]
                                        [--no-oriented] [--boxes] [--names FILE]

What runs on the device (csrc/segment_stats.hip) is the segmented reduction over the voxel rows: per segment the count, the
sums of the integer coordinates and of their products and the min / max per axis (segment_moments), and the extents of the
rows along a direction per segment (segment_extents).  They are integer sums, integer min / max and min / max of doubles, so
the same numbers come out on every run and on either path of the kernels.  `finish` turns the small tables into the records
on the host with Python integers and floats.  Device tensors are required (no CPU fallback).  segment_moments and
segment_extents issue one host read each (the status word); scene_objects reads the table with the status word and the keys
in one transfer, and the extents with theirs in a second.

EPRECON_SS_LDS=0 (tests / timing): the kernels never combine the table per workgroup in LDS first; every update goes straight
to memory, as it does above eprecon_segment_stats_lds_segments() segments.  The tables are the same.
"""
import argparse
import json
import math
import os
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import need_device, to_device
from .generate_semantic_instance import SCANNET20_MAPPING, mapping_list
from .panoptic_score import key_pairs, segment_table
from .scene_io import LABEL_KEYS, export_ply, raster_rows, read_scene, read_scene_list

MOMENT_COLUMNS, EXTENT_COLUMNS = 16, 4
MAX_ROWS = 1 << 24
RULE_KEYS = ("mapping", "surface", "min_voxels", "oriented")
RECORD_KEYS = ("id", "class_id", "instance", "voxels", "centroid", "aabb_min", "aabb_max", "heading", "obb_centre", "obb_size")
BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


# ------------------------------------------------------------------------------------------------------- the tables (device)

def _rows(coords, rank, n_segments, what):
    need_device(coords, rank)
    if coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int32:
        raise ValueError(f"{what}: expected int32 coords [M,3], got {coords.dtype} {tuple(coords.shape)}")
    m, n = coords.shape[0], int(n_segments)
    if rank.shape != (m,):
        raise ValueError(f"{what}: {m} rows, ranks of shape {tuple(rank.shape)}")
    if n < 0:
        raise ValueError(f"{what}: the segment count must not be negative, got {n}")
    if m >= MAX_ROWS:      # (the C entry refuses it too; no allocation first)
        raise _lib.EpreconError(f"{what}: {m} rows: 2^24 or more is unsupported (-3)")
    return coords.contiguous(), rank.to(torch.int32).contiguous(), m, n


def _launch_moments(coords, rank, n_segments):
    coords, rank, m, n = _rows(coords, rank, n_segments, "segment_moments")
    table = torch.empty((n, MOMENT_COLUMNS), dtype=torch.int64, device=coords.device)
    status = torch.empty(1, dtype=torch.int32, device=coords.device)
    _lib.check(_lib.load().eprecon_segment_moments_async(_lib.ptr(coords), _lib.ptr(rank), m, n, _lib.ptr(table), _lib.ptr(status),
                                                         _lib.current_stream()), "eprecon_segment_moments_async")
    return table, status


def _launch_extents(coords, rank, n_segments, dirs):
    coords, rank, m, n = _rows(coords, rank, n_segments, "segment_extents")
    need_device(dirs)
    if dirs.shape != (n, 2) or dirs.dtype != torch.float64:
        raise ValueError(f"segment_extents: expected float64 dirs [{n},2], got {dirs.dtype} {tuple(dirs.shape)}")
    dirs = dirs.contiguous()
    ext = torch.empty((n, EXTENT_COLUMNS), dtype=torch.float64, device=coords.device)
    status = torch.empty(1, dtype=torch.int32, device=coords.device)
    _lib.check(_lib.load().eprecon_segment_extents_async(_lib.ptr(coords), _lib.ptr(rank), m, n, _lib.ptr(dirs),
                                                         _lib.ptr(ext), _lib.ptr(status), _lib.current_stream()),
               "eprecon_segment_extents_async")
    return ext, status


def _status_error(what, status, n, table):
    parts = [p for bit, p in ((1, f"a rank outside [-1, {n}]"), (2, "a coordinate beyond +-(2^19 - 2)")) if status & bit]
    err = ValueError(f"{what}: {' and '.join(parts)} (status {status}); such rows were left out")
    err.status, err.table = int(status), table
    return err


def segment_moments(coords, rank, n_segments):
    """coords int32[M,3], rank int[M] on the device (M < 2^24) -> table int64[n_segments,16] on the device: per segment the
    count, the sums of x, y, z, of xx, xy, xz, yy, yz, zz, min x, y, z (INT32_MAX without a row) and max x, y, z (INT32_MIN).
    A rank of -1 or n_segments is skipped.  One host read (the status word): ValueError for any other rank outside the
    range (status 1) or a coordinate beyond +-(2^19 - 2) (status 2); such rows are left out, and the table of the others
    is on the error as `.table`, the word as `.status`."""
    table, status = _launch_moments(coords, rank, n_segments)
    word = _lib.read_counts(status)[0]
    if word:
        raise _status_error("segment_moments", word, int(n_segments), table)
    return table


def segment_extents(coords, rank, n_segments, dirs):
    """The same rows and dirs float64[n_segments,2] = (c, s) on the device -> ext float64[n_segments,4] on the device: (min u,
    max u, min v, max v) of u = x c + y s, v = y c - x s, every operation rounded in float64; (+inf, -inf, +inf, -inf)
    without a row; a zero is +0.  One host read and the errors of segment_moments (`.table` is ext)."""
    ext, status = _launch_extents(coords, rank, n_segments, dirs)
    word = _lib.read_counts(status)[0]
    if word:
        raise _status_error("segment_extents", word, int(n_segments), ext)
    return ext


# ------------------------------------------------------------------------------------------------------- the records (host)

def heading(row):
    """one row of the moments table -> theta in (-pi/2, pi/2]: the direction of the larger variance of the footprint, from
    Python integers; 0 for an isotropic footprint"""
    n, sx, sy, sxx, sxy, syy = (int(row[k]) for k in (0, 1, 2, 4, 5, 7))
    a, b, c = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    if c == 0 and a == b:
        return 0.0
    return 0.5 * math.atan2(float(2 * c), float(a - b))


def directions(table):
    """moments table (host) -> float64[n,2]: (cos theta, sin theta) per segment, (1, 0) for a segment without rows"""
    table = np.asarray(table, np.int64).reshape(-1, MOMENT_COLUMNS)
    out = np.zeros((table.shape[0], 2), np.float64)
    for r, row in enumerate(table):
        t = heading(row) if int(row[0]) > 0 else 0.0
        out[r] = math.cos(t), math.sin(t)
    return out


def finish(table, ext, keys, origin, voxel_size, min_voxels=1):
    """Moments table int64[n,16], extents float64[n,4] for directions(table) (None: no oriented box), keys int64[n] of
    segment_table, the file's float32 origin and the voxel size -> the records of the segments with at least
    max(min_voxels, 1) rows, in rank order.  Host only: Python integers and floats."""
    table = np.asarray(table, np.int64).reshape(-1, MOMENT_COLUMNS)
    pairs = key_pairs(np.asarray(keys, np.int64))
    n = table.shape[0]
    if pairs.shape[0] != n:
        raise ValueError(f"finish: a table of {n} segments and {pairs.shape[0]} keys")
    if ext is not None:
        ext = np.asarray(ext, np.float64)
        if ext.shape != (n, EXTENT_COLUMNS):
            raise ValueError(f"finish: a table of {n} segments and extents of shape {ext.shape}")
    o = [float(np.float64(v)) for v in np.asarray(origin, np.float32).reshape(3)]
    vs = float(voxel_size)
    out = []
    for r in range(n):
        row = [int(v) for v in table[r]]
        count = row[0]
        if count < max(int(min_voxels), 1):
            continue
        rec = {"id": r, "class_id": int(pairs[r, 0]), "instance": int(pairs[r, 1]), "voxels": count,
               "centroid": [o[a] + (float(row[1 + a]) / float(count)) * vs for a in range(3)],
               "aabb_min": [o[a] + (float(row[10 + a]) - 0.5) * vs for a in range(3)],
               "aabb_max": [o[a] + (float(row[13 + a]) + 0.5) * vs for a in range(3)]}
        if ext is not None:
            t = heading(row)
            c, s = math.cos(t), math.sin(t)
            u0, u1, v0, v1 = (float(v) for v in ext[r])
            z0, z1 = float(row[12]), float(row[15])
            cu, cv, cz = (u0 + u1) / 2, (v0 + v1) / 2, (z0 + z1) / 2
            rec["heading"] = t
            rec["obb_centre"] = [o[0] + vs * (c * cu - s * cv), o[1] + vs * (s * cu + c * cv), o[2] + vs * cz]
            rec["obb_size"] = [((u1 - u0) + 1) * vs, ((v1 - v0) + 1) * vs, ((z1 - z0) + 1) * vs]
        out.append(rec)
    return out


def scene_objects(coords, tsdf, semantic, instance, origin, voxel_size, mapping=SCANNET20_MAPPING, surface=1.0, min_voxels=1,
                  oriented=True):
    """Voxel rows on the device (coords int32[M,3], tsdf f32[M], semantic: class indices taken through `mapping`, None: ids
    already; instance) -> the records of the scene.  A row takes part when |tsdf| < surface (in float32) and its class maps
    to a non-zero id; the segments are panoptic_score.segment_table's.  ValueError for a class index outside the mapping."""
    need_device(coords, tsdf, semantic, instance)
    m = coords.shape[0]
    if tsdf.shape != (m,) or semantic.shape != (m,) or instance.shape != (m,):
        raise ValueError(f"scene_objects: {m} rows, values of shapes {tuple(tsdf.shape)}, {tuple(semantic.shape)}, {tuple(instance.shape)}")
    dev = coords.device
    near = tsdf.to(torch.float32).abs() < torch.tensor(float(surface), dtype=torch.float32, device=dev)
    coords = coords[near].contiguous()
    # (the segments are made of the rows that take part; class 0 gets rank -1 or the void rank, both skipped by the kernels)
    rank, _, keys = segment_table(semantic[near], instance[near], mapping=mapping)
    # (segment_table has checked the rows that take part; the others ride on the read of the table)
    stray = torch.zeros(1, dtype=torch.int64, device=dev)
    if mapping is not None:
        stray = ((semantic < 0) | (semantic >= len(mapping_list(mapping)))).any().to(torch.int64).reshape(1)
    n = keys.numel()
    table, status = _launch_moments(coords, rank, n)
    host = _lib.read_counts(torch.cat([status.to(torch.int64), stray, keys, table.reshape(-1)]))
    if host[1]:
        raise ValueError(f"semantic values outside [0, {len(mapping_list(mapping))})")
    if host[0]:
        raise _status_error("scene_objects", host[0], n, table)
    keys_h, table_h = np.array(host[2:2 + n], np.int64), np.array(host[2 + n:], np.int64).reshape(n, MOMENT_COLUMNS)
    ext_h = None
    if oriented:
        dirs = torch.from_numpy(directions(table_h)).to(dev)
        ext, status = _launch_extents(coords, rank, n, dirs)
        host = _lib.read_counts(torch.cat([status.to(torch.int64), ext.view(torch.int64).reshape(-1)]))
        if host[0]:
            raise _status_error("scene_objects", host[0], n, ext)
        ext_h = np.array(host[1:], np.int64).view(np.float64).reshape(n, EXTENT_COLUMNS)
    return finish(table_h, ext_h, keys_h, origin, voxel_size, min_voxels)


# ---------------------------------------------------------------------------------------------------------------- files

def box_corners(rec):
    """a record -> float64[8,3]: the corners of its oriented box (of its axis-aligned box without one), the bottom face
    counter-clockwise, then the top face"""
    if "obb_centre" in rec:
        c, s = math.cos(rec["heading"]), math.sin(rec["heading"])
        centre, half = np.array(rec["obb_centre"], np.float64), np.array(rec["obb_size"], np.float64) / 2
    else:
        c, s = 1.0, 0.0
        lo, hi = np.array(rec["aabb_min"], np.float64), np.array(rec["aabb_max"], np.float64)
        centre, half = (lo + hi) / 2, (hi - lo) / 2
    out = []
    for sz in (-1, 1):
        for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            du, dv = su * half[0], sv * half[1]
            out.append([centre[0] + c * du - s * dv, centre[1] + s * du + c * dv, centre[2] + sz * half[2]])
    return np.array(out, np.float64)


def write_boxes(objs, path):
    """the boxes of the records as a wireframe PLY: 8 vertices and 12 `edge` elements per record, coloured like the
    instance mesh (its instance id, the class id of a stuff segment, into save_scene.COLOR_PALETTE)"""
    from .save_scene import COLOR_PALETTE
    verts = np.concatenate([box_corners(r) for r in objs]) if objs else np.zeros((0, 3), np.float64)
    edges = np.concatenate([np.array(BOX_EDGES, np.int32) + 8 * k for k in range(len(objs))]) if objs else np.zeros((0, 2), np.int32)
    ids = np.array([r["instance"] if r["instance"] > 0 else r["class_id"] for r in objs], np.int64)
    colors = np.repeat(np.asarray(COLOR_PALETTE)[ids % len(COLOR_PALETTE)][:, :3], 8, axis=0).astype(np.uint8).reshape(-1, 3)
    export_ply({"vertices": verts, "edges": edges, "vertex_colors": colors}, path)
    return path


def read_names(path):
    """a text file of `id name` lines (blank lines skipped; the name is the rest of the line) -> {id: name}"""
    names = {}
    with open(path, "r", encoding="utf-8") as fh:
        for no, line in enumerate(fh, 1):
            tok = line.strip().split(None, 1)
            if not tok:
                continue
            try:
                names[int(tok[0])] = tok[1].strip() if len(tok) > 1 else ""
            except ValueError:
                raise ValueError(f"{path}:{no}: expected `id name`, got {line.strip()!r}") from None
    return names


def _rule(rule):
    unknown = set(rule) - set(RULE_KEYS)
    if unknown:
        raise TypeError(f"scene_objects: unknown keywords {sorted(unknown)}")
    full = dict(zip(RULE_KEYS, (SCANNET20_MAPPING, 1.0, 1, True)))
    full.update(rule)
    return full


def write_objects(scene, objs, origin, voxel_size, rule, out_json, boxes_ply, names):
    if names is not None:
        objs = [dict(r, class_name=names.get(r["class_id"], "")) for r in objs]
    if not objs:
        print(f"[eprecon_amd] warning: No valid data for scene {scene}")
    if out_json is not None:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        doc = {"scene": scene, "voxel_size": float(voxel_size), "origin": [float(v) for v in np.asarray(origin, np.float32).reshape(3)],
               "rule": {"surface": float(rule["surface"]), "min_voxels": int(rule["min_voxels"]), "oriented": bool(rule["oriented"]),
                        "mapping": None if rule["mapping"] is None else mapping_list(rule["mapping"])},
               "objects": objs}
        with open(out_json, "w") as fh:
            json.dump(doc, fh, indent=1)
    if boxes_ply is not None:
        os.makedirs(os.path.dirname(os.path.abspath(boxes_ply)), exist_ok=True)
        write_boxes(objs, boxes_ply)
    return objs


def describe_scene(npz, out_json=None, boxes_ply=None, names=None, device=None, **rule):
    """A scene file in either form SaveScene writes -> its records; written as <out_json> ({"scene", "voxel_size", "origin",
    "rule", "objects"}) and as the wireframe <boxes_ply> when asked for.  names: {class id: name} adds `class_name`.
    **rule: scene_objects' keywords.  An empty scene gives an empty list, with the export's warning."""
    rule = _rule(rule)
    dev = torch.device(device if device is not None else "cuda")
    scene = read_scene(npz)
    if scene.layout == "legacy":
        raise ValueError(f"{npz}: neither the dense nor the sparse form of a saved scene")
    rows, tsdf, semantic, instance, _ = raster_rows(scene)
    objs = scene_objects(to_device(rows, torch.int32, dev), to_device(tsdf, torch.float32, dev), to_device(semantic, torch.int64, dev),
                         to_device(instance, torch.int64, dev), scene.origin, scene.voxel_size, **rule)
    name = os.path.splitext(os.path.basename(npz))[0]
    return write_objects(name, objs, scene.origin, scene.voxel_size, rule, out_json, boxes_ply, names)


def _arr0(path):
    with np.load(path) as z:
        return z["arr_0"]


def describe_gt(gt_scene_dir, out_json=None, boxes_ply=None, names=None, device=None, **rule):
    """generate_gt's volumes of <gt_scene_dir> (tsdf_info.pkl, full_tsdf_layer0.npz, full_semantic_layer_interpolate0.npz,
    full_instance_layer_interpolate0.npz: the files panoptic_score.score_voxels reads) -> their records.  The labels are
    ScanNet ids already: mapping None."""
    rule = _rule(dict(rule, mapping=None))
    dev = torch.device(device if device is not None else "cuda")
    with open(os.path.join(gt_scene_dir, "tsdf_info.pkl"), "rb") as fh:
        info = pickle.load(fh)
    tsdf = to_device(_arr0(os.path.join(gt_scene_dir, "full_tsdf_layer0.npz")), torch.float32, dev)
    sem, ins = (to_device(np.ascontiguousarray(_arr0(os.path.join(gt_scene_dir, f"full_{k}_layer_interpolate0.npz"))).astype(np.int32),
                          torch.int64, dev) for k in LABEL_KEYS)
    if tsdf.dim() != 3 or sem.shape != tsdf.shape or ins.shape != tsdf.shape:
        raise ValueError(f"{gt_scene_dir}: volumes of shapes {tuple(tsdf.shape)}, {tuple(sem.shape)}, {tuple(ins.shape)}")
    cells = torch.nonzero(sem != 0)
    at = lambda vol: vol[cells[:, 0], cells[:, 1], cells[:, 2]]
    origin, voxel_size = np.asarray(info["vol_origin"], np.float32).reshape(3), float(info["voxel_size"])
    objs = scene_objects(cells.to(torch.int32), at(tsdf), at(sem), at(ins), origin, voxel_size, **rule)
    name = os.path.basename(os.path.normpath(gt_scene_dir))
    return write_objects(name, objs, origin, voxel_size, rule, out_json, boxes_ply, names)


def format_objects(scene, objs, path):
    return f"{scene}: {len(objs)} objects, {sum(r['voxels'] for r in objs)} voxels -> {path}"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="object inventory of saved scenes: count, centroid and boxes per segment")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="<scene>_objects.json (and boxes_<scene>.ply) go here")
    ap.add_argument("--gt", help="also describe generate_gt's volumes of DIR/<scene>/ into <scene>_objects_gt.json")
    ap.add_argument("--min_voxels", default=1, type=int, help="segments of fewer rows are left out of the list")
    ap.add_argument("--surface", default=1.0, type=float, help="a row takes part where |tsdf| is below this")
    ap.add_argument("--no-oriented", dest="oriented", action="store_false", help="no heading and no oriented box")
    ap.add_argument("--boxes", action="store_true", help="also write boxes_<scene>.ply, the boxes as a wireframe")
    ap.add_argument("--names", metavar="FILE", help="text file of `id name` lines: adds class_name to every record")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    names = read_names(args.names) if args.names else None
    rule = dict(min_voxels=args.min_voxels, surface=args.surface, oriented=args.oriented)
    for scene in read_scene_list(args.scenes):
        path = os.path.join(args.out, scene + "_objects.json")
        objs = describe_scene(os.path.join(args.pred, scene + ".npz"), path,
                              os.path.join(args.out, f"boxes_{scene}.ply") if args.boxes else None, names, **rule)
        print(format_objects(scene, objs, path))
        if args.gt:
            path = os.path.join(args.out, scene + "_objects_gt.json")
            objs = describe_gt(os.path.join(args.gt, scene), path,
                               os.path.join(args.out, f"boxes_{scene}_gt.ply") if args.boxes else None, names, **rule)
            print(format_objects(scene + " (ground truth)", objs, path))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Simplify a mesh by quadric vertex clustering: the vertices of a cell of size `cell` that carry the same labels become one
vertex, placed where the planes of the faces around them meet best, and the faces that collapse or repeat are dropped.  The
reference has no such stage (its users run open3d's simplify_vertex_clustering on the .ply afterwards); the rule is this
project's own:

    out   = simplify_device(verts, faces, cell, semantic=None, instance=None, colors=None, origin=None, regularize=1e-3)
    mesh, report = simplify_mesh(mesh, cell, origin=None, regularize=1e-3)      # mesh dicts of save_scene, on the host
    reports = simplify_scene("scene0000_00.npz", out_dir, cell)                 # the three meshes of a saved scene, *_lod.ply

    python -m eprecon_amd.simplify --pred DIR --scenes FILE --out DIR --cell 0.08 [--regularize 1e-3] [--ply FILE ...]

What runs on the device (csrc/mesh_simplify.hip): the fp64 cell and packed key of every vertex, the cluster triple, unordered
key and referenced marks of every face, and per cluster the quadrics, the 3x3 solve, the clip to the cell's box, the normal and
the colour.  The two CSR lists the cluster kernel walks are eprecon_segment_lists_async's.  The ranks of the keys
(torch.unique), the first face of every unordered triple (torch.unique + scatter_reduce amin) and the compaction are torch
calls on the device.  Device tensors are required (no CPU fallback).  Every fp64 sum runs in a fixed order: two runs give the
same bits.
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import need_device, to_device
from .scene_io import VOLUME_KEYS, export_ply, read_ply, read_scene_list, scene_volumes

REPORT_KEYS = ("vertices_in", "faces_in", "clusters", "vertices_out", "faces_out", "faces_degenerate", "faces_duplicate", "max_shift")
LOD_NAMES = ("{}_lod.ply", "mesh_semantic_{}_lod.ply", "mesh_instance_{}_lod.ply")


def _segment_lists(idx, m):
    """CSR lists of eprecon_segment_lists_async: idx int32[n] in [-1, m) -> (offsets int32[m+1], order int32[n])"""
    lib = _lib.load()
    n, dev = idx.numel(), idx.device
    offsets = torch.empty(m + 1, dtype=torch.int32, device=dev)
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.eprecon_segment_workspace_bytes(n, m), dev)
    _lib.check(lib.eprecon_segment_lists_async(_lib.ptr(idx), n, m, _lib.ptr(offsets), _lib.ptr(order), _lib.ptr(ws), ws.numel(),
                                               _lib.current_stream()), "eprecon_segment_lists_async")
    return offsets, order


def _origin(origin):
    o = np.zeros(3, np.float64) if origin is None else np.array(_lib.host64(origin), np.float64).reshape(3)
    if not np.isfinite(o).all():
        raise ValueError(f"simplify: the origin must be finite, got {o}")
    return np.ascontiguousarray(o)


def _labels(label, n, name):
    if label is None:
        return None
    need_device(label)
    if label.shape != (n,):
        raise ValueError(f"simplify: {n} vertices, {name} of shape {tuple(label.shape)}")
    return label.to(torch.int32).contiguous()


def cluster_ids(verts, cell, semantic=None, instance=None, origin=None):
    """verts f32[N,3] on the device -> (cluster int32[N], key int64[N], n_clusters): the ranks of (cx, cy, cz, semantic,
    instance) in lexicographic order, c = floor((float64(v) - origin) / cell).  A missing label counts as 0 everywhere.
    ValueError for a vertex that is not finite or a cell outside [-2^20, 2^20): the packed key would not hold it."""
    need_device(verts)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"simplify: expected float32 vertices [N,3], got {verts.dtype} {tuple(verts.shape)}")
    if not (float(cell) > 0 and math.isfinite(float(cell))):
        raise ValueError(f"simplify: the cell size must be positive, got {cell}")
    verts, n, dev = verts.contiguous(), verts.shape[0], verts.device
    semantic, instance = _labels(semantic, n, "semantic"), _labels(instance, n, "instance")
    o = _origin(origin)
    key = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().eprecon_simplify_keys_async(_lib.ptr(verts), n, o.ctypes.data, float(cell), _lib.ptr(key), _lib.ptr(status),
                                                       _lib.current_stream()), "eprecon_simplify_keys_async")
    word = _lib.read_counts(status)[0]
    if word:
        parts = [p for bit, p in ((2, "a vertex that is not finite"), (4, "a cell outside [-2^20, 2^20): the key cannot hold it")) if word & bit]
        raise ValueError(f"simplify: {' and '.join(parts)} (status {word})")
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), key, 0
    combined = key
    if semantic is not None or instance is not None:
        zero = torch.zeros(n, dtype=torch.int32, device=dev)
        sem, ins = (zero if semantic is None else semantic), (zero if instance is None else instance)
        # (semantic, instance) as one signed 64-bit word that orders like the pair; then (cell, labels) by their ranks: both
        # rank counts are at most N < 2^31, so the product fits
        pair = sem.to(torch.int64) * (1 << 32) + (ins.to(torch.int64) + (1 << 31))
        pairs, pair_rank = torch.unique(pair, return_inverse=True)
        _, cell_rank = torch.unique(key, return_inverse=True)
        combined = cell_rank * pairs.numel() + pair_rank
    uniq, cluster = torch.unique(combined, return_inverse=True)
    return cluster.to(torch.int32), key, int(uniq.numel())


def simplify_device(verts, faces, cell, semantic=None, instance=None, colors=None, origin=None, regularize=1e-3):
    """Device tensors in (verts f32[N,3], faces int32[M,3], semantic / instance int[N], colors u8[N,3]), device tensors out, as
    a dict: cluster int32[N]; positions f64[K,3], normals f32[K,3], rgb u8[K,3] (None without colours), cluster_semantic /
    cluster_instance int32[K] (None without the label) per cluster; written bool[K]; tri int32[M,3]; kept int64[F] the input
    indices of the surviving faces; vertices f32[V,3] (the written positions rounded once), faces int32[F,3] re-indexed; and
    `report` (REPORT_KEYS).  ValueError for a face index outside [0, N), a vertex that is not finite, a cell the key cannot
    hold, or more than 2^21 clusters."""
    need_device(verts, faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"simplify: expected int32 faces [M,3], got {faces.dtype} {tuple(faces.shape)}")
    if not (float(regularize) > 0 and math.isfinite(float(regularize))):
        raise ValueError(f"simplify: regularize must be positive, got {regularize}")
    m = faces.shape[0]
    if 3 * m >= 2 ** 31:
        raise ValueError(f"simplify: {m} faces: 3 M must stay below 2^31")
    lib = _lib.load()
    cluster, key, k = cluster_ids(verts, cell, semantic, instance, origin)
    if k > int(lib.eprecon_simplify_max_clusters()):
        raise ValueError(f"simplify: {k} clusters: the face key holds at most 2^21; use a larger cell")
    verts, faces, n, dev = verts.contiguous(), faces.contiguous(), verts.shape[0], verts.device
    o = _origin(origin)
    if colors is not None:
        need_device(colors)
        if colors.shape != (n, 3) or colors.dtype != torch.uint8:
            raise ValueError(f"simplify: expected uint8 colours [{n},3], got {colors.dtype} {tuple(colors.shape)}")
        colors = colors.contiguous()
    stream = _lib.current_stream()

    tri = torch.empty((m, 3), dtype=torch.int32, device=dev)
    face_key = torch.empty(m, dtype=torch.int64, device=dev)
    written = torch.empty(k, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.eprecon_simplify_faces_async(_lib.ptr(faces), m, _lib.ptr(cluster), n, k, _lib.ptr(tri), _lib.ptr(face_key),
                                                _lib.ptr(written), _lib.ptr(status), stream), "eprecon_simplify_faces_async")
    if _lib.read_counts(status)[0]:
        raise ValueError(f"simplify: a face index outside [0, {n})")

    # the first face of every unordered triple survives, in input order
    index = torch.nonzero(face_key >= 0).reshape(-1)
    uniq, inverse = torch.unique(face_key[index], return_inverse=True)
    first = torch.full((uniq.numel(),), m, dtype=torch.int64, device=dev).scatter_reduce(0, inverse, index, "amin")
    kept = index[first[inverse] == index]

    positions = torch.empty((k, 3), dtype=torch.float64, device=dev)
    normals = torch.empty((k, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((k, 3), dtype=torch.uint8, device=dev) if colors is not None else None
    if k > 0:
        corner_offsets, corner_order = _segment_lists(tri.reshape(-1), k)
        member_offsets, member_order = _segment_lists(cluster, k)
        _lib.check(lib.eprecon_simplify_quadrics_async(
            _lib.ptr(verts), n, _lib.ptr(faces), m, _lib.ptr(colors), _lib.ptr(key), _lib.ptr(corner_offsets), _lib.ptr(corner_order),
            _lib.ptr(member_offsets), _lib.ptr(member_order), k, o.ctypes.data, float(cell), float(regularize), _lib.ptr(positions),
            _lib.ptr(normals), _lib.ptr(rgb), stream), "eprecon_simplify_quadrics_async")

    written = written.bool()
    new_id = torch.cumsum(written.to(torch.int64), 0) - 1
    out_faces = new_id[tri[kept].to(torch.int64)].to(torch.int32).reshape(-1, 3)
    # (a label is the same on every member: the last writer is as good as any)
    of = lambda label: None if label is None else torch.zeros(k, dtype=torch.int32, device=dev).scatter_(0, cluster.long(), label.to(torch.int32))
    shift = (verts.to(torch.float64) - positions[cluster.long()]).square().sum(1).max().sqrt() if n > 0 else torch.zeros((), dtype=torch.float64, device=dev)
    counts = _lib.read_counts(torch.stack([written.sum(), shift.view(torch.int64)]))
    report = {"vertices_in": n, "faces_in": m, "clusters": k, "vertices_out": int(counts[0]), "faces_out": int(kept.numel()),
              "faces_degenerate": m - int(index.numel()), "faces_duplicate": int(index.numel()) - int(kept.numel()),
              "max_shift": float(np.array(counts[1], np.int64).view(np.float64))}
    return {"cluster": cluster, "positions": positions, "normals": normals, "rgb": rgb, "cluster_semantic": of(semantic),
            "cluster_instance": of(instance), "written": written, "tri": tri, "kept": kept,
            "vertices": positions[written].to(torch.float32), "faces": out_faces, "report": report}


def simplify_mesh(mesh, cell, origin=None, regularize=1e-3, device=None):
    """A mesh dict in save_scene's form (vertices f32[N,3], faces int32[M,3]; vertex_semantic, vertex_instance, vertex_colors
    carried when present) -> (the simplified mesh in the same form, with vertex_normals, on the host; the report)."""
    dev = torch.device(device if device is not None else "cuda")
    need_device(dev)
    opt = lambda k, dtype: None if mesh.get(k) is None else to_device(mesh[k], dtype, dev)
    colors = mesh.get("vertex_colors")
    if colors is not None:
        colors = to_device(np.ascontiguousarray(np.asarray(colors)[:, :3]), torch.uint8, dev)
    out = simplify_device(to_device(mesh["vertices"], torch.float32, dev).reshape(-1, 3), to_device(mesh["faces"], torch.int32, dev).reshape(-1, 3),
                          cell, opt("vertex_semantic", torch.int32), opt("vertex_instance", torch.int32), colors, origin, regularize)
    w = out["written"]
    host = lambda t: t[w].cpu().numpy()
    new = {"vertices": out["vertices"].cpu().numpy(), "faces": out["faces"].cpu().numpy(), "vertex_normals": host(out["normals"])}
    for k, v in (("vertex_colors", out["rgb"]), ("vertex_semantic", out["cluster_semantic"]), ("vertex_instance", out["cluster_instance"])):
        if v is not None:
            new[k] = host(v)
    return new, out["report"]


def simplify_scene(npz, out_dir, cell, origin=None, regularize=1e-3, device=None):
    """A scene file in either form SaveScene writes -> the three meshes of tsdf_panoptic2mesh, each simplified, as
    <scene>_lod.ply, mesh_semantic_<scene>_lod.ply and mesh_instance_<scene>_lod.ply in out_dir -> their three reports.
    The cells are counted from `origin` in world coordinates (default: zero), as in simplify_mesh."""
    from .save_scene import tsdf_panoptic2mesh
    dev = torch.device(device if device is not None else "cuda")
    tsdf, semantic, instance, scene_origin, voxel_size = scene_volumes(npz, dev, VOLUME_KEYS)
    meshes = tsdf_panoptic2mesh(voxel_size, torch.from_numpy(scene_origin).to(dev), tsdf, semantic, instance)
    name = os.path.splitext(os.path.basename(npz))[0]
    os.makedirs(out_dir, exist_ok=True)
    reports = []
    for mesh, pattern in zip(meshes, LOD_NAMES):
        lod, report = simplify_mesh(mesh, cell, origin, regularize, dev)
        export_ply(lod, os.path.join(out_dir, pattern.format(name)))
        reports.append(report)
    return reports


def simplify_ply(path, out_path, cell, origin=None, regularize=1e-3, device=None):
    """a plain PLY file (geometry only: read_ply reads no attributes) -> out_path -> the report"""
    verts, faces = read_ply(path)
    lod, report = simplify_mesh({"vertices": verts, "faces": faces}, cell, origin, regularize, device)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    export_ply(lod, out_path)
    return report


def format_report(name, report):
    return (f"{name}: {report['vertices_in']} -> {report['vertices_out']} vertices, {report['faces_in']} -> {report['faces_out']} faces "
            f"({report['clusters']} clusters, {report['faces_degenerate']} collapsed, {report['faces_duplicate']} duplicate), "
            f"largest shift {report['max_shift']:.4g}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="simplify the meshes of saved scenes (or plain PLY files) by quadric vertex clustering")
    ap.add_argument("--pred", help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--scenes", help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="the *_lod.ply files go here")
    ap.add_argument("--cell", required=True, type=float, help="the cell size, in the mesh's units")
    ap.add_argument("--regularize", default=1e-3, type=float, help="the pull towards the mean, relative to trace(A) / 3")
    ap.add_argument("--ply", nargs="+", default=[], metavar="FILE", help="plain PLY files (geometry only) -> <name>_lod.ply")
    args = ap.parse_args(argv)
    if not args.ply and not (args.pred and args.scenes):
        ap.error("give --pred and --scenes, or --ply")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.pred and args.scenes:
        for scene in read_scene_list(args.scenes):
            reports = simplify_scene(os.path.join(args.pred, scene + ".npz"), args.out, args.cell, regularize=args.regularize)
            print(format_report(scene, reports[0]))
    for path in args.ply:
        name = os.path.splitext(os.path.basename(path))[0]
        print(format_report(name, simplify_ply(path, os.path.join(args.out, name + "_lod.ply"), args.cell, regularize=args.regularize)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

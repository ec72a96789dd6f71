"""Vertex colours from the video: the pixels of posed colour frames carried onto the vertices of a mesh, on
libeprecon_hip.so (csrc/mesh_colorize.hip).  The reference has only a commented-out colour path in its ground-truth fusion;
the rule is this project's own:

    col = MeshColorizer(verts, faces, tolerance=0.04)          # verts f32[N,3] world, faces int32[M,3] on the device
    col.integrate(frames, K, poses)                            # frames u8[V,H,W,3] (device or host), K of the frames
    rgb, seen = col.colors()                                   # u8[N,3], int32[N]
    mesh = colorize_mesh(mesh, frames, K, poses)               # the mesh dict + vertex_colors, vertex_seen
    mesh = colorize_scene("scene0000_00.npz", data_path, "scene0000_00", every=10)

    python -m eprecon_amd.colorize --pred DIR --data_path DIR --scenes FILE [--out DIR] [--every 10] [--vis_size W H]
                                   [--min_views 1]

Per (vertex, view): the vertex must lie in [znear, zfar], be no farther than `tolerance` (one voxel) behind what the mesh's
own visibility buffer (render.visibility at `vis_size`) holds at its pixel, see the face that won that pixel at
cos >= min_cos, and project inside the frame; it then takes the bilinear sample with the weight cos / z^2.  The sums are
fp64 and sequential per vertex: bit-identical run to run and however the views are split into integrate() calls, so a scene
of hundreds of frames is integrated in chunks with only one chunk's frames resident.  Device tensors are required for the
mesh (no CPU fallback).
"""
import argparse
import os

import numpy as np
import torch

from . import _lib
from . import render as RD
from ._lib import host64, need_device
from .scene_io import export_ply, intrinsic, pose, pose_frame_ids, read_scene_list

DEFAULT_FALLBACK = (153, 153, 153)       # resolve's grey
DEFAULT_TOLERANCE = 0.04                 # one voxel of the default scene
DEFAULT_MIN_COS = 0.1
CHUNK = 32                               # views resident at a time


class MeshColorizer:
    """running sums acc f64[N,4] = sum of (w r, w g, w b, w) and seen int32[N] over every view integrated so far"""

    def __init__(self, verts, faces, vis_size=None, tolerance=DEFAULT_TOLERANCE, min_cos=DEFAULT_MIN_COS, znear=0.05,
                 zfar=100.0, pixel_center=0.5):
        self.verts, self.faces = RD.mesh_tensors(verts, faces)
        self.vis_size = None if vis_size is None else (int(vis_size[0]), int(vis_size[1]))
        self.tolerance, self.min_cos = float(tolerance), float(min_cos)
        self.znear, self.zfar, self.pixel_center = float(znear), float(zfar), float(pixel_center)
        n, dev = self.verts.shape[0], self.verts.device
        self.acc = torch.zeros((n, 4), dtype=torch.float64, device=dev)
        self.seen = torch.zeros(n, dtype=torch.int32, device=dev)

    def integrate(self, frames, K, poses):
        """frames uint8[V,H,W,3] on the device or the host (one copy), K [3,3] of the frames, poses [V,4,4] camera -> world"""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("integrate: expected uint8 frames [V,H,W,3]")
        v, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        p = host64(poses).reshape(-1, 4, 4)
        if p.shape[0] != v:
            raise ValueError(f"integrate: {v} frames, {p.shape[0]} poses")
        if v == 0 or self.verts.shape[0] == 0:
            return self
        if h < 2 or w < 2:
            raise ValueError(f"integrate: frames of {h} x {w}; at least 2 x 2")
        dev = self.verts.device
        frames = frames.to(dev).contiguous()
        k = host64(K).reshape(3, 3)
        if not np.array_equal(k[2], [0.0, 0.0, 1.0]):
            raise _lib.EpreconError("integrate: K must have the last row (0, 0, 1)")
        wd, hd = self.vis_size or RD.NATIVE_SIZE
        k_vis = RD.scaled_intrinsics(k, (wd, hd), native=(w, h))
        vis = RD.visibility(self.verts, self.faces, k_vis, p, hd, wd, znear=self.znear, zfar=self.zfar,
                            pixel_center=self.pixel_center)
        self.accumulate(frames, vis, k, k_vis, p)
        return self

    def accumulate(self, frames, vis, K, K_vis, poses):
        """the accumulate entry alone on a visibility buffer u64[V,Hd,Wd] of this mesh at K_vis (integrate() makes it)"""
        need_device(frames, vis)
        p = host64(poses).reshape(-1, 4, 4)
        cams = torch.from_numpy(np.concatenate([host64(K).reshape(9), host64(K_vis).reshape(9),
                                                np.linalg.inv(p)[:, :3, :4].ravel()])).to(self.verts.device)
        if frames.dtype != torch.uint8 or vis.dtype not in (torch.uint64, torch.int64) or vis.shape[0] != frames.shape[0] \
                or p.shape[0] != frames.shape[0]:
            raise ValueError("accumulate: expected uint8 frames [V,H,W,3], a 64-bit buffer [V,Hd,Wd] and V poses")
        frames, vis = frames.contiguous(), vis.contiguous()
        lib = _lib.load()
        _lib.check(lib.eprecon_colorize_accumulate_async(
            _lib.ptr(self.verts), self.verts.shape[0], _lib.ptr(self.faces), self.faces.shape[0], _lib.ptr(cams),
            int(frames.shape[0]), _lib.ptr(frames), int(frames.shape[1]), int(frames.shape[2]), _lib.ptr(vis), int(vis.shape[1]),
            int(vis.shape[2]), self.pixel_center, self.znear, self.zfar, self.tolerance, self.min_cos, _lib.ptr(self.acc),
            _lib.ptr(self.seen), _lib.current_stream()), "eprecon_colorize_accumulate_async")
        return self

    def colors(self, min_views=1, fallback=DEFAULT_FALLBACK):
        """-> (rgb uint8[N,3], seen int32[N]) on the device: the weighted mean rounded half up where seen >= min_views, the
        `fallback` colour elsewhere"""
        n = self.verts.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.uint8, device=self.verts.device)
        fb = [int(c) for c in fallback]
        _lib.check(_lib.load().eprecon_colorize_finish_async(
            _lib.ptr(self.acc), _lib.ptr(self.seen), n, int(min_views), fb[0], fb[1], fb[2], _lib.ptr(rgb),
            _lib.current_stream()), "eprecon_colorize_finish_async")
        return rgb, self.seen.clone()


def _split_rule(rule):
    finish = {k: rule.pop(k) for k in ("min_views", "fallback") if k in rule}
    return rule, finish


def colorize_mesh(mesh, frames, K, poses, chunk=CHUNK, **rule):
    """mesh: a mesh dict, a (verts, faces) pair or a .ply path (render.device_mesh) -> the mesh dict with vertex_colors
    uint8[N,3] and vertex_seen int32[N] (numpy; vertices and faces too when the mesh was not a dict).  **rule:
    MeshColorizer's and colors()' keywords."""
    verts, faces, extra = RD.device_mesh(mesh)
    rule, finish = _split_rule(dict(rule))
    col = MeshColorizer(verts, faces, **rule)
    p = host64(poses).reshape(-1, 4, 4)
    if len(frames) != p.shape[0]:
        raise ValueError(f"colorize_mesh: {len(frames)} frames, {p.shape[0]} poses")
    for s in range(0, p.shape[0], max(int(chunk), 1)):
        col.integrate(frames[s:s + chunk], K, p[s:s + chunk])
    rgb, seen = col.colors(**finish)
    out = dict(extra) if extra else {"vertices": verts.cpu().numpy(), "faces": faces.cpu().numpy()}
    out.update(vertex_colors=rgb.cpu().numpy(), vertex_seen=seen.cpu().numpy())
    return out


# ------------------------------------------------------------------------------------------------------------- frames

def scene_frames(data_path, scene, ids):
    """<data_path>/<scene>/color/color_<id>.jpg, pose/pose_<id>.txt and intrinsic/intrinsic_color.txt ->
    (frames uint8[V,H,W,3], K f64[3,3], poses f64[V,4,4], the ids kept); frames whose pose is not finite are skipped"""
    from PIL import Image
    root = os.path.join(data_path, scene)
    k = intrinsic(root, "color")
    frames, poses, kept = [], [], []
    for i in ids:
        p = pose(root, i)
        if not np.isfinite(p).all():
            continue
        with Image.open(os.path.join(root, "color", f"color_{int(i):d}.jpg")) as im:
            frames.append(np.asarray(im.convert("RGB"), np.uint8))
        poses.append(p)
        kept.append(int(i))
    if not kept:
        return np.zeros((0, 2, 2, 3), np.uint8), k, np.zeros((0, 4, 4)), kept
    return np.stack(frames), k, np.array(poses, np.float64).reshape(-1, 4, 4), kept


def colorize_scene(npz_path, data_path, scene, every=10, ids=None, chunk=CHUNK, **rule):
    """a saved scene (either .npz form) coloured from its frames 0, every, 2 every, ... (or `ids`), read and integrated
    `chunk` at a time; the tolerance is the file's voxel_size unless given -> {vertices, faces, vertex_normals,
    vertex_colors, vertex_seen} (numpy): scene_mesh's geometry with marching cubes' normals"""
    verts, faces, normals, _, _, voxel = RD.scene_mesh_normals(npz_path)
    rule, finish = _split_rule(dict(rule))
    rule.setdefault("tolerance", voxel)
    col = MeshColorizer(verts, faces, **rule)
    ids = pose_frame_ids(os.path.join(data_path, scene), every) if ids is None else [int(i) for i in ids]
    step = max(int(chunk), 1)
    for s in range(0, len(ids), step):
        frames, k, poses, kept = scene_frames(data_path, scene, ids[s:s + step])
        if kept:
            col.integrate(frames, k, poses)
    rgb, seen = col.colors(**finish)
    return {"vertices": verts.cpu().numpy(), "faces": faces.cpu().numpy(), "vertex_normals": normals.cpu().numpy(),
            "vertex_colors": rgb.cpu().numpy(), "vertex_seen": seen.cpu().numpy()}


def write_colored_scene(npz_path, data_path, scene, out_dir, **kwargs):
    """colorize_scene -> <out_dir>/mesh_color_<scene>.ply (export_ply: normals, then red / green / blue as the other
    coloured copies have them) -> (path, mesh)"""
    mesh = colorize_scene(npz_path, data_path, scene, **kwargs)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"mesh_color_{scene}.ply")
    export_ply(mesh, path)
    return path, mesh


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="colour the meshes of saved scenes from their colour frames")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--data_path", required=True, help="ScanNet-layout scenes: <scene>/color, pose, intrinsic")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", help="mesh_color_<scene>.ply goes here (default: --pred)")
    ap.add_argument("--every", default=10, type=int, help="use every n-th frame (default 10)")
    ap.add_argument("--vis_size", default=list(RD.NATIVE_SIZE), type=int, nargs=2, metavar=("W", "H"),
                    help="size of the visibility buffer (default 640 480)")
    ap.add_argument("--min_views", default=1, type=int, help="views a vertex needs to take a colour (default 1)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = args.out or args.pred
    for scene in read_scene_list(args.scenes):
        path, mesh = write_colored_scene(os.path.join(args.pred, scene + ".npz"), args.data_path, scene, out, every=args.every,
                                         vis_size=tuple(args.vis_size), min_views=args.min_views)
        seen = mesh["vertex_seen"]
        share = float((seen >= args.min_views).mean()) if len(seen) else 0.0
        print(f"{scene}: {len(seen)} vertices, {100.0 * share:.1f} % seen -> {path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

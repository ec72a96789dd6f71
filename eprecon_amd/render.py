"""View rendering: a mesh seen from camera poses as depth, face, label and flat-shaded images — what the reference's
tools/render.py and VIS_INCREMENTAL show in a pyrender window, on libeprecon_hip.so (csrc/mesh_render.hip), headless:

    vis = visibility(verts, faces, K, poses, 480, 640)                  # u64[V,H,W]: depth bits << 32 | face index
    out = resolve(vis, verts, faces, K, poses, labels=(sem, ins), backgrounds=(0, 0), colors=rgb)
    out["depth"], out["face"], out["corner"], out["labels"][0], out["rgb"]
    render_labels(mesh, K, poses, 480, 640)                             # mesh: a tsdf_panoptic2mesh dict or a .ply path
    render_shaded(mesh, K, poses, 480, 640)
    render_scene("scene0000_00.npz", K, poses, 480, 640)                # semantic / instance ids and palette images

    python -m eprecon_amd.render --pred DIR --data_path DIR --scenes FILE --out DIR [--every 10] [--size 640 480]
                                 [--mode semantic|instance|shaded|all]

Device tensors are required (no CPU fallback).  A pixel takes the id of the nearest corner of the triangle it sees (the
largest perspective-correct weight): ids are never interpolated.  Shading is this project's flat rule:
I = ambient + (1 - ambient) |n . d| per face, channel = min(255, floor(c I + 0.5)).
"""
import argparse
import os

import numpy as np
import torch

from . import _lib
from ._lib import host64, need_device, to_device
from .evaluation import QUEUE_CAP
from .save_scene import COLOR_PALETTE, marching_cubes
from .scene_io import intrinsic, load_mesh, pose, pose_frame_ids, read_scene_list, scene_volumes

DEFAULT_AMBIENT = 0.3                    # the reference's ambient_light
DEFAULT_BACKGROUND = (255, 255, 255)     # the reference's bg_color
NATIVE_SIZE = (640, 480)                 # ScanNet's depth sensor: what intrinsic_depth.txt refers to
CHUNK = 32                               # views per launch of the command-line tools
INF_BITS = 0x7F800000                    # upper word of a visibility entry at or above this: nothing is hit


def _cams(K, poses, dev, what):
    k = host64(K).reshape(3, 3)
    if not np.array_equal(k[2], [0.0, 0.0, 1.0]):
        raise _lib.EpreconError(f"{what}: K must have the last row (0, 0, 1)")
    p = host64(poses).reshape(-1, 4, 4)
    if p.shape[0] < 1:
        raise ValueError(f"{what}: no pose")
    w2c = np.linalg.inv(p)[:, :3, :4].reshape(-1, 12)
    return torch.from_numpy(np.concatenate([k.ravel(), np.linalg.inv(k).ravel(), w2c.ravel()])).to(dev), p.shape[0]


def mesh_tensors(verts, faces):
    need_device(verts, faces)
    verts, faces = verts.to(torch.float32).contiguous(), faces.to(torch.int32).contiguous()
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"expected verts [N,3] and faces [M,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    return verts, faces


def visibility(verts, faces, K, poses, height, width, znear=0.05, zfar=100.0, cull_back=True, pixel_center=0.5,
               queue_capacity=None):
    """verts f32[N,3] (world), faces int32[M,3] on the device; K [3,3]; poses [V,4,4] camera -> world -> u64[V,H,W] on the
    device (torch.uint64): (fp32 depth bits << 32) | index of the nearest face drawn at that pixel, all-ones where none
    is.  The arguments are evaluation.render_depth's, and the upper word is its result bit for bit (+inf bits or above
    instead of 0 where nothing is hit); at equal depth bits the smallest face index wins; run-to-run bit-identical."""
    verts, faces = mesh_tensors(verts, faces)
    lib = _lib.load()
    dev = verts.device
    cams, v = _cams(K, poses, dev, "visibility")
    out = torch.empty((v, int(height), int(width)), dtype=torch.uint64, device=dev)
    cap = int(min(v * max(faces.shape[0], 1), QUEUE_CAP)) if queue_capacity is None else int(queue_capacity)
    ws = torch.empty(int(lib.eprecon_render_visibility_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
    _lib.check(lib.eprecon_render_visibility_async(
        _lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(cams), v, int(height), int(width),
        float(pixel_center), float(znear), float(zfar), int(bool(cull_back)), _lib.ptr(out), cap, _lib.ptr(ws), ws.numel(),
        _lib.current_stream()), "eprecon_render_visibility_async")
    return out


def resolve(vis, verts, faces, K, poses, labels=(), backgrounds=(), colors=None, ambient=DEFAULT_AMBIENT,
            background_rgb=DEFAULT_BACKGROUND, pixel_center=0.5, outputs=("depth", "face", "corner", "rgb")):
    """vis: visibility()'s buffer for the same mesh, cameras and pixel_center -> a dict of device tensors [V,H,W]:
    depth f32 (0 where nothing is hit), face int32 (-1), corner int32: the vertex index of the face's corner with the
    largest perspective-correct weight (the earlier slot on ties; -1), labels: a list with one int32 image per array of
    `labels` (up to two per-vertex int32[N] device arrays; `backgrounds`, default 0, where nothing is hit), rgb
    uint8[V,H,W,3]: flat shading of `colors` uint8[N,3] (153 grey without) with `background_rgb` where nothing is hit.
    `outputs` names which of depth / face / corner / rgb are produced."""
    verts, faces = mesh_tensors(verts, faces)
    need_device(vis)
    if vis.dtype not in (torch.uint64, torch.int64) or vis.dim() != 3:
        raise ValueError(f"resolve: expected a 64-bit [V,H,W] visibility buffer, got {vis.dtype} {tuple(vis.shape)}")
    lib = _lib.load()
    dev = verts.device
    cams, v = _cams(K, poses, dev, "resolve")
    vis = vis.contiguous()
    if vis.shape[0] != v:
        raise ValueError(f"resolve: {vis.shape[0]} views in the buffer, {v} poses")
    labels = list(labels)
    if len(labels) > 2:
        raise ValueError("resolve: at most two label arrays per call")
    backgrounds = list(backgrounds) + [0] * (len(labels) - len(backgrounds))
    n = verts.shape[0]
    labs = []
    for a in labels:
        need_device(a)
        a = a.to(torch.int32).contiguous().reshape(-1)
        if a.numel() != n:
            raise ValueError(f"resolve: a label array of {a.numel()} entries for {n} vertices")
        labs.append(a)
    if colors is not None:
        need_device(colors)
        colors = colors.to(torch.uint8).contiguous()
        if tuple(colors.shape) != (n, 3):
            raise ValueError(f"resolve: colours {tuple(colors.shape)} for {n} vertices")
    unknown = set(outputs) - {"depth", "face", "corner", "rgb"}
    if unknown:
        raise ValueError(f"resolve: unknown outputs {sorted(unknown)}")
    shape = tuple(vis.shape)
    new = lambda name, dtype, extra=(): torch.empty(shape + extra, dtype=dtype, device=dev) if name in outputs else None
    depth, face, corner = new("depth", torch.float32), new("face", torch.int32), new("corner", torch.int32)
    rgb = new("rgb", torch.uint8, (3,))
    lab_out = [torch.empty(shape, dtype=torch.int32, device=dev) for _ in labs]
    la, lb = (labs + [None, None])[:2]
    oa, ob = (lab_out + [None, None])[:2]
    ba, bb = (backgrounds + [0, 0])[:2]
    bg = [int(c) for c in background_rgb]
    _lib.check(lib.eprecon_render_resolve_async(
        _lib.ptr(vis), _lib.ptr(verts), n, _lib.ptr(faces), faces.shape[0], _lib.ptr(cams), v, shape[1], shape[2],
        float(pixel_center), _lib.ptr(depth), _lib.ptr(face), _lib.ptr(corner), _lib.ptr(la), int(ba), _lib.ptr(oa),
        _lib.ptr(lb), int(bb), _lib.ptr(ob), _lib.ptr(colors), float(ambient), bg[0], bg[1], bg[2], _lib.ptr(rgb),
        _lib.current_stream()), "eprecon_render_resolve_async")
    out = {k: t for k, t in (("depth", depth), ("face", face), ("corner", corner), ("rgb", rgb)) if t is not None}
    out["labels"] = lab_out
    return out


# --------------------------------------------------------------------------------------------------------- conveniences

def device_mesh(mesh, device=None):
    """a tsdf_panoptic2mesh dict, a (verts, faces) pair or a .ply path -> (verts, faces on the device, the dict or {})"""
    verts, faces = load_mesh(mesh)
    dev = torch.device(device if device is not None else (verts.device if isinstance(verts, torch.Tensor) else "cuda"))
    return to_device(verts, torch.float32, dev), to_device(faces, torch.int32, dev), (mesh if isinstance(mesh, dict) else {})


def render_labels(mesh, K, poses, height, width, labels=None, backgrounds=(0, 0), device=None, **raster):
    """-> {depth, face, corner, labels: [...]}.  mesh: one of tsdf_panoptic2mesh's dicts (whichever of vertex_semantic,
    vertex_instance it carries are the default `labels`, in that order), a (verts, faces) pair or a .ply path (geometry
    only: give `labels`, per-vertex int arrays).  **raster: znear, zfar, cull_back, pixel_center."""
    verts, faces, extra = device_mesh(mesh, device)
    if labels is None:
        labels = [extra[k] for k in ("vertex_semantic", "vertex_instance") if k in extra]
    labs = [to_device(a, torch.int32, verts.device) for a in labels]
    vis = visibility(verts, faces, K, poses, height, width, **raster)
    return resolve(vis, verts, faces, K, poses, labels=labs, backgrounds=backgrounds,
                   pixel_center=raster.get("pixel_center", 0.5), outputs=("depth", "face", "corner"))


def render_shaded(mesh, K, poses, height, width, colors=None, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND,
                  device=None, **raster):
    """-> uint8[V,H,W,3] on the device.  colors default to the dict's vertex_colors, else the reference's 0.6 grey."""
    verts, faces, extra = device_mesh(mesh, device)
    if colors is None:
        colors = extra.get("vertex_colors")
    col = None if colors is None else to_device(colors, torch.uint8, verts.device)
    vis = visibility(verts, faces, K, poses, height, width, **raster)
    return resolve(vis, verts, faces, K, poses, colors=col, ambient=ambient, background_rgb=background_rgb,
                   pixel_center=raster.get("pixel_center", 0.5), outputs=("rgb",))["rgb"]


def scene_mesh(npz_path, device=None):
    """<scene>.npz in any layout (scene_io.py) -> (verts f32[N,3] world, faces int32[M,3], semantic, instance int32[N])
    on the device: marching cubes of the TSDF at level 0 with the label volumes sampled at the vertices, as
    tsdf_panoptic2mesh does.  Voxel rows become volumes on the device (TSDF default 1, ids default 0)."""
    verts, faces, _, vsem, vins, _ = scene_mesh_normals(npz_path, device)
    return verts, faces, vsem, vins


def scene_mesh_normals(npz_path, device=None):
    """scene_mesh with marching cubes' normals and the file's voxel_size -> (verts, faces, normals f32[N,3], semantic,
    instance, voxel_size)"""
    dev = torch.device(device if device is not None else "cuda")
    tsdf, sem, ins, origin, voxel_size = scene_volumes(npz_path, dev)
    verts, faces, normals, vsem, vins = marching_cubes(tsdf, 0.0, labels=(sem, ins))
    return verts * voxel_size + torch.from_numpy(origin.reshape(1, 3)).to(dev), faces, normals, vsem, vins, voxel_size


def palette_colors(ids):
    """per-vertex ids on the device -> uint8[N,3] of save_scene.COLOR_PALETTE (id modulo the palette size)"""
    pal = torch.from_numpy(COLOR_PALETTE).to(ids.device)
    return pal[ids.to(torch.int64) % len(COLOR_PALETTE)]


def render_scene(npz_path, K, poses, height, width, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND, device=None,
                 modes=("semantic", "instance", "shaded"), **raster):
    """A saved scene from the cameras `poses` -> {depth, face, semantic, instance int32[V,H,W] (the stored ids, 0 where
    nothing is seen), semantic_rgb, instance_rgb (the palette colours of tsdf_panoptic2mesh, shaded), shaded_rgb (grey)}
    on the device; `modes` selects the rgb images.  One visibility pass, one resolve per image kind."""
    return render_panoptic_mesh(scene_mesh(npz_path, device), K, poses, height, width, ambient, background_rgb, modes, **raster)


def render_panoptic_mesh(mesh, K, poses, height, width, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND,
                         modes=("semantic", "instance", "shaded"), **raster):
    """render_scene on scene_mesh's tuple (the command-line tool meshes a scene once and renders it in chunks of views)"""
    verts, faces, vsem, vins = mesh
    pc = raster.get("pixel_center", 0.5)
    vis = visibility(verts, faces, K, poses, height, width, **raster)
    colors = {"semantic": palette_colors(vsem), "instance": palette_colors(vins), "shaded": None}
    modes = [m for m in ("semantic", "instance", "shaded") if m in modes]
    out = {}
    for i, mode in enumerate(modes or [None]):
        first = i == 0
        r = resolve(vis, verts, faces, K, poses, labels=(vsem, vins) if first else (), backgrounds=(0, 0),
                    colors=colors.get(mode), ambient=ambient, background_rgb=background_rgb, pixel_center=pc,
                    outputs=(("depth", "face") if first else ()) + (("rgb",) if mode else ()))
        if first:
            out.update(depth=r["depth"], face=r["face"], semantic=r["labels"][0], instance=r["labels"][1])
        if mode:
            out[mode + "_rgb"] = r["rgb"]
    return out


def write_png(path, image):
    """uint8 [H,W,3] / [H,W] (device tensor or array) -> a PNG file"""
    from PIL import Image
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"write_png: expected uint8 [H,W] or [H,W,3], got {a.dtype} {a.shape}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(a)).save(path, format="PNG")
    return path


# ------------------------------------------------------------------------------------------------------------- frames

def scaled_intrinsics(K, size, native=NATIVE_SIZE):
    """K of a `native` (width, height) image -> K of the same view at `size` (width, height)"""
    k = np.array(np.asarray(K, np.float64)[:3, :3])
    k[0] *= float(size[0]) / float(native[0])
    k[1] *= float(size[1]) / float(native[1])
    k[2] = [0.0, 0.0, 1.0]
    return k


def scene_views(data_path, scene, every=10, size=NATIVE_SIZE):
    """<data_path>/<scene>/pose/pose_<i>.txt for i = 0, every, 2 every, ... below the number of pose files, and
    intrinsic/intrinsic_depth.txt scaled to `size` -> (frame ids, K f64[3,3], poses f64[n,4,4]); frames whose pose is not
    finite are skipped"""
    root = os.path.join(data_path, scene)
    ids, poses = [], []
    for i in pose_frame_ids(root, every):
        p = pose(root, i)
        if np.isfinite(p).all():
            ids.append(i)
            poses.append(p)
    return ids, scaled_intrinsics(intrinsic(root, "depth"), size), np.array(poses, np.float64).reshape(-1, 4, 4)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="semantic, instance and shaded views of saved scenes from their camera poses")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--data_path", required=True, help="ScanNet-layout scenes: <scene>/pose, intrinsic")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="images go to <out>/<scene>/<mode>_<i>.png")
    ap.add_argument("--every", default=10, type=int, help="render every n-th frame (default 10)")
    ap.add_argument("--size", default=list(NATIVE_SIZE), type=int, nargs=2, metavar=("W", "H"), help="image size (default 640 480)")
    ap.add_argument("--mode", default="all", choices=["semantic", "instance", "shaded", "all"])
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    modes = ("semantic", "instance", "shaded") if args.mode == "all" else (args.mode,)
    w, h = args.size
    written = []
    for scene in read_scene_list(args.scenes):
        ids, k, poses = scene_views(args.data_path, scene, args.every, (w, h))
        mesh = scene_mesh(os.path.join(args.pred, scene + ".npz"))
        for s in range(0, len(ids), CHUNK):
            out = render_panoptic_mesh(mesh, k, poses[s:s + CHUNK], h, w, modes=modes)
            for mode in modes:
                images = out[mode + "_rgb"].cpu().numpy()
                for j, i in enumerate(ids[s:s + CHUNK]):
                    written.append(write_png(os.path.join(args.out, scene, f"{mode}_{i:d}.png"), images[j]))
        print(f"{scene}: {len(ids)} frames")
    print(f"{len(written)} images under {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

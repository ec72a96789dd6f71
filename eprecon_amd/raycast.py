"""Ray casting: what a camera sees of a scene, straight from its voxel rows — depth, surface normal and the row each pixel
shows — on libeprecon_hip.so (csrc/tsdf_raycast.hip).  No dense volume, no mesh: the surface is the zero set of the trilinear
interpolation of the very TSDF samples the meshes are cut from (DESIGN.md §5b "ray-cast surface"), found by a walk over the
4x4x4-cell bricks that hold a cell with a non-positive corner.

    grid = SceneGrid(coords, tsdf, origin, voxel_size)                  # device rows; holds the row and brick tables
    grid = SceneGrid.from_file("scene0000_00.npz")                      # any of the three layouts (scene_io.py)
    grid = SceneGrid.from_outputs(outputs, batch_idx)                   # outputs["scene_sparse"] of NeuralRecon.forward
    out = raycast(grid, K, poses, 480, 640)                             # {"depth" f32, "normal" f32[...,3], "row" int32} [V,H,W]
    sem, ins = raycast_labels(grid, out, semantic, instance)            # sem[row], ins[row]: ids are never interpolated
    rgb = raycast_shaded(grid, out, K, poses, colors=None)              # render.py's flat rule with the ray-cast normal
    raycast_scene("scene0000_00.npz", K, poses, 480, 640)               # render.render_scene's dict, from the rows

    python -m eprecon_amd.raycast --pred DIR --data_path DIR --scenes FILE --out DIR [--every 10] [--size 640 480]
                                  [--mode depth|normal|semantic|instance|shaded|all]

Device tensors are required (no CPU fallback).  poses are camera -> world, depth is camera-z in metres (0 where nothing is
hit), normals are unit, in the world frame, towards positive TSDF; `row` indexes the caller's row arrays (-1).  The images
are bit-identical from run to run and however the views are split into calls.
"""
import argparse
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import host64, need_device, to_device
from .render import CHUNK, DEFAULT_AMBIENT, DEFAULT_BACKGROUND, NATIVE_SIZE, _cams, palette_colors, scene_views, write_png
from .scene_io import VOLUME_KEYS, raster_rows, read_scene, read_scene_list

DEFAULT_GREY = 153.0          # the reference's baseColorFactor 0.6, as render.py's resolve uses it
MODES = ("depth", "normal", "semantic", "instance", "shaded")
_INT_MAX = 0x7fffffff


class SceneGrid:
    """A scene's voxel rows with the tables a cast walks: coords int32[M,3] (sample c sits at origin + c * voxel_size; any
    coordinates the hash key allows, negative ones included; pairwise distinct — of rows that repeat a coordinate the first
    counts), tsdf f32[M], on the device.  One host read (the build's status and the box of the active cells); none, and no
    launch, for M == 0.  ValueError for mismatched lengths, EpreconError for CPU tensors or a coordinate out of range."""

    def __init__(self, coords, tsdf, origin, voxel_size):
        need_device(coords, tsdf)
        if coords.dim() != 2 or coords.shape[1] != 3 or tsdf.dim() != 1:
            raise ValueError(f"SceneGrid: expected coords [M,3] and tsdf [M], got {tuple(coords.shape)} and {tuple(tsdf.shape)}")
        if coords.shape[0] != tsdf.shape[0]:
            raise ValueError(f"SceneGrid: {coords.shape[0]} coordinate rows and {tsdf.shape[0]} tsdf values")
        self.coords = coords.to(torch.int32).contiguous()
        self.tsdf = tsdf.to(torch.float32).contiguous()
        self.origin = host64(origin).reshape(3)
        self.voxel_size = float(voxel_size)
        if not self.voxel_size > 0.0:
            raise ValueError(f"SceneGrid: voxel_size {voxel_size}")
        self.m = int(coords.shape[0])
        self.device = coords.device
        self.mem, self.box = None, None
        self.semantic = self.instance = None       # from_file / from_outputs leave the id rows here
        if self.m == 0:
            return
        lib = _lib.load()
        self.mem = torch.empty(int(lib.eprecon_raycast_workspace_bytes(self.m)), dtype=torch.uint8, device=self.device)
        _lib.check(lib.eprecon_raycast_build_async(_lib.ptr(self.coords), _lib.ptr(self.tsdf), self.m, _lib.ptr(self.mem),
                                                   self.mem.numel(), _lib.current_stream()), "eprecon_raycast_build_async")
        head = _lib.read_counts(self.mem[:32].view(torch.int32)[:7])
        if head[0] & 1:
            raise _lib.EpreconError("SceneGrid: a coordinate is outside the hash grid's range (|c| < 2^19 - 2)")
        if head[0]:
            raise _lib.EpreconError(f"eprecon_raycast_build_async: a table is full (status {head[0]})")
        if head[1] != _INT_MAX:
            self.box = (tuple(head[1:4]), tuple(head[4:7]))      # the smallest and the largest active cell

    active = property(lambda self: self.box is not None, doc="does any cell have a corner row with tsdf <= 0?")

    @classmethod
    def from_rows(cls, cells, tsdf, semantic, instance, origin, voxel_size, device):
        grid = cls(to_device(cells, torch.int32, device), to_device(tsdf, torch.float32, device), origin, voxel_size)
        grid.semantic, grid.instance = to_device(semantic, torch.int32, device), to_device(instance, torch.int32, device)
        return grid

    @classmethod
    def from_file(cls, npz_path, device=None):
        """<scene>.npz in any layout -> the grid of its rows in raster order (scene_io.raster_rows: the rows of a dense file
        are its cells that differ from the defaults); .semantic / .instance hold the id rows.  No dense volume is built."""
        scene = read_scene(npz_path, VOLUME_KEYS)
        cells, tsdf, sem, ins, _ = raster_rows(scene)
        return cls.from_rows(cells, tsdf, sem, ins, scene.origin, scene.voxel_size, torch.device(device if device is not None else "cuda"))

    @classmethod
    def from_outputs(cls, outputs, batch_idx, voxel_size=None):
        """outputs["scene_sparse"][batch_idx] with outputs["origin"][batch_idx] (scene_fusion.py) -> the grid of that scene;
        voxel_size: the model's MODEL.VOXEL_SIZE (default: config.ModelCfg's)"""
        if voxel_size is None:
            from .config import ModelCfg
            voxel_size = ModelCfg().VOXEL_SIZE
        rows = outputs["scene_sparse"][batch_idx]
        grid = cls(rows["coords"], rows["tsdf"], outputs["origin"][batch_idx], voxel_size)
        grid.semantic, grid.instance = rows["semantic"].to(torch.int32), rows["instance"].to(torch.int32)
        return grid


def raycast(grid, K, poses, height, width, znear=0.05, zfar=100.0, pixel_center=0.5, refine=1):
    """K [3,3] (last row 0 0 1), poses [V,4,4] camera -> world -> {"depth" f32[V,H,W], "normal" f32[V,H,W,3], "row"
    int32[V,H,W]} on the device.  `refine` further regula-falsi steps after the first interpolation.  A grid without rows or
    without an active cell gives empty images and no launch.  One host read (the status word of the walk's bounds)."""
    cams, v = _cams(K, poses, "cpu", "raycast")
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"raycast: image size {width} x {height}")
    dev = grid.device
    if not grid.active:
        return {"depth": torch.zeros((v, height, width), dtype=torch.float32, device=dev),
                "normal": torch.zeros((v, height, width, 3), dtype=torch.float32, device=dev),
                "row": torch.full((v, height, width), -1, dtype=torch.int32, device=dev)}
    lib = _lib.load()
    ext = torch.from_numpy(np.concatenate([grid.origin, [1.0 / grid.voxel_size]]))          # float64, as the block
    cams = torch.cat([cams, ext]).to(dev)
    depth = torch.empty((v, height, width), dtype=torch.float32, device=dev)
    normal = torch.empty((v, height, width, 3), dtype=torch.float32, device=dev)
    row = torch.empty((v, height, width), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.eprecon_raycast_async(
        _lib.ptr(grid.mem), grid.m, _lib.ptr(grid.tsdf), _lib.ptr(cams), v, height, width, float(pixel_center), float(znear),
        float(zfar), int(refine), _lib.ptr(depth), _lib.ptr(normal), _lib.ptr(row), _lib.ptr(status), _lib.current_stream()),
        "eprecon_raycast_async")
    bad, = _lib.read_counts(status)
    if bad:
        raise _lib.EpreconError(f"eprecon_raycast_async: a bounded walk gave up (status {bad})")
    return {"depth": depth, "normal": normal, "row": row}


def _gather(values, row, background, m):
    need_device(values)
    values = values.reshape(-1) if values.dim() == 1 else values
    if values.shape[0] != m:
        raise ValueError(f"{values.shape[0]} values for {m} rows")
    hit = row >= 0
    if m == 0:
        return hit, None
    return hit, values[row.clamp(min=0).to(torch.int64)]


def raycast_labels(grid, out, semantic, instance, backgrounds=(0, 0)):
    """per-row int arrays on the device -> (semantic, instance) int32[V,H,W]: sem[row], ins[row], `backgrounds` where
    nothing is hit"""
    images = []
    for values, bg in zip((semantic, instance), backgrounds):
        hit, picked = _gather(values.to(torch.int32), out["row"], bg, grid.m)
        image = torch.full(out["row"].shape, int(bg), dtype=torch.int32, device=out["row"].device)
        images.append(image if picked is None else torch.where(hit, picked, image))
    return tuple(images)


def pixel_rays(K, poses, height, width, pixel_center=0.5, device=None):
    """unit world-frame ray of every pixel, float64 [V,H,W,3] on `device`: R K^-1 (u + pixel_center, v + pixel_center, 1)"""
    kinv = np.linalg.inv(host64(K).reshape(3, 3)).tolist()
    rot = torch.from_numpy(np.ascontiguousarray(host64(poses).reshape(-1, 4, 4)[:, :3, :3])).to(device or "cpu")
    u = (torch.arange(width, dtype=torch.float64, device=rot.device) + float(pixel_center)).reshape(1, -1)
    v = (torch.arange(height, dtype=torch.float64, device=rot.device) + float(pixel_center)).reshape(-1, 1)
    cam = torch.stack([kinv[i][0] * u + kinv[i][1] * v + kinv[i][2] for i in range(3)], -1)             # [H,W,3]
    d = torch.einsum("vij,hwj->vhwi", rot, cam)
    return d / d.norm(dim=-1, keepdim=True)


def raycast_shaded(grid, out, K, poses, colors=None, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND, pixel_center=0.5):
    """-> uint8[V,H,W,3] on the device: render.py's flat rule, I = ambient + (1 - ambient) |n . d| with n the ray-cast normal
    and d the pixel's unit ray, channel = min(255, floor(c I + 0.5)), c = colors[row] (uint8[M,3], the reference's 0.6 grey
    without), `background_rgb` where nothing is hit.  Element-wise, in float64, composed in torch."""
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError(f"raycast_shaded: ambient {ambient}")
    row = out["row"]
    v, h, w = row.shape
    d = pixel_rays(K, poses, h, w, pixel_center, row.device)
    cosine = (out["normal"].to(torch.float64) * d).sum(-1).abs()
    intensity = float(ambient) + (1.0 - float(ambient)) * cosine
    if colors is None:
        hit, c = row >= 0, torch.full((v, h, w, 3), DEFAULT_GREY, dtype=torch.float64, device=row.device)
    else:
        hit, c = _gather(colors.to(torch.uint8).reshape(-1, 3), row, 0, grid.m)
        c = torch.zeros((v, h, w, 3), dtype=torch.float64, device=row.device) if c is None else c.to(torch.float64)
    rgb = torch.clamp(torch.floor(c * intensity.unsqueeze(-1) + 0.5), max=255.0).to(torch.uint8)
    bg = torch.tensor([int(x) for x in background_rgb], dtype=torch.uint8, device=row.device)
    return torch.where(hit.unsqueeze(-1), rgb, bg.expand(v, h, w, 3))


def normal_image(out, background_rgb=DEFAULT_BACKGROUND):
    """the normals as colours, channel = floor(127.5 (n + 1) + 0.5) -> uint8[V,H,W,3]"""
    rgb = torch.clamp(torch.floor(127.5 * (out["normal"].to(torch.float64) + 1.0) + 0.5), 0.0, 255.0).to(torch.uint8)
    bg = torch.tensor([int(x) for x in background_rgb], dtype=torch.uint8, device=rgb.device)
    return torch.where((out["row"] >= 0).unsqueeze(-1), rgb, bg.expand(rgb.shape))


def depth_millimetres(depth):
    """depth in metres -> uint16 millimetres, rounded to nearest (0 where nothing is hit, 65535 from 65.535 m on)"""
    return torch.clamp(torch.floor(depth.to(torch.float64) * 1000.0 + 0.5), 0.0, 65535.0).to(torch.int32)


def raycast_grid(grid, K, poses, height, width, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND,
                 modes=("semantic", "instance", "shaded"), **cast):
    """raycast_scene on a grid that carries its id rows (the command-line tool builds a scene's grid once and casts it in
    chunks of views).  **cast: znear, zfar, pixel_center, refine."""
    out = raycast(grid, K, poses, height, width, **cast)
    pc = cast.get("pixel_center", 0.5)
    sem, ins = raycast_labels(grid, out, grid.semantic, grid.instance)
    res = {"depth": out["depth"], "normal": out["normal"], "row": out["row"], "semantic": sem, "instance": ins}
    colors = {"semantic": lambda: palette_colors(grid.semantic), "instance": lambda: palette_colors(grid.instance), "shaded": lambda: None}
    for mode in ("semantic", "instance", "shaded"):
        if mode in modes:
            res[mode + "_rgb"] = raycast_shaded(grid, out, K, poses, colors[mode](), ambient, background_rgb, pc)
    if "normal" in modes:
        res["normal_rgb"] = normal_image(out, background_rgb)
    return res


def raycast_scene(npz_path, K, poses, height, width, ambient=DEFAULT_AMBIENT, background_rgb=DEFAULT_BACKGROUND, device=None,
                  modes=("semantic", "instance", "shaded"), **cast):
    """A saved scene from the cameras `poses` -> {depth, normal, row, semantic, instance int32[V,H,W] (the stored ids, 0
    where nothing is seen), semantic_rgb, instance_rgb (the palette colours, shaded), shaded_rgb (grey)} on the device;
    `modes` selects the rgb images.  render.render_scene's pictures without the mesh."""
    return raycast_grid(SceneGrid.from_file(npz_path, device), K, poses, height, width, ambient, background_rgb, modes, **cast)


def write_png16(path, image):
    """uint16 values [H,W] (device tensor or array of any integer type, 0 .. 65535) -> a 16-bit greyscale PNG"""
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.ndim != 2 or a.dtype.kind not in "iu" or a.size == 0 or a.min() < 0 or a.max() > 65535:
        raise ValueError(f"write_png16: expected integers 0 .. 65535 [H,W], got {a.dtype} {a.shape}")
    h, w = a.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.astype(">u2").view(np.uint8).reshape(h, 2 * w)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    return path


def camera_of_projection(proj, scale=1.0):
    """a 3x4 projection K' [R | t] (K' upper triangular without skew, K'[2,2] = 1) -> (K = K' with its first two rows times
    `scale`, pose float64[4,4] camera -> world)"""
    p = host64(proj).reshape(-1, 4)[:3]
    r3 = p[2, :3] / np.linalg.norm(p[2, :3])
    cx, cy = p[0, :3] @ r3, p[1, :3] @ r3
    r1, r2 = p[0, :3] - cx * r3, p[1, :3] - cy * r3
    fx, fy = np.linalg.norm(r1), np.linalg.norm(r2)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([r1 / fx, r2 / fy, r3])
    tz = p[2, 3] / np.linalg.norm(p[2, :3])
    w2c[:3, 3] = [(p[0, 3] - cx * tz) / fx, (p[1, 3] - cy * tz) / fy, tz]
    k = np.array([[fx * scale, 0.0, cx * scale], [0.0, fy * scale, cy * scale], [0.0, 0.0, 1.0]])
    return k, np.linalg.inv(w2c)


def preview(grid, K, pose, height, width, path):
    """the grid from one camera, shaded by instance id modulo the palette -> a PNG at `path`"""
    poses = host64(pose).reshape(1, 4, 4)
    out = raycast(grid, K, poses, height, width)
    colors = palette_colors(grid.instance) if grid.m else None
    return write_png(path, raycast_shaded(grid, out, K, poses, colors)[0])


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="depth, normal, semantic, instance and shaded views of saved scenes, ray-cast from "
                                             "their voxel rows")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--data_path", required=True, help="ScanNet-layout scenes: <scene>/pose, intrinsic")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="images go to <out>/<scene>/<mode>_<i>.png (depth: 16-bit millimetres)")
    ap.add_argument("--every", default=10, type=int, help="cast every n-th frame (default 10)")
    ap.add_argument("--size", default=list(NATIVE_SIZE), type=int, nargs=2, metavar=("W", "H"), help="image size (default 640 480)")
    ap.add_argument("--mode", default="all", choices=list(MODES) + ["all"])
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    modes = MODES if args.mode == "all" else (args.mode,)
    w, h = args.size
    written = []
    for scene in read_scene_list(args.scenes):
        ids, k, poses = scene_views(args.data_path, scene, args.every, (w, h))
        grid = SceneGrid.from_file(os.path.join(args.pred, scene + ".npz"))
        for s in range(0, len(ids), CHUNK):
            out = raycast_grid(grid, k, poses[s:s + CHUNK], h, w, modes=modes)
            for mode in modes:
                images = (depth_millimetres(out["depth"]) if mode == "depth" else out[mode + "_rgb"]).cpu().numpy()
                for j, i in enumerate(ids[s:s + CHUNK]):
                    path = os.path.join(args.out, scene, f"{mode}_{i:d}.png")
                    written.append(write_png16(path, images[j]) if mode == "depth" else write_png(path, images[j]))
        print(f"{scene}: {len(ids)} frames")
    print(f"{len(written)} images under {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Distance field of a scene: how far the nearest reconstructed surface is from every cell of a box, and which voxel row it is —
the exact squared Euclidean distance transform of the scene's surface samples with its nearest-site output, on
libeprecon_hip.so (csrc/distance_field.hip).  The reference exports no such product; the rule is this project's (DESIGN.md §5b
"distance field"):

    lattice  sample c sits at origin + c * voxel_size, as in raycast.SceneGrid
    inside   a row with tsdf <= 0; a coordinate that holds no row is outside (it reads 1, as in the ray caster); of rows that
             repeat a coordinate the first counts
    site     a row with a 6-neighbour coordinate whose inside-state differs from its own: the sites bracket every lattice edge
             that the ray-cast surface and the mesh cross
    dist2(x) the minimum over ALL sites s of the scene of the integer |x - s|^2; site(x) the smallest row index among the sites
             that attain it; with R = floor(max_distance / voxel_size) cells, a cell with dist2 > R^2 is far: dist2 = 0x7fffffff,
             site = -1
    state(x) uint8: 0 no row, 1 an outside row, 2 an inside row

    field = distance_field(grid, lo=None, hi=None, max_distance=2.0)     # a raycast.SceneGrid (its rows; not its tables) ...
    field = distance_field((coords, tsdf, origin, voxel_size))           # ... or the rows themselves, on the device
    field.dist2, field.site, field.state                                 # device [X,Y,Z] over the cells lo .. lo + (X,Y,Z)
    field.metres(signed=True)                                            # sqrt(dist2) * voxel_size, negative inside, inf far
    sem, ins = field.labels(semantic, instance)                          # sem[site], ins[site]: ids are never interpolated
    d2, row = field.at(points_world)                                     # the nearest cell's; far and -1 outside the box
    free = field.clearance(0.1, 1.8)                                     # int32[X,Y]: min dist2 over a slab above origin[2]
    write_distance(field, "scene0000_00_distance.npz"); read_distance(path)

    python -m eprecon_amd.distance_field --pred DIR --scenes FILE --out DIR [--max_distance 2.0] [--slab 0.1 1.8]

Accuracy: this is the distance to the nearest surface SAMPLE.  It is within one voxel_size of the distance to the nearest
crossed lattice edge: each site is an end of such an edge, one step long, and each such edge has a site at an end.  There is no
sub-voxel refinement.

Everything is integer arithmetic: the result is a function of the rows alone, bit-identical from run to run and however a box is
split into calls.  Device tensors are required (no CPU fallback).
"""
import argparse
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import host64, need_device, to_device
from .scene_io import VOLUME_KEYS, raster_rows, read_scene, read_scene_list

FAR = 0x7fffffff
MAX_EXTENT = 1 << 10            # per axis of the working box (csrc/distance_field.hip: keeps d2 far from overflow)
DEFAULT_MARGIN = 8              # cells around the rows in the default box when max_distance is None
KEY_LIMIT = (1 << 19) - 2       # |c| must stay below this: c - 1 .. c + 1 are looked up (csrc/hashgrid.hpp)
FILE_KEYS = ("dist2", "site", "state", "lo", "origin", "voxel_size", "radius")


class DistanceField:
    """dist2 int32, site int32, state uint8 [X,Y,Z] over the cells lo .. lo + (X,Y,Z) of the lattice origin + c * voxel_size;
    radius: the R in cells the field is exact within.  The methods are plain torch on the three volumes."""

    def __init__(self, dist2, site, state, lo, origin, voxel_size, radius):
        self.dist2, self.site, self.state = dist2, site, state
        self.lo = tuple(int(v) for v in lo)
        self.origin = host64(origin).reshape(3)
        self.voxel_size = float(voxel_size)
        self.radius = int(radius)

    shape = property(lambda self: tuple(self.dist2.shape))
    hi = property(lambda self: tuple(l + n for l, n in zip(self.lo, self.dist2.shape)))

    def metres(self, signed=True):
        """float32 [X,Y,Z]: sqrt(dist2) * voxel_size (the root in float64), inf where far; signed: negative where state == 2"""
        d = torch.sqrt(self.dist2.to(torch.float64)) * self.voxel_size
        d = torch.where(self.dist2 == FAR, torch.full_like(d, math.inf), d)
        if signed:
            d = torch.where(self.state == 2, -d, d)
        return d.to(torch.float32)

    def labels(self, semantic, instance, backgrounds=(0, 0)):
        """per-row int arrays, on the field's device -> (semantic, instance) int32 [X,Y,Z]: sem[site], ins[site], `backgrounds`
        where far"""
        near = self.site >= 0
        index = self.site.clamp(min=0).to(torch.int64)
        out = []
        for values, bg in zip((semantic, instance), backgrounds):
            values = values.to(device=self.site.device, dtype=torch.int32).reshape(-1)
            image = torch.full(self.site.shape, int(bg), dtype=torch.int32, device=self.site.device)
            out.append(image if values.numel() == 0 else torch.where(near, values[index], image))
        return tuple(out)

    def at(self, points_world):
        """points [N,3] in the world -> (dist2 int32[N], site int32[N]) of the nearest cell, floor((p - origin) / voxel_size
        + 0.5) (a point half-way between two cells takes the upper one); 0x7fffffff and -1 for a point whose cell lies outside
        the box"""
        dev = self.dist2.device
        p = to_device(points_world, torch.float64, dev).reshape(-1, 3)
        origin = torch.from_numpy(self.origin).to(dev)
        c = torch.floor((p - origin) / self.voxel_size + 0.5).to(torch.int64) - torch.tensor(self.lo, dtype=torch.int64, device=dev)
        size = torch.tensor(self.shape, dtype=torch.int64, device=dev)
        ok = ((c >= 0) & (c < size)).all(1)
        c = torch.where(ok.unsqueeze(1), c, torch.zeros_like(c))
        if self.dist2.numel() == 0:
            return (torch.full((p.shape[0],), FAR, dtype=torch.int32, device=dev), torch.full((p.shape[0],), -1, dtype=torch.int32, device=dev))
        d2, row = self.dist2[c[:, 0], c[:, 1], c[:, 2]], self.site[c[:, 0], c[:, 1], c[:, 2]]
        return torch.where(ok, d2, torch.full_like(d2, FAR)), torch.where(ok, row, torch.full_like(row, -1))

    def slab_cells(self, z_lo, z_hi):
        """the local z indices [k0, k1) of the cells whose height above origin[2] lies in [z_lo, z_hi] metres"""
        k0 = int(math.ceil(float(z_lo) / self.voxel_size - 1e-9)) - self.lo[2]
        k1 = int(math.floor(float(z_hi) / self.voxel_size + 1e-9)) + 1 - self.lo[2]
        return max(k0, 0), min(k1, self.shape[2])

    def clearance(self, z_lo, z_hi):
        """int32 [X,Y]: the minimum of dist2 over the cells of every column whose height above origin[2] lies in [z_lo, z_hi]
        metres (the free-space map of a robot of that height); 0x7fffffff where the slab is far or holds no cell"""
        k0, k1 = self.slab_cells(z_lo, z_hi)
        if k1 <= k0:
            return torch.full(self.shape[:2], FAR, dtype=torch.int32, device=self.dist2.device)
        return self.dist2[:, :, k0:k1].amin(2)


def _rows_of(grid_or_rows):
    if isinstance(grid_or_rows, (tuple, list)):
        if len(grid_or_rows) != 4:
            raise ValueError("distance_field: expected a SceneGrid or (coords, tsdf, origin, voxel_size)")
        coords, tsdf, origin, voxel_size = grid_or_rows
    else:
        coords, tsdf, origin, voxel_size = (getattr(grid_or_rows, k) for k in ("coords", "tsdf", "origin", "voxel_size"))
    need_device(coords, tsdf)
    if coords.dim() != 2 or coords.shape[1] != 3 or tsdf.dim() != 1 or coords.shape[0] != tsdf.shape[0]:
        raise ValueError(f"distance_field: expected coords [M,3] and tsdf [M], got {tuple(coords.shape)} and {tuple(tsdf.shape)}")
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"distance_field: voxel_size {voxel_size}")
    return coords.to(torch.int32).contiguous(), tsdf.to(torch.float32).contiguous(), host64(origin).reshape(3), voxel_size


def _triple(v, name):
    t = tuple(int(x) for x in (v.tolist() if hasattr(v, "tolist") else v))
    if len(t) != 3:
        raise ValueError(f"distance_field: {name} must have three components, got {v!r}")
    return t


def _all_far(lo, hi, origin, voxel_size, radius, device):
    shape = tuple(h - l for l, h in zip(lo, hi))
    return DistanceField(torch.full(shape, FAR, dtype=torch.int32, device=device), torch.full(shape, -1, dtype=torch.int32, device=device),
                         torch.zeros(shape, dtype=torch.uint8, device=device), lo, origin, voxel_size, radius)


def _guarded_extents(lo, hi, max_cells):
    ext = tuple(h - l for l, h in zip(lo, hi))
    cells = ext[0] * ext[1] * ext[2]
    if max(ext) > MAX_EXTENT or cells > int(max_cells):
        raise ValueError(f"distance_field: the working box {ext[0]} x {ext[1]} x {ext[2]} = {cells} cells exceeds max_cells = "
                         f"{int(max_cells)} cells or {MAX_EXTENT} cells per axis; give a smaller box or max_distance")
    return ext


def working_box(lo, hi, box_lo, box_hi, radius):
    """the box a call runs on: the requested cells [lo, hi) grown towards the rows' box [box_lo, box_hi) by at most `radius`
    (None: all the way).  It holds the request and every site within `radius` of one of its cells, per axis.  None when no
    row lies within `radius` of the request."""
    if radius is None:
        return tuple(min(l, b) for l, b in zip(lo, box_lo)), tuple(max(h, b) for h, b in zip(hi, box_hi))
    if any(l - radius >= bh or h + radius <= bl for l, h, bl, bh in zip(lo, hi, box_lo, box_hi)):
        return None
    return (tuple(min(l, max(l - radius, bl)) for l, bl in zip(lo, box_lo)),
            tuple(max(h, min(h + radius, bh)) for h, bh in zip(hi, box_hi)))


def distance_field(grid_or_rows, lo=None, hi=None, max_distance=None, max_cells=1 << 27, margin=DEFAULT_MARGIN):
    """-> the DistanceField of the cells [lo, hi) (lattice coordinates; default: the rows' bounding box dilated by R, or by
    `margin` cells when max_distance is None).

    Every site of the scene counts, wherever it lies: the kernel runs on the request grown towards the rows' bounding box by
    at most R (working_box) and the request is cut out of its answer; sites further than R from the request cannot change a
    kept value.  R = floor(max_distance / voxel_size) (a quotient within 1e-9 below an integer counts as that integer).
    max_distance=None: no cell is far unless the scene has no site; the working box then holds all rows and R is its diagonal
    rounded up (the largest extent alone would cut corner cells, whose dist2 reaches three times its square).

    One host read (the rows' bounding box, which also tells whether a coordinate is outside the key range; the kernel's status
    word rides on the stream's next read, _lib.defer_check); none, and no launch, without rows or when no row lies within R
    of the request.  ValueError, before any allocation, for an empty or inverted box and when the working box exceeds
    `max_cells` cells or 2^10 per axis; EpreconError for CPU tensors or a coordinate out of range."""
    coords, tsdf, origin, voxel_size = _rows_of(grid_or_rows)
    dev, m = coords.device, int(coords.shape[0])
    radius = None
    if max_distance is not None:
        if not float(max_distance) >= 0.0:
            raise ValueError(f"distance_field: max_distance {max_distance}")
        radius = int(math.floor(float(max_distance) / voxel_size + 1e-9))
    if (lo is None) != (hi is None):
        raise ValueError("distance_field: give both lo and hi, or neither")
    if lo is not None:
        lo, hi = _triple(lo, "lo"), _triple(hi, "hi")
        if any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"distance_field: empty or inverted box {lo} .. {hi}")
        _guarded_extents(lo, hi, max_cells)         # (the working box holds the request: too large a request fails before the read)
    if m == 0:
        if lo is None:
            raise ValueError("distance_field: no rows and no box")
        return _all_far(lo, hi, origin, voxel_size, radius or 0, dev)
    box = _lib.read_counts(torch.cat([coords.amin(0), coords.amax(0)]))
    box_lo, box_hi = tuple(box[:3]), tuple(v + 1 for v in box[3:])
    if min(box_lo) <= -KEY_LIMIT or max(box[3:]) >= KEY_LIMIT:
        raise _lib.EpreconError("distance_field: a coordinate is outside the hash grid's range (|c| < 2^19 - 2)")
    if lo is None:
        grow = margin if radius is None else radius
        lo, hi = tuple(v - grow for v in box_lo), tuple(v + grow for v in box_hi)
    work = working_box(lo, hi, box_lo, box_hi, radius)
    if work is None:
        return _all_far(lo, hi, origin, voxel_size, radius, dev)
    wlo, whi = work
    ext = _guarded_extents(wlo, whi, max_cells)
    if radius is None:
        radius = int(math.ceil(math.sqrt(sum(e * e for e in ext))))
    lib = _lib.load()
    c_lo, c_hi = (ctypes.c_int32 * 3)(*wlo), (ctypes.c_int32 * 3)(*whi)
    nbytes = int(lib.eprecon_distance_field_workspace_bytes(m, c_lo, c_hi))
    dist2 = torch.empty(ext, dtype=torch.int32, device=dev)
    site = torch.empty(ext, dtype=torch.int32, device=dev)
    state = torch.empty(ext, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    mem = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.eprecon_distance_field_async(_lib.ptr(coords), _lib.ptr(tsdf), m, c_lo, c_hi, radius, _lib.ptr(dist2), _lib.ptr(site),
                                                _lib.ptr(state), _lib.ptr(status), _lib.ptr(mem), nbytes, _lib.current_stream()),
               "eprecon_distance_field_async")
    _lib.defer_check(status, 0, "eprecon_distance_field_async: status (bit 0 a coordinate out of range, bit 1 a table full)")
    if (wlo, whi) != (lo, hi):
        cut = tuple(slice(l - wl, h - wl) for l, h, wl in zip(lo, hi, wlo))
        dist2, site, state = (v[cut].contiguous() for v in (dist2, site, state))
    return DistanceField(dist2, site, state, lo, origin, voxel_size, radius)


def write_distance(field, path):
    """-> <scene>_distance.npz with the keys FILE_KEYS (written through a file object: numpy appends no .npz to the name)"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        np.savez_compressed(fh, dist2=field.dist2.cpu().numpy(), site=field.site.cpu().numpy(), state=field.state.cpu().numpy(),
                            lo=np.asarray(field.lo, np.int32), origin=field.origin, voxel_size=np.float64(field.voxel_size),
                            radius=np.int32(field.radius))
    return path


def read_distance(path, device=None):
    """the file of write_distance -> a DistanceField with its volumes on `device` (None: the host)"""
    with np.load(path) as z:
        missing = [k for k in FILE_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no distance field (missing {missing})")
        vols = [torch.from_numpy(z[k]).to(device or "cpu") for k in ("dist2", "site", "state")]
        return DistanceField(*vols, z["lo"], z["origin"], float(z["voxel_size"]), int(z["radius"]))


def clearance_millimetres(clearance, voxel_size):
    """clearance (dist2 in cells) -> int32 millimetres, rounded to nearest, 65535 where far and from 65.535 m on"""
    mm = torch.floor(torch.sqrt(clearance.to(torch.float64)) * (float(voxel_size) * 1000.0) + 0.5)
    return torch.where(clearance == FAR, torch.full_like(mm, 65535.0), torch.clamp(mm, max=65535.0)).to(torch.int32)


def distance_scene(npz_path, out_dir, max_distance=None, slab=None, device=None):
    """A saved scene in any layout (scene_io.py) -> <out_dir>/<scene>_distance.npz over the default box and, with slab =
    (z_lo, z_hi) metres, <scene>_clearance.png: the clearance map [X,Y] as 16-bit millimetres.  -> (field, paths written)"""
    scene = read_scene(npz_path, VOLUME_KEYS)
    cells, tsdf, _, _, _ = raster_rows(scene)
    dev = torch.device(device if device is not None else "cuda")
    rows = (to_device(cells, torch.int32, dev), to_device(tsdf, torch.float32, dev), scene.origin, scene.voxel_size)
    if rows[0].shape[0] == 0:
        field = _all_far((0, 0, 0), tuple(max(int(d), 1) for d in scene.dims), scene.origin, scene.voxel_size, 0, dev)
    else:
        field = distance_field(rows, max_distance=max_distance)
    name = os.path.splitext(os.path.basename(npz_path))[0]
    written = [write_distance(field, os.path.join(out_dir, name + "_distance.npz"))]
    if slab is not None:
        from .raycast import write_png16
        image = clearance_millimetres(field.clearance(float(slab[0]), float(slab[1])), field.voxel_size)
        written.append(write_png16(os.path.join(out_dir, name + "_clearance.png"), image))
    return field, written


def format_report(name, field):
    near = int((field.dist2 != FAR).sum())
    return (f"{name}: {field.shape[0]} x {field.shape[1]} x {field.shape[2]} cells from {field.lo}, R = {field.radius} cells, "
            f"{near} within it")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="distance fields of saved scenes: the exact distance of every cell to the nearest "
                                             "surface sample, and which voxel row that is")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    ap.add_argument("--out", required=True, help="<scene>_distance.npz (and <scene>_clearance.png) go here")
    ap.add_argument("--max_distance", type=float, default=None, metavar="METRES", help="cells further than this are far "
                                                                                        "(default: unbounded)")
    ap.add_argument("--slab", type=float, nargs=2, default=None, metavar=("Z_LO", "Z_HI"),
                    help="also write the clearance map of this slab (metres above the scene's origin) as 16-bit millimetres")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    count = 0
    for scene in read_scene_list(args.scenes):
        field, written = distance_scene(os.path.join(args.pred, scene + ".npz"), args.out, args.max_distance, args.slab)
        count += len(written)
        print(format_report(scene, field))
    print(f"{count} files under {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

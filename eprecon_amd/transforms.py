"""The reference's sample transforms (datasets/transforms.py) with the per-sample volume work on the GPU.

    from eprecon_amd.transforms import (Compose, ToTensor, RandomTransformSpace, IntrinsicsPoseToProjection,
                                        SceneVolumes, collate_fragments)
    scene = SceneVolumes.load(tsdf_dir, "scene0000_00", panoptic=True)         # uploaded once per scene
    tf = Compose([ToTensor(), RandomTransformSpace(n_vox, voxel_size, ...), IntrinsicsPoseToProjection(9, 4)])
    sample = tf({"imgs": ..., "depth": ..., "intrinsics": ..., "extrinsics": ..., "tsdf_list_full": scene,
                 "vol_origin": ..., "scene": ..., "fragment": ..., "epoch": [epoch]})
    inputs = collate_fragments([sample, ...])                                  # what NeuConNet.forward takes

Same names, constructor arguments and dict contract as the reference.  `RandomTransformSpace` keeps the small host-side
algebra (the augmentation transform, the transformed extrinsics, the frustum bounds, `vol_origin_partial`) as the reference's
torch CPU operations, split into functions; the occupancy targets come from TSDFVolumeHIP.integrate_views and every other
target from ONE eprecon_gt_crop_async launch (csrc/gt_crop.hip).  A scene's full volumes live on the device in a
`SceneVolumes`, instead of being converted to float tensors for every sample; the reference's lists are accepted too.

`PrepareViews` stands for the reference's ResizeImage + ToTensor where the frames come decoded from disk (scannet.py): the
resize, the float conversion and the re-layout run in one launch of csrc/prepare_views.hip, bit-identical to PIL's.

`IntrinsicsPoseToProjection.world_to_aligned_camera` is a RESTATEMENT: the reference builds the rotation with transforms3d
(axis-angle -> quaternion -> matrix), which is not available to this project; synthetic.world_to_aligned_camera builds the
same rotation with Rodrigues' formula.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import synthetic as S
from .tsdf_fusion import TSDFVolumeHIP

NUM_LAYERS = 3      # datasets/transforms.py:249


class Compose:
    """A pipeline of sample transforms: every stage is called with the dict the stage before it returned."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, data):
        for stage in self.transforms:
            data = stage(data)
        return data

    def __repr__(self):
        return "Compose(" + ", ".join(repr(t) for t in self.transforms) + ")"


class SceneVolumes(object):
    """A scene's full volumes on the device, one entry per level: TSDF f32[X,Y,Z], colour f32[X,Y,Z,3], semantic and instance
    labels int32[X,Y,Z] (colour and labels are optional, all three or none).  The levels' shapes are independent."""

    def __init__(self, tsdf_list_full, rgb_list_full=None, semantic_list_full=None, instance_list_full=None, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise _lib.EpreconError("SceneVolumes needs a GPU (no CPU fallback)")
        given = [x is not None for x in (rgb_list_full, semantic_list_full, instance_list_full)]
        if any(given) and not all(given):
            raise ValueError("colour, semantic and instance volumes come together (the reference's two forms)")
        if not 1 <= len(tsdf_list_full) <= NUM_LAYERS:
            raise ValueError(f"1..{NUM_LAYERS} levels, got {len(tsdf_list_full)}")

        def up(vols, dtype):
            return None if vols is None else [torch.as_tensor(v).to(device=self.device, dtype=dtype).contiguous() for v in vols]

        self.tsdf = up(tsdf_list_full, torch.float32)
        self.rgb = up(rgb_list_full, torch.float32)
        self.semantic = up(semantic_list_full, torch.int32)
        self.instance = up(instance_list_full, torch.int32)
        self.shapes = [tuple(t.shape) for t in self.tsdf]
        for l, shape in enumerate(self.shapes):
            if len(shape) != 3:
                raise ValueError(f"level {l}: a TSDF volume is [X,Y,Z], got {shape}")
            if self.rgb is not None and (len(self.rgb) != len(self.tsdf) or tuple(self.rgb[l].shape) != shape + (3,)
                                         or tuple(self.semantic[l].shape) != shape or tuple(self.instance[l].shape) != shape):
                raise ValueError(f"level {l}: colour [X,Y,Z,3] and label [X,Y,Z] volumes must match the TSDF's {shape}")

    @property
    def panoptic(self):
        return self.rgb is not None

    def __len__(self):
        return len(self.tsdf)

    @classmethod
    def load(cls, data_path, scene, panoptic=True, n_scales=2, device=None):
        """the reference's file layout (datasets/scannet.py:65-110): <data_path>/<scene>/full_tsdf_layer{l}.npz and, for
        training, full_rgb_layer{l}.npz, full_semantic_layer_interpolate{l}.npz, full_instance_layer_interpolate{l}.npz"""
        def read(pattern):
            levels = []
            for l in range(n_scales + 1):
                with np.load(os.path.join(data_path, scene, pattern.format(l)), allow_pickle=True) as archive:
                    levels.append(archive["arr_0"])
            return levels

        tsdf = read("full_tsdf_layer{}.npz")
        if not panoptic:
            return cls(tsdf, device=device)
        return cls(tsdf, read("full_rgb_layer{}.npz"), read("full_semantic_layer_interpolate{}.npz"),
                   read("full_instance_layer_interpolate{}.npz"), device=device)


FULL_VOLUME_KEYS = ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full")


def _float_tensor(x):
    """float32 CPU tensor of an array, a list of arrays or a tensor"""
    if torch.is_tensor(x):
        return x.detach().to(device="cpu", dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))


class ToTensor:
    """numpy sample -> float32 torch tensors: images channels-first [V,3,H,W], intrinsics [V,3,3], extrinsics [V,4,4], depth
    [V,H,W] and the scene's full volumes level by level.  A SceneVolumes under 'tsdf_list_full' lives on the device already
    and passes through."""

    def __call__(self, data):
        data["imgs"] = _float_tensor(np.stack(data["imgs"])).permute(0, 3, 1, 2).contiguous()
        for key in ("intrinsics", "extrinsics"):
            data[key] = _float_tensor(data[key])
        if "depth" in data:
            data["depth"] = _float_tensor(np.stack(data["depth"]))
        if not isinstance(data.get("tsdf_list_full"), SceneVolumes):
            for key in FULL_VOLUME_KEYS:
                if key in data:
                    data[key] = [_float_tensor(v) for v in data[key]]
        return data

    def __repr__(self):
        return "ToTensor()"


def projection_matrices(intrinsics, extrinsics, stride=1):
    """f32[V,3,4,4]: for view v and level l the world->camera matrix (torch.inverse of the pose, on the host) with its rows 0..2
    multiplied from the left by the intrinsics at 1 / (stride * 2^l) of the image resolution, K[2,2] kept at 1."""
    world2cam = torch.stack([torch.inverse(pose.detach().float().cpu()) for pose in extrinsics])          # [V,4,4]
    k = torch.as_tensor(intrinsics).detach().float().cpu()
    out = world2cam.unsqueeze(1).repeat(1, NUM_LAYERS, 1, 1)
    for l in range(NUM_LAYERS):
        k_l = k / stride / 2 ** l
        k_l[:, 2, 2] = 1
        out[:, l, :3] = k_l @ world2cam[:, :3]
    return out


class IntrinsicsPoseToProjection:
    """Replaces 'intrinsics' and 'extrinsics' by 'proj_matrices' (projection_matrices) and adds 'world_to_aligned_camera',
    built from the middle view's pose."""

    def __init__(self, n_views, stride=1):
        self.nviews = n_views
        self.stride = stride

    def __call__(self, data):
        poses = data.pop("extrinsics")
        # a restatement (module docstring): synthetic's Rodrigues form, in float64 on the host
        aligned = S.world_to_aligned_camera(poses[self.nviews // 2].double().cpu().numpy())
        data["world_to_aligned_camera"] = torch.from_numpy(aligned)
        data["proj_matrices"] = projection_matrices(data.pop("intrinsics"), poses, self.stride)
        return data

    def __repr__(self):
        return f"IntrinsicsPoseToProjection(n_views={self.nviews}, stride={self.stride})"


def frame_padding(image_wh):
    """black rows above (and as many below) a frame of image_wh = (width, height) before it is resized"""
    return 2 if tuple(image_wh) == (1296, 968) else 0


def fit_intrinsics(k, image_wh, size):
    """The intrinsics `k` (3x3, for an image of image_wh = (width, height)) follow the image to `size` = (width, height), in
    place.  A 1296 x 968 ScanNet colour frame is first centred between 2 + 2 black rows, which makes it 4:3 like the target;
    the principal point moves down with it.  Returns that padding in rows (0 for every other size)."""
    w, h = image_wh
    pad = frame_padding(image_wh)
    if pad:
        h += 2 * pad
        k[1, 2] += pad
    k[0, :] /= w / size[0]
    k[1, :] /= h / size[1]
    return pad


def _resize_image_class():
    from PIL import Image

    class ResizeImage:
        """PIL images of a sample -> float32 arrays of `size` = (width, height), bilinear, with the intrinsics (given for the
        images as they come) following (fit_intrinsics, which also says when a frame is padded first)."""

        def __init__(self, size):
            self.size = tuple(size)

        def __call__(self, data):
            new_w, new_h = self.size
            for v, img in enumerate(data["imgs"]):
                k = data["intrinsics"][v]
                pad = fit_intrinsics(k, img.size, self.size)
                if pad:
                    canvas = Image.new(img.mode, (img.size[0], img.size[1] + 2 * pad))
                    canvas.paste(img, (0, pad))
                    img = canvas
                data["imgs"][v] = np.asarray(img.resize((new_w, new_h), Image.BILINEAR), dtype=np.float32)
                data["intrinsics"][v] = k
            return data

        def __repr__(self):
            return f"ResizeImage(size={self.size})"

    return ResizeImage


def __getattr__(name):
    # ResizeImage exists only where PIL imports; nothing else of the module needs PIL
    if name == "ResizeImage":
        try:
            cls = _resize_image_class()
        except ImportError as e:
            raise AttributeError(f"eprecon_amd.transforms.ResizeImage needs PIL ({e})") from None
        globals()[name] = cls
        return cls
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---------------------------------------------------------------- view preparation on the device (csrc/prepare_views.hip)
MAX_RESAMPLE_SCALE = 4      # per axis: 2 * ceil(4) + 1 = _lib.VIEWS_MAX_KSIZE taps
_RESAMPLE_BITS = 22


def resample_table(n_in, n_out):
    """int32[n_out, 2 + ksize]: per output index of one axis the first tap, the number of taps and their coefficients with
    22 fractional bits — PIL's 8-bit bilinear resampling of n_in samples to n_out (include/eprecon_hip.h states the
    arithmetic), float64 on the host.  The identity's rows are (xx, 2 | 1, 0): no special case anywhere."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"cannot resample {n_in} samples to {n_out}")
    scale = n_in / n_out
    if scale > MAX_RESAMPLE_SCALE:
        raise ValueError(f"{n_in} -> {n_out} shrinks by {scale:.3f}, more than the {MAX_RESAMPLE_SCALE} view preparation accepts")
    fs = max(scale, 1.0)
    ksize = 2 * int(np.ceil(fs)) + 1
    centre = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(centre - fs + 0.5), 0)
    taps = np.minimum(np.trunc(centre + fs + 0.5), n_in) - first
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((x + first[:, None] - centre[:, None] + 0.5) / fs))
    w[x >= taps[:, None]] = 0.0
    total = np.zeros(n_out)
    for j in range(ksize):                  # the sum in index order
        total += w[:, j]
    table = np.empty((n_out, 2 + ksize), np.int32)
    table[:, 0], table[:, 1] = first, taps
    table[:, 2:] = np.trunc(0.5 + w / total[:, None] * (1 << _RESAMPLE_BITS))
    return table


def _window_rows(table, tile):
    """the most source rows a tile of `tile` consecutive outputs reaches: what a workgroup keeps in LDS"""
    first, end = table[:, 0].astype(np.int64), table[:, 0].astype(np.int64) + table[:, 1]
    starts = np.arange(0, len(table), tile)
    return int((end[np.minimum(starts + tile, len(table)) - 1] - first[starts]).max())


_TABLES = {}


def _device_table(n_in, n_out, device):
    """(table on the device, ksize, host table), built once per (n_in, n_out, device)"""
    key = (int(n_in), int(n_out), device.type, device.index)
    hit = _TABLES.get(key)
    if hit is None:
        host = resample_table(n_in, n_out)
        hit = _TABLES[key] = (torch.from_numpy(host).to(device), host.shape[1] - 2, host)
    return hit


def prepare_views(frames, size, pad_top=0, pad_bottom=0, out=None):
    """frames: uint8[V,H,W,3] device tensor -> f32[V,3,h,w] for `size` = (w, h): every frame, standing between pad_top and
    pad_bottom black rows, resized as PIL's resize(size, BILINEAR) does it and converted to float.  One launch."""
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise _lib.EpreconError("prepare_views needs a GPU tensor (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError(f"frames are contiguous uint8[V,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
    n_views, height, width = (int(s) for s in frames.shape[:3])
    out_w, out_h = int(size[0]), int(size[1])
    table_x, ksize_x, _ = _device_table(width, out_w, frames.device)
    table_y, ksize_y, host_y = _device_table(pad_top + height + pad_bottom, out_h, frames.device)
    if out is None:
        out = torch.empty((n_views, 3, out_h, out_w), dtype=torch.float32, device=frames.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n_views, 3, out_h, out_w) or not out.is_contiguous():
        raise ValueError(f"out is contiguous f32{(n_views, 3, out_h, out_w)}")
    with torch.cuda.device(frames.device):
        _lib.check(_lib.load().eprecon_prepare_views_async(
            _lib.ptr(frames), n_views, height, width, int(pad_top), int(pad_bottom), _lib.ptr(table_x), ksize_x,
            _lib.ptr(table_y), ksize_y, _window_rows(host_y, _lib.VIEWS_TILE_H), out_h, out_w, _lib.ptr(out),
            _lib.current_stream()), "eprecon_prepare_views_async")
    return out


def depth_to_metres(depth_mm, max_depth=3.0):
    """depth_mm: 16-bit device tensor of any shape holding uint16 millimetres (torch.uint16, or the same bits as int16) ->
    f32 metres of that shape, d / 1000 and 0 beyond max_depth (datasets/scannet.py:57-63)"""
    if not (torch.is_tensor(depth_mm) and depth_mm.is_cuda):
        raise _lib.EpreconError("depth_to_metres needs a GPU tensor (no CPU fallback)")
    if depth_mm.element_size() != 2 or depth_mm.is_floating_point() or not depth_mm.is_contiguous():
        raise ValueError(f"depth is a contiguous 16-bit integer tensor, got {depth_mm.dtype}")
    out = torch.empty(depth_mm.shape, dtype=torch.float32, device=depth_mm.device)
    with torch.cuda.device(depth_mm.device):
        _lib.check(_lib.load().eprecon_depth_to_metres_async(_lib.ptr(depth_mm), depth_mm.numel(), float(max_depth),
                                                             _lib.ptr(out), _lib.current_stream()),
                   "eprecon_depth_to_metres_async")
    return out


class PrepareViews:
    """Stands where the reference has ResizeImage followed by ToTensor, with the resize, the float conversion and the
    re-layout on the device: 'imgs' (PIL images or uint8[H,W,3] arrays, as decoded) become f32[V,3,h,w] there, bit for bit
    what the two host stages make; 'intrinsics' follow by fit_intrinsics; 'depth' given as uint16 millimetres becomes f32
    metres on the device (float depth goes the host way, as in ToTensor).  The frames (and the depth) of a sample cross in
    ONE copy from a reused pinned buffer; views of different sizes are resized group by group, one launch per size."""

    def __init__(self, size=(640, 480), max_depth=3.0, device=None):
        self.size = (int(size[0]), int(size[1]))
        self.max_depth = max_depth
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise _lib.EpreconError("PrepareViews needs a GPU (no CPU fallback)")
        self._pinned = None
        self._copied = None      # event behind the last copy out of the pinned buffer

    def _stage(self, nbytes):
        """the pinned buffer as a numpy byte array of at least nbytes, free to be written (the last copy has left it)"""
        if self._copied is not None:
            self._copied.synchronize()
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._pinned.numpy()

    def __call__(self, data):
        frames = [np.asarray(img) for img in data["imgs"]]
        for f in frames:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError(f"a colour frame is uint8[H,W,3] (or an RGB PIL image), got {f.dtype} {f.shape}")
        groups = {}                       # (H, W) -> the views of that size, in order
        for v, f in enumerate(frames):
            groups.setdefault(f.shape[:2], []).append(v)
        for shape in groups:              # refuse a size before anything is copied
            for n_in, n_out in ((shape[1], self.size[0]), (shape[0] + 2 * frame_padding(shape[::-1]), self.size[1])):
                if n_in > MAX_RESAMPLE_SCALE * n_out:
                    raise ValueError(f"a {shape[1]} x {shape[0]} frame shrinks by more than {MAX_RESAMPLE_SCALE} to {self.size}")
        depth = data.get("depth")
        raw_depth = depth is not None and all(isinstance(d, np.ndarray) and d.dtype == np.uint16 for d in depth)
        if raw_depth:
            depth = np.stack(depth)
        align = lambda n: (n + 255) // 256 * 256
        offsets, total = {}, 0
        for shape, views in groups.items():
            offsets[shape] = total
            total = align(total + len(views) * shape[0] * shape[1] * 3)
        depth_offset = total
        if raw_depth:
            total += depth.nbytes
        host = self._stage(total)
        for shape, views in groups.items():
            dst = host[offsets[shape]:offsets[shape] + len(views) * shape[0] * shape[1] * 3].reshape((len(views),) + shape + (3,))
            for j, v in enumerate(views):
                dst[j] = frames[v]
        if raw_depth:
            host[depth_offset:total] = depth.reshape(-1).view(np.uint8)
        with torch.cuda.device(self.device):
            staged = torch.empty(total, dtype=torch.uint8, device=self.device)
            staged.copy_(self._pinned[:total], non_blocking=True)
            if self._copied is None:
                self._copied = torch.cuda.Event()
            self._copied.record()
            n_views, (out_w, out_h) = len(frames), self.size
            imgs = torch.empty((n_views, 3, out_h, out_w), dtype=torch.float32, device=self.device)
            for shape, views in groups.items():
                src = staged[offsets[shape]:offsets[shape] + len(views) * shape[0] * shape[1] * 3].view((len(views),) + shape + (3,))
                pads = [fit_intrinsics(data["intrinsics"][v], (shape[1], shape[0]), self.size) for v in views]
                if len(groups) == 1:
                    prepare_views(src, self.size, pads[0], pads[0], out=imgs)
                else:
                    imgs[torch.as_tensor(views, device=self.device)] = prepare_views(src, self.size, pads[0], pads[0])
            data["imgs"] = imgs
            if raw_depth:
                mm = staged[depth_offset:total].view(torch.int16).view(depth.shape)
                data["depth"] = depth_to_metres(mm, self.max_depth)
        for key in ("intrinsics", "extrinsics"):
            data[key] = _float_tensor(data[key])
        if depth is not None and not raw_depth:
            data["depth"] = _float_tensor(np.stack(depth))
        if not isinstance(data.get("tsdf_list_full"), SceneVolumes):
            for key in FULL_VOLUME_KEYS:
                if key in data:
                    data[key] = [_float_tensor(v) for v in data[key]]
        return data

    def __repr__(self):
        return f"PrepareViews(size={self.size}, max_depth={self.max_depth})"


# ---------------------------------------------------------------- host side: float32 torch CPU operations, pinned by the golden
def frustum_corners(max_depth, image_hw, intrinsics, extrinsics):
    """f32[V,5,3]: per view the camera centre and the four image corners pushed out to max_depth, in world coordinates.
    Pixel (px, py) at depth d sits at ((px - cx) d / fx, (py - cy) d / fy, d) in the camera frame."""
    h, w = int(image_hw[0]), int(image_hw[1])
    k = torch.as_tensor(intrinsics).float()
    poses = torch.as_tensor(extrinsics).float()
    px = torch.tensor([0.0, 0.0, 0.0, w, w])
    py = torch.tensor([0.0, 0.0, h, 0.0, h])
    depth = torch.tensor([0.0] + [float(max_depth)] * 4)
    x = (px - k[:, 0, 2:3]) * depth / k[:, 0, 0:1]
    y = (py - k[:, 1, 2:3]) * depth / k[:, 1, 1:2]
    cam = torch.stack([x, y, depth.expand_as(x), torch.ones_like(x)], dim=1)          # [V,4,5] homogeneous columns
    return (poses @ cam)[:, :3].transpose(1, 2)


def frustum_bounds(max_depth, image_hw, intrinsics, extrinsics):
    """f32[3,2]: per world axis the (min, max) over every view's frustum corners"""
    pts = frustum_corners(max_depth, image_hw, intrinsics, extrinsics).reshape(-1, 3)
    return torch.stack([pts.min(dim=0).values, pts.max(dim=0).values], dim=1)


def fragment_origin(bnds, vol_origin, voxel_dim, voxel_size):
    """vol_origin_partial f32[3]: where the fragment volume of voxel_dim cells starts.  In x and y it is centred on the middle
    of the frusta's bounding box, in z it starts 0.2 m below the world's origin plane; all three in cells from vol_origin and
    snapped to the coarsest level's cell (2^NUM_LAYERS fine cells: nearest in x and y, downwards in z), so that every level's
    grid starts on a whole cell."""
    snap = 2 ** NUM_LAYERS
    middle = (bnds[:, 1] + bnds[:, 0]) / 2
    middle[2] = -0.2
    cells = (middle - vol_origin) / voxel_size / snap
    cells = torch.cat([torch.round(cells[:2]), torch.floor(cells[2:])]) * snap
    cells[:2] -= torch.tensor([int(voxel_dim[0]) // 2, int(voxel_dim[1]) // 2])
    return cells * voxel_size + vol_origin


def space_transform(origin, full_shape, voxel_size, r, t, pad_low, pad_high):
    """The 4x4 augmentation: a rotation by r (radians: python float or 0-d float32 tensor) about z, then a shift.  The
    rotated scene box (origin f32[3], full_shape finest cells), grown by pad_low below and pad_high above, bounds where a box
    of the scene's own extent may start; t in [0, 1] (f32[3] or a scalar) blends between the lowest (t = 1) and the highest
    (t = 0) start, and the shift moves that start onto the scene's origin."""
    angle = np.float32(r) if not torch.is_tensor(r) else r.numpy()          # float32 cos / sin of a float32 draw
    c, s = float(np.cos(angle)), float(np.sin(angle))
    rot = torch.tensor([[c, -s], [s, c]], dtype=torch.float32)
    extent = torch.tensor([float(n) for n in full_shape]) * voxel_size
    lo, hi = origin, origin + extent
    footprint = rot @ torch.stack([torch.stack([lo[0], lo[0], hi[0], hi[0]]), torch.stack([lo[1], hi[1], lo[1], hi[1]])])
    box_lo = torch.cat([footprint.min(dim=1).values, lo[2:]])
    box_hi = torch.cat([footprint.max(dim=1).values, hi[2:]])
    first = box_lo - pad_low
    last = -extent + box_hi + pad_high
    shift = t * first + (1 - t) * last - origin
    out = torch.eye(4)
    out[:2, :2] = rot
    out[:3, 3] = -shift
    return out


# ---------------------------------------------------------------- device side
def _host3(x):
    return [float(v) for v in torch.as_tensor(x).detach().float().cpu().reshape(-1).tolist()]


def crop_ground_truth(scene, voxel_dim, voxel_size, vol_origin_partial, transform, old_origin):
    """The fragment's tsdf / rgb / semantic / instance targets at every level of `scene` (a SceneVolumes) in one launch.
    transform: the 4x4 (or its rows 0..2) that takes fragment world coordinates back to the scene's — the reference's
    T.inverse(); old_origin: the scene volumes' origin.  Returns {'tsdf_list': [...]} plus 'rgb_list', 'semantic_list' and
    'instance_list' for a panoptic scene, f32 device tensors of the reference's shapes."""
    lib = _lib.load()
    dims = [int(v) for v in voxel_dim]
    d = _lib.GtCropDesc()
    d.levels = len(scene)
    d.voxel_size = float(voxel_size)
    m = _host3(torch.as_tensor(transform)[:3, :4])
    for k in range(12):
        d.transform[k] = m[k]
    for k, (a, b, c) in enumerate(zip(dims, _host3(vol_origin_partial), _host3(old_origin))):
        d.dims[k], d.origin_partial[k], d.old_origin[k] = a, b, c
    out = {"tsdf_list": []}
    if scene.panoptic:
        out.update(rgb_list=[], semantic_list=[], instance_list=[])
    for l in range(len(scene)):
        shape = [-(-n // 2 ** l) for n in dims]
        for k in range(3):
            d.full_dims[l][k] = scene.shapes[l][k]
        d.tsdf_full[l] = _lib.ptr(scene.tsdf[l])
        out["tsdf_list"].append(torch.empty(shape, dtype=torch.float32, device=scene.device))
        d.tsdf_out[l] = _lib.ptr(out["tsdf_list"][l])
        if scene.panoptic:
            out["rgb_list"].append(torch.empty(shape + [3], dtype=torch.float32, device=scene.device))
            out["semantic_list"].append(torch.empty(shape, dtype=torch.float32, device=scene.device))
            out["instance_list"].append(torch.empty(shape, dtype=torch.float32, device=scene.device))
            d.rgb_full[l], d.rgb_out[l] = _lib.ptr(scene.rgb[l]), _lib.ptr(out["rgb_list"][l])
            d.semantic_full[l], d.semantic_out[l] = _lib.ptr(scene.semantic[l]), _lib.ptr(out["semantic_list"][l])
            d.instance_full[l], d.instance_out[l] = _lib.ptr(scene.instance[l]), _lib.ptr(out["instance_list"][l])
    with torch.cuda.device(scene.device):
        _lib.check(lib.eprecon_gt_crop_async(ctypes.addressof(d), _lib.current_stream()), "eprecon_gt_crop_async")
    return out


def fragment_occupancy(voxel_dim, voxel_size, vol_origin_partial, depth, intrinsics, extrinsics, levels=NUM_LAYERS,
                       world2cam=None, device=None):
    """occ_list: per level the depth frames integrated at voxel size voxel_size * 2^l over voxel_dim // 2^l cells, occupied
    where |tsdf| < 0.999 and at least two views saw the voxel (datasets/transforms.py:285-297).  bool device tensors."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    depth = torch.as_tensor(depth).to(device=device, dtype=torch.float32)
    occ = []
    for l in range(levels):
        vol_dim_s = torch.div(torch.tensor([int(v) for v in voxel_dim]), 2 ** l, rounding_mode='floor')
        vol = TSDFVolumeHIP(vol_dim_s, vol_origin_partial, voxel_size=voxel_size * 2 ** l, margin=3, device=device)
        vol.integrate_views(depth, intrinsics, extrinsics, obs_weight=1., world2cam=world2cam)
        occ.append(vol.occupancy())
    return occ


class RandomTransformSpace:
    """Moves a sample into an augmented world (a rotation about z and a shift, one draw per epoch) and cuts the fragment's
    ground truth out of the scene's volumes there: the poses are transformed, the targets are sampled through the inverse."""

    def __init__(self, voxel_dim, voxel_size, random_rotation=True, random_translation=True,
                 paddingXY=1.5, paddingZ=.25, origin=[0, 0, 0], max_epoch=999, max_depth=3.0, device=None):
        """voxel_dim: the fragment volume's cells (nx, ny, nz); voxel_size in metres; random_rotation / random_translation:
        which parts of the augmentation are on; paddingXY / paddingZ: how far (metres) a fragment may start outside the
        rotated scene box; origin: the fragment world's origin; max_epoch: how many epochs get a draw; max_depth: the reach of
        the view frusta; device: where the targets are made (default: the current GPU, or the SceneVolumes' own)."""
        self.voxel_dim, self.voxel_size, self.origin = voxel_dim, voxel_size, origin
        self.random_rotation, self.random_translation = random_rotation, random_translation
        self.max_depth = max_depth
        self.device = device
        # room for the crop: on every side in x and y, below the floor in z, none above the ceiling
        self.pad_low = torch.tensor([paddingXY, paddingXY, paddingZ], dtype=torch.float32)
        self.pad_high = torch.tensor([paddingXY, paddingXY, 0.0], dtype=torch.float32)
        # Two draws from torch's global generator, the angles first: after torch.manual_seed(s) they are the reference's, and
        # every sample of an epoch shares that epoch's transform.
        self.random_r = torch.rand(max_epoch)
        self.random_t = torch.rand((max_epoch, 3))

    def epoch_transform(self, origin, full_shape, epoch):
        """the 4x4 augmentation of `epoch` for a scene volume of finest dims full_shape at `origin` (f32[3]).  With the
        rotation off the angle is 0; with the translation off the crop sits half-way between its two extreme starts."""
        if not (self.random_rotation or self.random_translation):
            return torch.eye(4)
        angle = self.random_r[epoch] * 2 * np.pi if self.random_rotation else 0
        blend = self.random_t[epoch] if self.random_translation else 0.5
        return space_transform(origin, full_shape, self.voxel_size, angle, blend, self.pad_low, self.pad_high)

    def __call__(self, data):
        scene_origin = _float_tensor(data["vol_origin"])
        full = data.get("tsdf_list_full")
        full_shape = None if full is None else (full.shapes[0] if isinstance(full, SceneVolumes) else tuple(full[0].shape))
        to_fragment_world = self.epoch_transform(scene_origin, full_shape, data["epoch"][0])
        data["extrinsics"] = torch.stack([to_fragment_world @ pose for pose in data["extrinsics"]])
        data["vol_origin"] = torch.tensor(self.origin, dtype=torch.float32)
        return self.transform(data, to_fragment_world.inverse(), old_origin=scene_origin)

    def transform(self, data, transform=None, old_origin=None):
        """Adds 'vol_origin_partial' and, where the sample carries a scene, the fragment's targets under the 4x4 `transform`
        (fragment world -> scene world).  An optional data['world2cam'] (f32[V,4,4], the inverses of the transformed
        extrinsics) is handed to the integration instead of torch.inverse, for results that must not depend on the host."""
        bnds = frustum_bounds(self.max_depth, data["imgs"].shape[2:], data["intrinsics"], data["extrinsics"])
        partial = data["vol_origin_partial"] = fragment_origin(bnds, data["vol_origin"], self.voxel_dim, self.voxel_size)
        world2cam = data.pop("world2cam", None)
        data.pop("epoch")
        scene = data.pop("tsdf_list_full", None)
        lists = [data.pop(key, None) for key in FULL_VOLUME_KEYS[1:]]
        if scene is None:
            return data
        if not isinstance(scene, SceneVolumes):      # the reference's lists: uploaded for this call
            scene = SceneVolumes(scene, *lists, device=self.device)
        data["occ_list"] = fragment_occupancy(self.voxel_dim, self.voxel_size, partial, data.pop("depth"), data["intrinsics"],
                                              data["extrinsics"], len(scene), world2cam, scene.device)
        data.update(crop_ground_truth(scene, self.voxel_dim, self.voxel_size, partial, transform, old_origin))
        return data

    def __repr__(self):
        return (f"RandomTransformSpace(voxel_dim={list(self.voxel_dim)}, voxel_size={self.voxel_size}, "
                f"rotation={self.random_rotation}, translation={self.random_translation})")


def collate_fragments(samples, device=None):
    """Samples of the transform pipeline -> the batched `inputs` dict of NeuConNet.forward, on the device: tensors are stacked
    along a new batch axis (target lists level by level), everything else becomes a list.  The volume origins also stay on the
    host as 'vol_origin_host' / 'vol_origin_partial_host' (what synthetic.to_device adds: GRUFusion reads them there)."""
    if device is None:
        levels = samples[0].get('tsdf_list')
        device = levels[0].device if levels else torch.device("cuda")
    out = {}
    for key, first in samples[0].items():
        vals = [s[key] for s in samples]
        if torch.is_tensor(first):
            out[key] = torch.stack(vals).to(device)
        elif isinstance(first, (list, tuple)) and len(first) and all(torch.is_tensor(t) for t in first):
            out[key] = [torch.stack([v[l] for v in vals]).to(device) for l in range(len(first))]
        else:
            out[key] = vals
    for key in ('vol_origin', 'vol_origin_partial'):
        if key in out:
            out[key + '_host'] = torch.stack([s[key].detach().float().cpu() for s in samples])
    return out

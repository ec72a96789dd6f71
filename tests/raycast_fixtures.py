"""Scenes, cameras and cached references of the ray-cast tests (tests/test_raycast_host.py and tests/test_raycast_gpu.py share
them; nothing of the package is imported).  Cameras and surfaces are tilted off the lattice and the focal lengths are odd, so that
few pixels fall on the ties tests/raycast_ref.py leaves out."""
import functools

import numpy as np

import raycast_ref as R

VOXEL = 0.04
ORIGIN = np.array([-0.31, 0.17, 0.05])
BAND = 3.0                       # the truncation distance in cells
LEFT_OUT_CAP = 0.02
DEPTH_CEILING = NORMAL_CEILING = 1e-3      # cells / per normal component: the hard ceilings of the GPU tolerances
# the float32 twin of tests/raycast_ref.py against float64 over CASES, outside left_out (tests/test_raycast_host.py measures and
# bounds them): cells, and per normal component.  The GPU tolerances are 4 x these.
TWIN_DEPTH, TWIN_NORMAL = 3.9e-5, 3.1e-6
W, H = 61, 45


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera -> world pose: z forward, x right, y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, :3] = np.stack([x, np.cross(z, x), z], 1)
    pose[:3, 3] = eye
    return pose


def world(cell, origin=ORIGIN):
    return origin + np.asarray(cell, np.float64) * VOXEL


def intrinsics(w, h, focal=None):
    f = 0.93 * w + 0.37 if focal is None else focal
    return np.array([[f, 0.0, 0.5 * w + 0.21], [0.0, 0.97 * f, 0.5 * h - 0.13], [0.0, 0.0, 1.0]])


def _rows_of(sdf_cells, dim, labels=None):
    """tsdf = clamp(sdf / BAND, -1, 1) on the dim^3 samples; rows where |tsdf| < 1, in raster order"""
    grid = np.stack(np.meshgrid(*(np.arange(d) for d in dim), indexing="ij"), -1).reshape(-1, 3)
    tsdf = np.clip(sdf_cells(grid.astype(np.float64)) / BAND, -1.0, 1.0).astype(np.float32)
    keep = np.abs(tsdf) < 1.0
    coords = grid[keep].astype(np.int32)
    sem, ins = labels(coords.astype(np.float64)) if labels else (np.ones(len(coords), np.int32), np.ones(len(coords), np.int32))
    return {"coords": coords, "tsdf": tsdf[keep], "semantic": sem.astype(np.int32), "instance": ins.astype(np.int32),
            "origin": ORIGIN, "voxel_size": VOXEL, "dims": tuple(dim)}


SPHERE_CENTRE, SPHERE_RADIUS = np.array([11.37, 12.21, 10.83]), 8.3


@functools.lru_cache(None)
def sphere():
    def labels(c):
        octant = (c > SPHERE_CENTRE).astype(np.int64) @ [1, 2, 4]
        return 1 + octant, 10 + octant % 3
    return _rows_of(lambda c: np.linalg.norm(c - SPHERE_CENTRE, axis=1) - SPHERE_RADIUS, (24, 24, 24), labels)


@functools.lru_cache(None)
def sphere_shifted():
    """the sphere's rows 40 cells down every axis, the origin 40 cells up: the same surface in the world"""
    s = dict(sphere())
    s["coords"] = s["coords"] - 40
    s["origin"] = ORIGIN + 40 * VOXEL
    return s


SLAB_NORMAL = np.array([0.17, -0.11, 1.0]) / np.linalg.norm([0.17, -0.11, 1.0])
BOX_LO, BOX_HI = np.array([7.3, 8.6, 0.0]), np.array([15.8, 17.1, 14.4])


def _slab_sdf(c):
    return (c - np.array([12.0, 12.0, 6.4])) @ SLAB_NORMAL        # the floor: solid below a tilted plane


def _box_sdf(c):
    q = np.maximum(BOX_LO - c, c - BOX_HI)
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


@functools.lru_cache(None)
def slab_box():
    def labels(c):
        box = _box_sdf(c) < _slab_sdf(c)
        return np.where(box, 5, 1), np.where(box, 7, 2)
    return _rows_of(lambda c: np.minimum(_slab_sdf(c), _box_sdf(c)), (24, 24, 22), labels)


@functools.lru_cache(None)
def patch(n):
    """n rows with tsdf = -0.4 on the plane z = 5, x fastest in rows of 19: nothing else is a row"""
    i = np.arange(n)
    coords = np.stack([2 + i % 19, 1 + i // 19, np.full(n, 5)], 1).astype(np.int32)
    return {"coords": coords, "tsdf": np.full(n, -0.4, np.float32), "semantic": (1 + i % 3).astype(np.int32),
            "instance": (1 + i // 19).astype(np.int32), "origin": ORIGIN, "voxel_size": VOXEL, "dims": (24, 24, 8)}


PATCH_SIZES = (63, 64, 65, 255, 256, 257)
SCENES = {"sphere": sphere, "sphere_shifted": sphere_shifted, "slab_box": slab_box, **{f"patch{n}": functools.partial(patch, n) for n in PATCH_SIZES}}

_c = SPHERE_CENTRE
SPHERE_POSES = (look_at(world(_c + [-24.3, -9.7, 6.1]), world(_c + [0.4, -0.3, 0.2])),          # outside, looking in
                look_at(world(_c + [1.3, -0.8, 0.6]), world(_c + [9.0, 5.1, -2.7])),            # inside, looking out
                look_at(world(_c + [-21.0, 8.9, 2.2]), world(_c + [0.3, 8.1, 1.4])))            # grazing
SLAB_POSES = (look_at(world([-9.6, -5.2, 21.3]), world([11.2, 12.7, 7.9])),
              look_at(world([30.1, 3.3, 12.9]), world([11.9, 12.2, 8.8])))
PATCH_POSE = look_at(world([10.1, 6.2, 31.4]), world([11.3, 7.9, 5.0]), up=(0.0, 1.0, 0.0))     # from above: every row is seen

# every view the GPU tests compare with the reference: name -> (scene, K, poses, height, width)
CASES = {
    "sphere": ("sphere", intrinsics(W, H), SPHERE_POSES, H, W),
    "sphere_shifted": ("sphere_shifted", intrinsics(W, H), SPHERE_POSES[:1], H, W),
    "slab_box": ("slab_box", intrinsics(W, H, 47.9), SLAB_POSES, H, W),
    "sphere_8x8": ("sphere", intrinsics(8, 8), SPHERE_POSES[:1], 8, 8),
    "sphere_1x1": ("sphere", intrinsics(1, 1), SPHERE_POSES[:1], 1, 1),
    "sphere_64x9": ("sphere", intrinsics(64, 9), SPHERE_POSES[:1], 9, 64),
    **{f"patch{n}": (f"patch{n}", intrinsics(40, 30, 45.3), (PATCH_POSE,), 30, 40) for n in PATCH_SIZES},
}


@functools.lru_cache(None)
def rows_of(scene):
    s = SCENES[scene]()
    return R.row_dict(s["coords"], s["tsdf"])


@functools.lru_cache(None)
def reference(case, dtype=np.float64):
    """the reference's images of a case, one dict per view: computed once per process"""
    scene, k, poses, h, w = CASES[case]
    s = SCENES[scene]()
    return tuple(R.cast_view(rows_of(scene), k, pose, h, w, s["origin"], s["voxel_size"], dtype=dtype) for pose in poses)

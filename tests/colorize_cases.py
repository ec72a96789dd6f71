"""The fixtures of the vertex-colouring tests (tests/test_colorize_host.py, tests/test_colorize_gpu.py): small meshes with
cameras and seeded frames, the analytic room painted with a smooth colour function, and a scene directory on disk.  The
visibility buffers come from the caller: tests/render_ref.py's rasteriser on the CPU, render.visibility on the GPU."""
import os

import numpy as np

import colorize_ref as CR
import render_ref as RR

FRAME_H, FRAME_W = RR.H, RR.W                  # 48 x 64 frames with RR.K_SMALL (off-dyadic intrinsics)
VIS_SIZES = ((32, 24), (64, 48))               # (W, H) of the visibility buffers
BLOCK = 256                                    # threads per workgroup of the accumulate kernel


def vis_intrinsics(k, size, native):
    """K of a `native` (W, H) image at `size` (W, H): the rows scaled, as render.scaled_intrinsics does"""
    k = np.array(np.asarray(k, np.float64)[:3, :3])
    k[0] *= float(size[0]) / float(native[0])
    k[1] *= float(size[1]) / float(native[1])
    k[2] = [0.0, 0.0, 1.0]
    return k


def seeded_frames(n_views, seed=5, h=FRAME_H, w=FRAME_W):
    return np.random.default_rng(seed).integers(0, 256, (n_views, h, w, 3)).astype(np.uint8)


def _rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def patch_poses():
    """four cameras for RR.patch (which faces a camera at the origin looking along +z): the origin, a shifted one, a turned
    one, and one that looks the other way (the whole patch behind it: every wave skips that view)"""
    poses = np.stack([np.eye(4)] * 4)
    poses[1, :3, 3] = [0.21, -0.12, 0.13]
    poses[2, :3, :3], poses[2, :3, 3] = _rot_y(0.17), [-0.33, 0.07, -0.22]
    poses[3, :3, :3], poses[3, :3, 3] = _rot_y(np.pi - 0.05), [0.02, 0.01, 0.0]
    return poses


def truncated_patch(count):
    """the first `count` vertices of a patch grid with the faces that lie among them"""
    verts, faces = RR.patch(9 if count <= 81 else 17)
    assert count <= len(verts)
    return verts[:count], faces[(faces < count).all(1)]


def small_cases():
    """-> [(name, verts, faces, poses)]: RR.fixture() and patch grids of 1, 63, 64, 65 and BLOCK + 1 vertices"""
    verts, faces, poses = RR.fixture()
    cases = [("fixture", verts, faces, poses)]
    for count in (1, 63, 64, 65, BLOCK + 1):
        v, f = truncated_patch(count)
        cases.append((f"patch{count}", v, f, patch_poses()))
    return cases


def cpu_visibility(verts, faces, k, poses, height, width, pixel_center=0.5):
    """a visibility buffer u64[V,H,W] from tests/render_ref.py's float64 rasteriser"""
    if len(faces) == 0:
        return np.full((len(poses), height, width), np.uint64(0xFFFFFFFFFFFFFFFF))
    out = []
    for pose in poses:
        r = RR.render_view(verts, faces, k, pose, height, width, pixel_center=pixel_center)
        out.append(CR.pack_visibility(r["depth"], r["face"]))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------- the analytic room

SCENE_LEVEL = 2                       # 24^3 voxels of 16 cm: the smallest volume of synthetic.analytic_tsdf
SCENE_VIEWS = (0, 4, 8)
SCENE_VIS_SIZE = (40, 30)


def colour_of(points):
    """a smooth colour function of the world point -> f64[...,3] in [27.5, 227.5]"""
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    return 127.5 + 100.0 * np.stack([np.sin(1.3 * x + 0.4), np.sin(1.1 * y + 0.2 * z), np.cos(0.9 * z - 0.5 * x)], -1)


def analytic_scene():
    """one window of eprecon_amd.synthetic at 320 x 240: the room's TSDF at SCENE_LEVEL, and the window's views SCENE_VIEWS
    sphere-traced (synthetic.render_depth: pixel (r, c) looks through the image point (c, r), so pixel_center is 0) with
    every pixel painted by colour_of at the world point it sees (black where the ray leaves the room)"""
    from eprecon_amd import synthetic as S
    window = S.make_window(seed=0, width=320, height=240)
    tsdf = S.analytic_tsdf(dict(window, vol_origin_partial=window["vol_origin"]), SCENE_LEVEL)
    k = window["intrinsics"].astype(np.float64)
    h, w = window["image_hw"]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], -1)
    frames = []
    for view in SCENE_VIEWS:
        pose = window["poses"][view].astype(np.float64)
        depth = S.render_depth(window, view).astype(np.float64)
        points = pose[:3, 3] + depth[..., None] * (rays @ pose[:3, :3].T)
        frames.append(np.where(depth[..., None] > 0, np.floor(colour_of(points) + 0.5), 0.0).astype(np.uint8))
    return {"tsdf": tsdf, "origin": window["vol_origin"].astype(np.float32), "voxel": window["voxel_size"] * 2 ** SCENE_LEVEL,
            "k": k, "poses": window["poses"][list(SCENE_VIEWS)].astype(np.float64), "frames": np.stack(frames)}


def scene_error(verts, result):
    """-> (worst |channel before rounding - colour_of(vertex)| over the vertices seen, share of vertices seen)"""
    seen = result["seen"] >= 1
    err = np.abs(result["value"][seen] - colour_of(np.asarray(verts, np.float64)[seen]))
    return (float(err.max()) if seen.any() else 0.0), float(seen.mean())


# --------------------------------------------------------------------------------------------------- a scene on disk

DISK_SCENE = "scene_c"


def write_disk_scene(root):
    """RR.scene24 as a saved scene <root>/pred/<scene>.npz and its four views as a ScanNet-layout directory under
    <root>/data/<scene>: 64 x 48 colour JPEGs of a smooth pattern, pose and colour-intrinsic text files -> (pred, data)"""
    from PIL import Image
    tsdf, sem, ins, poses = RR.scene24()
    pred, frames = os.path.join(root, "pred"), os.path.join(root, "data", DISK_SCENE)
    for d in (pred, os.path.join(frames, "color"), os.path.join(frames, "pose"), os.path.join(frames, "intrinsic")):
        os.makedirs(d)
    np.savez_compressed(os.path.join(pred, DISK_SCENE + ".npz"), origin=RR.ORIGIN, voxel_size=RR.VOXEL, tsdf=tsdf, semantic=sem,
                        instance=ins)
    k4 = np.eye(4)
    k4[:3, :3] = RR.K_SMALL
    np.savetxt(os.path.join(frames, "intrinsic", "intrinsic_color.txt"), k4, delimiter=" ")
    y, x = np.mgrid[0:FRAME_H, 0:FRAME_W]
    for i, pose in enumerate(poses):
        image = np.stack([(4 * x + 20 * i) % 256, (5 * y + 9 * i) % 256, (2 * x + 3 * y) % 256], -1).astype(np.uint8)
        Image.fromarray(image).save(os.path.join(frames, "color", f"color_{i}.jpg"))
        np.savetxt(os.path.join(frames, "pose", f"pose_{i}.txt"), pose)
    return pred, os.path.join(root, "data")

"""Scene ground truth on libeprecon_hip.so: the files SceneVolumes.load and the fragment loader read, written from a ScanNet
export without PyCUDA, numba or scipy — mirror of tools/tsdf_fusion/generate_gt.py and
datasets/scannet/label_interpolate.py of the reference, with the reference's function names where one is mirrored.

    python -m eprecon_amd.generate_gt --data_path DIR --save_name NAME [--test] [--num_layers 3] [--voxel_size 0.04] ...

Per scene, under <save_path>/<scene>/ (every array stored as arr_0, dtypes and shapes as the reference writes them):
    tsdf_info.pkl                                {'vol_origin': f32[3], 'voxel_size': float}
    full_tsdf_layer{l}.npz                       f32[X,Y,Z]
    full_rgb_layer{l}.npz                        f64[X,Y,Z,3]      \
    full_semantic_layer{l}.npz                   int64[X,Y,Z]       |  with a labelled point cloud (training scenes)
    full_instance_layer{l}.npz                   int64[X,Y,Z]       |
    full_{semantic,instance}_layer_interpolate{l}.npz  int64[X,Y,Z] /
    fragments.pkl                                [{'scene', 'fragment_id', 'image_ids', 'vol_origin', 'voxel_size'}, ...]
    mesh_layer{l}.ply                            optional (marching cubes of the level's TSDF; parity unpinned)

Host bookkeeping (bounds, level dimensions, fragment windows) is float64 numpy written to give the reference's values; the
volumes come from the GPU: TSDFVolumeHIP(variant="cuda") for the TSDF, csrc/label_volume.hip for the label volumes and
their nearest-label fill.  There is no CPU fallback.
"""
import argparse
import ctypes
import os
import pickle

import numpy as np
import torch

from . import _lib
from .scene_io import count_depth_frames, depth_metres, intrinsic, pose, read_scene_list
from .tsdf_fusion import TSDFVolumeHIP

MAX_BOUND_FRAMES = 200          # generate_gt.py:126-127
MAX_LABEL = 32767
MAX_FILL_AXIS = 4096


# ------------------------------------------------------------------------------------------------------------------
# 1. host bookkeeping
# ------------------------------------------------------------------------------------------------------------------
def get_view_frustum(depth_im, cam_intr, cam_pose):
    """corners of a frame's view frustum in world coordinates, f64[3,5] (tools/tsdf_fusion/fusion.py:352-374); max_depth
    is the frame's own np.max"""
    depth_im = np.asarray(depth_im)
    cam_intr = np.asarray(cam_intr)
    im_h, im_w = depth_im.shape[0], depth_im.shape[1]
    max_depth = np.max(depth_im)
    reach = np.array([0, max_depth, max_depth, max_depth, max_depth])
    pts = np.array([(np.array([0, 0, 0, im_w, im_w]) - cam_intr[0, 2]) * reach / cam_intr[0, 0],
                    (np.array([0, 0, im_h, 0, im_h]) - cam_intr[1, 2]) * reach / cam_intr[1, 1],
                    reach])
    xyz_h = np.hstack([pts.T, np.ones((pts.shape[1], 1), dtype=np.float32)])
    return np.dot(np.asarray(cam_pose), xyz_h.T).T[:, :3].T


def valid_frames(poses):
    """indices of the frames that enter at all: a pose with +-inf in [0][0] is an untracked frame (generate_gt.py:334)"""
    return [i for i, p in enumerate(poses) if not np.isinf(np.asarray(p)[0][0]).any()]


def scene_bounds(depths, cam_intr, poses):
    """f64[3,2] (min, max) of the view frusta (generate_gt.py:123-138).  The bounds start at ZEROS, not +-inf, so the world
    origin is always inside; with more than 200 (valid) frames only the np.linspace(0, n - 1, 200).astype(int32) subset is
    looked at."""
    ids = valid_frames(poses)
    n = len(ids)
    if n > MAX_BOUND_FRAMES:
        ids = [ids[i] for i in np.linspace(0, n - 1, MAX_BOUND_FRAMES).astype(np.int32)]
    vol_bnds = np.zeros((3, 2))
    for i in ids:
        pts = get_view_frustum(depths[i], cam_intr, poses[i])
        vol_bnds[:, 0] = np.minimum(vol_bnds[:, 0], np.amin(pts, axis=1))
        vol_bnds[:, 1] = np.maximum(vol_bnds[:, 1], np.amax(pts, axis=1))
    return vol_bnds


def level_volumes(vol_bnds, voxel_size, num_layers=3, margin=3):
    """per level {'vol_dim': int[3], 'vol_origin': f32[3], 'voxel_size': float, 'sdf_trunc': float} as the reference's
    TSDFVolume(vol_bnds, voxel_size * 2**l, margin) would hold them (fusion.py:34-47).  That constructor keeps the caller's
    array and overwrites vol_bnds[:, 1] with min + dim * size, so level l + 1 derives its dimensions from level l's ADJUSTED
    upper bound, not from the frustum bound; reproduced here on a copy (the argument is left alone)."""
    bnds = np.array(vol_bnds, dtype=np.float64)
    assert bnds.shape == (3, 2)
    levels = []
    for l in range(num_layers):
        size = float(voxel_size * 2 ** l)
        dim = np.round((bnds[:, 1] - bnds[:, 0]) / size).copy(order="C").astype(int)
        bnds[:, 1] = bnds[:, 0] + dim * size
        levels.append({"vol_dim": dim, "vol_origin": bnds[:, 0].copy(order="C").astype(np.float32), "voxel_size": size,
                       "sdf_trunc": margin * size})
    return levels


def select_fragments(depths, cam_intr, poses, window_size=9, min_angle=15, min_distance=0.1, scene=None, vol_origin=None,
                     voxel_size=None):
    """the fragment windows of a scene (generate_gt.py:243-307): the first frame of a window is always taken; a later one
    when the angle between its viewing direction and that of the last TAKEN frame exceeds min_angle (degrees) or the
    translation exceeds min_distance (metres); a window closes at window_size taken frames; an unfinished window at the end
    is dropped; frames with an infinite pose never enter.  `depths` is accepted for the reference's signature (its frusta
    are computed and thrown away there).  -> the list of dicts the reference pickles."""
    z = np.array([0, 0, 1])
    all_ids, ids, count, last_pose = [], [], 0, None
    for i in valid_frames(poses):
        cam_pose = np.asarray(poses[i])
        if count == 0:
            ids.append(i)
            last_pose = cam_pose
            count += 1
            continue
        with np.errstate(invalid="ignore"):
            angle = np.arccos(((np.linalg.inv(cam_pose[:3, :3]) @ last_pose[:3, :3] @ z.T) * z).sum())
        dis = np.linalg.norm(cam_pose[:3, 3] - last_pose[:3, 3])
        if angle > (min_angle / 180) * np.pi or dis > min_distance:
            ids.append(i)
            last_pose = cam_pose
            count += 1
            if count == window_size:
                all_ids.append(ids)
                ids, count = [], 0
    return [{"scene": scene, "fragment_id": k, "image_ids": w, "vol_origin": vol_origin, "voxel_size": voxel_size}
            for k, w in enumerate(all_ids)]


# ------------------------------------------------------------------------------------------------------------------
# 2. full-scene TSDF
# ------------------------------------------------------------------------------------------------------------------
def fuse_scene_tsdf(depths, cam_intr, poses, levels, margin=3, chunk=256, device=None):
    """One TSDFVolumeHIP(dim, origin, size, margin, variant="cuda") per entry of `levels` (level_volumes), every valid
    frame integrated in order, `chunk` frames per integrate_views call so that the depth upload stays bounded (the C call
    walks them 16 per launch).  The levels are independent, so level-by-level equals the reference's frame-by-frame loop
    (generate_gt.py:153-165).  -> the list of volumes.

    The reference's PyCUDA kernel derives a voxel's coordinates from a float cast of its linear index
    (fusion.py:89-91), which loses bits above 2^24 cells; the HIP kernel uses integers.  The two agree up to 2^24 cells,
    which covers ScanNet rooms at 4 cm; beyond that the HIP result is the intended one and is unpinned."""
    ids = valid_frames(poses)
    intr = np.asarray(cam_intr, np.float32)[:3, :3]
    vols = [TSDFVolumeHIP(torch.as_tensor(np.asarray(lv["vol_dim"], np.int64)), torch.from_numpy(np.asarray(lv["vol_origin"], np.float32)),
                          lv["voxel_size"], margin=margin, device=device, variant="cuda") for lv in levels]
    for c0 in range(0, len(ids), chunk):
        part = ids[c0:c0 + chunk]
        d = torch.from_numpy(np.stack([np.asarray(depths[i], np.float32) for i in part]))
        p = torch.from_numpy(np.stack([np.asarray(poses[i], np.float32) for i in part]))
        k = torch.from_numpy(np.repeat(intr[None], len(part), 0))
        d = d.to(vols[0].device) if vols else d
        for vol in vols:
            vol.integrate_views(d, k, p)
    return vols


# ------------------------------------------------------------------------------------------------------------------
# 3. label volumes from a labelled point cloud
# ------------------------------------------------------------------------------------------------------------------
def _device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise _lib.EpreconError("eprecon_amd.generate_gt needs a GPU (no CPU fallback)")
    return dev


def _labels(x, n, what):
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).reshape(-1)
    if x.dtype.kind not in "iub" or len(x) != n:
        raise _lib.EpreconError(f"voxelize_labels: {what} labels must be {n} integers (EPRECON_ERR_ARG)")
    if x.dtype == np.uint64 and len(x) and int(x.max()) > MAX_LABEL:
        raise _lib.EpreconError(f"voxelize_labels: {what} label outside [0, {MAX_LABEL}] (EPRECON_ERR_ARG)")
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64))


def voxelize_labels(xyz, rgb, semantic, instance, vol_min, voxel_size, dims, device=None):
    """integrate_semantic (generate_gt.py:77-114) with the coordinate step of :199-202, on the GPU.
    xyz / rgb [N,3] (any float type: the reference's arithmetic promotes to float64), semantic / instance N integers in
    [0, 32767] (anything else raises EpreconError: EPRECON_ERR_ARG), vol_min the float64 LOWER FRUSTUM BOUND (not the
    float32 _vol_origin), dims (X, Y, Z).
    -> rgb_vol f64[X,Y,Z,3], semantic_vol int64[X,Y,Z], instance_vol int64[X,Y,Z] as numpy arrays:
    cell = clip(rint((xyz - vol_min) / voxel_size), 0, dim - 1), ties to even; colour = the cell's sum in ascending point
    index / max(count, 1); label = the cell's mode, ties to the smallest label (label 0 votes like any other); empty
    cells are 0 everywhere."""
    lib = _lib.load()
    dev = _device(device)
    xyz_h = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    rgb_h = np.ascontiguousarray(np.asarray(rgb, dtype=np.float64).reshape(-1, 3))
    n = len(xyz_h)
    if len(rgb_h) != n:
        raise _lib.EpreconError("voxelize_labels: xyz and rgb differ in length (EPRECON_ERR_ARG)")
    sem_d, ins_d = _labels(semantic, n, "semantic").to(dev), _labels(instance, n, "instance").to(dev)
    xyz_d, rgb_d = torch.from_numpy(xyz_h).to(dev), torch.from_numpy(rgb_h).to(dev)
    dims = [int(v) for v in dims]
    cells = int(np.prod(dims, dtype=np.int64)) if min(dims) > 0 else 0
    shape = tuple(max(v, 0) for v in dims)
    rgb_vol = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
    sem_vol = torch.empty(shape, dtype=torch.int64, device=dev)
    ins_vol = torch.empty(shape, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.eprecon_label_volumes_workspace_bytes(n, cells)), dtype=torch.uint8, device=dev)
    vmin = np.ascontiguousarray(np.asarray(vol_min, dtype=np.float64).reshape(3))
    dims_c = (ctypes.c_int32 * 3)(*dims)
    _lib.count_host_read()
    with torch.cuda.device(dev):
        _lib.check(lib.eprecon_label_volumes(
            _lib.ptr(xyz_d), _lib.ptr(rgb_d), _lib.ptr(sem_d), _lib.ptr(ins_d), n, vmin.ctypes.data_as(ctypes.c_void_p),
            float(voxel_size), ctypes.cast(dims_c, ctypes.c_void_p), _lib.ptr(rgb_vol), _lib.ptr(sem_vol), _lib.ptr(ins_vol),
            _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_label_volumes")
    return rgb_vol.cpu().numpy(), sem_vol.cpu().numpy(), ins_vol.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# 4. nearest-label fill
# ------------------------------------------------------------------------------------------------------------------
def interpolate_labels(vol, device=None):
    """label_interpolate.py:25-48 on the GPU: vol integer [X,Y,Z] -> int64[X,Y,Z] in which every cell carries the label of
    a nearest non-zero cell (a "site") by Euclidean distance in index space; non-zero cells keep their own label.

    The distance is the exact integer squared distance.  Ties are FIXED (scipy's KD-tree leaves them to its traversal):
    among the sites at the minimal distance from cell (x, y, z) the winner is the one with the smallest |dx|; among those
    the lower x; then the smallest |dy|, the lower y, the smallest |dz|, the lower z.  Two runs are bit-identical.
    A volume without a site comes back all zero (the reference raises there: NearestNDInterpolator of no points).
    Axes above 4,096 cells raise EpreconError (EPRECON_ERR_UNSUPPORTED); labels must fit int32."""
    lib = _lib.load()
    dev = _device(device)
    if torch.is_tensor(vol):
        v = vol.detach()
        if v.dtype.is_floating_point or v.dim() != 3:
            raise _lib.EpreconError("interpolate_labels: an integer [X,Y,Z] volume is needed (EPRECON_ERR_ARG)")
        v = v.to(device=dev, dtype=torch.int32).contiguous()
    else:
        a = np.asarray(vol)
        if a.dtype.kind not in "iub" or a.ndim != 3:
            raise _lib.EpreconError("interpolate_labels: an integer [X,Y,Z] volume is needed (EPRECON_ERR_ARG)")
        if a.size and (int(a.max()) > 2 ** 31 - 1 or int(a.min()) < -2 ** 31):
            raise _lib.EpreconError("interpolate_labels: labels must fit int32 (EPRECON_ERR_ARG)")
        v = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    out = torch.empty_like(v)
    _label_fill(lib, v, tuple(v.shape), out)
    return out.cpu().numpy().astype(np.int64)


def _label_fill(lib, v, dims, out, workspace=None):
    """the C call on device tensors; `dims` is passed as given (the argument checks come before any pointer is used)"""
    dims_c = (ctypes.c_int32 * 3)(*[int(d) for d in dims])
    if workspace is None:
        workspace = torch.empty(max(int(lib.eprecon_label_fill_workspace_bytes(*dims_c)), 4), dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(lib.eprecon_label_fill_async(_lib.ptr(v), ctypes.cast(dims_c, ctypes.c_void_p), _lib.ptr(out), _lib.ptr(workspace),
                                                workspace.numel(), _lib.current_stream()), "eprecon_label_fill_async")


# ------------------------------------------------------------------------------------------------------------------
# 5. driver, files, CLI
# ------------------------------------------------------------------------------------------------------------------
def _savez(path, arr):
    np.savez_compressed(path, arr)          # (positional: stored as arr_0, like the reference)


def generate_scene(scene, depths, cam_intr, poses, save_path, points=None, num_layers=3, margin=3, voxel_size=0.04,
                   window_size=9, min_angle=15, min_distance=0.1, save_mesh=False, chunk=256, device=None):
    """save_tsdf_full + label_interpolate + save_fragment_pkl for one scene (generate_gt.py:117-307, label_interpolate.py).
    depths: per frame f32[H,W] metres (0 = invalid); poses: per frame camera->world 4x4 (float64 as read from the export);
    points: None (a test scene: TSDF and fragments only) or (vertices [N,6] xyzrgb, semantic [N], instance [N]).
    -> the fragment list written to fragments.pkl."""
    out_dir = os.path.join(save_path, scene)
    os.makedirs(out_dir, exist_ok=True)
    vol_bnds = scene_bounds(depths, cam_intr, poses)
    levels = level_volumes(vol_bnds, voxel_size, num_layers, margin)
    vols = fuse_scene_tsdf(depths, cam_intr, poses, levels, margin=margin, chunk=chunk, device=device)
    tsdf_info = {"vol_origin": levels[0]["vol_origin"], "voxel_size": levels[0]["voxel_size"]}
    with open(os.path.join(out_dir, "tsdf_info.pkl"), "wb") as f:
        pickle.dump(tsdf_info, f)
    for l, vol in enumerate(vols):
        _savez(os.path.join(out_dir, f"full_tsdf_layer{l}"), vol.get_volume()[0].cpu().numpy())
    if points is not None:
        vertices, semantic, instance = points
        vertices = np.asarray(vertices)
        for l, lv in enumerate(levels):
            rgb_vol, sem_vol, ins_vol = voxelize_labels(vertices[:, :3], vertices[:, 3:6], semantic, instance, vol_bnds[:, 0],
                                                        voxel_size * 2 ** l, lv["vol_dim"], device=device)
            _savez(os.path.join(out_dir, f"full_rgb_layer{l}"), rgb_vol)
            _savez(os.path.join(out_dir, f"full_semantic_layer{l}"), sem_vol)
            _savez(os.path.join(out_dir, f"full_instance_layer{l}"), ins_vol)
            _savez(os.path.join(out_dir, f"full_instance_layer_interpolate{l}"), interpolate_labels(ins_vol, device=device))
            _savez(os.path.join(out_dir, f"full_semantic_layer_interpolate{l}"), interpolate_labels(sem_vol, device=device))
    if save_mesh:
        from .save_scene import export_ply, tsdf2mesh
        for l, (lv, vol) in enumerate(zip(levels, vols)):
            export_ply(tsdf2mesh(lv["voxel_size"], lv["vol_origin"], vol.get_volume()[0]), os.path.join(out_dir, f"mesh_layer{l}.ply"))
    fragments = select_fragments(depths, cam_intr, poses, window_size, min_angle, min_distance, scene=scene,
                                 vol_origin=tsdf_info["vol_origin"], voxel_size=tsdf_info["voxel_size"])
    with open(os.path.join(out_dir, "fragments.pkl"), "wb") as f:
        pickle.dump(fragments, f)
    return fragments


def generate_pkl(save_path, split_file, split):
    """fragments_{split}.pkl = the fragments.pkl of the scenes the split file names, in sorted scene order
    (generate_gt.py:352-374)"""
    wanted = set(read_scene_list(split_file))
    fragments = []
    for scene in sorted(os.listdir(save_path)):
        if "scene" not in scene or scene not in wanted:
            continue
        with open(os.path.join(save_path, scene, "fragments.pkl"), "rb") as f:
            fragments.extend(pickle.load(f))
    with open(os.path.join(save_path, f"fragments_{split}.pkl"), "wb") as f:
        pickle.dump(fragments, f)
    return fragments


def load_scannet_scene(data_path, scene, max_depth=3.0):
    """-> depths [f32[H,W]], cam_intr f64[3,3], poses [f64[4,4]] of an exported scene: pose/pose_{i}.txt,
    depth/depth_{i}.png, intrinsic/intrinsic_depth.txt (tools/simple_loader.py; the frame count is that of the depth maps)"""
    root = os.path.join(data_path, scene)
    n_imgs = count_depth_frames(root)
    depths = [depth_metres(os.path.join(root, "depth", f"depth_{i}.png"), max_depth) for i in range(n_imgs)]
    return depths, intrinsic(root, "depth"), [pose(root, i) for i in range(n_imgs)]


def load_panoptic_points(info_dir, scene):
    """panoptic_info/<scene>_{vert,sem_label,ins_label}.npy (generate_gt.py:193-195)"""
    return (np.load(os.path.join(info_dir, scene + "_vert.npy")), np.load(os.path.join(info_dir, scene + "_sem_label.npy")),
            np.load(os.path.join(info_dir, scene + "_ins_label.npy")))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Fuse ground truth tsdf, label volumes and fragments on the GPU")
    parser.add_argument("--data_path", metavar="DIR", default="datasets/scannet/", help="path to the exported dataset")
    parser.add_argument("--save_name", metavar="DIR", default="all_tsdf_9", help="output directory under data_path")
    # (the reference declares --test with default=True, which makes its training branch unreachable; a real switch here)
    parser.add_argument("--test", action="store_true", help="prepare the test set (scans_test, no label volumes)")
    parser.add_argument("--max_depth", default=3., type=float, help="mask out large depth values since they are noisy")
    parser.add_argument("--num_layers", default=3, type=int)
    parser.add_argument("--margin", default=3, type=int)
    parser.add_argument("--voxel_size", default=0.04, type=float)
    parser.add_argument("--window_size", default=9, type=int)
    parser.add_argument("--min_angle", default=15, type=float)
    parser.add_argument("--min_distance", default=0.1, type=float, help="m")
    parser.add_argument("--save_mesh", action="store_true", help="also write mesh_layer{l}.ply")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    save_path = os.path.join(args.data_path, args.save_name)
    scans = os.path.join(args.data_path, "scans_test" if args.test else "scans")
    for scene in sorted(os.listdir(scans)):
        if os.path.exists(os.path.join(save_path, scene, "fragments.pkl")):
            continue
        depths, cam_intr, poses = load_scannet_scene(scans, scene, args.max_depth)
        points = None if args.test else load_panoptic_points(os.path.join(args.data_path, "panoptic_info"), scene)
        generate_scene(scene, depths, cam_intr, poses, save_path, points=points, num_layers=args.num_layers, margin=args.margin,
                       voxel_size=args.voxel_size, window_size=args.window_size, min_angle=args.min_angle,
                       min_distance=args.min_distance, save_mesh=args.save_mesh)
        print(f"{scene}: {len(depths)} frames", flush=True)
    for split in (["test"] if args.test else ["train", "val"]):
        generate_pkl(save_path, os.path.join(args.data_path, f"scannetv2_{split}.txt"), split)


if __name__ == "__main__":
    main()

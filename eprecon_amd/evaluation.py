"""Scene evaluation: depth rendering, mesh trimming and F-score — the reference's tools/evaluation.py and
tools/evaluation_utils.py (pyrender + open3d there, neither available here), on libeprecon_hip.so (csrc/mesh_eval.hip):

    depth = render_depth(verts, faces, K, poses, 480, 640)            # pyrender's depth of the mesh, all views in one go
    per_frame = eval_depth(depth_pred, depth_trgt)                     # eval_depth, batched over frames
    pts = voxel_down_sample(points, 0.02)                              # open3d VoxelDownSample
    idx, dist = nn_correspondance(verts1, verts2)                      # nearest point of verts1 for every point of verts2
    m = eval_mesh(verts_pred, verts_trgt)                              # dist1 dist2 prec recal fscore
    metrics = evaluate_scene(mesh_or_path, frames, K, gt_mesh_or_path, out_dir)     # tools/evaluation.py:process

    python -m eprecon_amd.evaluation --model DIR --data_path DIR --gt_path DIR [--max_depth 10] [--scenes ...]

Device tensors are required (no CPU fallback); only the file readers (scene_io.py) and the metric assembly run on the
host.  DESIGN.md §5 lists where this deviates from pyrender / open3d.
"""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import host64, need_device, to_device
from .save_scene import marching_cubes, world_mesh
from .scene_io import count_depth_frames, depth_metres, export_ply, intrinsic, load_mesh, pose, read_ply  # noqa: F401  (read_ply: for callers)
from .tsdf_fusion import TSDFVolumeHIP

DEPTH_KEYS = ["AbsRel", "AbsDiff", "SqRel", "RMSE", "LogRMSE", "r1", "r2", "r3", "complete"]
MESH_KEYS = ["dist1", "dist2", "prec", "recal", "fscore"]
METRIC_KEYS = DEPTH_KEYS + MESH_KEYS          # tools/visualize_metrics.py key_names

VOXEL_SIZE = 0.04          # re-fusion: voxel_length 4 cm, sdf_trunc 3 voxels (tools/evaluation.py:94-99)
SDF_TRUNC_VOXELS = 3
DEPTH_TRUNC = 5.0          # create_from_color_and_depth(depth_trunc=5.0)
QUEUE_CAP = 1 << 22        # large-triangle queue of the rasteriser (overflow is walked in place: slower, same result)
_SLAB_CELLS = 1 << 24      # voxel down-sample: dense cells per pass


# ------------------------------------------------------------------------------------------------------ rasteriser

def render_depth(verts, faces, K, poses, height, width, znear=0.05, zfar=100.0, cull_back=True, pixel_center=0.5):
    """verts f32[N,3] (world), faces int32[M,3] on the device; K [3,3]; poses [V,4,4] camera -> world -> depth f32[V,H,W]
    on the device: camera-frame z of the nearest surface in [znear, zfar], 0 where nothing is hit.  Pixel (r, c) samples
    the ray through (c + pixel_center, r + pixel_center): 0.5 is pyrender's (OpenGL) convention, 0 synthetic.render_depth's.
    cull_back: only faces with ((v1-v0) x (v2-v0)) . v0_cam < 0 are drawn (pyrender culls back faces by default)."""
    need_device(verts, faces)
    lib = _lib.load()
    dev = verts.device
    verts = verts.to(torch.float32).contiguous()
    faces = faces.to(torch.int32).contiguous()
    k = host64(K).reshape(3, 3)
    if not np.array_equal(k[2], [0.0, 0.0, 1.0]):
        raise _lib.EpreconError("render_depth: K must have the last row (0, 0, 1)")
    p = host64(poses).reshape(-1, 4, 4)
    w2c = np.linalg.inv(p)[:, :3, :4].reshape(-1, 12)
    cams = torch.from_numpy(np.concatenate([k.ravel(), np.linalg.inv(k).ravel(), w2c.ravel()])).to(dev)
    v = p.shape[0]
    out = torch.empty((v, height, width), dtype=torch.float32, device=dev)
    cap = int(min(v * max(faces.shape[0], 1), QUEUE_CAP))
    ws = torch.empty(int(lib.eprecon_render_depth_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
    _lib.check(lib.eprecon_render_depth_async(
        _lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(cams), v, int(height), int(width),
        float(pixel_center), float(znear), float(zfar), int(bool(cull_back)), _lib.ptr(out), cap, _lib.ptr(ws), ws.numel(),
        _lib.current_stream()), "eprecon_render_depth_async")
    return out


# ------------------------------------------------------------------------------------------------------ depth metrics

def depth_sums(depth_pred, depth_trgt):
    """[V,H,W] device pair -> f64[V,10] per-frame sums (include/eprecon_hip.h: eprecon_depth_metrics_async), one reduction"""
    need_device(depth_pred, depth_trgt)
    lib = _lib.load()
    pred = depth_pred.to(torch.float32).contiguous()
    trgt = depth_trgt.to(device=pred.device, dtype=torch.float32).contiguous()
    if pred.dim() == 2:
        pred, trgt = pred[None], trgt[None]
    if pred.shape != trgt.shape:
        raise ValueError(f"eval_depth: shapes differ {tuple(pred.shape)} vs {tuple(trgt.shape)}")
    v, n_pix = pred.shape[0], pred[0].numel()
    out = torch.empty((v, 10), dtype=torch.float64, device=pred.device)
    ws = torch.empty(int(lib.eprecon_depth_metrics_workspace_bytes(v)), dtype=torch.uint8, device=pred.device)
    _lib.check(lib.eprecon_depth_metrics_async(_lib.ptr(pred), _lib.ptr(trgt), v, n_pix, _lib.ptr(out), _lib.ptr(ws),
                                               ws.numel(), _lib.current_stream()), "eprecon_depth_metrics_async")
    return out


def depth_metrics_from_sums(sums, n_pix):
    """f64[V,10] sums -> one dict of the nine eval_depth keys per frame; a frame without a valid pixel gives NaN
    (numpy's mean of an empty array)"""
    out = []
    for s in np.asarray(sums, np.float64).reshape(-1, 10):
        n = s[0]
        mean = (lambda x: x / n) if n > 0 else (lambda x: float("nan"))
        out.append({"AbsRel": mean(s[2]), "AbsDiff": mean(s[3]), "SqRel": mean(s[4]), "RMSE": math.sqrt(mean(s[5])),
                    "LogRMSE": math.sqrt(mean(s[6])), "r1": mean(s[7]), "r2": mean(s[8]), "r3": mean(s[9]),
                    "complete": s[1] / n_pix})
    return [{k: float(d[k]) for k in DEPTH_KEYS} for d in out]


def eval_depth(depth_pred, depth_trgt):
    """tools/evaluation_utils.py eval_depth over a batch: [V,H,W] device tensors -> a list of V dicts (one dict for a
    single [H,W] pair).  Mask pred > 0 & 0 < trgt < 10; complete = mean(pred > 0); fp64 per element and per sum."""
    sums = depth_sums(depth_pred, depth_trgt)
    res = depth_metrics_from_sums(sums.cpu().numpy(), depth_pred.shape[-1] * depth_pred.shape[-2])
    return res[0] if depth_pred.dim() == 2 else res


def average_depth_metrics(per_frame, n_frames):
    """tools/evaluation.py:123-131,150-151: the sum over the frames that were evaluated, divided by the number of frames
    of the scene (skipped frames included); a NaN frame makes the scene NaN, as there"""
    total = {k: 0.0 for k in DEPTH_KEYS}
    for m in per_frame:
        for k in DEPTH_KEYS:
            total[k] += m[k]
    if not per_frame:
        return {k: float("nan") for k in DEPTH_KEYS}
    return {k: total[k] / n_frames for k in DEPTH_KEYS}


# ------------------------------------------------------------------------------------------------------ point clouds

def point_bounds(points):
    """points f32[N,3] on the device (N >= 1) -> (min, max) float64[3] host arrays"""
    need_device(points)
    lib = _lib.load()
    out = torch.empty(6 + 256 * 6, dtype=torch.float32, device=points.device)
    _lib.check(lib.eprecon_point_bounds_async(_lib.ptr(points), points.shape[0], _lib.ptr(out), _lib.ptr(out[6:]),
                                              _lib.current_stream()), "eprecon_point_bounds_async")
    b = out[:6].cpu().numpy().astype(np.float64)
    return b[:3], b[3:]


def voxel_down_sample(points, voxel):
    """open3d PointCloud.voxel_down_sample: min_bound = points.min(0) - voxel / 2, idx = floor((p - min_bound) / voxel)
    (fp64), out = mean of each occupied voxel's points (fp32), in voxel-key (x, y, z) order.  points f32[N,3] device.
    Dense cells in x slabs of <= 2^24: the cost grows with the extent of the cloud, not only with N."""
    need_device(points)
    pts = points.to(torch.float32).contiguous()
    if pts.shape[0] == 0:
        return pts.reshape(0, 3).clone()
    lib = _lib.load()
    lo, hi = point_bounds(pts)
    voxel = float(voxel)
    mb = lo - voxel * 0.5
    dims = (np.floor((hi - mb) / voxel) + 1).astype(np.int64)
    plane = int(dims[1] * dims[2])
    slab = max(plane, min(int(np.prod(dims)), _SLAB_CELLS))
    out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device=pts.device)
    ws = torch.empty(int(lib.eprecon_voxel_down_sample_workspace_bytes(pts.shape[0], slab)), dtype=torch.uint8,
                     device=pts.device)
    n_out = ctypes.c_int64(0)
    mb_c, dims_c = (ctypes.c_double * 3)(*mb), (ctypes.c_int64 * 3)(*dims.tolist())
    _lib.check(lib.eprecon_voxel_down_sample(
        _lib.ptr(pts), pts.shape[0], ctypes.cast(mb_c, ctypes.c_void_p), voxel, ctypes.cast(dims_c, ctypes.c_void_p),
        _lib.ptr(out), ctypes.byref(n_out), slab, _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_voxel_down_sample")
    return out[:n_out.value]


def nn_grid(lo, hi, n, cells_per_point=4, max_cells=1 << 26):
    """uniform grid over the box [lo, hi] with about cells_per_point * n cells -> (cell, dims int32[3])"""
    ext = np.maximum(hi - lo, 0.0)
    target = min(max(cells_per_point * n, 1), max_cells)
    if ext.max() <= 0.0:
        return 1.0, np.ones(3, np.int32)
    cells = lambda h: float(np.prod(np.floor(ext / h) + 1))
    a, b = ext.max() / target, ext.max() * 2.0       # cells(a) >= target, cells(b) == 1
    for _ in range(60):
        m = math.sqrt(a * b)
        a, b = (m, b) if cells(m) > target else (a, m)
    return b, (np.floor(ext / b) + 1).astype(np.int32)


def nn_correspondance(verts1, verts2):
    """tools/evaluation_utils.py nn_correspondance: for each point of verts2 the nearest point of verts1 (exact, fp64
    squared distances, smallest index on ties) -> (idx int64[n2], dist f32[n2]) on the device; empty when either is"""
    need_device(verts1, verts2)
    dev = verts2.device
    v1 = verts1.to(torch.float32).contiguous()
    v2 = verts2.to(torch.float32).contiguous()
    if v1.shape[0] == 0 or v2.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    lib = _lib.load()
    lo, hi = point_bounds(v1)
    cell, dims = nn_grid(lo, hi, v1.shape[0])
    idx = torch.empty(v2.shape[0], dtype=torch.int64, device=dev)
    dist = torch.empty(v2.shape[0], dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.eprecon_nn_search_workspace_bytes(v1.shape[0], int(np.prod(dims.astype(np.int64))))),
                     dtype=torch.uint8, device=dev)
    lo_c, dims_c = (ctypes.c_double * 3)(*lo), (ctypes.c_int32 * 3)(*dims.tolist())
    _lib.check(lib.eprecon_nn_search_async(
        _lib.ptr(v1), v1.shape[0], _lib.ptr(v2), v2.shape[0], ctypes.cast(lo_c, ctypes.c_void_p), float(cell),
        ctypes.cast(dims_c, ctypes.c_void_p), _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
        "eprecon_nn_search_async")
    return idx, dist


def mesh_metrics(dist1, dist2, threshold=0.05):
    """tools/evaluation_utils.py:31-45 from the two distance arrays (host numpy): dist1[i] = distance of target point i
    to the prediction, dist2[j] = of predicted point j to the target.  Keys as the reference names them: 'dist1' is the
    mean over the PREDICTED points, 'dist2' over the target points; fscore is NaN when prec + recal == 0."""
    d1, d2 = np.asarray(dist1, np.float64), np.asarray(dist2, np.float64)
    nan = float("nan")
    prec = float(np.mean(d2 < threshold)) if len(d2) else nan
    recal = float(np.mean(d1 < threshold)) if len(d1) else nan
    den = prec + recal
    fscore = 2 * prec * recal / den if den != 0 and not math.isnan(den) else nan
    return {"dist1": float(np.mean(d2)) if len(d2) else nan, "dist2": float(np.mean(d1)) if len(d1) else nan,
            "prec": prec, "recal": recal, "fscore": fscore}


def eval_mesh(verts_pred, verts_trgt, threshold=0.05, down_sample=0.02):
    """tools/evaluation_utils.py eval_mesh on device point sets (the meshes' vertices, as open3d's read_point_cloud
    of a .ply gives them)"""
    need_device(verts_pred, verts_trgt)
    p, t = verts_pred.to(torch.float32), verts_trgt.to(device=verts_pred.device, dtype=torch.float32)
    if down_sample:
        p, t = voxel_down_sample(p, down_sample), voxel_down_sample(t, down_sample)
    _, dist1 = nn_correspondance(p, t)
    _, dist2 = nn_correspondance(t, p)
    return mesh_metrics(dist1.cpu().numpy(), dist2.cpu().numpy(), threshold)


# ------------------------------------------------------------------------------------------------------ trimmed surface

class Refusion:
    """tools/evaluation.py:94-143: the rendered depths fused into a dense TSDF (4 cm, sdf_trunc 12 cm, depth_trunc 5 m)
    over the predicted mesh's bounding box padded by sdf_trunc + one voxel; voxel centres at (k + 0.5) * voxel_size;
    extract() is the masked marching cubes (no cell with an unobserved corner)."""

    def __init__(self, verts, voxel_size=VOXEL_SIZE, device=None):
        vs = float(voxel_size)
        lo, hi = point_bounds(verts)
        pad = SDF_TRUNC_VOXELS * vs + vs
        k0, k1 = np.floor((lo - pad) / vs - 0.5), np.ceil((hi + pad) / vs - 0.5)
        self.dims = (k1 - k0 + 1).astype(np.int64)
        self.origin = ((k0 + 0.5) * vs).astype(np.float32)
        self.voxel_size = vs
        self.vol = TSDFVolumeHIP(self.dims, self.origin, vs, margin=SDF_TRUNC_VOXELS, device=device or verts.device,
                                 variant="torch")

    def integrate(self, depths, K, poses):
        d = depths.clone()
        d[d > DEPTH_TRUNC] = 0.0
        k = torch.as_tensor(np.asarray(host64(K), np.float32)).reshape(1, 3, 3).expand(d.shape[0], 3, 3)
        self.vol.integrate_views(d, k, torch.as_tensor(host64(poses), dtype=torch.float32).reshape(-1, 4, 4))

    def extract(self):
        """-> mesh dict {vertices, faces, vertex_normals} (host numpy, world metres)"""
        tsdf, weight = self.vol.get_volume()
        verts, faces, normals = marching_cubes(tsdf, 0.0, weight=weight)
        return world_mesh(self.voxel_size, self.origin, verts, faces, normals)


# ------------------------------------------------------------------------------------------------------ driver

def _chunks(frames, size):
    buf = []
    for f in frames:
        buf.append(f)
        if len(buf) == size:
            yield buf
            buf = []
    if buf:
        yield buf


def evaluate_scene(mesh_or_path, frames, K, gt_mesh_or_path, out_dir=None, scene="scene", chunk=32, device=None):
    """tools/evaluation.py:process for one scene.  frames: iterable of (pose [4,4] camera -> world, depth [H,W] metres);
    frames whose pose[0,0] is +-inf are skipped, but still count in the depth metrics' denominator.  Renders the mesh at
    every pose, scores the depths, re-fuses them, extracts the trimmed mesh and scores it against the ground truth.
    Writes <scene>_trim_single.ply and <scene>_metrics.json into out_dir (when given) -> dict of the 14 metrics."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise _lib.EpreconError("evaluate_scene needs a GPU (no CPU fallback)")
    v_np, f_np = load_mesh(mesh_or_path)
    verts, faces = to_device(v_np, torch.float32, dev), to_device(f_np, torch.int32, dev)
    k = host64(K)[:3, :3]
    fusion = Refusion(verts, device=dev) if verts.shape[0] else None
    per_frame, n_frames = [], 0
    for group in _chunks(frames, chunk):
        n_frames += len(group)
        keep = [(p, d) for p, d in group if not np.isinf(host64(p)[0, 0])]
        if not keep:
            continue
        poses = np.stack([host64(p) for p, _ in keep])
        trgt = torch.stack([to_device(d, torch.float32, dev) for _, d in keep])
        h, w = trgt.shape[-2:]
        pred = render_depth(verts, faces, k, poses, h, w)
        per_frame += eval_depth(pred, trgt)
        if fusion is not None:
            fusion.integrate(pred, k, poses)
    metrics = average_depth_metrics(per_frame, n_frames)
    trim = fusion.extract() if fusion is not None else {"vertices": np.zeros((0, 3), np.float32),
                                                        "faces": np.zeros((0, 3), np.int32),
                                                        "vertex_normals": np.zeros((0, 3), np.float32)}
    gt_v, _ = load_mesh(gt_mesh_or_path)
    metrics.update(eval_mesh(to_device(trim["vertices"], torch.float32, dev), to_device(gt_v, torch.float32, dev)))
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        name = scene.replace("/", "-")
        export_ply(trim, os.path.join(out_dir, f"{name}_trim_single.ply"))
        with open(os.path.join(out_dir, f"{name}_metrics.json"), "w") as fh:
            json.dump(metrics, fh)
    return metrics


def scannet_frames(scene_dir, max_depth=10.0):
    """(pose, depth) of every frame of a ScanNet-layout scene directory (tools/simple_loader.py): pose/pose_<i>.txt,
    depth/depth_<i>.png (16-bit millimetres), depth above max_depth zeroed; frames 0 .. (number of depth images) - 1"""
    for i in range(count_depth_frames(scene_dir)):
        yield pose(scene_dir, i), depth_metres(os.path.join(scene_dir, "depth", f"depth_{i:d}.png"), max_depth)


def visualize(fname):
    """tools/visualize_metrics.py: nanmean of every key over the scenes -> the printed table (also returned)"""
    with open(fname) as fh:
        metrics = json.load(fh)
    rows = [metrics[s] for s in sorted(metrics)]
    lines = []
    for k in METRIC_KEYS:
        vals = np.array([r[k] for r in rows if k in r], np.float64)
        with np.errstate(all="ignore"):
            v = np.nanmean(vals) if len(vals) and not np.isnan(vals).all() else float("nan")
        lines.append("%10s %0.3f" % (k, v))
    text = "\n".join(lines)
    print(text)
    return text


def main(argv=None):
    ap = argparse.ArgumentParser(description="scene evaluation (tools/evaluation.py of the reference)")
    ap.add_argument("--model", required=True, help="directory of the predicted <scene>.ply meshes; results go there")
    ap.add_argument("--data_path", required=True, help="ScanNet-layout scenes: <scene>/depth, pose, intrinsic")
    ap.add_argument("--gt_path", required=True, help="ground-truth meshes <scene>_vh_clean_2.ply")
    ap.add_argument("--max_depth", default=10.0, type=float, help="sensor depth above this is zeroed")
    ap.add_argument("--scenes", nargs="*", default=None, help="scene names (default: every directory of --data_path)")
    ap.add_argument("--chunk", default=32, type=int, help="frames per rendering / fusion launch")
    args = ap.parse_args(argv)
    scenes = args.scenes or sorted(os.listdir(args.data_path))
    results = {}
    for scene in scenes:
        sdir = os.path.join(args.data_path, scene)
        k = intrinsic(sdir, "depth")
        mesh = os.path.join(args.model, "%s.ply" % scene.replace("/", "-"))
        gt = os.path.join(args.gt_path, scene + "_vh_clean_2.ply")
        results[scene] = evaluate_scene(mesh, scannet_frames(sdir, args.max_depth), k, gt, out_dir=args.model, scene=scene,
                                        chunk=args.chunk)
    rslt = os.path.join(args.model, "metrics.json")
    with open(rslt, "w") as fh:
        json.dump(results, fh)
    visualize(rslt)
    return results


if __name__ == "__main__":
    main()

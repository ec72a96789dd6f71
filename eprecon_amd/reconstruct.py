"""Reconstruct scenes from disk — the reference's test loop (main.py:104-121, :376-405, :429-436) as a tool:

    python -m eprecon_amd.reconstruct --data_path DIR [--source_path DIR] [--mode test|val] [--ckpt FILE] --out DIR \\
           [--scenes FILE] [--n_views 9] [--size 640 480] [--host-views] [--color] [--clean N [--clean_segments N]] [--objects]
           [--simplify CELL] [--distance METRES] [--preview]

reads <data_path>/all_tsdf_<n_views>_1/fragments_<mode>.pkl (eprecon_amd.generate_gt writes it) and the frames it names
(scannet.ScanNetDataset), and walks the fragments in file order, one per step: PrepareViews -> RandomTransformSpace (no
rotation, no translation, no padding) -> IntrinsicsPoseToProjection(n_views, 4) -> NeuralRecon.forward(inputs, save_mesh,
training=False) under no_grad -> SaveScene.  A scene is written when the next one begins and after the last fragment
(scene_fusion.py); its <scene>.npz and .ply files land in <out>/scene_scannet_fusion_eval_<epoch>/, ready for
eprecon_amd.evaluation, generate_semantic_instance, panoptic_score and render.

--ckpt is a checkpoint of the reference ({'model': state_dict, 'epoch': n}, keys with or without DataParallel's
'module.'); the layers convert its layouts as they load.  Without it the weights are seeded and UNTRAINED, and the
occupancy heads are calibrated on the first fragment so that the walk reaches the finest level at all: such a run
exercises the pipeline, its meshes mean nothing.

--host-views prepares the views as the reference does (ResizeImage + ToTensor on the host) instead of PrepareViews on the
device; the two give the same tensors bit for bit.  The frames of the next fragment are read and decoded on up to 9
threads while the current fragment runs.

--color (off by default) colours every saved scene from its key frames — the image_ids of its fragments — once the scene
is written (eprecon_amd.colorize) and puts mesh_color_<scene>.ply beside the other meshes; no other file changes.

--clean N (off by default) cleans every saved scene once it is written (eprecon_amd.clean_scene: connected pieces of the
surface below N voxels are removed; with --clean_segments N, pieces of a segment below N voxels lose their ids) and puts
the cleaned <scene>.npz and its three meshes into clean/ beside the saved scene; no other file changes.

--objects (off by default) writes <scene>_objects.json beside every saved scene once it is written: one record per segment
with its voxel count, centroid, axis-aligned box and upright oriented box (eprecon_amd.scene_objects); no other file changes.

--simplify CELL (off by default) writes the three meshes of every saved scene once more, simplified by quadric vertex
clustering in cells of CELL metres (eprecon_amd.simplify), as <scene>_lod.ply, mesh_semantic_<scene>_lod.ply and
mesh_instance_<scene>_lod.ply beside them; no other file changes.

--distance METRES (off by default) writes <scene>_distance.npz beside every saved scene once it is written: for every cell
of the scene's box dilated by METRES the exact squared distance, in cells, to the nearest surface sample within METRES, that
sample's voxel row and the cell's own state (eprecon_amd.distance_field); no other file changes.

--preview (off by default) writes <out>/preview/<scene>/<fragment_id:05d>.png after every fragment: the scene so far, ray-cast
from its voxel rows (eprecon_amd.raycast) from that fragment's last key-frame camera at the network's image size, shaded by
instance id modulo the palette; no other file changes.
"""
import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import transforms as T
from .config import ModelCfg
from .save_scene import SaveScene
from .scannet import ScanNetDataset
from .scene_io import read_scene_list

MAX_READERS = 9       # one per view of a fragment; never sized from the machine


class RunCfg:
    """what SaveScene and NeuralRecon read of the reference's config node"""

    def __init__(self, out):
        self.MODEL = ModelCfg()
        self.DATASET = "scannet"
        self.LOGDIR = out
        self.SAVE_SCENE_MESH = True
        self.SAVE_INCREMENTAL = False


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="reconstruct the scenes of a fragment list from their frames on disk")
    ap.add_argument("--data_path", required=True, help="directory holding all_tsdf_<n_views>_1/ (generate_gt's output)")
    ap.add_argument("--source_path", help="directory of the <scene>/{color,depth,pose,intrinsic} frames "
                                          "(default: <data_path>/scans, or scans_test in test mode)")
    ap.add_argument("--mode", default="test", choices=["test", "val"])
    ap.add_argument("--ckpt", help="checkpoint of the reference; without it the weights are seeded and untrained")
    ap.add_argument("--out", required=True, help="where the scenes are written")
    ap.add_argument("--scenes", help="text file, one scene name per line: only these scenes")
    ap.add_argument("--n_views", default=9, type=int)
    ap.add_argument("--size", default=[640, 480], type=int, nargs=2, metavar=("W", "H"), help="image size the network sees")
    ap.add_argument("--host-views", action="store_true", help="ResizeImage + ToTensor on the host instead of PrepareViews")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--color", action="store_true", help="also write mesh_color_<scene>.ply, coloured from the scene's key frames")
    ap.add_argument("--clean", type=int, metavar="N", help="also write clean/<scene>.npz and its meshes: the scene without "
                                                            "its connected pieces of fewer than N voxels")
    ap.add_argument("--clean_segments", default=0, type=int, metavar="N", help="with --clean: pieces of a segment of fewer "
                                                                                "than N voxels lose their ids")
    ap.add_argument("--objects", action="store_true", help="also write <scene>_objects.json: count, centroid and boxes per segment")
    ap.add_argument("--simplify", type=float, metavar="CELL", help="also write the scene's meshes simplified by vertex clustering "
                                                                   "in cells of CELL metres, as *_lod.ply")
    ap.add_argument("--distance", type=float, metavar="METRES", help="also write <scene>_distance.npz: the distance of every cell "
                                                                     "to the nearest surface sample within METRES, and its row")
    ap.add_argument("--preview", action="store_true", help="also write preview/<scene>/<fragment_id>.png after every fragment: "
                    "the scene so far, ray-cast from the fragment's last key-frame camera")
    return ap.parse_args(argv)


def build_transforms(cfg, n_views, size, host_views, device):
    if host_views:
        head = [T.ResizeImage(size), T.ToTensor()]
    else:
        head = [T.PrepareViews(size, device=device)]
    return T.Compose(head + [
        T.RandomTransformSpace(cfg.MODEL.N_VOX, cfg.MODEL.VOXEL_SIZE, False, False, 0, 0, max_epoch=1, device=device),
        T.IntrinsicsPoseToProjection(n_views, 4)])


def load_checkpoint(model, path):
    """-> the checkpoint's epoch.  Every key must find its parameter and the other way round."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    sd = state.get("model", state)
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"{path}: {len(missing)} parameters without a value (first: {list(missing)[:3]}), "
                           f"{len(unexpected)} values without a parameter (first: {list(unexpected)[:3]})")
    return int(state.get("epoch", 0)) if isinstance(state, dict) else 0


def calibrate(model, inputs):
    """untrained weights: the occupancy heads rescaled on this fragment (fragment_step.calibrate_occupancy_heads)"""
    from .fragment_step import calibrate_occupancy_heads
    norm = [model.normalizer(img) for img in torch.unbind(inputs["imgs"], 1)]
    frag = (model.backbone2d.forward_views(norm), model.backbone_occ_pano.forward_views(norm), inputs)
    calibrate_occupancy_heads(model.neucon_net, [frag])


def color_saved_scenes(outputs, saver, epoch, source_path, key_frames, voxel_size):
    """--color: the scenes this step saved, coloured from the key frames of their fragments"""
    from .colorize import write_colored_scene
    save_path = "{}_fusion_eval_{}".format(saver.log_dir, epoch)
    for name in outputs.get("scene_name", []):
        npz = os.path.join(save_path, name.replace("/", "-") + ".npz")
        if os.path.exists(npz):
            path, mesh = write_colored_scene(npz, source_path, name, save_path, ids=sorted(set(key_frames.get(name, []))),
                                             tolerance=voxel_size)
            print(f"[reconstruct] {name}: {100.0 * float((mesh['vertex_seen'] > 0).mean()):.1f} % of the vertices coloured -> {path}")


def clean_saved_scenes(outputs, saver, epoch, min_voxels, min_segment_voxels):
    """--clean: the scenes this step saved, cleaned into clean/ beside them"""
    from .clean_scene import clean_scene, format_report
    save_path = "{}_fusion_eval_{}".format(saver.log_dir, epoch)
    for name in outputs.get("scene_name", []):
        scene = name.replace("/", "-")
        npz = os.path.join(save_path, scene + ".npz")
        if os.path.exists(npz):
            report = clean_scene(npz, os.path.join(save_path, "clean", scene + ".npz"), mesh=True, min_voxels=min_voxels,
                                 min_segment_voxels=min_segment_voxels)
            print(f"[reconstruct] {format_report(name, report)}")


def describe_saved_scenes(outputs, saver, epoch):
    """--objects: the inventory of the scenes this step saved, as <scene>_objects.json beside them"""
    from .scene_objects import describe_scene, format_objects
    save_path = "{}_fusion_eval_{}".format(saver.log_dir, epoch)
    for name in outputs.get("scene_name", []):
        scene = name.replace("/", "-")
        npz = os.path.join(save_path, scene + ".npz")
        if os.path.exists(npz):
            path = os.path.join(save_path, scene + "_objects.json")
            print(f"[reconstruct] {format_objects(name, describe_scene(npz, path), path)}")


def simplify_saved_scenes(outputs, saver, epoch, cell):
    """--simplify: the meshes of the scenes this step saved, simplified into *_lod.ply beside them"""
    from .simplify import format_report, simplify_scene
    save_path = "{}_fusion_eval_{}".format(saver.log_dir, epoch)
    for name in outputs.get("scene_name", []):
        npz = os.path.join(save_path, name.replace("/", "-") + ".npz")
        if os.path.exists(npz):
            print(f"[reconstruct] {format_report(name, simplify_scene(npz, save_path, cell)[0])}")


def distance_saved_scenes(outputs, saver, epoch, max_distance):
    """--distance: the distance fields of the scenes this step saved, as <scene>_distance.npz beside them"""
    from .distance_field import distance_scene, format_report
    save_path = "{}_fusion_eval_{}".format(saver.log_dir, epoch)
    for name in outputs.get("scene_name", []):
        npz = os.path.join(save_path, name.replace("/", "-") + ".npz")
        if os.path.exists(npz):
            print(f"[reconstruct] {format_report(name, distance_scene(npz, save_path, max_distance)[0])}")


def preview_fragment(model, inputs, meta, out, voxel_size, stride=4):
    """--preview: the scene map as it stands after this fragment, seen from the fragment's last key-frame camera"""
    from .raycast import SceneGrid, camera_of_projection, preview
    from .render import DEFAULT_BACKGROUND, write_png
    height, width = (int(x) for x in inputs["imgs"].shape[-2:])
    path = os.path.join(out, "preview", meta["scene"].replace("/", "-"), "{:05d}.png".format(int(meta["fragment_id"])))
    fusion = model.fuse_to_global._scene
    if fusion is None or fusion.C is None or fusion.C.shape[0] == 0 or fusion.scene_name != meta["scene"]:
        return write_png(path, np.full((height, width, 3), DEFAULT_BACKGROUND, np.uint8))
    so_far = fusion.save_mesh(None, meta["scene"])          # a dict of its own: the step's outputs are not touched
    k, pose = camera_of_projection(inputs["proj_matrices"].reshape(-1, 3, 4, 4)[-1, 0], float(stride))
    return preview(SceneGrid.from_outputs(so_far, 0, voxel_size), k, pose, height, width, path)


def main(argv=None):
    args = parse_args(argv)
    from .neuralrecon import NeuralRecon
    device = torch.device("cuda")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    cfg = RunCfg(args.out)
    size = tuple(args.size)
    dataset = ScanNetDataset(args.data_path, args.mode, build_transforms(cfg, args.n_views, size, args.host_views, device),
                             args.n_views, len(cfg.MODEL.THRESHOLDS) - 1, source_path=args.source_path,
                             raw=not args.host_views, device=device)
    if args.scenes:
        wanted = set(read_scene_list(args.scenes))
        dataset.metas = [m for m in dataset.metas if m["scene"] in wanted]
    n = len(dataset)
    if n == 0:
        raise SystemExit("no fragment to run")

    model = NeuralRecon(cfg).to(device)
    model.train()         # main.py:357: BatchNorm keeps batch statistics at test time
    epoch = 0
    if args.ckpt:
        epoch = load_checkpoint(model, args.ckpt)
    else:
        print("[reconstruct] no --ckpt: the weights are seeded and UNTRAINED (occupancy heads calibrated on the first "
              "fragment); the scenes written exercise the pipeline and mean nothing")
    saver = SaveScene(cfg)
    saver.log_dir = os.path.join(args.out, "scene_" + cfg.DATASET)
    os.makedirs(args.out, exist_ok=True)
    print(f"[reconstruct] {n} fragments, views prepared on the {'host (ResizeImage + ToTensor)' if args.host_views else 'device (PrepareViews)'}")

    def timed_read(meta, vid):
        t0 = time.perf_counter()
        return dataset.read_view(meta, vid), time.perf_counter() - t0

    def report(scene, count, seconds, read_s, prepare_s):
        print(f"[reconstruct] {scene}: {count} fragments in {seconds:.2f} s = {count / max(seconds, 1e-9):.2f} fragments/s  "
              f"(per fragment: read + decode {1e3 * read_s / count:.1f} ms summed over its reader threads, "
              f"transforms {1e3 * prepare_s / count:.1f} ms)")

    with ThreadPoolExecutor(max_workers=min(MAX_READERS, max(1, args.n_views)), thread_name_prefix="eprecon-read") as pool:
        def start(idx):
            return [pool.submit(timed_read, dataset.metas[idx], vid) for vid in dataset.metas[idx]["image_ids"]]

        pending = start(0)
        scene, count, read_s, prepare_s, t_scene = None, 0, 0.0, 0.0, time.perf_counter()
        key_frames = {}
        for idx in range(n):
            done = [f.result() for f in pending]
            pending = start(idx + 1) if idx + 1 < n else None          # the lookahead: one fragment
            meta = dataset.metas[idx]
            if scene is not None and meta["scene"] != scene:
                torch.cuda.synchronize(device)
                report(scene, count, time.perf_counter() - t_scene, read_s, prepare_s)
                count, read_s, prepare_s, t_scene = 0, 0.0, 0.0, time.perf_counter()
            scene = meta["scene"]
            read_s += sum(t for _, t in done)
            t0 = time.perf_counter()
            sample = dataset.make_item(idx, dataset.stack_views([view for view, _ in done]))
            inputs = T.collate_fragments([sample], device=device)
            prepare_s += time.perf_counter() - t0
            with torch.no_grad():
                if idx == 0 and not args.ckpt:
                    calibrate(model, inputs)
                saver.keyframe_id = idx
                outputs, _ = model(inputs, idx == n - 1, training=False)
            saver(outputs, inputs, epoch)
            if args.color:
                key_frames.setdefault(meta["scene"], []).extend(int(i) for i in meta["image_ids"])
                color_saved_scenes(outputs, saver, epoch, dataset.source_path, key_frames, float(cfg.MODEL.VOXEL_SIZE))
            if args.clean is not None:
                clean_saved_scenes(outputs, saver, epoch, args.clean, args.clean_segments)
            if args.objects:
                describe_saved_scenes(outputs, saver, epoch)
            if args.simplify is not None:
                simplify_saved_scenes(outputs, saver, epoch, args.simplify)
            if args.distance is not None:
                distance_saved_scenes(outputs, saver, epoch, args.distance)
            if args.preview:
                preview_fragment(model, inputs, meta, args.out, float(cfg.MODEL.VOXEL_SIZE))
            count += 1
        torch.cuda.synchronize(device)
        report(scene, count, time.perf_counter() - t_scene, read_s, prepare_s)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Writes tests/golden/generate_gt.npz from the reference's own scene ground-truth programs, run in place under ref_shim on the
seeded inputs of tests/generate_gt_ref.py.  Build container only.

    python tests/golden/make_generate_gt_golden.py

Recorded (outputs only; the inputs come from the seeds):
    frustum/<k>                    get_view_frustum of a few frames                     tools/tsdf_fusion/fusion.py:360-374
    bounds/<case>                  vol_bnds as save_tsdf_full hands them to TSDFVolume  tools/tsdf_fusion/generate_gt.py:123-138
    fragments/ids, /lens           image_ids of save_fragment_pkl's fragments.pkl       :243-307
    labels/<case>/{rgb,sem,ins}    integrate_semantic on the cells of :199-202          :77-114
    fill/<case>                    label_interpolate.main()'s *_interpolate files       datasets/scannet/label_interpolate.py
TSDFVolume itself needs PyCUDA: save_tsdf_full is stopped at its first TSDFVolume(...) call, whose argument is the bounds
array.  `ray` and `pycuda` get stand-ins of this file's own in sys.modules; ref_shim.py supplies the rest.
Every case is checked for what it is meant to exercise; the file is not written otherwise.
"""
import argparse
import importlib.util
import os
import pickle
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shim  # noqa: E402

ref_shim.install()
for name in ("ray", "pycuda", "pycuda.driver", "pycuda.autoinit", "pycuda.compiler"):
    sys.modules.setdefault(name, MagicMock())
sys.argv = [sys.argv[0]]                                   # generate_gt.py parses the command line when it is imported
import generate_gt_ref as R  # noqa: E402
from tools.tsdf_fusion import generate_gt as G  # noqa: E402


class _Stop(Exception):
    pass


def ref_args(save_path):
    return argparse.Namespace(save_path=save_path, num_layers=R.NUM_LAYERS, voxel_size=R.VOXEL_SIZE, margin=3, test=True,
                              data_path=save_path, **R.FRAGMENT_ARGS)


def frame_dicts(depths, poses):
    """what process_with_single_worker collects (:330-337): frames with an infinite pose never enter"""
    depth_all, pose_all = {}, {}
    for i, (d, p) in enumerate(zip(depths, poses)):
        if p[0][0] == np.inf or p[0][0] == -np.inf:
            continue
        depth_all[i], pose_all[i] = d, p
    return depth_all, pose_all


def ref_bounds(depths, intr, poses):
    seen = {}

    def stop(vol_bnds, voxel_size, margin):
        seen["bnds"] = np.array(vol_bnds)
        raise _Stop

    real, G.TSDFVolume = G.TSDFVolume, stop
    try:
        depth_all, pose_all = frame_dicts(depths, poses)
        G.save_tsdf_full(ref_args("/nonexistent"), "scene", intr, depth_all, pose_all, {}, save_mesh=False)
    except _Stop:
        pass
    finally:
        G.TSDFVolume = real
    return seen["bnds"]


def gen_bounds(out):
    for name in R.BOUNDS_CASES:
        depths, intr, poses = R.bounds_case(name)
        bnds = ref_bounds(depths, intr, poses)
        out[f"bounds/{name}"] = bnds
        dims = [d for d, _ in R.level_dims_f64(bnds, R.VOXEL_SIZE, R.NUM_LAYERS)]
        print(name, "bounds", bnds.tolist(), "dims", [d.tolist() for d in dims])
        if name == "many_frames":       # the subsample matters: all frames give other bounds (and other dimensions)
            depth_all, pose_all = frame_dicts(depths, poses)
            assert len(depth_all) > 200
            full = np.zeros((3, 2))
            for i in depth_all:
                pts = G.get_view_frustum(depth_all[i], intr, pose_all[i])
                full[:, 0] = np.minimum(full[:, 0], pts.min(1))
                full[:, 1] = np.maximum(full[:, 1], pts.max(1))
            assert not np.array_equal(R.naive_dims(full, R.VOXEL_SIZE, 0), dims[0]), "the 200-frame subset changes nothing"
        if name == "few_frames":        # the in-place adjustment matters
            assert not np.array_equal(R.naive_dims(bnds, R.VOXEL_SIZE, 1), dims[1]), "level 1 equals the unadjusted rule"
    depths, intr, poses = R.bounds_case("few_frames")
    for k in range(3):
        out[f"frustum/{k}"] = G.get_view_frustum(depths[k], intr, poses[k])


def gen_fragments(out):
    depths, intr, poses, script = R.fragment_case()
    fa = R.FRAGMENT_ARGS
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "scene0000_00"))
        info = {"vol_origin": np.array([-1.0, 0.5, 0.25], np.float32), "voxel_size": 0.04}
        with open(os.path.join(tmp, "scene0000_00", "tsdf_info.pkl"), "wb") as f:
            pickle.dump(info, f)
        depth_all, pose_all = frame_dicts(depths, poses)
        G.save_fragment_pkl(ref_args(tmp), "scene0000_00", intr, depth_all, pose_all)
        with open(os.path.join(tmp, "scene0000_00", "fragments.pkl"), "rb") as f:
            frags = pickle.load(f)
    ids = [fr["image_ids"] for fr in frags]
    assert [fr["fragment_id"] for fr in frags] == list(range(len(frags))) and all(fr["scene"] == "scene0000_00" for fr in frags)
    print("fragments", ids)
    # what the walk is meant to contain, judged by the reference's own two measures against the last taken frame
    taken = {i for w in ids for i in w}
    seen, last, count = set(), None, 0
    for i, kind in enumerate(script):
        if kind == "inf":
            assert np.isinf(poses[i][0][0]) and i not in taken
            seen.add("inf")
            continue
        if count == 0:
            last, count = poses[i], 1
            continue
        angle = np.arccos(((np.linalg.inv(poses[i][:3, :3]) @ last[:3, :3] @ np.array([0, 0, 1]).T) * np.array([0, 0, 1])).sum())
        dis = np.linalg.norm(poses[i][:3, 3] - last[:3, 3])
        by_angle, by_dis = angle > fa["min_angle"] / 180 * np.pi, dis > fa["min_distance"]
        seen.add("angle only" if by_angle and not by_dis else "distance only" if by_dis and not by_angle else
                 "both" if by_angle else "rejected")
        if by_angle or by_dis:
            last, count = poses[i], (count + 1) % fa["window_size"]
    assert {"inf", "angle only", "distance only", "rejected"} <= seen, seen
    assert count != 0 and max(taken) < len(script) - 1, "no trailing unfinished window"
    assert len(ids) >= 2
    out["fragments/ids"] = np.array([i for w in ids for i in w], np.int64)
    out["fragments/lens"] = np.array([len(w) for w in ids], np.int64)


def check_label_case(name, xyz, sem, ins, vol_min, vs, dims, sem_vol):
    raw = np.round((xyz - vol_min[None]) / vs).astype(int)
    cells = R.cell_of(xyz, vol_min, vs, dims)
    flat = np.ravel_multi_index(cells.T, dims)
    counts = np.bincount(flat, minlength=int(np.prod(dims)))
    print(name, "points", len(xyz), "cells", int(np.prod(dims)), "max per cell", counts.max(), "empty", int((counts == 0).sum()))
    if name != "main":
        assert dims[1] == 1
        return
    at = lambda c: counts[np.ravel_multi_index(c, dims)]
    assert at(R.CELL_EMPTY) == 0 and at(R.CELL_ONE) == 1 and 64 < at(R.CELL_64) <= 256 and at(R.CELL_256) > 256
    for k in range(3):
        assert (raw[:, k] < 0).any() and (raw[:, k] > dims[k] - 1).any(), f"no point beyond a face of axis {k}"
    frac = (xyz[:, 0] - vol_min[0]) / vs
    on_half = frac - np.floor(frac) == 0.5
    assert on_half.sum() >= 2 and len({int(np.floor(f)) % 2 for f in frac[on_half]}) == 2, "half-way coordinates, both parities"
    assert ins.max() > 255
    # ties: the two top counts of the cell are equal (and one of the tied labels is 0 in CELL_TIE0)
    for cell, with_zero in ((R.CELL_TIE, False), (R.CELL_TIE0, True)):
        labs, cnt = np.unique(sem[flat == np.ravel_multi_index(cell, dims)], return_counts=True)
        top = labs[cnt == cnt.max()]
        assert len(top) >= 2 and (not with_zero or 0 in top), (cell, labs, cnt)
        assert sem_vol[cell] == top.min()


def gen_labels(out):
    for name in R.LABEL_CASES:
        xyz, rgb, sem, ins, vol_min, vs, dims = R.label_case(name)
        # generate_gt.py:199-202, restated (the lines sit inside save_tsdf_full, behind the PyCUDA volume)
        coords = np.round((xyz - np.tile(vol_min, (xyz.shape[0], 1))) / vs).astype(int)
        for k in range(3):
            coords[:, k] = np.clip(coords[:, k], 0, dims[k] - 1)
        rgb_vol, sem_vol, ins_vol = G.integrate_semantic(coords, rgb, sem.reshape(-1, 1), ins.reshape(-1, 1), tuple(dims))
        assert rgb_vol.dtype == np.float64 and sem_vol.dtype == np.int64 and ins_vol.dtype == np.int64
        check_label_case(name, xyz, sem, ins, vol_min, vs, dims, sem_vol)
        out[f"labels/{name}/rgb"] = rgb_vol
        out[f"labels/{name}/sem"] = sem_vol.astype(np.int16)
        out[f"labels/{name}/ins"] = ins_vol.astype(np.int16)


def gen_fill(out):
    spec = importlib.util.spec_from_file_location("ref_label_interpolate", os.path.join(ref_shim.REF, "datasets", "scannet",
                                                                                        "label_interpolate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    names = list(R.FILL_CASES)
    assert len(names) == 3                                  # main() reads layers 0, 1, 2 of a scene folder
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "datasets", "scannet", "all_tsdf_9", "scene0000_00")
        os.makedirs(folder)
        for l, name in enumerate(names):
            vol = R.fill_case(name)
            np.savez_compressed(os.path.join(folder, f"full_instance_layer{l}"), vol)
            np.savez_compressed(os.path.join(folder, f"full_semantic_layer{l}"), vol[::-1].copy())
        os.chdir(tmp)
        try:
            mod.main()
        finally:
            os.chdir(cwd)
        for l, name in enumerate(names):
            vol = R.fill_case(name)
            got = np.load(os.path.join(folder, f"full_instance_layer_interpolate{l}.npz"))["arr_0"]
            # (scipy >= 1.12 hands the values back as float64 — its result array starts as NaN; older ones keep int64)
            assert got.shape == vol.shape and np.array_equal(got, got.astype(np.int64))
            got = got.astype(np.int64)
            dmin, allowed, labels, rule = R.fill_bruteforce(vol)
            multi = allowed.sum(-1) > 1
            inside = np.take_along_axis(allowed, np.searchsorted(labels, got)[..., None], -1)[..., 0]
            print(f"fill {name}: sites {int((vol != 0).sum())} labels {labels.tolist()} multi-label cells {multi.mean():.4f} "
                  f"scipy inside the set {inside.mean():.4f} scipy == tie rule {(got == rule).mean():.4f}")
            assert multi.mean() <= 0.05 and inside.all()
            if name == "surface":
                assert len(labels) == 5 and 1200 <= (vol != 0).sum() <= 2200
            out[f"fill/{name}"] = got.astype(np.uint8)


def main():
    out = {}
    gen_bounds(out)
    gen_fragments(out)
    gen_labels(out)
    gen_fill(out)
    path = os.path.join(HERE, "generate_gt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()

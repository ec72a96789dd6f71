"""GPU: the fragment ground-truth transform (eprecon_amd/transforms.py, csrc/gt_crop.hip) against the reference's own
RandomTransformSpace (tests/golden/transform_space.npz), against torch's CPU grid_sample on a sample no golden knows, on an
aligned crop, through both input forms and through collate_fragments (into NeuConNet.forward: tests/test_fragment_pipeline_gpu.py).

Comparison rule (tests/transform_ref.py): colour and labels exact, TSDF within 1e-3, occupancy exact; a voxel may be left
out only where its float64 coordinate lies within 1e-3 cell of a nearest-cell or inside-test decision, at most 2 % per level."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import transform_ref as R  # noqa: E402
from eprecon_amd import transforms as T  # noqa: E402

PANOPTIC_KEYS = ("rgb", "semantic", "instance")
FULL_KEYS = ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "transform_space.npz"))


def scene_of(inp):
    return T.SceneVolumes(*[inp.get(k) for k in FULL_KEYS])


def level_volumes(inp, l):
    return [inp["tsdf_list_full"][l]] + [inp[f"{k}_list_full"][l] if f"{k}_list_full" in inp else None for k in PANOPTIC_KEYS]


def level_of(out, l):
    return {k: out[f"{k}_list"][l].cpu().numpy() for k in ("tsdf",) + PANOPTIC_KEYS if f"{k}_list" in out}


def make_transform(name):
    rot, trans, seed, _, _ = R.CASES[name]
    torch.manual_seed(seed)
    pad_xy, pad_z = R.paddings(rot, trans)
    return T.RandomTransformSpace(list(R.N_VOX), R.VOXEL_SIZE, rot, trans, pad_xy, pad_z, max_epoch=R.MAX_EPOCH)


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_the_reference_golden(gold, name):
    """every case and level, fed with the reference's own T^-1, fragment origin and world->camera matrices"""
    inp = R.case_inputs(name)
    partial, tinv = gold[f"{name}/vol_origin_partial"], gold[f"{name}/Tinv"]
    out = T.crop_ground_truth(scene_of(inp), R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"])
    occ = T.fragment_occupancy(R.N_VOX, R.VOXEL_SIZE, torch.from_numpy(partial), inp["depth"], inp["intrinsics"],
                               gold[f"{name}/extrinsics"], world2cam=gold[f"{name}/world2cam"])
    assert ("rgb_list" in out) == R.CASES[name][3]
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"], l, *level_volumes(inp, l))
        want = {"tsdf": gold[f"{name}/tsdf_{l}"].astype(np.float64),
                **{k: gold[f"{name}/{k}_{l}"].astype(np.float64) for k in PANOPTIC_KEYS if f"{name}/{k}_{l}" in gold.files}}
        got = level_of(out, l)
        assert all(got[k].shape == want[k].shape and got[k].dtype == np.float32 for k in want)
        R.compare(got, want, ref["excluded"], f"{name} level {l}")
        print(f"{name} level {l}: TSDF bit-equal to the golden on {float((got['tsdf'] == want['tsdf']).mean()):.4f} of ALL voxels, "
              f"max error over all voxels {float(np.abs(got['tsdf'] - want['tsdf']).max()):.3e}")
        assert occ[l].dtype == torch.bool and np.array_equal(occ[l].cpu().numpy(), gold[f"{name}/occ_{l}"])


def test_kernel_matches_grid_sample_on_a_second_seed():
    """no reference tree involved: the rule through torch.nn.functional.grid_sample on the CPU, computed here"""
    inp, tinv, partial = R.second_seed_case()
    out = T.crop_ground_truth(scene_of(inp), R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"])
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"], l, *level_volumes(inp, l))
        want = R.crop_grid_sample(torch, R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"], l, *level_volumes(inp, l))
        R.compare(level_of(out, l), {k: v.astype(np.float64) for k, v in want.items()}, ref["excluded"], f"second seed level {l}")


def test_aligned_crop_returns_the_scenes_own_cells():
    """T = I and a fragment origin (8, 8, 4) cells inside the scene: output voxel i of level l samples the scene's cell
    i + (8, 8, 4) / 2^l at all three levels.  Colour and labels are that cell's, exactly.  TSDF is that cell's, exactly, where
    the cell is outside the band (|v| = 1).  Inside the band the reference's rule does NOT return the cell: it normalises by
    D - 1 and samples with align_corners=False, so its sample point is u = c D / (D - 1) - 1/2, up to half a cell off the cell
    centre c, and the trilinear value there differs from the cell by whatever the neighbours differ: in the float64 restatement
    of the rule the in-band voxels of this random scene are up to 1.05 / 1.03 / 1.02 (level 0 / 1 / 2) away from their own cell,
    so "TSDF within 1e-3 of the own cell" cannot hold for an implementation that matches the reference's golden.  Those voxels
    are held within 1e-3 to the trilinear value AT u instead, in float64 (the figures are printed)."""
    inp = R.make_inputs(21)
    k = np.array([8, 8, 4])
    vs = np.float32(R.VOXEL_SIZE)
    partial = (inp["vol_origin"] + k.astype(np.float32) * vs).astype(np.float32)
    out = T.crop_ground_truth(scene_of(inp), R.N_VOX, R.VOXEL_SIZE, partial, torch.eye(4), inp["vol_origin"])
    for l in range(3):
        lo = k // 2 ** l
        dims = [n // 2 ** l for n in R.N_VOX]
        cell = tuple(slice(int(a), int(a + d)) for a, d in zip(lo, dims))
        got = level_of(out, l)
        for key in PANOPTIC_KEYS:
            assert np.array_equal(got[key], inp[f"{key}_list_full"][l][cell]), (l, key)
        own = inp["tsdf_list_full"][l][cell]
        edge = np.abs(own) >= 1
        assert edge.sum() > 0.2 * own.size and (~edge).sum() > 0.2 * own.size
        assert np.array_equal(got["tsdf"][edge], own[edge]), l
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, partial, np.eye(4), inp["vol_origin"], l, inp["tsdf_list_full"][l])
        assert not ref["excluded"].any() and not ref["outside"].any()
        print(f"level {l}: in-band max |crop - own cell| {np.abs(got['tsdf'] - own)[~edge].max():.3f}, "
              f"max |crop - trilinear at u| {np.abs(got['tsdf'] - ref['tsdf']).max():.3e}")
        assert np.abs(got["tsdf"] - ref["tsdf"]).max() <= R.TSDF_TOL, l


def test_aligned_crop_of_a_linear_scene_has_the_closed_form_value():
    """independent of tests/transform_ref.py: a TSDF linear in the cell index, v = a . cell + b with |v| < 1 everywhere, so every
    voxel takes the trilinear branch, and trilinear interpolation of a linear function is that function.  With T = I and the
    fragment starting k fine cells inside the scene, output voxel i of level l has the scene coordinate c = i + k / 2^l and is
    sampled at u = c D / (D - 1) - 1/2 per axis, so it must hold a . u + b wherever the eight taps lie inside the volume
    (elsewhere zero padding enters).  Slopes <= 0.04 per cell: a coordinate error of 1e-3 cell moves the value by 4e-5."""
    origin = np.array(R.SCENE_ORIGIN, np.float32)
    k = np.array([8, 8, 4])
    partial = (origin + k.astype(np.float32) * np.float32(R.VOXEL_SIZE)).astype(np.float32)
    a = [np.array((0.0049, -0.0041, 0.0093)) * 2 ** l for l in range(3)]
    b = -0.05
    vols = []
    for l, dims in enumerate(R.SCENE_DIMS):
        cell = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"))
        vols.append((np.tensordot(a[l], cell, 1) + b).astype(np.float32))
        assert np.abs(vols[-1]).max() < 0.95
    out = T.crop_ground_truth(T.SceneVolumes(vols), R.N_VOX, R.VOXEL_SIZE, partial, torch.eye(4), origin)
    for l, dims in enumerate(R.SCENE_DIMS):
        got = out["tsdf_list"][l].cpu().numpy().astype(np.float64)
        u = [(np.arange(n // 2 ** l) + k[ax] / 2 ** l) * dims[ax] / (dims[ax] - 1) - 0.5 for ax, n in enumerate(R.N_VOX)]
        ok = [(np.floor(x) >= 0) & (np.floor(x) + 1 <= dims[ax] - 1) for ax, x in enumerate(u)]
        inner = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        want = b + a[l][0] * u[0][:, None, None] + a[l][1] * u[1][None, :, None] + a[l][2] * u[2][None, None, :]
        err = np.abs(got - want)[inner].max()
        print(f"level {l}: {int(inner.sum())} of {inner.size} voxels with an inner stencil, max |crop - closed form| {err:.3e}")
        assert inner.mean() > 0.5 and err <= R.TSDF_TOL, (l, err)


def test_scene_volumes_load_reads_the_scene_directory(tmp_path):
    """SceneVolumes.load on the reference's file layout (<dir>/<scene>/full_*_layer{l}.npz, array under arr_0), with and
    without the panoptic volumes, against the SceneVolumes built from the same arrays"""
    inp = R.make_inputs(5)
    folder = tmp_path / "scene0000_00"
    folder.mkdir()
    names = {"tsdf_list_full": "full_tsdf_layer{}.npz", "rgb_list_full": "full_rgb_layer{}.npz",
             "semantic_list_full": "full_semantic_layer_interpolate{}.npz", "instance_list_full": "full_instance_layer_interpolate{}.npz"}
    for key, pattern in names.items():
        for l in range(3):
            np.savez_compressed(str(folder / pattern.format(l)), inp[key][l])
    want = scene_of(inp)
    got = T.SceneVolumes.load(str(tmp_path), "scene0000_00", panoptic=True)
    assert got.panoptic and got.shapes == want.shapes == [tuple(d) for d in R.SCENE_DIMS]
    for attr, dtype in (("tsdf", torch.float32), ("rgb", torch.float32), ("semantic", torch.int32), ("instance", torch.int32)):
        for x, y in zip(getattr(got, attr), getattr(want, attr)):
            assert x.is_cuda and x.dtype == dtype and torch.equal(x, y), attr
    plain = T.SceneVolumes.load(str(tmp_path), "scene0000_00", panoptic=False)
    assert not plain.panoptic and plain.semantic is None and all(torch.equal(x, y) for x, y in zip(plain.tsdf, want.tsdf))


def run_sample(name, gold, scene=None, inp=None):
    inp = inp or R.case_inputs(name)
    data = R.sample_dict(inp, torch, scene=scene)
    data["world2cam"] = gold[f"{name}/world2cam"]
    return make_transform(name)(data)


@pytest.mark.parametrize("name", ["rot_trans_1", "tsdf_only"])
def test_scene_volumes_and_lists_give_identical_samples(gold, name):
    """__call__ on a SceneVolumes and on the reference's lists: bit-identical targets, the reference's keys, and the
    reference's values (T computed here may differ from the reference's in the last bit: 1e-6 of a cell at most)"""
    inp = R.case_inputs(name)
    a = run_sample(name, gold, inp=inp)
    b = run_sample(name, gold, scene=scene_of(inp), inp=inp)
    lists = ["tsdf_list", "occ_list"] + (["rgb_list", "semantic_list", "instance_list"] if R.CASES[name][3] else [])
    assert set(a) == set(b) == {"imgs", "intrinsics", "extrinsics", "vol_origin", "vol_origin_partial"} | set(lists)
    for key in lists:
        assert len(a[key]) == 3 and all(x.is_cuda and torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert np.array_equal(a["vol_origin_partial"].numpy(), gold[f"{name}/vol_origin_partial"])
    assert np.abs(a["extrinsics"].numpy() - gold[f"{name}/extrinsics"]).max() <= 1e-6
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, gold[f"{name}/vol_origin_partial"], gold[f"{name}/Tinv"], inp["vol_origin"], l,
                         *level_volumes(inp, l))
        want = {"tsdf": gold[f"{name}/tsdf_{l}"].astype(np.float64),
                **{k: gold[f"{name}/{k}_{l}"].astype(np.float64) for k in PANOPTIC_KEYS if f"{name}/{k}_{l}" in gold.files}}
        R.compare(level_of(a, l), want, ref["excluded"], f"{name} level {l} through __call__")
        assert np.array_equal(a["occ_list"][l].cpu().numpy(), gold[f"{name}/occ_{l}"])


def test_two_samples_through_collate_fragments(gold):
    pipe = T.IntrinsicsPoseToProjection(R.VIEWS, 4)
    samples = []
    for name in ("rot_trans_1", "rot_trans_2"):
        s = pipe(run_sample(name, gold))
        s.update(scene="scene", fragment=f"scene_{name}")
        samples.append(s)
    batch = T.collate_fragments(samples)
    x, y, z = R.N_VOX
    for l in range(3):
        shape = (2, x >> l, y >> l, z >> l)
        assert batch["tsdf_list"][l].shape == batch["semantic_list"][l].shape == batch["occ_list"][l].shape == shape
        assert batch["rgb_list"][l].shape == shape + (3,) and batch["occ_list"][l].dtype == torch.bool
        for b, name in enumerate(("rot_trans_1", "rot_trans_2")):
            assert torch.equal(batch["tsdf_list"][l][b], samples[b]["tsdf_list"][l])
            assert np.array_equal(batch["occ_list"][l][b].cpu().numpy(), gold[f"{name}/occ_{l}"])
    assert batch["proj_matrices"].shape == (2, R.VIEWS, 3, 4, 4) and batch["world_to_aligned_camera"].shape == (2, 4, 4)
    assert all(batch[k].is_cuda for k in ("proj_matrices", "vol_origin", "vol_origin_partial", "world_to_aligned_camera", "imgs"))
    assert not batch["vol_origin_partial_host"].is_cuda and not batch["vol_origin_host"].is_cuda
    assert torch.equal(batch["vol_origin_partial_host"], batch["vol_origin_partial"].cpu())
    assert batch["fragment"] == ["scene_rot_trans_1", "scene_rot_trans_2"]

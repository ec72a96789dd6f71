"""CPU: the host side of eprecon_amd.transforms against the reference's own RandomTransformSpace
(tests/golden/transform_space.npz, written by tests/golden/make_transform_golden.py), the float64 restatement of the crop
rule (tests/transform_ref.py) against torch's CPU grid_sample and against the golden, the descriptor's ctypes layout and
the entry point's argument checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import transform_ref as R  # noqa: E402
from eprecon_amd import _lib  # noqa: E402
from eprecon_amd import synthetic as S  # noqa: E402
from eprecon_amd import transforms as T  # noqa: E402

PANOPTIC_KEYS = ("rgb", "semantic", "instance")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "transform_space.npz"))


def make_transform(name, **kw):
    rot, trans, seed, _, _ = R.CASES[name]
    torch.manual_seed(seed)
    pad_xy, pad_z = R.paddings(rot, trans)
    return T.RandomTransformSpace(list(R.N_VOX), R.VOXEL_SIZE, rot, trans, pad_xy, pad_z, max_epoch=R.MAX_EPOCH, **kw)


@pytest.mark.parametrize("name", list(R.CASES))
def test_same_seed_gives_the_reference_draws(gold, name):
    rts = make_transform(name)
    assert np.array_equal(rts.random_r.numpy(), gold[f"{name}/random_r"])
    assert np.array_equal(rts.random_t.numpy(), gold[f"{name}/random_t"])
    again = make_transform(name)
    assert torch.equal(rts.random_r, again.random_r) and torch.equal(rts.random_t, again.random_t)


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_quantities_match_the_reference(gold, name):
    """T and the transformed extrinsics to 1e-6 (cos / sin and a 4x4 inverse may differ in the last bit between hosts),
    vol_origin_partial exactly (it is snapped to 8 cells, and the generator keeps the cases away from a rounding tie)"""
    rts = make_transform(name)
    inp = R.case_inputs(name)
    t_mat = rts.epoch_transform(torch.Tensor(inp["vol_origin"]), R.SCENE_DIMS[0], R.EPOCH)
    assert np.abs(t_mat.numpy() - gold[f"{name}/T"]).max() <= 1e-6
    assert np.abs(t_mat.inverse().numpy() - gold[f"{name}/Tinv"]).max() <= 1e-6
    ext = torch.stack([t_mat @ e for e in torch.from_numpy(inp["extrinsics"])])
    assert np.abs(ext.numpy() - gold[f"{name}/extrinsics"]).max() <= 1e-6
    assert np.abs(torch.inverse(ext).numpy() - gold[f"{name}/world2cam"]).max() <= 1e-6
    bnds = T.frustum_bounds(3.0, (R.IMG_H, R.IMG_W), torch.from_numpy(inp["intrinsics"]), ext)
    partial = T.fragment_origin(bnds, torch.zeros(3), list(R.N_VOX), R.VOXEL_SIZE)
    assert np.array_equal(partial.numpy(), gold[f"{name}/vol_origin_partial"])
    # the same through __call__ on a sample without a scene (only the host side runs); the unaugmented form needs no volumes
    if name == "plain":
        data = R.sample_dict(inp, torch)
        for k in ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full"):
            data.pop(k)
        out = rts(data)
        assert np.array_equal(out["vol_origin_partial"].numpy(), gold[f"{name}/vol_origin_partial"])
        assert torch.equal(out["vol_origin"], torch.zeros(3)) and "epoch" not in out and "depth" in out
        assert torch.equal(out["extrinsics"], torch.from_numpy(inp["extrinsics"]))


def test_unaugmented_transform_is_the_identity():
    assert torch.equal(make_transform("plain").epoch_transform(torch.zeros(3), (4, 4, 4), 0), torch.eye(4))


def test_projection_matrices_and_aligned_camera():
    """proj_matrices against the reference's formula restated in float64 numpy (datasets/transforms.py:65-77);
    world_to_aligned_camera is synthetic's (a restatement: the reference builds it with transforms3d)"""
    w = S.make_window(seed=3, width=320, height=240)
    data = {"intrinsics": torch.from_numpy(np.stack([w["intrinsics"]] * 9)), "extrinsics": torch.from_numpy(w["poses"].copy()),
            "scene": "s"}
    out = T.IntrinsicsPoseToProjection(9, 4)(dict(data))
    assert "intrinsics" not in out and "extrinsics" not in out and out["scene"] == "s"
    assert out["proj_matrices"].shape == (9, 3, 4, 4) and out["proj_matrices"].dtype == torch.float32
    for v in range(9):
        inv = np.linalg.inv(w["poses"][v].astype(np.float64))
        for l in range(3):
            k = w["intrinsics"].astype(np.float64) / 4 / 2 ** l
            k[2, 2] = 1
            want = inv.copy()
            want[:3] = k @ inv[:3]
            assert np.abs(out["proj_matrices"][v, l].numpy() - want).max() <= 1e-5 * np.abs(want).max()
    # (and the generator's own matrices, which go through the same float32 steps)
    assert np.abs(out["proj_matrices"].numpy() - w["proj_matrices"]).max() <= 1e-5 * np.abs(w["proj_matrices"]).max()
    assert np.array_equal(out["world_to_aligned_camera"].numpy(), S.world_to_aligned_camera(w["poses"][4].astype(np.float64)))
    assert np.abs(out["world_to_aligned_camera"].numpy() - w["world_to_aligned_camera"]).max() <= 1e-6


def test_to_tensor_compose_and_resize_image():
    imgs = [np.zeros((6, 8, 3), np.float32) for _ in range(2)]
    data = {"imgs": imgs, "intrinsics": np.stack([np.eye(3)] * 2), "extrinsics": np.stack([np.eye(4)] * 2),
            "depth": [np.ones((6, 8), np.float32)] * 2, "tsdf_list_full": [np.zeros((2, 2, 2))],
            "rgb_list_full": [np.zeros((2, 2, 2, 3))], "semantic_list_full": [np.zeros((2, 2, 2), np.int64)],
            "instance_list_full": [np.zeros((2, 2, 2), np.int64)]}
    out = T.Compose([T.ToTensor()])(data)
    assert out["imgs"].shape == (2, 3, 6, 8) and out["depth"].shape == (2, 6, 8)
    assert all(out[k][0].dtype == torch.float32 for k in ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full"))
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    assert hasattr(T, "ResizeImage") == have_pil


def test_collate_fragments_on_the_host():
    def sample(k):
        return {"imgs": torch.zeros(9, 3, 4, 4), "vol_origin": torch.zeros(3), "vol_origin_partial": torch.full((3,), float(k)),
                "tsdf_list": [torch.zeros(4, 4, 4), torch.zeros(2, 2, 2)], "occ_list": [torch.zeros(4, 4, 4, dtype=torch.bool)] * 2,
                "scene": "s", "fragment": f"s_{k}", "proj_matrices": torch.zeros(9, 3, 4, 4), "world_to_aligned_camera": torch.eye(4)}
    out = T.collate_fragments([sample(0), sample(1)], device="cpu")
    assert out["imgs"].shape == (2, 9, 3, 4, 4) and out["proj_matrices"].shape == (2, 9, 3, 4, 4)
    assert [tuple(t.shape) for t in out["tsdf_list"]] == [(2, 4, 4, 4), (2, 2, 2, 2)] and out["occ_list"][0].dtype == torch.bool
    assert out["scene"] == ["s", "s"] and out["fragment"] == ["s_0", "s_1"]
    assert torch.equal(out["vol_origin_partial_host"], torch.tensor([[0.0] * 3, [1.0] * 3])) and out["vol_origin_host"].shape == (2, 3)


# ---------------------------------------------------------------- the float64 restatement
def level_volumes(inp, l):
    return [inp["tsdf_list_full"][l]] + [inp[f"{k}_list_full"][l] if f"{k}_list_full" in inp else None for k in PANOPTIC_KEYS]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_agrees_with_the_reference_golden(gold, name):
    inp = R.case_inputs(name)
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, gold[f"{name}/vol_origin_partial"], gold[f"{name}/Tinv"], inp["vol_origin"], l,
                         *level_volumes(inp, l))
        got = {"tsdf": gold[f"{name}/tsdf_{l}"], **{k: gold[f"{name}/{k}_{l}"] for k in PANOPTIC_KEYS if k in ref}}
        assert got["tsdf"].shape == ref["tsdf"].shape == tuple(n // 2 ** l for n in R.N_VOX)
        assert (f"{name}/rgb_{l}" in gold.files) == R.CASES[name][3]
        R.compare(got, ref, ref["excluded"], f"{name} level {l}")


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_operation_order_reproduces_the_golden_bit_for_bit(gold, name):
    """the fp32 operation order csrc/gt_crop.hip is written in (transform_ref.crop_f32: the matrix rows as a k-ordered fma
    chain, every other step rounded to nearest) gives the reference's TSDF and labels on EVERY voxel of the golden, the
    excluded ones too: with the BLAS the golden was generated with, the order is the reference's"""
    inp = R.case_inputs(name)
    for l in range(3):
        label = inp["semantic_list_full"][l] if R.CASES[name][3] else None
        t, lab = R.crop_f32(R.N_VOX, R.VOXEL_SIZE, gold[f"{name}/vol_origin_partial"], gold[f"{name}/Tinv"], inp["vol_origin"], l,
                            inp["tsdf_list_full"][l], label)
        assert np.array_equal(t, gold[f"{name}/tsdf_{l}"]), (name, l, float(np.abs(t - gold[f"{name}/tsdf_{l}"]).max()))
        if lab is not None:
            assert np.array_equal(lab, gold[f"{name}/semantic_{l}"]), (name, l)


def test_restatement_agrees_with_grid_sample():
    inp, tinv, partial = R.second_seed_case()
    crossing = 0
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"], l, *level_volumes(inp, l))
        got = R.crop_grid_sample(torch, R.N_VOX, R.VOXEL_SIZE, partial, tinv, inp["vol_origin"], l, *level_volumes(inp, l))
        R.compare(got, ref, ref["excluded"], f"second seed level {l}")
        if l < 2:
            assert 0.25 <= 1 - ref["outside"].mean() <= 0.9 and ref["in_band"].mean() >= 0.1
        crossing += int(ref["crossing"].sum())
    assert crossing > 0


# ---------------------------------------------------------------- C ABI
def test_gt_crop_desc_layout_matches_header(tmp_path):
    """size and field offsets of the ctypes mirror against the C compiler's (as tests/test_cabi_symbols.py does for the others)"""
    mirror = _lib.GtCropDesc
    fields = [f[0] for f in mirror._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eprecon_hip.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(eprecon_gt_crop_desc));']
    src += [f'  printf("%zu\\n", offsetof(eprecon_gt_crop_desc, {name}));' for name in fields]
    src += ['  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(mirror)
    assert out[1:] == [getattr(mirror, name).offset for name in fields]


def test_entry_point_rejects_bad_descriptors():
    """the argument checks return before anything touches a device"""
    from eprecon_amd import build
    build.build()
    lib = _lib.load()

    def desc(levels=1, dims=(4, 4, 4), full=(5, 5, 5), tsdf=(8, 8), rgb=(0, 0)):
        d = _lib.GtCropDesc()
        d.levels, d.voxel_size = levels, 0.04
        for k in range(3):
            d.dims[k], d.full_dims[0][k] = dims[k], full[k]
        d.tsdf_full[0], d.tsdf_out[0] = tsdf[0] or None, tsdf[1] or None
        d.rgb_full[0], d.rgb_out[0] = rgb[0] or None, rgb[1] or None
        return d

    call = lambda d: lib.eprecon_gt_crop_async(ctypes.addressof(d), None)
    assert lib.eprecon_gt_crop_async(None, None) == -1
    assert call(desc(levels=0)) == -1 and call(desc(levels=4)) == -1
    assert call(desc(tsdf=(0, 8))) == -1 and call(desc(tsdf=(8, 0))) == -1
    assert call(desc(rgb=(8, 0))) == -1 and call(desc(rgb=(0, 8))) == -1
    assert call(desc(dims=(4, 0, 4))) == -1 and call(desc(full=(5, 0, 5))) == -1
    assert call(desc(full=(5, 1, 5))) == -3
    assert call(desc(dims=(2048, 2048, 2048))) == -3

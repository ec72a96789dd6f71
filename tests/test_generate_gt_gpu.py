"""GPU: the scene ground truth of eprecon_amd/generate_gt.py (csrc/label_volume.hip, TSDFVolumeHIP variant "cuda") against the
reference's own programs (tests/golden/generate_gt.npz), brute force over every cell, and the numpy oracle of the PyCUDA
kernel; then the whole chain: generate_scene -> SceneVolumes.load -> RandomTransformSpace."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_gt_ref as R  # noqa: E402
from oracle import tsdf_fusion as OT  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "generate_gt.npz"))


# ------------------------------------------------------------------------------------------------------------------
# label volumes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LABEL_CASES))
def test_label_volumes_bit_equal_reference(gold, name):
    from eprecon_amd.generate_gt import voxelize_labels
    xyz, rgb, sem, ins, vol_min, vs, dims = R.label_case(name)
    rgb_vol, sem_vol, ins_vol = voxelize_labels(xyz, rgb, sem, ins, vol_min, vs, dims)
    assert rgb_vol.dtype == np.float64 and rgb_vol.shape == tuple(dims) + (3,)
    assert sem_vol.dtype == np.int64 and ins_vol.dtype == np.int64 and sem_vol.shape == ins_vol.shape == tuple(dims)
    want = gold[f"labels/{name}/rgb"]
    differ = rgb_vol.view(np.int64) != want.view(np.int64)
    print(f"{name}: colour words that differ {int(differ.sum())} of {differ.size}, max |diff| {np.abs(rgb_vol - want).max():.3e}; "
          f"semantic cells that differ {int((sem_vol != gold[f'labels/{name}/sem']).sum())}, "
          f"instance {int((ins_vol != gold[f'labels/{name}/ins']).sum())}")
    assert not differ.any()                                       # the float64 bit patterns: summation order included
    assert np.array_equal(sem_vol, gold[f"labels/{name}/sem"].astype(np.int64))
    assert np.array_equal(ins_vol, gold[f"labels/{name}/ins"].astype(np.int64))
    if name == "main":
        assert sem_vol[R.CELL_EMPTY] == 0 and ins_vol[R.CELL_EMPTY] == 0 and not rgb_vol[R.CELL_EMPTY].any()
        assert sem_vol[R.CELL_TIE] == 3 and sem_vol[R.CELL_TIE0] == 0 and ins_vol[R.CELL_TIE0] == 2 and ins_vol.max() > 255
    # and again: bit-identical from run to run
    again = voxelize_labels(xyz, rgb, sem, ins, vol_min, vs, dims)
    assert np.array_equal(again[0].view(np.int64), rgb_vol.view(np.int64)) and np.array_equal(again[1], sem_vol) \
        and np.array_equal(again[2], ins_vol)


@pytest.mark.parametrize("bad", [-1, 32768, 2 ** 40])
def test_bad_label_is_err_arg(bad):
    from eprecon_amd import _lib
    from eprecon_amd.generate_gt import voxelize_labels
    xyz, rgb, sem, ins, vol_min, vs, dims = R.label_case("thin")
    for which in (0, 1):
        labels = [sem.copy(), ins.copy()]
        labels[which][17] = bad
        with pytest.raises(_lib.EpreconError, match="error -1"):
            voxelize_labels(xyz, rgb, labels[0], labels[1], vol_min, vs, dims)
    with pytest.raises(_lib.EpreconError):
        voxelize_labels(xyz, rgb, sem.astype(np.float64), ins, vol_min, vs, dims)


# ------------------------------------------------------------------------------------------------------------------
# nearest-label fill
# ------------------------------------------------------------------------------------------------------------------
def check_fill(vol, got, scipy_answer=None, what=""):
    dmin, allowed, labels, rule = R.fill_bruteforce(vol)
    assert got.dtype == np.int64 and got.shape == vol.shape
    known = np.isin(got, labels)
    member = np.zeros(vol.shape, bool)
    member[known] = np.take_along_axis(allowed, np.searchsorted(labels, np.where(known, got, labels[0]))[..., None], -1)[..., 0][known]
    multi = allowed.sum(-1) > 1
    print(f"{what}: cells {vol.size} sites {int((vol != 0).sum())} outside the nearest set {int((~member).sum())} "
          f"multi-label share {multi.mean():.4f} differ from the tie rule {int((got != rule).sum())}"
          + ("" if scipy_answer is None else f" differ from scipy where unique {int(((got != scipy_answer) & ~multi).sum())}"))
    assert member.all()                                           # EVERY cell: a label of a site at the exact minimal distance
    assert np.array_equal(got[vol != 0], vol[vol != 0])           # sites keep their own label
    assert np.array_equal(got, rule)                              # the documented tie rule, cell for cell
    if scipy_answer is not None:
        assert np.array_equal(got[~multi], scipy_answer[~multi])
        assert multi.mean() <= 0.05
    return multi


@pytest.mark.parametrize("name", list(R.FILL_CASES))
def test_fill_matches_bruteforce_and_scipy(gold, name):
    from eprecon_amd.generate_gt import interpolate_labels
    vol = R.fill_case(name)
    got = interpolate_labels(vol)
    check_fill(vol, got, gold[f"fill/{name}"].astype(np.int64), name)
    assert np.array_equal(interpolate_labels(vol), got)           # two runs: bit-identical
    assert np.array_equal(interpolate_labels(torch.from_numpy(vol).cuda()), got)


@pytest.mark.parametrize("name", ["corner", "face", "gaps"])
def test_fill_edge_inputs(name):
    from eprecon_amd.generate_gt import interpolate_labels
    vol = R.fill_edge_case(name)
    check_fill(vol, interpolate_labels(vol), what=name)


def test_fill_of_an_empty_volume_is_zero():
    from eprecon_amd.generate_gt import interpolate_labels
    got = interpolate_labels(R.fill_edge_case("zero"))
    assert got.dtype == np.int64 and got.shape == (13, 9, 21) and not got.any()


@pytest.mark.parametrize("dims", [(4097, 1, 1), (1, 4097, 1), (1, 1, 4097)])
def test_fill_refuses_an_axis_above_4096(dims):
    """on the host argument path: the dimensions are refused before any pointer is used, so four bytes stand in for the volume"""
    from eprecon_amd import _lib
    from eprecon_amd import generate_gt as GG
    tiny = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.EpreconError, match="error -3"):
        GG._label_fill(_lib.load(), tiny, dims, torch.zeros_like(tiny), workspace=torch.zeros(4, dtype=torch.uint8, device="cuda"))
    assert _lib.load().eprecon_label_fill_async(None, ctypes.cast((ctypes.c_int32 * 3)(0, 1, 1), ctypes.c_void_p), None, None, 0,
                                                None) == -1


# ------------------------------------------------------------------------------------------------------------------
# scene TSDF and the whole chain
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from eprecon_amd import generate_gt as GG
    depths, intr, poses = R.scene_case()
    bnds = GG.scene_bounds(depths, intr, poses)
    return depths, intr, poses, bnds, GG.level_volumes(bnds, R.SCENE_VOXEL, 3, 3)


def test_scene_tsdf_chunked_equals_frame_by_frame_and_oracle(scene):
    from eprecon_amd import generate_gt as GG
    from eprecon_amd.tsdf_fusion import TSDFVolumeHIP
    depths, intr, poses, bnds, levels = scene
    print("level dimensions", [lv["vol_dim"].tolist() for lv in levels])
    want = R.level_dims_f64(bnds, R.SCENE_VOXEL, 3)
    assert all(np.array_equal(lv["vol_dim"], dim) and np.array_equal(lv["vol_origin"], org) for lv, (dim, org) in zip(levels, want))
    assert len(set(levels[0]["vol_dim"].tolist())) == 3 and levels[0]["vol_dim"].max() <= 96       # small and non-cubic
    chunked = GG.fuse_scene_tsdf(depths, intr, poses, levels, margin=3, chunk=7)          # 7 + 7 + 6 frames
    whole = GG.fuse_scene_tsdf(depths, intr, poses, levels, margin=3)
    d_dev = torch.from_numpy(depths).cuda()
    for l, lv in enumerate(levels):
        single = TSDFVolumeHIP(torch.as_tensor(lv["vol_dim"]), torch.from_numpy(lv["vol_origin"]), lv["voxel_size"], margin=3,
                               variant="cuda")
        for v in range(len(depths)):
            single.integrate(d_dev[v], torch.from_numpy(intr.astype(np.float32)), torch.from_numpy(poses[v].astype(np.float32)),
                             obs_weight=1.)
        for other in (chunked[l], whole[l]):
            assert torch.equal(other.get_volume()[0], single.get_volume()[0])
            assert torch.equal(other.get_volume()[1], single.get_volume()[1])
        ref = OT.fuse_views([int(d) for d in lv["vol_dim"]], lv["vol_origin"], lv["voxel_size"], depths,
                            np.repeat(intr.astype(np.float32)[None], len(depths), 0), poses.astype(np.float32), margin=3, variant="cuda")
        tsdf, weight = (t.cpu().numpy() for t in chunked[l].get_volume())
        print(f"level {l}: weights that differ {int((weight != ref[1]).sum())}, max |tsdf - oracle| {np.abs(tsdf - ref[0]).max():.3e}, "
              f"observed cells {int((weight > 0).sum())}")
        assert np.array_equal(weight, ref[1])
        assert np.abs(tsdf - ref[0]).max() < 1e-6
        assert (weight > 0).sum() > 0.1 * weight.size


def test_generate_scene_feeds_the_fragment_ground_truth(scene, tmp_path):
    from eprecon_amd import generate_gt as GG
    from eprecon_amd.transforms import RandomTransformSpace, SceneVolumes
    depths, intr, poses, bnds, levels = scene
    cloud = R.scene_cloud(depths, intr, poses)
    args = dict(window_size=3, min_angle=15, min_distance=0.1)
    frags = GG.generate_scene("scene0000_00", depths, intr, poses, str(tmp_path), points=cloud, voxel_size=R.SCENE_VOXEL,
                              save_mesh=True, **args)
    root = tmp_path / "scene0000_00"
    with open(root / "fragments.pkl", "rb") as f:
        stored = pickle.load(f)
    with open(root / "tsdf_info.pkl", "rb") as f:
        info = pickle.load(f)
    want = GG.select_fragments(depths, intr, poses, scene="scene0000_00", vol_origin=info["vol_origin"],
                               voxel_size=info["voxel_size"], **args)
    assert len(stored) >= 2 and [s["image_ids"] for s in stored] == [w["image_ids"] for w in want] == [f["image_ids"] for f in frags]
    assert all(s["scene"] == "scene0000_00" and s["voxel_size"] == R.SCENE_VOXEL and np.array_equal(s["vol_origin"], info["vol_origin"])
               for s in stored)
    assert all((root / f"mesh_layer{l}.ply").stat().st_size > 1000 for l in range(3))
    # the label files: what voxelize_labels / interpolate_labels give for that cloud, with the reference's dtypes
    with np.load(root / "full_semantic_layer_interpolate1.npz") as z:
        filled = z["arr_0"]
    with np.load(root / "full_semantic_layer1.npz") as z:
        raw = z["arr_0"]
    assert filled.dtype == np.int64 and raw.dtype == np.int64 and filled.shape == tuple(levels[1]["vol_dim"])
    assert (raw != 0).any() and (raw == 0).any() and (filled != 0).all() and np.array_equal(filled[raw != 0], raw[raw != 0])
    vols = SceneVolumes.load(str(tmp_path), "scene0000_00")
    assert len(vols) == 3 and vols.panoptic and vols.shapes == [tuple(int(d) for d in lv["vol_dim"]) for lv in levels]
    ids = stored[0]["image_ids"]
    rts = RandomTransformSpace([24, 24, 16], R.SCENE_VOXEL, random_rotation=False, random_translation=False, paddingXY=0.0,
                               paddingZ=0.0, max_depth=R.SCENE_MAX_DEPTH)
    h, w = R.SCENE_HW
    sample = rts({"imgs": torch.zeros(len(ids), 3, h, w), "depth": torch.from_numpy(depths[ids]),
                  "intrinsics": torch.from_numpy(np.repeat(intr.astype(np.float32)[None], len(ids), 0)),
                  "extrinsics": torch.from_numpy(poses[ids].astype(np.float32)), "vol_origin": info["vol_origin"].copy(), "epoch": [0],
                  "tsdf_list_full": vols})
    tsdf, sem, ins = sample["tsdf_list"][0], sample["semantic_list"][0], sample["instance_list"][0]
    in_band = int((tsdf.abs() < 1).sum())
    print(f"fragment target: cells {tsdf.numel()} in band {in_band} labelled {int((sem != 0).sum())}")
    assert tuple(tsdf.shape) == (24, 24, 16) and in_band > 200
    assert int((sem != 0).sum()) > 200 and int((ins != 0).sum()) > 200
    assert set(sem.unique().tolist()) <= {0.0, 1.0, 2.0, 5.0, 6.0, 7.0}

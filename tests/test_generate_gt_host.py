"""CPU: the host bookkeeping of eprecon_amd/generate_gt.py — view frusta, scene bounds, level dimensions, fragment windows —
against the reference's own functions (tests/golden/generate_gt.npz, written by tests/golden/make_generate_gt_golden.py on
the seeded inputs of tests/generate_gt_ref.py), and the writer's file layout."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_gt_ref as R  # noqa: E402
from eprecon_amd import generate_gt as GG  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "generate_gt.npz"))


def test_view_frustum_equals_reference(gold):
    depths, intr, poses = R.bounds_case("few_frames")
    for k in range(3):
        assert np.array_equal(GG.get_view_frustum(depths[k], intr, poses[k]), gold[f"frustum/{k}"])


@pytest.mark.parametrize("name", list(R.BOUNDS_CASES))
def test_bounds_and_level_dimensions_equal_reference(gold, name):
    depths, intr, poses = R.bounds_case(name)
    bnds = GG.scene_bounds(depths, intr, poses)
    assert np.array_equal(bnds, gold[f"bounds/{name}"])
    assert (bnds[:, 0] <= 0).all() and (bnds[:, 1] >= 0).all()              # the bounds start at zeros
    kept = bnds.copy()
    levels = GG.level_volumes(bnds, R.VOXEL_SIZE, R.NUM_LAYERS, margin=3)
    assert np.array_equal(bnds, kept)                                       # the caller's array is left alone
    want = R.level_dims_f64(gold[f"bounds/{name}"], R.VOXEL_SIZE, R.NUM_LAYERS)
    for l, (lv, (dim, origin)) in enumerate(zip(levels, want)):
        assert np.array_equal(lv["vol_dim"], dim), (l, lv["vol_dim"], dim)
        assert lv["vol_origin"].dtype == np.float32 and np.array_equal(lv["vol_origin"], origin)
        assert lv["voxel_size"] == R.VOXEL_SIZE * 2 ** l and lv["sdf_trunc"] == 3 * lv["voxel_size"]


def test_subsample_and_adjustment_matter(gold):
    """the two cases are there for a reason: with every frame the many-frame bounds differ, and level 1 of the few-frame case
    is not round((frustum max - min) / size)"""
    depths, intr, poses = R.bounds_case("many_frames")
    ids = GG.valid_frames(poses)
    assert len(ids) > GG.MAX_BOUND_FRAMES and len(ids) == len(poses) - 1
    every = np.zeros((3, 2))
    for i in ids:
        pts = GG.get_view_frustum(depths[i], intr, poses[i])
        every[:, 0], every[:, 1] = np.minimum(every[:, 0], pts.min(1)), np.maximum(every[:, 1], pts.max(1))
    assert not np.array_equal(every, gold["bounds/many_frames"])
    bnds = gold["bounds/few_frames"]
    levels = GG.level_volumes(bnds, R.VOXEL_SIZE, R.NUM_LAYERS)
    assert not np.array_equal(levels[1]["vol_dim"], R.naive_dims(bnds, R.VOXEL_SIZE, 1))


def test_fragment_selection_equals_reference(gold):
    depths, intr, poses, script = R.fragment_case()
    origin = np.array([-1.0, 0.5, 0.25], np.float32)
    frags = GG.select_fragments(depths, intr, poses, scene="scene0000_00", vol_origin=origin, voxel_size=0.04, **R.FRAGMENT_ARGS)
    lens = gold["fragments/lens"].tolist()
    want = np.split(gold["fragments/ids"], np.cumsum(lens)[:-1])
    assert [f["image_ids"] for f in frags] == [w.tolist() for w in want]
    assert [f["fragment_id"] for f in frags] == list(range(len(lens)))
    assert all(sorted(f) == ["fragment_id", "image_ids", "scene", "vol_origin", "voxel_size"] for f in frags)
    assert all(f["scene"] == "scene0000_00" and f["voxel_size"] == 0.04 and f["vol_origin"] is origin for f in frags)
    taken = {i for f in frags for i in f["image_ids"]}
    assert not taken & {i for i, kind in enumerate(script) if kind in ("inf", "reject")}
    assert max(taken) < len(script) - 1                                      # the unfinished window at the end is dropped


def test_generate_pkl_concatenates_split_scenes(tmp_path):
    for scene, n in (("scene0001_00", 2), ("scene0000_00", 3), ("scene0002_00", 1)):
        os.makedirs(tmp_path / "out" / scene)
        with open(tmp_path / "out" / scene / "fragments.pkl", "wb") as f:
            pickle.dump([{"scene": scene, "fragment_id": k} for k in range(n)], f)
    os.makedirs(tmp_path / "out" / "splits")                                 # a folder that is no scene
    (tmp_path / "scannetv2_val.txt").write_text("scene0000_00\nscene0001_00\nscene0700_00\n")
    frags = GG.generate_pkl(str(tmp_path / "out"), str(tmp_path / "scannetv2_val.txt"), "val")
    assert [(f["scene"], f["fragment_id"]) for f in frags] == [("scene0000_00", 0), ("scene0000_00", 1), ("scene0000_00", 2),
                                                               ("scene0001_00", 0), ("scene0001_00", 1)]
    with open(tmp_path / "out" / "fragments_val.pkl", "rb") as f:
        assert pickle.load(f) == frags


def test_file_layout_round_trip(tmp_path, monkeypatch):
    """generate_scene's writer with the GPU stages replaced by arrays of the right kind: the key names, dtypes and shapes
    that come back through np.load and pickle are the reference's"""
    depths, intr, poses = R.bounds_case("few_frames")
    levels = GG.level_volumes(GG.scene_bounds(depths, intr, poses), 0.32, 3)
    import torch

    class FakeVolume:
        def __init__(self, dim):
            self.t = torch.ones(tuple(int(d) for d in dim), dtype=torch.float32)

        def get_volume(self):
            return self.t, self.t

    monkeypatch.setattr(GG, "fuse_scene_tsdf", lambda d, k, p, lv, **kw: [FakeVolume(x["vol_dim"]) for x in lv])
    monkeypatch.setattr(GG, "voxelize_labels", lambda xyz, rgb, s, i, vmin, vs, dims, device=None: (
        np.zeros(tuple(dims) + (3,), np.float64), np.ones(tuple(dims), np.int64), np.ones(tuple(dims), np.int64)))
    monkeypatch.setattr(GG, "interpolate_labels", lambda vol, device=None: vol.astype(np.int64))
    points = (np.zeros((5, 6)), np.ones(5, np.int64), np.ones(5, np.int64))
    frags = GG.generate_scene("scene0000_00", depths, intr, poses, str(tmp_path), points=points, voxel_size=0.32, window_size=3)
    root = tmp_path / "scene0000_00"
    with open(root / "tsdf_info.pkl", "rb") as f:
        info = pickle.load(f)
    assert sorted(info) == ["vol_origin", "voxel_size"] and info["vol_origin"].dtype == np.float32 and info["voxel_size"] == 0.32
    assert np.array_equal(info["vol_origin"], levels[0]["vol_origin"])
    for l, lv in enumerate(levels):
        shape = tuple(int(d) for d in lv["vol_dim"])
        for stem, dtype, shp in (("full_tsdf_layer", np.float32, shape), ("full_rgb_layer", np.float64, shape + (3,)),
                                 ("full_semantic_layer", np.int64, shape), ("full_instance_layer", np.int64, shape),
                                 ("full_semantic_layer_interpolate", np.int64, shape),
                                 ("full_instance_layer_interpolate", np.int64, shape)):
            with np.load(root / f"{stem}{l}.npz", allow_pickle=True) as z:
                assert z.files == ["arr_0"] and z["arr_0"].dtype == dtype and z["arr_0"].shape == shp, (stem, l)
    with open(root / "fragments.pkl", "rb") as f:
        stored = pickle.load(f)
    assert [s["image_ids"] for s in stored] == [f["image_ids"] for f in frags] and len(stored) >= 1
    assert stored[0]["scene"] == "scene0000_00" and np.array_equal(stored[0]["vol_origin"], info["vol_origin"])
    # a test scene (no labelled cloud) writes the TSDF and the fragments only
    GG.generate_scene("scene0707_00", depths, intr, poses, str(tmp_path), voxel_size=0.32, window_size=3)
    assert sorted(os.listdir(tmp_path / "scene0707_00")) == ["fragments.pkl", "full_tsdf_layer0.npz", "full_tsdf_layer1.npz",
                                                             "full_tsdf_layer2.npz", "tsdf_info.pkl"]


def test_cli_test_switch_is_a_real_switch():
    assert GG.parse_args([]).test is False and GG.parse_args(["--test"]).test is True
    args = GG.parse_args([])
    assert (args.max_depth, args.num_layers, args.margin, args.voxel_size, args.window_size, args.min_angle,
            args.min_distance) == (3.0, 3, 3, 0.04, 9, 15, 0.1)


def test_depth_png_reader(tmp_path):
    from PIL import Image
    mm = np.array([[0, 500, 2999], [3000, 3001, 65535]], np.uint16)
    Image.fromarray(mm).save(tmp_path / "depth_0.png")
    d = GG.depth_metres(str(tmp_path / "depth_0.png"), 3.0)
    assert d.dtype == np.float32 and np.array_equal(d, np.array([[0, 0.5, 2.999], [3.0, 0, 0]], np.float32))

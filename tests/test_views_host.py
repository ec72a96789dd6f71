"""CPU: the view preparation's references agree with each other and with PIL, the library's host tables are the restatement's,
and ScanNetDataset hands out the reference's item dict (datasets/scannet.py:112-172) from a tiny scene on disk."""
import os
import pickle

import numpy as np
import pytest

import views_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")
CASES = ("strip", "strip_padded", "upscale")
# (in_h, in_w, pad, out_h, out_w): the production frame, two down-scalings, an up-scaling, the identity, one axis only
LIVE_SIZES = [(968, 1296, 2, 480, 640), (97, 131, 0, 48, 64), (61, 83, 0, 48, 64), (30, 40, 0, 48, 64), (480, 640, 0, 480, 640),
              (50, 64, 0, 24, 64)]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case):
    with np.load(GOLDEN) as z:
        frame, (top, bottom), want = z[case + "/frame"], z[case + "/pad"], z[case + "/resized"]
    got = R.resize(frame, want.shape[:2], int(top), int(bottom))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # the channels are independent: what lets the GPU test make a second view of the same golden
    assert np.array_equal(R.resize(frame[..., ::-1], want.shape[:2], int(top), int(bottom)), want[..., ::-1])


@pytest.mark.parametrize("size", LIVE_SIZES, ids=lambda s: "{}x{}+{}to{}x{}".format(*s))
def test_restatement_reproduces_pil(size):
    Image = pytest.importorskip("PIL.Image")
    in_h, in_w, pad, out_h, out_w = size
    frame = np.random.default_rng(in_h).integers(0, 256, (in_h, in_w, 3), dtype=np.uint8)
    canvas = Image.new("RGB", (in_w, in_h + 2 * pad))
    canvas.paste(Image.fromarray(frame), (0, pad))
    want = np.asarray(canvas.resize((out_w, out_h), Image.BILINEAR))
    assert np.array_equal(R.resize(frame, (out_h, out_w), pad, pad), want)


@pytest.mark.parametrize("n_in,n_out", [(972, 480), (1296, 640), (97, 48), (131, 64), (61, 48), (83, 64), (30, 48), (40, 64),
                                        (480, 480), (50, 24), (160, 40), (256, 64), (9, 4), (11, 5), (83, 37), (131, 70),
                                        (81, 40), (1, 1), (3, 7)])
def test_host_tables_equal_the_restatement(n_in, n_out):
    from eprecon_amd import _lib
    from eprecon_amd.transforms import resample_table
    bounds, k = R.coefficients(n_in, n_out)
    table = resample_table(n_in, n_out)
    assert table.dtype == np.int32 and table.shape == (n_out, 2 + k.shape[1]) and k.shape[1] <= _lib.VIEWS_MAX_KSIZE
    assert np.array_equal(table[:, :2], bounds) and np.array_equal(table[:, 2:], k)
    # what the kernel relies on: the windows move forward only, and stay inside the input
    assert (np.diff(table[:, 0]) >= 0).all() and (np.diff(table[:, 0] + table[:, 1]) >= 0).all()
    assert table[:, 0].min() >= 0 and (table[:, 0] + table[:, 1]).max() <= n_in and table[:, 1].min() >= 1


def test_identity_table_is_one_zero():
    from eprecon_amd.transforms import resample_table
    table = resample_table(64, 64)
    assert np.array_equal(table[:, 0], np.arange(64)) and np.array_equal(table[:, 2], np.full(64, 1 << 22))
    assert not table[:, 3:].any()


def test_window_rows_cover_every_tile():
    from eprecon_amd import _lib
    from eprecon_amd.transforms import _window_rows, resample_table
    for n_in, n_out in ((972, 480), (83, 37), (30, 48), (160, 40), (9, 4)):
        table = resample_table(n_in, n_out)
        rows = _window_rows(table, _lib.VIEWS_TILE_H)
        for start in range(0, n_out, _lib.VIEWS_TILE_H):
            tile = table[start:start + _lib.VIEWS_TILE_H]
            assert (tile[:, 0] + tile[:, 1]).max() - tile[:, 0].min() <= rows
    assert _window_rows(resample_table(972, 480), _lib.VIEWS_TILE_H) == 35


@pytest.mark.parametrize("n_in,n_out", [(161, 40), (1296, 300), (5, 1)])
def test_scale_above_four_raises(n_in, n_out):
    from eprecon_amd.transforms import resample_table
    with pytest.raises(ValueError):
        resample_table(n_in, n_out)


def test_fit_intrinsics_is_resize_images_rule():
    """the shared rule against the arithmetic ResizeImage has always done (datasets/transforms.py:60-80), float32 in place"""
    from eprecon_amd.transforms import fit_intrinsics, frame_padding
    k0 = np.array([[1170.1, 0, 647.7], [0, 1170.2, 483.7], [0, 0, 1]], np.float32)
    for (w, h), canvas_h in (((1296, 968), 972), ((640, 480), 480), ((83, 61), 61)):
        want = k0.copy()
        if (w, h) == (1296, 968):
            want[1, 2] += 2
        want[0, :] /= w / 640
        want[1, :] /= canvas_h / 480
        got = k0.copy()
        assert fit_intrinsics(got, (w, h), (640, 480)) == frame_padding((w, h)) == (canvas_h - h) // 2
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------ the dataset

N_FRAGMENTS, N_VIEWS, SCENE = 3, 3, "scene0707_00"


@pytest.fixture(scope="module")
def tiny_scene(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("scannet_tiny")
    rng = np.random.default_rng(5)
    frames = root / "scans_test" / SCENE
    for d in ("color", "depth", "pose", "intrinsic"):
        os.makedirs(frames / d)
    k4 = np.eye(4)
    k4[:3, :3] = [[28.5, 0, 19.5], [0, 28.5, 14.5], [0, 0, 1]]
    np.savetxt(frames / "intrinsic" / "intrinsic_color.txt", k4, delimiter=" ")
    truth = {"depth": {}, "pose": {}, "k": k4[:3, :3].astype(np.float32)}
    for vid in range(0, 10 * N_FRAGMENTS * N_VIEWS, 10):
        y, x = np.mgrid[0:30, 0:40]
        colour = np.stack([(x * 6 + vid) % 256, (y * 8 + vid) % 256, (x + y + vid) % 256], -1).astype(np.uint8)
        Image.fromarray(colour).save(frames / "color" / f"color_{vid}.jpg", quality=95)
        depth = rng.integers(0, 6000, (30, 40)).astype(np.uint16)
        depth[0, :6] = [0, 1, 2999, 3000, 3001, 65535]
        Image.fromarray(depth).save(frames / "depth" / f"depth_{vid}.png")
        pose = np.eye(4)
        pose[:3, 3] = rng.normal(size=3)
        np.savetxt(frames / "pose" / f"pose_{vid}.txt", pose)
        truth["depth"][vid], truth["pose"][vid] = depth, np.loadtxt(frames / "pose" / f"pose_{vid}.txt")
    tsdf_dir = root / f"all_tsdf_{N_VIEWS}_1"
    os.makedirs(tsdf_dir / SCENE)
    metas = [{"scene": SCENE, "fragment_id": f, "image_ids": [10 * (f * N_VIEWS + v) for v in range(N_VIEWS)],
              "vol_origin": np.array([-1.0, 0.5, -0.25], np.float32)} for f in range(N_FRAGMENTS)]
    with open(tsdf_dir / "fragments_test.pkl", "wb") as fh:
        pickle.dump(metas, fh)
    truth["tsdf"] = []
    for l in range(3):
        vol = rng.random((8 >> l, 6 >> l, 4 >> l)).astype(np.float32)
        np.savez_compressed(tsdf_dir / SCENE / f"full_tsdf_layer{l}.npz", vol)
        truth["tsdf"].append(vol)
    return {"root": str(root), "metas": metas, "truth": truth, "frames": frames}


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "host"])
def test_dataset_items(tiny_scene, raw):
    from PIL import Image
    from eprecon_amd.scannet import ScanNetDataset
    truth = tiny_scene["truth"]
    ds = ScanNetDataset(tiny_scene["root"], "test", None, N_VIEWS, 2, raw=raw, device="cpu")
    assert len(ds) == N_FRAGMENTS and ds.epoch is None
    assert [m["image_ids"] for m in ds.metas] == [m["image_ids"] for m in tiny_scene["metas"]]
    assert ds.source_path == os.path.join(tiny_scene["root"], "scans_test")
    ds.epoch = 4
    for f, meta in enumerate(tiny_scene["metas"]):
        item = ds[f]
        assert list(item) == ["imgs", "depth", "intrinsics", "extrinsics", "tsdf_list_full", "vol_origin", "scene", "fragment",
                              "epoch"]
        assert item["scene"] == SCENE and item["fragment"] == f"{SCENE}_{f}" and item["epoch"] == [4]
        assert np.array_equal(item["vol_origin"], meta["vol_origin"])
        assert item["intrinsics"].dtype == np.float32 and item["intrinsics"].shape == (N_VIEWS, 3, 3)
        assert item["extrinsics"].dtype == np.float64 and item["extrinsics"].shape == (N_VIEWS, 4, 4)
        assert len(item["tsdf_list_full"]) == 3
        assert all(np.array_equal(a, b) for a, b in zip(item["tsdf_list_full"], truth["tsdf"]))
        for v, vid in enumerate(meta["image_ids"]):
            img = item["imgs"][v]
            assert isinstance(img, Image.Image) and img.size == (40, 30) and img.mode == "RGB"
            assert np.array_equal(np.asarray(img), np.asarray(Image.open(tiny_scene["frames"] / "color" / f"color_{vid}.jpg")))
            assert np.array_equal(item["intrinsics"][v], truth["k"])
            assert np.array_equal(item["extrinsics"][v], truth["pose"][vid])
            depth = item["depth"][v]
            if raw:
                assert depth.dtype == np.uint16 and np.array_equal(depth, truth["depth"][vid])
            else:
                want = truth["depth"][vid].astype(np.float32)
                want /= 1000.
                want[want > 3.0] = 0
                assert depth.dtype == np.float32 and np.array_equal(depth, want)
                assert depth[0, 3] == np.float32(3.0) and depth[0, 4] == 0 and depth[0, 5] == 0
                assert np.array_equal(depth, R.depth_to_metres(truth["depth"][vid]))
    assert list(ds.tsdf_cashe) == [SCENE]            # read once, kept


def test_dataset_source_path_and_threaded_reads(tiny_scene):
    """the source directory is an argument; a fragment read view by view (what the driver's reader threads do) is the fragment"""
    from eprecon_amd.scannet import ScanNetDataset
    ds = ScanNetDataset(tiny_scene["root"], "test", None, N_VIEWS, 2, source_path=os.path.join(tiny_scene["root"], "scans_test"),
                        device="cpu")
    meta = ds.metas[1]
    whole = ds.read_frames(meta)
    by_view = ds.stack_views([ds.read_view(meta, vid) for vid in meta["image_ids"]])
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(whole[0], by_view[0]))
    assert all(np.array_equal(a, b) for a, b in zip(whole[1], by_view[1]))
    assert np.array_equal(whole[2], by_view[2]) and np.array_equal(whole[3], by_view[3])
    with pytest.raises(FileNotFoundError):
        ScanNetDataset(tiny_scene["root"], "test", None, N_VIEWS, 2, source_path=os.path.join(tiny_scene["root"], "nowhere"),
                       device="cpu")[0]

"""GPU: view preparation (csrc/prepare_views.hip) is PIL's resize + the float conversion bit for bit — against a committed
PIL result and against the numpy restatement (tests/views_ref.py) at the kernel's edges — and PrepareViews stands for
ResizeImage + ToTensor in the sample pipeline without changing a value.  Exact equality throughout, no tolerance."""
import os

import numpy as np
import pytest

import views_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(frames, out_hw, pad=(0, 0)):
    from eprecon_amd.transforms import prepare_views
    return prepare_views(dev(frames), (out_hw[1], out_hw[0]), pad[0], pad[1])


def check(frames, out_hw, pad=(0, 0)):
    got = run(frames, out_hw, pad)
    want = R.prepare_views(frames, out_hw, pad[0], pad[1])
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def noise(v, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (v, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("case", ["strip", "strip_padded", "upscale"])
def test_golden_pil_results(case):
    """V = 2: the committed frame, and the same frame with its channels reversed (resampled independently, so PIL's result
    for it is the committed one with the channels reversed: tests/test_views_host.py)"""
    with np.load(GOLDEN) as z:
        frame, pad, resized = z[case + "/frame"], z[case + "/pad"], z[case + "/resized"]
    frames = np.stack([frame, frame[..., ::-1]])
    want = np.stack([resized, resized[..., ::-1]]).transpose(0, 3, 1, 2).astype(np.float32)
    got = run(frames, resized.shape[:2], (int(pad[0]), int(pad[1])))
    assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize("shape", [
    (83, 131, 37, 70),      # output no multiple of the 64 x 16 tile in either axis, more than one tile in both
    (9, 11, 4, 5),          # smaller than one tile
    (50, 64, 24, 64),       # one axis only
    (48, 64, 48, 64),       # identity
    (30, 40, 48, 64),       # up-scaling
    (160, 256, 40, 64),     # the accepted limit, 9 taps per axis
], ids=lambda s: "{}x{}to{}x{}".format(*s))
def test_shapes_against_restatement(shape):
    in_h, in_w, out_h, out_w = shape
    check(noise(2, in_h, in_w, seed=in_h), (out_h, out_w))


@pytest.mark.parametrize("views", [1, 9])
def test_view_counts(views):
    check(noise(views, 61, 83, seed=views), (48, 64))


@pytest.mark.parametrize("pad", [(0, 0), (2, 2), (3, 0)])
def test_padding_rows_are_black_and_never_read(pad):
    check(noise(2, 77, 131, seed=pad[0]), (40, 70), pad)


def test_saturated_and_checkerboard_frames():
    """all 255: the accumulator's headroom and the clamp (every output exactly 255); a one-pixel 0 / 255 checkerboard: the
    largest tap-to-tap swings"""
    white = np.full((1, 83, 131, 3), 255, np.uint8)
    check(white, (37, 70))
    assert bool((run(white, (37, 70)) == 255).all())
    check(white, (37, 70), (2, 2))
    y, x = np.mgrid[0:83, 0:131]
    board = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)
    board[..., 1] = 255 - board[..., 1]
    check(board, (37, 70))
    check(board, (83, 131))


def test_scale_above_four_raises():
    from eprecon_amd.transforms import prepare_views
    with pytest.raises(ValueError):
        prepare_views(dev(noise(1, 161, 64)), (64, 40))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 640 * 480])
def test_depth_to_metres(n):
    from eprecon_amd.transforms import depth_to_metres
    mm = np.random.default_rng(n).integers(0, 65536, n).astype(np.uint16)
    edge = np.array([0, 1, 2999, 3000, 3001, 65535], np.uint16)
    mm[:min(n, 6)] = edge[:min(n, 6)]
    if n >= 12:
        mm[-6:] = edge
    want = R.depth_to_metres(mm)
    got = depth_to_metres(dev(mm.view(np.int16)))
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want))
    if n >= 12:
        assert want[3] == np.float32(3.0) and want[4] == 0 and want[5] == 0      # 3000 mm is kept, 3001 is not


# ------------------------------------------------------------------------------------------------------ the transform

def _sample(seed=0, sizes=((968, 1296),) * 3, depth_hw=(48, 64)):
    """a raw sample as scannet.ScanNetDataset(raw=True) hands it out: PIL colour frames, uint16 depth"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    views = len(sizes)
    k = np.array([[1170.2, 0, 647.7], [0, 1170.2, 483.8], [0, 0, 1]], np.float32)
    poses = np.stack([np.eye(4) for _ in range(views)])
    poses[:, :3, 3] = rng.normal(size=(views, 3))
    return {"imgs": [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes],
            "depth": [rng.integers(0, 6000, depth_hw).astype(np.uint16) for _ in range(views)],
            "intrinsics": np.stack([k] * views), "extrinsics": poses,
            "vol_origin": np.zeros(3, np.float32), "scene": "scene0000_00", "fragment": "scene0000_00_0", "epoch": [0]}


def _host_form(sample):
    """the same sample as raw=False hands it out: the depth in float32 metres"""
    out = dict(sample, imgs=list(sample["imgs"]), intrinsics=sample["intrinsics"].copy(), extrinsics=sample["extrinsics"].copy())
    out["depth"] = [R.depth_to_metres(d) for d in sample["depth"]]
    return out


@pytest.mark.parametrize("sizes", [((968, 1296),) * 2, ((97, 131), (61, 83), (97, 131))], ids=["scannet", "mixed"])
def test_prepare_views_equals_resize_image_and_to_tensor(sizes):
    pytest.importorskip("PIL")
    from eprecon_amd import transforms as T
    size = (64, 48) if sizes[0] != (968, 1296) else (640, 480)
    depth_hw = (size[1], size[0])
    raw = _sample(1, sizes, depth_hw)
    host = T.ToTensor()(T.ResizeImage(size)(_host_form(raw)))
    stage = T.PrepareViews(size)
    for _ in range(2):                       # the second call reuses the pinned buffer and the cached tables
        got = stage(dict(raw, imgs=list(raw["imgs"]), intrinsics=raw["intrinsics"].copy(), extrinsics=raw["extrinsics"].copy()))
        assert got["imgs"].is_cuda and got["depth"].is_cuda
        assert torch.equal(got["imgs"].cpu(), host["imgs"])
        assert torch.equal(got["depth"].cpu(), host["depth"])
        assert torch.equal(got["intrinsics"], host["intrinsics"]) and torch.equal(got["extrinsics"], host["extrinsics"])
    # uint8 arrays instead of PIL images, float depth passed through as ToTensor does
    arrays = dict(_host_form(raw), imgs=[np.asarray(i) for i in raw["imgs"]])
    got = stage(arrays)
    assert torch.equal(got["imgs"].cpu(), host["imgs"]) and not got["depth"].is_cuda and torch.equal(got["depth"], host["depth"])


def test_prepare_views_refuses_a_scale_above_four():
    pytest.importorskip("PIL")
    from eprecon_amd import transforms as T
    raw = _sample(2, ((97, 131),), (8, 8))
    with pytest.raises(ValueError):
        T.PrepareViews((32, 24))(raw)


def test_full_pipelines_agree_through_collate():
    """PrepareViews -> RandomTransformSpace -> IntrinsicsPoseToProjection -> collate_fragments against the same with
    ResizeImage + ToTensor in front, a scene's volumes attached (occupancy from the depth, the cropped targets): every
    tensor equal"""
    pytest.importorskip("PIL")
    from eprecon_amd import synthetic as S
    from eprecon_amd import transforms as T
    size, n_vox = (64, 48), (32, 24, 16)        # (the volume of tests/test_transforms_gpu.py)
    window = S.make_window(seed=0, width=64, height=48, n_vox=n_vox)
    raw = _sample(3, ((97, 131),) * 9, (48, 64))
    raw["intrinsics"] = np.stack([window["intrinsics"] * np.array([[131 / 64], [97 / 48], [1]], np.float32)] * 9).astype(np.float32)
    raw["extrinsics"] = window["poses"].astype(np.float64)
    raw["depth"] = [np.round(S.render_depth(window, v) * 1000).astype(np.uint16) for v in range(9)]
    raw["vol_origin"] = window["vol_origin"]
    volumes = [S.analytic_tsdf(dict(window, vol_origin_partial=window["vol_origin"]), l) for l in range(3)]
    scene = T.SceneVolumes(volumes)
    results = []
    for head, sample in (([T.PrepareViews(size)], raw), ([T.ResizeImage(size), T.ToTensor()], _host_form(raw))):
        torch.manual_seed(0)
        tf = T.Compose(head + [T.RandomTransformSpace(n_vox, 0.04, False, False, 0, 0, max_epoch=1),
                               T.IntrinsicsPoseToProjection(9, 4)])
        sample = dict(sample, imgs=list(sample["imgs"]), intrinsics=sample["intrinsics"].copy(), tsdf_list_full=scene, epoch=[0])
        results.append(T.collate_fragments([tf(sample)]))
    device_way, host_way = results
    assert sorted(device_way) == sorted(host_way)
    for key, a in device_way.items():
        b = host_way[key]
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), key
        elif isinstance(a, list) and a and torch.is_tensor(a[0]):
            assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b)), key
        else:
            assert a == b, key
    assert device_way["imgs"].shape == (1, 9, 3, 48, 64) and "occ_list" in device_way and "tsdf_list" in device_way

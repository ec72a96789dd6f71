"""GPU: python -m eprecon_amd.reconstruct walks a scene on disk into a saved scene, and preparing the views on the device
instead of the host changes no value of it."""
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCENE = "scene0707_00"
N_FRAGMENTS, N_VIEWS = 2, 9
WIDTH, HEIGHT = 320, 240          # what tests/test_neucon_gpu.py runs NeuralRecon.forward at, in the default 96^3 volume


def write_scene(root):
    """two consecutive fragments of the analytic room (eprecon_amd.synthetic) in the ScanNet layout: 640 x 480 colour JPEGs
    (the network sees them at 320 x 240), 320 x 240 depth PNGs in millimetres sphere-traced from the fragment's poses, pose
    and intrinsic text files, the fragment list and the room's TSDF volumes at three levels"""
    from PIL import Image
    from eprecon_amd import synthetic as S
    frames = os.path.join(root, "scans_test", SCENE)
    for d in ("color", "depth", "pose", "intrinsic"):
        os.makedirs(os.path.join(frames, d))
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:2 * HEIGHT, 0:2 * WIDTH]
    pattern = np.stack([x % 256, (y * 2) % 256, (x + y) // 5 % 256], -1).astype(np.uint8)
    metas = []
    for f in range(N_FRAGMENTS):
        window = S.make_window(seed=f, width=WIDTH, height=HEIGHT, advance=0.32 * f)
        if f == 0:
            k4 = np.eye(4)
            k4[:3, :3] = window["intrinsics"]
            k4[:2] *= 2                                   # the colour frames are twice the size
            np.savetxt(os.path.join(frames, "intrinsic", "intrinsic_color.txt"), k4, delimiter=" ")
            tsdf_dir = os.path.join(root, f"all_tsdf_{N_VIEWS}_1", SCENE)
            os.makedirs(tsdf_dir)
            for l in range(3):
                np.savez(os.path.join(tsdf_dir, f"full_tsdf_layer{l}.npz"),
                         S.analytic_tsdf(dict(window, vol_origin_partial=window["vol_origin"]), l))
        # (the depth is traced at half the size and every pixel repeated 2 x 2: a quarter of the rays, and all this test needs)
        coarse = dict(S.make_window(seed=f, width=WIDTH // 2, height=HEIGHT // 2, advance=0.32 * f), poses=window["poses"])
        ids = [f * N_VIEWS + v for v in range(N_VIEWS)]
        for v, vid in enumerate(ids):
            colour = np.roll(pattern, 37 * vid, axis=1) ^ rng.integers(0, 32, pattern.shape, dtype=np.uint8)
            Image.fromarray(colour).save(os.path.join(frames, "color", f"color_{vid}.jpg"))
            depth = np.repeat(np.repeat(S.render_depth(coarse, v), 2, axis=0), 2, axis=1)
            Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(os.path.join(frames, "depth", f"depth_{vid}.png"))
            np.savetxt(os.path.join(frames, "pose", f"pose_{vid}.txt"), window["poses"][v])
        metas.append({"scene": SCENE, "fragment_id": f, "image_ids": ids, "vol_origin": window["vol_origin"]})
    with open(os.path.join(root, f"all_tsdf_{N_VIEWS}_1", "fragments_test.pkl"), "wb") as fh:
        pickle.dump(metas, fh)


def test_device_and_host_views_write_the_same_scene(tmp_path, capsys):
    pytest.importorskip("PIL")
    from eprecon_amd import reconstruct
    root = str(tmp_path / "data")
    write_scene(root)
    written = {}
    for name, extra in (("device", []), ("host", ["--host-views"])):
        out = str(tmp_path / name)
        assert reconstruct.main(["--data_path", root, "--out", out, "--size", str(WIDTH), str(HEIGHT)] + extra) == 0
        path = os.path.join(out, "scene_scannet_fusion_eval_0", SCENE + ".npz")
        assert os.path.exists(path), sorted(os.listdir(out))
        with np.load(path) as z:
            written[name] = {k: z[k] for k in z.files}
    log = capsys.readouterr().out
    assert "UNTRAINED" in log and log.count(f"{SCENE}: {N_FRAGMENTS} fragments") == 2 and "fragments/s" in log
    device_way, host_way = written["device"], written["host"]
    assert sorted(device_way) == sorted(host_way) and {"origin", "voxel_size", "tsdf", "semantic", "instance"} <= set(device_way)
    assert (device_way["tsdf"] != 1).sum() > 500          # a scene, not an empty volume
    for key in device_way:
        assert device_way[key].dtype == host_way[key].dtype and np.array_equal(device_way[key], host_way[key]), key

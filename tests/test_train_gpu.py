"""GPU: python -m eprecon_amd.train walks a training scene on disk — epochs, accumulation, checkpoints, resume — and its
checkpoint loads into eprecon_amd.reconstruct's model."""
import contextlib
import io
import json
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCENE = "scene0000_00"
N_FRAGMENTS, N_VIEWS = 3, 9
WIDTH, HEIGHT = 320, 240
LR, LREPOCHS = 1e-4, "2,3:10"          # milestones inside the three epochs run here
SCENE_ORIGIN = np.array([-2.56, -1.6, -0.64], np.float32)
SCENE_DIMS = (128, 128, 112)           # 5.12 x 5.12 x 4.48 m around the 3.84 m fragments: room for the augmentation's crop
FROZEN_PREFIXES = ("backbone2d.", "neucon_net.initialization.")


def write_scene(root):
    """three consecutive fragments of the analytic room (eprecon_amd.synthetic) in the ScanNet layout, train mode: 640 x 480
    colour JPEGs (the network sees them at 320 x 240), depth PNGs in millimetres, pose and intrinsic text files,
    fragments_train.pkl and the room's TSDF, colour, semantic and instance volumes at three levels"""
    from PIL import Image
    from eprecon_amd import synthetic as S
    frames = os.path.join(root, "scans", SCENE)
    for d in ("color", "depth", "pose", "intrinsic"):
        os.makedirs(os.path.join(frames, d))
    volumes = os.path.join(root, f"all_tsdf_{N_VIEWS}_1", SCENE)
    os.makedirs(volumes)
    vs = S.make_window(seed=0, width=WIDTH, height=HEIGHT)["voxel_size"]
    for l in range(3):
        box = {"voxel_size": vs, "n_vox": SCENE_DIMS, "vol_origin_partial": SCENE_ORIGIN}
        tsdf = S.analytic_tsdf(box, l)
        semantic, instance = S.analytic_panoptic(box, l)
        np.savez(os.path.join(volumes, f"full_tsdf_layer{l}.npz"), tsdf)
        np.savez(os.path.join(volumes, f"full_rgb_layer{l}.npz"), np.full(tsdf.shape + (3,), 128, np.uint8))
        np.savez(os.path.join(volumes, f"full_semantic_layer_interpolate{l}.npz"), semantic.astype(np.int32))
        np.savez(os.path.join(volumes, f"full_instance_layer_interpolate{l}.npz"), instance.astype(np.int32))
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
        # (the depth is traced at half the size and every pixel repeated 2 x 2: a quarter of the rays)
        coarse = dict(S.make_window(seed=f, width=WIDTH // 2, height=HEIGHT // 2, advance=0.32 * f), poses=window["poses"])
        ids = [f * N_VIEWS + v for v in range(N_VIEWS)]
        for v, vid in enumerate(ids):
            colour = np.roll(pattern, 37 * vid, axis=1) ^ rng.integers(0, 32, pattern.shape, dtype=np.uint8)
            Image.fromarray(colour).save(os.path.join(frames, "color", f"color_{vid}.jpg"))
            depth = np.repeat(np.repeat(S.render_depth(coarse, v), 2, axis=0), 2, axis=1)
            Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(os.path.join(frames, "depth", f"depth_{vid}.png"))
            np.savetxt(os.path.join(frames, "pose", f"pose_{vid}.txt"), window["poses"][v])
        metas.append({"scene": SCENE, "fragment_id": f, "image_ids": ids, "vol_origin": SCENE_ORIGIN})
    with open(os.path.join(root, f"all_tsdf_{N_VIEWS}_1", "fragments_train.pkl"), "wb") as fh:
        pickle.dump(metas, fh)


def run_train(argv):
    from eprecon_amd import train
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = train.main(argv)
    print(out.getvalue())
    return rc, out.getvalue()


def common(root, logdir):
    return ["--data_path", root, "--logdir", logdir, "--size", str(WIDTH), str(HEIGHT), "--batch_size", "1",
            "--accumulation_steps", "2", "--save_freq", "1", "--summary_freq", "1", "--lr", str(LR), "--lrepochs", LREPOCHS]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    pytest.importorskip("PIL")
    base = tmp_path_factory.mktemp("train")
    root, logdir = str(base / "data"), str(base / "log")
    write_scene(root)
    rc, log = run_train(common(root, logdir) + ["--epochs", "2"])
    return {"root": root, "logdir": logdir, "rc": rc, "log": log}


def initial_parameters(epochs):
    """the seeded initial values train.main starts from: the same draws in the same order"""
    from eprecon_amd import train
    from eprecon_amd.neuralrecon import NeuralRecon
    torch.manual_seed(0)
    cfg = train.RunCfg("unused")
    train.build_transforms(cfg, N_VIEWS, (WIDTH, HEIGHT), epochs, torch.device("cuda"))
    return dict(NeuralRecon(cfg).named_parameters())


def test_two_epochs_write_checkpoints_and_scalars(trained):
    from eprecon_amd.train import lr_at
    assert trained["rc"] == 0
    logdir = trained["logdir"]
    assert {"model_000000.ckpt", "model_000001.ckpt", "train_scalars.jsonl"} <= set(os.listdir(logdir))
    assert "start at epoch 0" in trained["log"] and f"Iter 2/{N_FRAGMENTS}, train loss" in trained["log"]
    assert f"Current learning rate: {lr_at(1, LR, LREPOCHS)}" in trained["log"]
    with open(os.path.join(logdir, "train_scalars.jsonl")) as fh:
        records = [json.loads(line) for line in fh]
    assert records and all(np.isfinite(r["total_loss"]) and r["total_loss"] > 0 for r in records)
    assert records[-1]["optimizer_steps"] >= 1
    norms = [r["grad_norm"] for r in records if r["grad_norm"] is not None]
    assert norms and all(np.isfinite(n) and n > 0 for n in norms)
    assert records[-1]["lr"] == lr_at(1, LR, LREPOCHS) and records[0]["lr"] == LR

    initial = initial_parameters(2)
    for epoch in (0, 1):
        state = torch.load(os.path.join(logdir, f"model_{epoch:06d}.ckpt"), map_location="cpu", weights_only=False)
        assert set(state) == {"epoch", "model", "optimizer"} and state["epoch"] == epoch
        assert all(k.startswith("module.") for k in state["model"])
        names = [n for n in initial]
        assert {"module." + n for n in names} <= set(state["model"])
        trainable = [n for n in names if not n.startswith(FROZEN_PREFIXES)]
        assert 0 < len(trainable) < len(names)
        group, = state["optimizer"]["param_groups"]
        assert len(group["params"]) == len(trainable)                 # the optimiser holds exactly the trainable parameters
        held = state["optimizer"]["state"]
        assert held and set(held) <= set(group["params"])
        assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in held.values())
    changed = 0
    for n in names:
        now, then = state["model"]["module." + n], initial[n].detach()
        if n.startswith(FROZEN_PREFIXES):
            assert torch.equal(now, then), n
        else:
            changed += int(not torch.equal(now, then))
    assert changed >= 1


def test_resume_continues_at_the_next_epoch(trained):
    from eprecon_amd.train import lr_at
    rc, log = run_train(common(trained["root"], trained["logdir"]) + ["--epochs", "3", "--resume"])
    assert rc == 0
    assert "resuming" in log and "model_000001.ckpt" in log and "start at epoch 2" in log
    assert "Epoch 2:" in log and "Epoch 1:" not in log and "Epoch 3:" not in log
    assert lr_at(2, LR, LREPOCHS) == pytest.approx(LR / 100)
    assert f"Current learning rate: {lr_at(2, LR, LREPOCHS)}" in log
    assert os.path.exists(os.path.join(trained["logdir"], "model_000002.ckpt"))
    before = torch.load(os.path.join(trained["logdir"], "model_000001.ckpt"), map_location="cpu", weights_only=False)
    after = torch.load(os.path.join(trained["logdir"], "model_000002.ckpt"), map_location="cpu", weights_only=False)
    assert after["epoch"] == 2
    # the moments came along: the step counts go on from the checkpoint's
    top = lambda s: max(float(v["step"]) for v in s["optimizer"]["state"].values())
    assert top(after) > top(before) >= 1


def test_checkpoint_loads_into_reconstruct(trained):
    from eprecon_amd import reconstruct, train
    from eprecon_amd.neuralrecon import NeuralRecon
    model = NeuralRecon(train.RunCfg("unused"))
    assert reconstruct.load_checkpoint(model, os.path.join(trained["logdir"], "model_000001.ckpt")) == 1


def test_torch_optimizer_runs_to_max_steps(trained, tmp_path):
    logdir = str(tmp_path / "log_torch")
    rc, log = run_train(common(trained["root"], logdir) + ["--epochs", "2", "--optimizer", "torch", "--max_steps", "2",
                                                           "--freeze", "none"])
    assert rc == 0 and "2 batches, 1 optimiser steps" in log and "Iter 1/3" in log and "Iter 2/3" not in log
    assert not [n for n in os.listdir(logdir) if n.endswith(".ckpt")]       # stopped inside epoch 0

"""GPU: a scene through the sample transforms (eprecon_amd/transforms.py) into NeuConNet.forward under autograd.

(A module of its own, named so that it is collected in front of tests/test_switches_gpu.py and tests/test_training_gpu.py: the
network built here captures and replays NEW HIP graphs while its occupancy heads are calibrated, and a new capture + replay in
a process that has been through RCCL process-group set-up and tear-down several times can crash inside the runtime's graph
launch in the whole-suite order, see test_training_step_on_a_batch_of_two_windows there.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eprecon_amd import synthetic as S  # noqa: E402
from eprecon_amd import transforms as T  # noqa: E402


# modules of this suite that set up and tear down an RCCL process group inside the test process
RCCL_MODULES = ("test_cfg4_gpu", "test_switches_gpu", "test_training_gpu")


def test_pipeline_feeds_the_network_under_autograd(request):
    """a scene built from `synthetic` (analytic TSDF and labels over a box larger than the fragment, rendered depths) through
    Compose([ToTensor, RandomTransformSpace, IntrinsicsPoseToProjection]) and collate_fragments into NeuConNet.forward with
    autograd on: the five finite losses of tests/test_training_gpu.py, and a gradient at the image features"""
    # the order this module's name buys is asserted, not assumed: at most one of the RCCL modules may have run in front of
    # this test (as for every other module that builds a network); selection, reordering or a rename fails here, by name
    items = request.session.items
    before = {it.module.__name__.rsplit(".", 1)[-1] for it in items[:items.index(request.node)]}
    assert len(before & set(RCCL_MODULES)) <= 1, f"runs after {sorted(before & set(RCCL_MODULES))}: see the module docstring"
    from eprecon_amd.config import ModelCfg
    from eprecon_amd.fragment_step import TrainStep, calibrate_occupancy_heads, seed_subsampling
    from eprecon_amd.neucon_network import NeuConNet
    h, w = 240, 320
    window = S.make_window(seed=0, width=w, height=h)
    vs = window["voxel_size"]
    scene_origin = np.array([-2.56, -1.6, -0.64], np.float32)
    dims0 = (128, 128, 112)                                   # 5.12 x 5.12 x 4.48 m around the 3.84 m fragment
    tsdf, rgb, sem, ins = [], [], [], []
    for l in range(3):
        box = {"voxel_size": vs, "n_vox": dims0, "vol_origin_partial": scene_origin}
        tsdf.append(S.analytic_tsdf(box, l))
        s_l, i_l = S.analytic_panoptic(box, l)
        sem.append(s_l.astype(np.int32))
        ins.append(i_l.astype(np.int32))
        rgb.append(np.zeros(tsdf[-1].shape + (3,), np.float32))
    scene = T.SceneVolumes(tsdf, rgb, sem, ins)
    sample = {
        "imgs": [np.zeros((h, w, 3), np.float32) for _ in range(9)],
        "depth": [S.render_depth(window, v, max_depth=3.0) for v in range(9)],
        "intrinsics": np.stack([window["intrinsics"]] * 9), "extrinsics": window["poses"].copy(),
        "tsdf_list_full": scene, "vol_origin": scene_origin, "scene": "scene0000", "fragment": "scene0000_0", "epoch": [0],
    }
    torch.manual_seed(0)
    pipe = T.Compose([T.ToTensor(), T.RandomTransformSpace(window["n_vox"], vs, False, False, 0, 0, max_epoch=1),
                      T.IntrinsicsPoseToProjection(9, 4)])
    inputs = T.collate_fragments([pipe(sample)])
    assert inputs["tsdf_list"][0].shape == (1, 96, 96, 96) and inputs["proj_matrices"].shape == (1, 9, 3, 4, 4)
    band = [float((t.abs() < 1).float().mean()) for t in inputs["tsdf_list"]]
    occ = [float(o.float().mean()) for o in inputs["occ_list"]]
    print("in-band share per level", band, "occupied share per level", occ)
    assert min(band) > 0.01 and min(occ) > 0.001 and int(inputs["instance_list"][0].max()) >= 5

    f1, f2, _ = S.make_model_inputs([window], feat_seed=0, scene="scene0000")
    dev = torch.device("cuda")
    f1, f2 = S.to_device(f1, dev), S.to_device(f2, dev)
    torch.manual_seed(4321)
    net = NeuConNet(ModelCfg()).to(dev)
    net.train()
    calibrate_occupancy_heads(net, f1, f2, inputs)
    for views in (f1, f2):
        for levels in views:
            for t in levels:
                t.requires_grad_()
    net.gru_fusion.scene_name = [None, None, None]
    seed_subsampling(0)
    outputs, losses = net(f1, f2, inputs, {})
    total = sum(v * TrainStep.LW[min(i, 3)] for i, v in enumerate(losses.values()))
    losses["total_loss"] = total
    assert "coords" in outputs and outputs["coords"].shape[0] > 500
    assert set(losses) == {"tsdf_occ_loss_0", "tsdf_occ_loss_1", "tsdf_occ_loss_2", "panoptic_loss", "total_loss"}
    assert all(torch.isfinite(v).all() and float(v.detach()) > 0 for v in losses.values()), losses
    total.backward()
    grads = [levels[0].grad for levels in f2]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0

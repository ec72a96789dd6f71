"""Train from disk — the reference's train() (main.py:95-166, 183-348) as a tool:

    python -m eprecon_amd.train --data_path DIR [--source_path DIR] --logdir DIR [--epochs 100] [--batch_size 4] \\
           [--accumulation_steps 8] [--lr 1e-4] [--wd 0] [--lrepochs 70,90:10] [--save_freq 1] [--summary_freq 20] \\
           [--resume] [--loadckpt FILE] [--freeze init|mnasnet|none] [--optimizer fused|torch] [--n_views 9] \\
           [--size 640 480] [--seed 0] [--scenes FILE] [--max_steps N]

reads <data_path>/all_tsdf_<n_views>_1/fragments_train.pkl (eprecon_amd.generate_gt writes it), the frames it names and the
scenes' TSDF, colour and label volumes (scannet.ScanNetDataset in train mode), and walks the fragments in file order,
batch_size at a time: PrepareViews -> RandomTransformSpace (rotation and translation drawn per epoch, main.py:98-103) ->
IntrinsicsPoseToProjection(n_views, 4) -> collate_fragments -> NeuralRecon.forward under autograd -> backward.  A batch whose
total loss is 0 is skipped; every accumulation_steps kept batches the gradients (summed, not averaged: main.py:306) are
clipped at norm 1 and Adam steps.  The learning rate follows lr_at; <logdir>/model_<epoch:06d>.ckpt is written every
save_freq epochs as {'epoch', 'model' (keys with the 'module.' prefix of the reference's wrapped model), 'optimizer'} —
a --ckpt for eprecon_amd.reconstruct, and a file the reference loads.  --resume continues from the highest-numbered
checkpoint of --logdir at its epoch + 1, optimiser moments included; --loadckpt loads a model only.

The frames of the next batch are read and decoded on up to 9 threads while the current step runs.  With WORLD_SIZE > 1
(torchrun) the model is wrapped in DistributedDataParallel over RCCL and every rank walks its own contiguous block of the
fragment list (rank_indices); rank 0 logs and saves.
"""
import argparse
import json
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import transforms as T
from .config import ModelCfg
from .scannet import ScanNetDataset
from .scene_io import read_scene_list

MAX_READERS = 9       # never sized from the machine
LW = (1.0, 0.8, 0.64, 1.2)           # config/train.yaml:44
# config/default.py:31-34: TRAIN.RANDOM_ROTATION_3D, RANDOM_TRANSLATION_3D, PAD_XY_3D, PAD_Z_3D
RANDOM_ROTATION_3D, RANDOM_TRANSLATION_3D, PAD_XY_3D, PAD_Z_3D = True, True, .1, .025


class RunCfg:
    """what NeuralRecon reads of the reference's config node"""

    def __init__(self, logdir):
        self.MODEL = ModelCfg()
        self.MODEL.LW = list(LW)
        self.DATASET = "scannet"
        self.LOGDIR = logdir


def parse_lrepochs(lrepochs):
    """'70,90:10' -> ([70, 90], 0.1)   (main.py:250-251)"""
    head, down = lrepochs.split(':')
    return [int(e) for e in head.split(',')], 1 / float(down)


def lr_at(epoch, lr, lrepochs):
    """The learning rate of epoch `epoch` in the reference's call order: MultiStepLR is constructed with
    last_epoch = start_epoch - 1 and stepped at the TOP of every epoch (main.py:252-257), so during epoch e it stands at
    e + 1 and every milestone m <= e + 1 has been applied — one epoch earlier than the milestones read."""
    milestones, gamma = parse_lrepochs(lrepochs)
    value = lr
    for m in sorted(milestones):
        if m <= epoch + 1:
            value = value * gamma
    return value


def rank_indices(n, world, rank):
    """datasets/sampler.py:40-76 without shuffling: the n fragments padded to a multiple of `world` by wrapping around, then
    cut into CONTIGUOUS blocks, one per rank (not strided): a rank walks consecutive fragments of a scene."""
    per_rank = (n + world - 1) // world
    padded = [i % n for i in range(per_rank * world)]
    return padded[per_rank * rank:per_rank * (rank + 1)]


def checkpoint_name(epoch):
    return "model_{:0>6}.ckpt".format(epoch)


def latest_checkpoint(names):
    """the highest-numbered model_<n>.ckpt of `names` (main.py:187-191 sorts by the number, not the text), or None"""
    found = [(int(m.group(1)), name) for name in names for m in [re.fullmatch(r"model_(\d+)\.ckpt", name)] if m]
    return max(found)[1] if found else None


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="train on the fragments of a ScanNet-layout dataset on disk")
    ap.add_argument("--data_path", required=True, help="directory holding all_tsdf_<n_views>_1/ (generate_gt's output)")
    ap.add_argument("--source_path", help="directory of the <scene>/{color,depth,pose,intrinsic} frames (default: <data_path>/scans)")
    ap.add_argument("--logdir", required=True, help="checkpoints and train_scalars.jsonl go here")
    ap.add_argument("--epochs", default=100, type=int)
    ap.add_argument("--batch_size", default=4, type=int)
    ap.add_argument("--accumulation_steps", default=8, type=int)
    ap.add_argument("--lr", default=1e-4, type=float)
    ap.add_argument("--wd", default=0.0, type=float)
    ap.add_argument("--lrepochs", default="70,90:10", help="milestone epochs and the divisor applied at each")
    ap.add_argument("--save_freq", default=1, type=int)
    ap.add_argument("--summary_freq", default=20, type=int)
    ap.add_argument("--resume", action="store_true", help="continue from the highest-numbered checkpoint of --logdir")
    ap.add_argument("--loadckpt", help="load this checkpoint's model (ignored when --resume finds one)")
    ap.add_argument("--freeze", default="init", choices=["none", "mnasnet", "init"],
                    help="init: backbone2d and neucon_net.initialization (what the reference hard-codes); mnasnet: the first six "
                         "layers of backbone2d.conv0")
    ap.add_argument("--optimizer", default="fused", choices=["fused", "torch"])
    ap.add_argument("--n_views", default=9, type=int)
    ap.add_argument("--size", default=[640, 480], type=int, nargs=2, metavar=("W", "H"), help="image size the network sees")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--scenes", help="text file, one scene name per line: only these scenes")
    ap.add_argument("--max_steps", type=int, help="stop after this many batches")
    return ap.parse_args(argv)


def build_transforms(cfg, n_views, size, epochs, device):
    return T.Compose([
        T.PrepareViews(size, device=device),
        T.RandomTransformSpace(cfg.MODEL.N_VOX, cfg.MODEL.VOXEL_SIZE, RANDOM_ROTATION_3D, RANDOM_TRANSLATION_3D, PAD_XY_3D,
                               PAD_Z_3D, max_epoch=epochs, device=device),
        T.IntrinsicsPoseToProjection(n_views, 4)])


def freeze(net, what):
    """main.py:221-230"""
    if what == "mnasnet":
        frozen = list(net.backbone2d.conv0[:6].parameters())
    elif what == "init":
        frozen = list(net.backbone2d.parameters()) + list(net.neucon_net.initialization.parameters())
    else:
        frozen = []
    for p in frozen:
        p.requires_grad = False
    return len(frozen)


def load_model(net, state):
    """a checkpoint's 'model' (keys with or without 'module.') into the bare network, strictly; the layers' packed weight
    copies are dropped, since a load writes through .data"""
    from .sparse import clear_packed_weights
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    net.load_state_dict(sd, strict=True)
    clear_packed_weights(net)


def main(argv=None):
    args = parse_args(argv)
    from .neuralrecon import NeuralRecon
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if distributed:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl")        # RCCL
    device = torch.device("cuda", torch.cuda.current_device())
    main_process = rank == 0
    log = (lambda *a: print("[train]", *a, flush=True)) if main_process else (lambda *a: None)

    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    cfg = RunCfg(args.logdir)
    dataset = ScanNetDataset(args.data_path, "train", build_transforms(cfg, args.n_views, tuple(args.size), args.epochs, device),
                             args.n_views, len(cfg.MODEL.THRESHOLDS) - 1, source_path=args.source_path, raw=True, device=device)
    if args.scenes:
        wanted = set(read_scene_list(args.scenes))
        dataset.metas = [m for m in dataset.metas if m["scene"] in wanted]
    if len(dataset) == 0:
        raise SystemExit("no fragment to train on")
    indices = rank_indices(len(dataset), world, rank)
    batches = [indices[i:i + args.batch_size] for i in range(0, len(indices) - args.batch_size + 1, args.batch_size)]  # drop_last
    if not batches:
        raise SystemExit(f"{len(indices)} fragments per rank do not fill one batch of {args.batch_size}")

    net = NeuralRecon(cfg).to(device)
    os.makedirs(args.logdir, exist_ok=True)
    start_epoch, resumed = 0, None
    if args.resume:
        name = latest_checkpoint(os.listdir(args.logdir))
        if name is not None:
            log("resuming " + os.path.join(args.logdir, name))
            resumed = torch.load(os.path.join(args.logdir, name), map_location="cpu", weights_only=False)
            load_model(net, resumed["model"])
            start_epoch = int(resumed["epoch"]) + 1
    if resumed is None and args.loadckpt:
        log("loading model {}".format(args.loadckpt))
        load_model(net, torch.load(args.loadckpt, map_location="cpu", weights_only=False)["model"])
    n_frozen = freeze(net, args.freeze)

    model = net
    if distributed:
        from torch.nn.parallel import DistributedDataParallel
        model = DistributedDataParallel(net, device_ids=[local_rank], output_device=local_rank, broadcast_buffers=False,
                                        find_unused_parameters=True)
    # the optimiser holds the trainable parameters only: its state_dict is theirs, in the order of net.parameters()
    trainable = [p for p in net.parameters() if p.requires_grad]
    if args.optimizer == "fused":
        from .optim import FusedAdam
        optimizer = FusedAdam(trainable, lr=args.lr, betas=(0.9, 0.999), weight_decay=args.wd)
    else:
        optimizer = torch.optim.Adam(trainable, lr=args.lr, betas=(0.9, 0.999), weight_decay=args.wd)
    if resumed is not None:
        optimizer.load_state_dict(resumed["optimizer"])      # (the moments too; the lr below is lr_at's, not the file's)
    del resumed
    log("start at epoch {}".format(start_epoch))
    log("Number of model parameters: {} M ({} tensors frozen by --freeze {})".format(
        sum(p.data.nelement() for p in net.parameters()) / 1e6, n_frozen, args.freeze))

    scalars_path = os.path.join(args.logdir, "train_scalars.jsonl")
    steps_run, optimizer_steps, stop = 0, 0, False
    last_norm = None           # device scalar of the last optimiser step; read only beside the losses
    with ThreadPoolExecutor(max_workers=min(MAX_READERS, max(1, args.n_views * args.batch_size)),
                            thread_name_prefix="eprecon-read") as pool:
        def start(batch):
            return [[pool.submit(dataset.read_view, dataset.metas[idx], vid) for vid in dataset.metas[idx]["image_ids"]]
                    for idx in batch]

        for epoch_idx in range(start_epoch, args.epochs):
            if stop:
                break
            log("Epoch {}:".format(epoch_idx))
            lr = lr_at(epoch_idx, args.lr, args.lrepochs)
            optimizer.param_groups[0]["lr"] = lr
            log("Current learning rate:", lr)
            dataset.epoch = epoch_idx
            dataset.tsdf_cashe = {}
            optimizer.zero_grad()          # (a partial accumulation of the last epoch is dropped, main.py:261)
            step_count = 0
            model.train()
            pending = start(batches[0])
            for batch_idx, batch in enumerate(batches):
                if args.max_steps is not None and steps_run >= args.max_steps:
                    stop = True
                    for sample in pending:
                        for f in sample:
                            f.cancel()
                    break
                global_step = len(batches) * epoch_idx + batch_idx
                do_summary = global_step % args.summary_freq == 0
                start_time = time.time()
                frames = [[f.result() for f in sample] for sample in pending]
                pending = start(batches[batch_idx + 1]) if batch_idx + 1 < len(batches) else []       # the look-ahead: one batch
                samples = [dataset.make_item(idx, dataset.stack_views(views)) for idx, views in zip(batch, frames)]
                inputs = T.collate_fragments(samples, device=device)
                steps_run += 1
                outputs, loss_dict = model(inputs)
                total = loss_dict["total_loss"]
                loss = float(total.detach()) if torch.is_tensor(total) else float(total)        # (the read main.py:303 makes)
                if loss == 0:
                    continue
                total.backward()
                step_count += 1
                if step_count % args.accumulation_steps == 0:
                    if args.optimizer == "fused":
                        last_norm = optimizer.clip_and_step(1.0)
                    else:
                        last_norm = torch.nn.utils.clip_grad_norm_(trainable, 1.0)
                        optimizer.step()
                        from .sparse import repack_registered
                        repack_registered()
                    optimizer.zero_grad()
                    step_count = 0
                    optimizer_steps += 1
                if do_summary and main_process:
                    # one read: the scalar losses and, beside them, the gradient norm of the last optimiser step
                    keys = [k for k, v in loss_dict.items() if torch.is_tensor(v)]
                    vals = [loss_dict[k].detach().reshape(()).float() for k in keys]
                    if last_norm is not None:
                        vals.append(last_norm.detach().reshape(()).float())
                    host = torch.stack(vals).tolist()
                    record = {"step": global_step, "epoch": epoch_idx, "lr": lr, "optimizer_steps": optimizer_steps,
                              "grad_norm": host[len(keys)] if last_norm is not None else None}
                    record.update(zip(keys, host))
                    with open(scalars_path, "a", encoding="utf-8") as fh:
                        fh.write(json.dumps(record) + "\n")
                log("Epoch {}/{}, Iter {}/{}, train loss = {:.3f}, time = {:.3f}".format(
                    epoch_idx, args.epochs, batch_idx, len(batches), loss, time.time() - start_time))
            if stop:
                break
            if (epoch_idx + 1) % args.save_freq == 0 and main_process:
                torch.save({"epoch": epoch_idx,
                            "model": {"module." + k: v for k, v in net.state_dict().items()},
                            "optimizer": optimizer.state_dict()},
                           os.path.join(args.logdir, checkpoint_name(epoch_idx)))
    log("{} batches, {} optimiser steps".format(steps_run, optimizer_steps))
    torch.cuda.synchronize(device)
    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

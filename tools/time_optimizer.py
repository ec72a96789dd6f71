"""What the last stage of an optimisation step costs — gradient clipping, Adam, the weight repack — on three paths, over
the trainable parameters of a NeuralRecon with random gradients, in one process.

    python tools/time_optimizer.py [--reps 50] [--freeze init none] [--train-steps 0] [--out FILE.json]

  a  torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (its defaults: the multi-tensor form) + sparse.repack_registered
  b  the same with Adam(fused=True)
  c  eprecon_amd.optim.FusedAdam.clip_and_step, with the one-workgroup finish launch ("c") and with every workgroup of the
     update launch re-summing the partial sums ("c_resum")

The network has run one fragment (fragment_step.E2EStep at 320 x 240), so its operand-order weight copies are registered
and every path's step ends in the same repack launch.  After warm-up, --reps repetitions between device events, the paths
alternating repetition by repetition; every entry is [median, min, max] in ms.  Launch counts are the device activities
torch.profiler records for one step of a path, device_busy_us the sum of their durations in that one step.  bytes_moved is what c must move (the norm reads the gradients; the update
reads parameter, gradient and both moments and writes parameter and both moments), over c's median against the HBM peak —
a floor, since the median also holds the repack launch.

--train-steps N: also N steps each of fragment_step.TrainStep(optimizer="torch") and ("fused") at 640 x 480, alternating
step by step, wall clock with a device synchronise (what bench.py --workload train times).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, the datasheet's


def spread(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def device_activities(fn):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    device = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    return len(device), sum(e.time_range.elapsed_us() for e in device)


def time_paths(model, freeze, reps):
    import torch
    from eprecon_amd import train
    from eprecon_amd.optim import FusedAdam
    from eprecon_amd.sparse import repack_registered
    for p in model.parameters():
        p.requires_grad = True
    train.freeze(model, freeze)
    params = [p for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = [torch.randn(p.shape, device=p.device, generator=gen) * 1e-2 for p in params]
    lr = 1e-8          # (the weights stay where they are over a few hundred steps)

    def torch_path(opt):
        def run():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
            return repack_registered()
        return run

    paths = {"a": torch_path(torch.optim.Adam(params, lr=lr)), "b": torch_path(torch.optim.Adam(params, lr=lr, fused=True))}
    fused = {"c": FusedAdam(params, lr=lr, finish="launch"), "c_resum": FusedAdam(params, lr=lr, finish="resum")}
    paths.update({k: (lambda o=o: o.clip_and_step(1.0)) for k, o in fused.items()})
    times = {k: [] for k in paths}
    for rep in range(-5, reps):
        for name, run in paths.items():
            for p, g in zip(params, grads):
                p.grad = g.clone()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            if rep >= 0:
                times[name].append(t0.elapsed_time(t1))
    out = {"freeze": freeze, "tensors": len(params), "floats": sum(p.numel() for p in params), "reps": reps,
           "ms": {k: spread(v) for k, v in times.items()}, "device_activities": {}, "device_busy_us": {}}
    for name, run in paths.items():
        for p, g in zip(params, grads):
            p.grad = g.clone()
        out["device_activities"][name], out["device_busy_us"][name] = device_activities(run)
    out["c_launches"] = fused["c"].launches              # norm, finish, update (+ the repack when weight copies are registered)
    out["c_chunks"] = fused["c"]._tables["nchunks"]
    out["c_bytes_moved"] = fused["c"].bytes_moved()
    out["c_fraction_of_hbm_peak"] = out["c_bytes_moved"] / (out["ms"]["c"][0] * 1e-3) / HBM_PEAK
    out["c_fraction_of_hbm_peak_while_busy"] = out["c_bytes_moved"] / (out["device_busy_us"]["c"] * 1e-6) / HBM_PEAK
    for p in params:
        p.grad = None
    return out


def time_train_steps(steps):
    import torch
    from eprecon_amd.fragment_step import TrainStep
    runs = {name: TrainStep(seed=0, lr=1e-6, optimizer=name) for name in ("torch", "fused")}
    times = {k: [] for k in runs}
    for rep in range(-3, steps):
        for name, s in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.run()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {"steps": steps, "ms": {k: spread(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--freeze", nargs="+", default=["init", "none"], choices=["init", "mnasnet", "none"])
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from eprecon_amd.fragment_step import E2EStep
    assert torch.cuda.is_available(), "time_optimizer needs a GPU"
    step = E2EStep(height=240, width=320, n_fragments=1)
    step.run()
    result = {"optimizer_step": [time_paths(step.model, freeze, args.reps) for freeze in args.freeze]}
    del step
    if args.train_steps:
        result["train_step"] = time_train_steps(args.train_steps)
    for row in result["optimizer_step"]:
        print(f"--freeze {row['freeze']}: {row['tensors']} tensors, {row['floats']} floats, {row['c_chunks']} chunks")
        for k, (med, lo, hi) in row["ms"].items():
            print(f"  {k:8s} {med:.3f} ms [{lo:.3f} - {hi:.3f}]   device activities per step: {row['device_activities'][k]}, "
                  f"busy {row['device_busy_us'][k]:.0f} us")
        print(f"  c moves {row['c_bytes_moved'] / 1e6:.1f} MB: {100 * row['c_fraction_of_hbm_peak']:.1f} % of the HBM peak at its median, "
              f"{100 * row['c_fraction_of_hbm_peak_while_busy']:.1f} % over the time its launches are busy (the repack among them)")
    if "train_step" in result:
        for k, (med, lo, hi) in result["train_step"]["ms"].items():
            print(f"TrainStep(optimizer={k!r}) {med:.2f} ms [{lo:.2f} - {hi:.2f}] over {result['train_step']['steps']} steps")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()

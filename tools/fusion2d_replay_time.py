"""untraced time of one feat_fusion_pre HIP-graph replay and of one cfg2 step, in one process; prints one JSON line.
    python tools/fusion2d_replay_time.py   (from the root of the tree to time)"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())   # (run from the root of the tree to time)
import torch
from eprecon_amd.fragment_step import Cfg2Step


def main():
    step = Cfg2Step(seed=0)
    net = step.init_net
    f = step.features_init
    views = [[v[lvl][0] for v in f] for lvl in (2, 1, 0)]
    with torch.no_grad():
        for _ in range(10):
            step.run()
        torch.cuda.synchronize()
        for _ in range(20):
            net._fusion_graphed(views)
        torch.cuda.synchronize()
        reps = []
        for blk in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                net._fusion_graphed(views)
            b.record()
            torch.cuda.synchronize()
            reps.append(a.elapsed_time(b) / 200 * 1e3)
        steps = []
        for blk in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                step.run()
            torch.cuda.synchronize()
            steps.append((time.perf_counter() - t0) / 100 * 1e3)
    reps.sort(); steps.sort()
    print(json.dumps({"lib": os.environ.get("EPRECON_LIB_PATH", "default"), "replay_us_median": reps[len(reps) // 2],
                      "replay_us": reps, "step_ms_median": steps[len(steps) // 2], "step_ms": steps}))


if __name__ == "__main__":
    main()

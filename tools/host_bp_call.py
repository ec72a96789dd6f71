"""host-side cost of one back-projection call through the Python wrappers: a loop of run_async(...).result() on a 4,096-voxel
list (dense 16^3 on the 1/4-res maps of a 320x240 window; the device part of such a call is a few microseconds of kernels and
one pinned read, the rest is the wrapper, the descriptor and the library's host path); and the same calls queued with
hold_read=True and no wait inside the loop, which leaves the host path alone"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eprecon_amd import back_project as BP  # noqa: E402
from eprecon_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)
w = S.make_window(seed=1, width=320, height=240, n_vox=(16, 16, 16))
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
coords = t(S.dense_coords((16, 16, 16), 1))
feats = BP.to_channels_last(t(S.make_features(7, 9, S.pyramid_shapes(240, 320)[0])))
kr, origin = t(w["proj_matrices"][:, 0][:, None]), t(w["vol_origin_partial"][None])
assert coords.shape[0] == 4096
call = lambda: BP.run_async(coords, origin, 0.04, feats, kr, 2).result()
with torch.no_grad():
    for _ in range(300):
        res = call()
    loops = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(1000):
            call()
        loops.append((time.perf_counter() - t0) / 1000 * 1e6)
    queued = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(1000):
            BP.run_async(coords, origin, 0.04, feats, kr, 2, hold_read=True)
        queued.append((time.perf_counter() - t0) / 1000 * 1e6)
    torch.cuda.synchronize()
fmt = lambda xs: "  ".join(f"{x:.2f}" for x in xs) + f"  median {sorted(xs)[2]:.2f}"
print(f"n_valid {res['n_valid']}  us per call in five loops of 1,000: run_async().result() {fmt(loops)} | run_async(hold_read=True), queued {fmt(queued)}")

"""python tools/bp_fold_sweep.py (from the repository root; profiles/r12/fold_cap.txt): sweep of list lengths: count -> scan -> gather (EPRECON_BP_FOLD=0) against count -> gather with the scan folded in
(EPRECON_BP_FOLD=1000000), channels-last maps, C = 24, V = 9, 40 x 30 maps, min_view 1; us per call, median of 7 rounds of 30 calls"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import back_project_ref as R
from eprecon_amd import _lib, back_project as BP
lib = _lib.load()
dev = torch.device("cuda", 0)
V, C = 9, 24
big = R.scene(seed=0, nvox=176, interval=1, lvl=1, V=V, C=C, n=(4300000,))
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
feats = t(big["feats"]).permute(0, 1, 3, 4, 2).contiguous()   # NHWC storage
H, W = big["feats"].shape[3:]
origin, kr = t(big["origin"]), t(big["kr"])
allc = t(big["coords"])
nmax = allc.shape[0]
out_f = torch.empty((nmax, C), dtype=torch.float32, device=dev)
out_c = torch.empty((nmax, 4), dtype=torch.int32, device=dev)
cnt = torch.empty((nmax,), dtype=torch.float32, device=dev)
nv = torch.empty((2,), dtype=torch.int32, device=dev)
ws_b = lib.eprecon_back_project_workspace_bytes(nmax, 1, V, C, H, W, BP.LAYOUT_NHWC)
ws = torch.empty((ws_b,), dtype=torch.uint8, device=dev)

def call(n):
    rc = lib.eprecon_back_project_async(_lib.ptr(allc), n, _lib.ptr(origin), 1, float(big["voxel_size"]), _lib.ptr(feats), BP.LAYOUT_NHWC,
        _lib.ptr(kr), V, C, H, W, 1, BP.MODE_MEAN, _lib.ptr(out_f), None, _lib.ptr(out_c), _lib.ptr(cnt), None, None,
        _lib.ptr(nv), _lib.ptr(ws), ws.numel(), _lib.current_stream())
    assert rc == 0, rc

def timed(n, fold, reps=30):
    os.environ["EPRECON_BP_FOLD"] = str(fold)
    for _ in range(3): call(n)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): call(n)
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps

print(f"{'tiles':>7s} {'vox':>4s} {'n':>9s} {'n_valid':>9s} {'scan_us':>9s} {'fold_us':>9s} {'fold-scan':>10s}")
cases = [(16, t_) for t_ in (864, 1728, 3071)] + [(64, t_) for t_ in (768, 1728, 3456, 4096, 6144, 8191)] + \
        [(256, t_) for t_ in (2048, 3456, 4096, 5120, 6144, 8192, 12288, 16384)]
for vox, tiles in cases:
    n = tiles * vox
    s, f = [], []
    for r in range(7):
        s.append(timed(n, 0)); f.append(timed(n, 1000000))
    call(n); torch.cuda.synchronize()
    print(f"{tiles:7d} {vox:4d} {n:9d} {int(nv[0]):9d} {np.median(s):9.2f} {np.median(f):9.2f} {np.median(f) - np.median(s):+10.2f}", flush=True)

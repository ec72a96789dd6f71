"""The cases of the point-voxel module witnesses (test_pointvoxel_modules_host.py on the CPU, test_pointvoxel_modules_gpu.py on
the GPU): the point cloud, the seeded modules, the compared quantities of each case, their scales and their TWIN_* constants.

A compared quantity is a tensor named "out", "grad:input" / "grad:h" / "grad:x" / "grad:values_in" or "grad:<state_dict name>".
Its error is max |got - witness| / scale over ALL elements; scale = max |witness| for an output and for an input gradient, and
the largest |witness gradient| over the parameters of the same block (stem, a stage, an up stage, a point MLP, a gate
convolution) for a parameter gradient — a Linear bias in front of a train-mode BatchNorm has an exactly zero gradient and
would otherwise be measured against its own round-off.

TWIN_*[case][quantity] is the distance between the float64 restatement and the SAME restatement in float32 on the CPU (one
thread: the summation order of the float32 run is part of the number), measured once and written down below with ~40 % head
room; the host test recomputes it and asserts recomputed <= constant <= 2 x recomputed.  (The recomputed number is the
round-off of the CPU's float32 kernels, whose summation order follows the vector instruction set: measured with torch's
AVX-512 kernels; an AVX2-only run of the same build moves a quarter of the 298 figures out of that window.  The GPU bounds
use the constants, not the recomputation, and do not move.)  The GPU bound of a quantity is
FACTOR x TWIN (bound() below; two quantities are WIDENED to the next power of two, with figures and reason): the HIP path and
the twin are the same precision and differ in summation order, fused multiply-adds and MFMA accumulation."""
import contextlib

import numpy as np
import torch

import pointvoxel_modules_ref as R
from oracle import gru_fusion as OGF
from oracle import pointvoxel as PV
from test_oracle_dense import face_points, metric_points, with_far_points
from test_oracle_gru_fusion import sequence

RES = 0.37                      # voxel size of the SPVCNN / ConvGRU cases (pres = 1)
FACTOR = 4                      # GPU bound = FACTOR x TWIN (the project's convention, tests/test_raycast_gpu.py)
FORWARD_CEILING, GRADIENT_CEILING = 1e-3, 2e-3      # what test_autograd_gpu.py allows the same paths
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# the point cloud

def cloud():
    """<= 1,500 metric points (x, y, z, batch) f32 from the edge generators of test_oracle_dense.py, cropped to the voxels
    [-8, 8) per axis at RES: random points with negative coordinates on every axis, multiples k RES formed in float32 (voxel
    faces) and one ulp below them, face / edge / corner points of the scaled frame, -0.0, one voxel with > 50 points, and the
    far points of with_far_points folded to x in [6, 8) (isolated: most of their corners are absent)."""
    rng = np.random.default_rng(11)
    mp = metric_points(11, RES, crowd=150)
    fp = with_far_points(face_points(12, n_random=80), 12, n=24)
    fp[-24:, 0] = 6 + (fp[-24:, 0] - 40) / 4
    fp[:, :3] *= np.float32(RES)
    pts = np.concatenate([mp[rng.random(len(mp)) < 0.55], fp]).astype(np.float32)
    vox = np.floor((pts[:, :3] / np.float32(RES)).astype(np.float64))
    pts = pts[((vox >= -8) & (vox < 8)).all(1)]
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


# ---------------------------------------------------------------------------------------------------------------------
# quantities, scales, errors

def group_of(name):
    """the block a compared gradient is scaled with (a fragment prefix "f1:" / "f2:" of the fusion walk stays in front)"""
    if name[:1] == "f" and name[1:2].isdigit() and name[2:3] == ":":
        return name[:3] + group_of(name[3:])
    if not name.startswith("grad:") or name in ("grad:input", "grad:h", "grad:x", "grad:values_in"):
        return name
    parts = name[5:].split(".")
    for i, p in enumerate(parts):
        if p in ("convz", "convr", "convq"):
            return ".".join(parts[:i + 1])
    return ".".join(parts[:2] if parts[0] == "point_transforms" else parts[:1])


def scales(q64):
    top = {}
    for name, t in q64.items():
        g = group_of(name)
        top[g] = max(top.get(g, 0.0), float(t.abs().max()))
    return {name: top[group_of(name)] for name in q64}


def errors(q, q64):
    """{quantity of q: max |q - q64| / scale} over every element; q64 holds ALL quantities of the case (the block scales)"""
    sc = scales(q64)
    out = {}
    for name, got in q.items():
        ref = q64[name]
        got = got.detach().cpu().to(F64)
        assert got.shape == ref.shape, name
        assert torch.isfinite(got).all(), name
        out[name] = float((got - ref).abs().max()) / sc[name]
    return out


def ceiling(name):
    return GRADIENT_CEILING if "grad:" in name else FORWARD_CEILING


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _grads(loss, named, retain=False):
    gs = torch.autograd.grad(loss, list(named.values()), allow_unused=True, retain_graph=retain)
    return {"grad:" + k: (torch.zeros_like(t) if g is None else g).detach() for (k, t), g in zip(named.items(), gs)}


# ---------------------------------------------------------------------------------------------------------------------
# SPVCNN

class SpvcnnCase:
    def __init__(self, name, cr, cin):
        from eprecon_amd.modules import SPVCNN
        self.name, self.cr, self.cin, self.vres = name, cr, cin, RES
        self.pts = cloud()
        rng = np.random.default_rng(cin)
        self.feat = rng.standard_normal((len(self.pts), cin)).astype(np.float32)
        torch.manual_seed(cin)
        self.net = SPVCNN(num_classes=1, in_channels=cin, pres=1, cr=cr, vres=RES, dropout=False)
        with torch.no_grad():
            for _, p in self.net.named_parameters():
                if p.dim() == 1:                     # BatchNorm weights / biases and Linear biases off their defaults
                    p.add_(torch.randn_like(p) * 0.1)
        self.sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.probe = rng.standard_normal((len(self.pts), self.net.cs[4])).astype(np.float32)
        self.geometry = R.SpvcnnGeometry(self.pts, 1, RES)

    def quantities(self, dtype, perturb=None):
        params = R.leaves(self.sd, dtype)
        feat = R.tens(self.feat, dtype).requires_grad_()
        out = R.spvcnn(params, feat, self.pts, 1, self.vres, dtype, perturb, self.geometry)
        loss = (torch.tanh(out) * R.tens(self.probe, dtype)).sum()
        return {"out": out.detach(), **_grads(loss, {"input": feat, **params})}


SPVCNN_CASES = {"A": (1 / 4, 11), "B": (1 / 2, 41)}


# ---------------------------------------------------------------------------------------------------------------------
# ConvGRU

class GruCase:
    def __init__(self, name, hidden, inp, literal):
        from eprecon_amd.modules import ConvGRU
        self.name, self.hidden, self.inp, self.literal, self.vres = name, hidden, inp, literal, RES
        self.pts = cloud()
        rng = np.random.default_rng(hidden)
        self.h = rng.standard_normal((len(self.pts), hidden)).astype(np.float32)
        self.x = rng.standard_normal((len(self.pts), inp)).astype(np.float32)
        torch.manual_seed(hidden)
        self.net = ConvGRU(hidden_dim=hidden, input_dim=inp, pres=1, vres=RES)
        self.sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.geometry = R.GruGeometry(self.pts, 1, RES, literal)

    def quantities(self, dtype, perturb=None):
        params = R.leaves(self.sd, dtype)
        h, x = (R.tens(a, dtype).requires_grad_() for a in (self.h, self.x))
        out = R.convgru(params, "", h, x, self.pts, 1, self.vres, self.literal, dtype, perturb, self.geometry)
        return {"out": out.detach(), **_grads(out.square().mean(), {"h": h, "x": x, **params})}


GRU_CASES = {"A": (24, 24), "B": (5, 7)}


# ---------------------------------------------------------------------------------------------------------------------
# one GRUFusion level over a walk of three fragments

CH_IN, CH_VOXEL = [6, 4, 3], [4, 3, 2]
W2AC = np.eye(4, dtype=np.float32)
W2AC[:3, :3] = np.array([[0.8, 0.6, 0], [-0.6, 0.8, 0], [0, 0, 1]], np.float32)
W2AC[:3, 3] = [0.1, -0.2, 0.3]


class FusionCase:
    """sequence(scale) of test_oracle_gru_fusion.py through one level: fragment 0 seeds the map, fragments 1 and 2 are
    differentiated.  The union order, the map bookkeeping and (through the cell lookup below, checked against the rows the
    oracle gathers) src_cur come from oracle/gru_fusion.py; the map's rows are kept here at the precision of the walk."""

    def __init__(self, scale, literal=True):
        from eprecon_amd.config import ModelCfg
        from eprecon_amd.gru_fusion import GRUFusion
        self.scale, self.literal = scale, literal
        self.frags, self.origin, self.interval, self.dim, self.channels = sequence(scale)
        self.cfg = ModelCfg(N_VOX=[24, 24, 24])
        torch.manual_seed(scale)
        self.net = GRUFusion(self.cfg, ch_in=CH_IN, ch_voxel=CH_VOXEL)
        self.sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.vres = 0.04 * self.interval
        self.prefixes = (f"fusion_nets_voxel.{scale}.", f"fusion_nets_img.{scale}.")
        self._geometry = {}

    def walk(self, dtype, perturb=None):
        """-> [per fragment: dict(q = quantities (fragments 1, 2), out, updated, src_cur, pts, h / x = the float32 rows the oracle
        gathered, kinds = rows (map only, fragment only, both), unused = rows of values_in outside the union, map_C)]"""
        params = {k: v for k, v in R.leaves(self.sd, dtype).items() if k.startswith(self.prefixes)}
        st = OGF.ScaleState(self.channels, self.origin)
        map_rows = torch.zeros((0, self.channels), dtype=dtype)
        steps = []
        for k, fr in enumerate(self.frags):
            cur = R.tens(fr["values"], dtype)
            if k:
                cur.requires_grad_()
            step = {}

            def fuse(gvals, vals, updated, rel, cur=cur, fr=fr, k=k, step=step):
                cells = np.concatenate([np.zeros((len(fr["coords"]), 1), np.int64), fr["coords"][:, 1:] // self.interval], 1)
                union = np.concatenate([np.zeros((len(updated), 1), np.int64), updated], 1)
                src_cur = R.DR.lookup(cells, union)
                src_glob = R.DR.lookup(np.concatenate([np.zeros((len(st.C), 1), np.int64), st.C - rel], 1), union)
                pad = torch.cat([map_rows, map_rows.new_zeros(1, self.channels)])
                h_rows = pad[torch.from_numpy(np.where(src_glob >= 0, src_glob, len(map_rows)))]
                x_rows = np.where(src_cur[:, None] >= 0, fr["values"][np.maximum(src_cur, 0)], 0)
                assert np.array_equal(x_rows, vals), "src_cur does not gather the rows the oracle gathers"
                np.testing.assert_allclose(h_rows.detach().numpy(), gvals, rtol=1e-5, atol=1e-6)
                c4 = np.concatenate([np.zeros((len(updated), 1), np.int32), (updated * self.interval).astype(np.int32)], 1)
                pts = PV.aligned_coords(c4, fr["origin_partial"][None], 0.04, W2AC[None])
                if k not in self._geometry:
                    self._geometry[k] = R.GruGeometry(pts, 1, self.vres, self.literal)
                with torch.set_grad_enabled(k > 0):
                    out = R.fuse_level(params, self.scale, h_rows, cur, src_cur, pts, 1, self.vres, CH_VOXEL[self.scale],
                                       self.literal, dtype, perturb, self._geometry[k])
                used = np.zeros(len(fr["values"]), bool)
                used[src_cur[src_cur >= 0]] = True
                step.update(out=out, updated=updated, src_cur=src_cur, unused=~used, pts=pts, h=gvals, x=vals,
                            kinds=(int(((src_glob >= 0) & (src_cur < 0)).sum()), int(((src_glob < 0) & (src_cur >= 0)).sum()),
                                   int(((src_glob >= 0) & (src_cur >= 0)).sum())))
                return out.detach().numpy().astype(np.float32)

            r = OGF.fuse_fragment(st, fr["coords"], fr["values"], fr["origin_partial"], fr["tsdf"], fr["occ"], self.interval,
                                  self.dim, fuse=fuse)
            out = step["out"]
            if k:
                step["q"] = {"out": out.detach(), **_grads(out.square().mean(), {"values_in": cur, **params},
                                                           retain=perturb == "map_grad")}
            keep = torch.from_numpy(~r["valid"])
            map_rows = torch.cat([map_rows[keep], out if perturb == "map_grad" else out.detach()])
            step["map_C"] = st.C.copy()
            steps.append(step)
        return steps

    def quantities(self, dtype, perturb=None):
        """the compared quantities of fragments 1 and 2 under one name space ("f1:out", "f2:grad:values_in", ...)"""
        return {f"f{k}:{name}": t for k, s in enumerate(self.walk(dtype, perturb)) if k for name, t in s["q"].items()}



# ---------------------------------------------------------------------------------------------------------------------
# GPU bounds

# Quantities that missed FACTOR x TWIN on the MI355X with no defect found in the code they run, bounded by the next power of two
# instead (never above the ceilings).  Both are the bias gradient of convq's point-wise Linear in fragment 2, which
# eprecon_amd/autograd.py forms as dy.sum(0), torch's own column sum over the union's 297 / 2,382 float32 rows.  The twin's sum
# happened to land within a tenth of an ulp of the float64 value, so 4 x TWIN (6.0e-8 and 3.1e-8 of the block scale) is at or
# under HALF an ulp of float32 (2^-24 = 5.96e-8) for a value at the block scale: a correctly rounded float32 result can miss
# it.  Measured: 7.7e-8 = 1.29 x (4 x TWIN) and 3.2e-8 = 1.02 x (4 x TWIN), i.e. one ulp of another summation order.
WIDENED = {
    ("fusion", 1, "f2:grad:fusion_nets_img.1.convq.point_transforms.0.bias"): 8,
    ("fusion", 2, "f2:grad:fusion_nets_voxel.2.convq.point_transforms.0.bias"): 8,
}


def twin_table(kind, key):
    return {"spvcnn": TWIN_SPVCNN, "convgru": TWIN_CONVGRU, "fusion": TWIN_FUSION}[kind][key]


def bound(kind, key, name):
    """the GPU bound of one compared quantity: FACTOR x its twin distance (WIDENED: the stated power of two instead)"""
    return WIDENED.get((kind, key, name), FACTOR) * twin_table(kind, key)[name]


# ---------------------------------------------------------------------------------------------------------------------
# twin distances: max |float32 restatement - float64 restatement| / scale, measured on the CPU on one thread, x 1.4
# (keys: SPVCNN case; (ConvGRU case, LITERAL_CONVR); fusion scale)

TWIN_SPVCNN = {
    "A": {
        "out": 7.8e-07, "grad:input": 1.3e-06, "grad:stem.0.kernel": 2.3e-06, "grad:stem.1.weight": 9.7e-08,
        "grad:stem.1.bias": 1.1e-07, "grad:stage1.0.net.0.kernel": 2.2e-06, "grad:stage1.0.net.1.weight": 6.3e-07,
        "grad:stage1.0.net.1.bias": 2.3e-07, "grad:stage1.1.net.0.kernel": 9.3e-07, "grad:stage1.1.net.1.weight":
        2e-07, "grad:stage1.1.net.1.bias": 2.6e-07, "grad:stage1.1.net.3.kernel": 1.1e-06,
        "grad:stage1.1.net.4.weight": 2.2e-07, "grad:stage1.1.net.4.bias": 1.4e-07,
        "grad:stage1.1.downsample.0.kernel": 7.8e-07, "grad:stage1.1.downsample.1.weight": 1.7e-07,
        "grad:stage1.1.downsample.1.bias": 1.4e-07, "grad:stage1.2.net.0.kernel": 1.1e-06,
        "grad:stage1.2.net.1.weight": 1.6e-07, "grad:stage1.2.net.1.bias": 1.4e-07, "grad:stage1.2.net.3.kernel":
        8e-07, "grad:stage1.2.net.4.weight": 1.6e-07, "grad:stage1.2.net.4.bias": 1.3e-07,
        "grad:stage2.0.net.0.kernel": 2.7e-06, "grad:stage2.0.net.1.weight": 3.5e-07, "grad:stage2.0.net.1.bias":
        2.6e-07, "grad:stage2.1.net.0.kernel": 1.5e-06, "grad:stage2.1.net.1.weight": 2.9e-07,
        "grad:stage2.1.net.1.bias": 2.6e-07, "grad:stage2.1.net.3.kernel": 1.1e-06, "grad:stage2.1.net.4.weight":
        2.2e-07, "grad:stage2.1.net.4.bias": 1.4e-07, "grad:stage2.1.downsample.0.kernel": 6.6e-07,
        "grad:stage2.1.downsample.1.weight": 3e-07, "grad:stage2.1.downsample.1.bias": 1.4e-07,
        "grad:stage2.2.net.0.kernel": 1e-06, "grad:stage2.2.net.1.weight": 2.5e-07, "grad:stage2.2.net.1.bias":
        2.1e-07, "grad:stage2.2.net.3.kernel": 1.7e-06, "grad:stage2.2.net.4.weight": 1.8e-07,
        "grad:stage2.2.net.4.bias": 1.4e-07, "grad:up1.0.net.0.kernel": 1.6e-06, "grad:up1.0.net.1.weight": 2.7e-07,
        "grad:up1.0.net.1.bias": 2.2e-07, "grad:up1.1.0.net.0.kernel": 2.2e-06, "grad:up1.1.0.net.1.weight": 3.1e-07,
        "grad:up1.1.0.net.1.bias": 1.9e-07, "grad:up1.1.0.net.3.kernel": 1.9e-06, "grad:up1.1.0.net.4.weight":
        3.2e-07, "grad:up1.1.0.net.4.bias": 2.4e-07, "grad:up1.1.0.downsample.0.kernel": 1.3e-06,
        "grad:up1.1.0.downsample.1.weight": 3.3e-07, "grad:up1.1.0.downsample.1.bias": 2.4e-07,
        "grad:up1.1.1.net.0.kernel": 2e-06, "grad:up1.1.1.net.1.weight": 3.3e-07, "grad:up1.1.1.net.1.bias": 2.2e-07,
        "grad:up1.1.1.net.3.kernel": 1.9e-06, "grad:up1.1.1.net.4.weight": 3.6e-07, "grad:up1.1.1.net.4.bias":
        1.6e-07, "grad:up2.0.net.0.kernel": 1.9e-06, "grad:up2.0.net.1.weight": 2.1e-07, "grad:up2.0.net.1.bias":
        1.3e-07, "grad:up2.1.0.net.0.kernel": 1.8e-06, "grad:up2.1.0.net.1.weight": 2.6e-07,
        "grad:up2.1.0.net.1.bias": 1.9e-07, "grad:up2.1.0.net.3.kernel": 1.8e-06, "grad:up2.1.0.net.4.weight":
        3.8e-07, "grad:up2.1.0.net.4.bias": 1.4e-07, "grad:up2.1.0.downsample.0.kernel": 7e-07,
        "grad:up2.1.0.downsample.1.weight": 2.3e-07, "grad:up2.1.0.downsample.1.bias": 1.4e-07,
        "grad:up2.1.1.net.0.kernel": 1.6e-06, "grad:up2.1.1.net.1.weight": 2.2e-07, "grad:up2.1.1.net.1.bias":
        1.5e-07, "grad:up2.1.1.net.3.kernel": 2.3e-06, "grad:up2.1.1.net.4.weight": 2.1e-07,
        "grad:up2.1.1.net.4.bias": 1.2e-07, "grad:point_transforms.0.0.weight": 1.9e-06,
        "grad:point_transforms.0.0.bias": 4.8e-07, "grad:point_transforms.0.1.weight": 7.1e-07,
        "grad:point_transforms.0.1.bias": 5.6e-07, "grad:point_transforms.1.0.weight": 3.6e-06,
        "grad:point_transforms.1.0.bias": 1.6e-07, "grad:point_transforms.1.1.weight": 4.7e-07,
        "grad:point_transforms.1.1.bias": 4.2e-07
    },
    "B": {
        "out": 2e-06, "grad:input": 3.1e-06, "grad:stem.0.kernel": 2.6e-06, "grad:stem.1.weight": 4.1e-07,
        "grad:stem.1.bias": 3.5e-07, "grad:stage1.0.net.0.kernel": 3.6e-06, "grad:stage1.0.net.1.weight": 6.6e-07,
        "grad:stage1.0.net.1.bias": 3.8e-07, "grad:stage1.1.net.0.kernel": 1.8e-06, "grad:stage1.1.net.1.weight":
        4.1e-07, "grad:stage1.1.net.1.bias": 3.2e-07, "grad:stage1.1.net.3.kernel": 1.8e-06,
        "grad:stage1.1.net.4.weight": 3.2e-07, "grad:stage1.1.net.4.bias": 2.1e-07,
        "grad:stage1.1.downsample.0.kernel": 8e-07, "grad:stage1.1.downsample.1.weight": 2.3e-07,
        "grad:stage1.1.downsample.1.bias": 2.1e-07, "grad:stage1.2.net.0.kernel": 1.5e-06,
        "grad:stage1.2.net.1.weight": 3.7e-07, "grad:stage1.2.net.1.bias": 2.2e-07, "grad:stage1.2.net.3.kernel":
        1.7e-06, "grad:stage1.2.net.4.weight": 2e-07, "grad:stage1.2.net.4.bias": 2e-07,
        "grad:stage2.0.net.0.kernel": 3.4e-06, "grad:stage2.0.net.1.weight": 6.5e-07, "grad:stage2.0.net.1.bias":
        4.8e-07, "grad:stage2.1.net.0.kernel": 1.6e-06, "grad:stage2.1.net.1.weight": 3.2e-07,
        "grad:stage2.1.net.1.bias": 2.2e-07, "grad:stage2.1.net.3.kernel": 1.1e-06, "grad:stage2.1.net.4.weight":
        2.9e-07, "grad:stage2.1.net.4.bias": 2.1e-07, "grad:stage2.1.downsample.0.kernel": 8e-07,
        "grad:stage2.1.downsample.1.weight": 3.2e-07, "grad:stage2.1.downsample.1.bias": 2.1e-07,
        "grad:stage2.2.net.0.kernel": 1.2e-06, "grad:stage2.2.net.1.weight": 2.6e-07, "grad:stage2.2.net.1.bias":
        1.5e-07, "grad:stage2.2.net.3.kernel": 1.8e-06, "grad:stage2.2.net.4.weight": 2.9e-07,
        "grad:stage2.2.net.4.bias": 2e-07, "grad:up1.0.net.0.kernel": 2.2e-06, "grad:up1.0.net.1.weight": 4.5e-07,
        "grad:up1.0.net.1.bias": 3.7e-07, "grad:up1.1.0.net.0.kernel": 5.5e-06, "grad:up1.1.0.net.1.weight": 5.9e-07,
        "grad:up1.1.0.net.1.bias": 4.3e-07, "grad:up1.1.0.net.3.kernel": 3.8e-06, "grad:up1.1.0.net.4.weight":
        5.7e-07, "grad:up1.1.0.net.4.bias": 3.2e-07, "grad:up1.1.0.downsample.0.kernel": 3.1e-06,
        "grad:up1.1.0.downsample.1.weight": 7.2e-07, "grad:up1.1.0.downsample.1.bias": 3.2e-07,
        "grad:up1.1.1.net.0.kernel": 2.7e-06, "grad:up1.1.1.net.1.weight": 8.7e-07, "grad:up1.1.1.net.1.bias":
        3.4e-07, "grad:up1.1.1.net.3.kernel": 2.9e-06, "grad:up1.1.1.net.4.weight": 6.1e-07,
        "grad:up1.1.1.net.4.bias": 3.1e-07, "grad:up2.0.net.0.kernel": 2.4e-06, "grad:up2.0.net.1.weight": 3e-07,
        "grad:up2.0.net.1.bias": 1.7e-07, "grad:up2.1.0.net.0.kernel": 2.6e-06, "grad:up2.1.0.net.1.weight": 2.9e-07,
        "grad:up2.1.0.net.1.bias": 9.7e-08, "grad:up2.1.0.net.3.kernel": 2.5e-06, "grad:up2.1.0.net.4.weight":
        2.5e-07, "grad:up2.1.0.net.4.bias": 1.5e-07, "grad:up2.1.0.downsample.0.kernel": 7.3e-07,
        "grad:up2.1.0.downsample.1.weight": 2.3e-07, "grad:up2.1.0.downsample.1.bias": 1.5e-07,
        "grad:up2.1.1.net.0.kernel": 1.9e-06, "grad:up2.1.1.net.1.weight": 1.5e-07, "grad:up2.1.1.net.1.bias":
        1.1e-07, "grad:up2.1.1.net.3.kernel": 2.5e-06, "grad:up2.1.1.net.4.weight": 2.8e-07,
        "grad:up2.1.1.net.4.bias": 1.4e-07, "grad:point_transforms.0.0.weight": 1.7e-06,
        "grad:point_transforms.0.0.bias": 3.4e-07, "grad:point_transforms.0.1.weight": 4.1e-07,
        "grad:point_transforms.0.1.bias": 3.7e-07, "grad:point_transforms.1.0.weight": 2.6e-06,
        "grad:point_transforms.1.0.bias": 2.3e-07, "grad:point_transforms.1.1.weight": 3.1e-07,
        "grad:point_transforms.1.1.bias": 4.8e-07
    },
}

TWIN_CONVGRU = {
    ("A", True): {
        "out": 1.6e-07, "grad:h": 2.2e-07, "grad:x": 3.2e-07, "grad:convz.net.kernel": 2e-07,
        "grad:convz.point_transforms.0.weight": 1.6e-07, "grad:convz.point_transforms.0.bias": 1.9e-07,
        "grad:convr.net.kernel": 2.7e-07, "grad:convr.point_transforms.0.weight": 2.3e-07,
        "grad:convr.point_transforms.0.bias": 1.1e-07, "grad:convq.net.kernel": 5.8e-07,
        "grad:convq.point_transforms.0.weight": 4.5e-07, "grad:convq.point_transforms.0.bias": 3.9e-08
    },
    ("A", False): {
        "out": 1.7e-07, "grad:h": 2.5e-07, "grad:x": 2e-07, "grad:convz.net.kernel": 1.7e-07,
        "grad:convz.point_transforms.0.weight": 1.9e-07, "grad:convz.point_transforms.0.bias": 1.4e-07,
        "grad:convr.net.kernel": 1.5e-07, "grad:convr.point_transforms.0.weight": 1.9e-07,
        "grad:convr.point_transforms.0.bias": 1.1e-07, "grad:convq.net.kernel": 5.4e-07,
        "grad:convq.point_transforms.0.weight": 3.6e-07, "grad:convq.point_transforms.0.bias": 4.5e-08
    },
    ("B", True): {
        "out": 1.5e-07, "grad:h": 2.4e-07, "grad:x": 5.1e-07, "grad:convz.net.kernel": 1.9e-07,
        "grad:convz.point_transforms.0.weight": 1.3e-07, "grad:convz.point_transforms.0.bias": 8.4e-08,
        "grad:convr.net.kernel": 1.5e-07, "grad:convr.point_transforms.0.weight": 8.8e-08,
        "grad:convr.point_transforms.0.bias": 1.2e-07, "grad:convq.net.kernel": 8.7e-08,
        "grad:convq.point_transforms.0.weight": 2.8e-07, "grad:convq.point_transforms.0.bias": 1.8e-08
    },
    ("B", False): {
        "out": 1.5e-07, "grad:h": 2.1e-07, "grad:x": 2.9e-07, "grad:convz.net.kernel": 8.7e-08,
        "grad:convz.point_transforms.0.weight": 9.6e-08, "grad:convz.point_transforms.0.bias": 1.9e-07,
        "grad:convr.net.kernel": 6.2e-08, "grad:convr.point_transforms.0.weight": 1.4e-07,
        "grad:convr.point_transforms.0.bias": 1.3e-07, "grad:convq.net.kernel": 4.7e-08,
        "grad:convq.point_transforms.0.weight": 2.2e-07, "grad:convq.point_transforms.0.bias": 3.9e-08
    },
}

TWIN_FUSION = {
    1: {
        "f1:out": 1.3e-07, "f1:grad:values_in": 1.2e-07, "f1:grad:fusion_nets_voxel.1.convz.net.kernel": 2.1e-08,
        "f1:grad:fusion_nets_voxel.1.convz.point_transforms.0.weight": 1.7e-07,
        "f1:grad:fusion_nets_voxel.1.convz.point_transforms.0.bias": 2.3e-08,
        "f1:grad:fusion_nets_voxel.1.convr.net.kernel": 3.1e-08,
        "f1:grad:fusion_nets_voxel.1.convr.point_transforms.0.weight": 6.9e-08,
        "f1:grad:fusion_nets_voxel.1.convr.point_transforms.0.bias": 1.7e-07,
        "f1:grad:fusion_nets_voxel.1.convq.net.kernel": 1.9e-08,
        "f1:grad:fusion_nets_voxel.1.convq.point_transforms.0.weight": 7.7e-08,
        "f1:grad:fusion_nets_voxel.1.convq.point_transforms.0.bias": 2.1e-08,
        "f1:grad:fusion_nets_img.1.convz.net.kernel": 1.3e-08,
        "f1:grad:fusion_nets_img.1.convz.point_transforms.0.weight": 1.4e-08,
        "f1:grad:fusion_nets_img.1.convz.point_transforms.0.bias": 8.2e-08,
        "f1:grad:fusion_nets_img.1.convr.net.kernel": 8.7e-09,
        "f1:grad:fusion_nets_img.1.convr.point_transforms.0.weight": 2.4e-08,
        "f1:grad:fusion_nets_img.1.convr.point_transforms.0.bias": 1e-07,
        "f1:grad:fusion_nets_img.1.convq.net.kernel": 2.2e-08,
        "f1:grad:fusion_nets_img.1.convq.point_transforms.0.weight": 9.5e-08,
        "f1:grad:fusion_nets_img.1.convq.point_transforms.0.bias": 9.4e-08, "f2:out": 1.5e-07, "f2:grad:values_in":
        2e-07, "f2:grad:fusion_nets_voxel.1.convz.net.kernel": 4.3e-08,
        "f2:grad:fusion_nets_voxel.1.convz.point_transforms.0.weight": 6.4e-08,
        "f2:grad:fusion_nets_voxel.1.convz.point_transforms.0.bias": 6.5e-08,
        "f2:grad:fusion_nets_voxel.1.convr.net.kernel": 5.8e-08,
        "f2:grad:fusion_nets_voxel.1.convr.point_transforms.0.weight": 4.9e-08,
        "f2:grad:fusion_nets_voxel.1.convr.point_transforms.0.bias": 8.6e-08,
        "f2:grad:fusion_nets_voxel.1.convq.net.kernel": 1.9e-08,
        "f2:grad:fusion_nets_voxel.1.convq.point_transforms.0.weight": 8.7e-08,
        "f2:grad:fusion_nets_voxel.1.convq.point_transforms.0.bias": 1e-07,
        "f2:grad:fusion_nets_img.1.convz.net.kernel": 2.7e-08,
        "f2:grad:fusion_nets_img.1.convz.point_transforms.0.weight": 1.6e-08,
        "f2:grad:fusion_nets_img.1.convz.point_transforms.0.bias": 9.9e-08,
        "f2:grad:fusion_nets_img.1.convr.net.kernel": 1.3e-08,
        "f2:grad:fusion_nets_img.1.convr.point_transforms.0.weight": 5.1e-09,
        "f2:grad:fusion_nets_img.1.convr.point_transforms.0.bias": 1.3e-08,
        "f2:grad:fusion_nets_img.1.convq.net.kernel": 7.1e-09,
        "f2:grad:fusion_nets_img.1.convq.point_transforms.0.weight": 9.5e-08,
        "f2:grad:fusion_nets_img.1.convq.point_transforms.0.bias": 1.5e-08
    },
    2: {
        "f1:out": 1.6e-07, "f1:grad:values_in": 1.6e-07, "f1:grad:fusion_nets_voxel.2.convz.net.kernel": 8.8e-09,
        "f1:grad:fusion_nets_voxel.2.convz.point_transforms.0.weight": 1e-08,
        "f1:grad:fusion_nets_voxel.2.convz.point_transforms.0.bias": 4.6e-08,
        "f1:grad:fusion_nets_voxel.2.convr.net.kernel": 3.2e-08,
        "f1:grad:fusion_nets_voxel.2.convr.point_transforms.0.weight": 7.7e-09,
        "f1:grad:fusion_nets_voxel.2.convr.point_transforms.0.bias": 1.2e-07,
        "f1:grad:fusion_nets_voxel.2.convq.net.kernel": 9.3e-08,
        "f1:grad:fusion_nets_voxel.2.convq.point_transforms.0.weight": 1.6e-07,
        "f1:grad:fusion_nets_voxel.2.convq.point_transforms.0.bias": 6.3e-09,
        "f1:grad:fusion_nets_img.2.convz.net.kernel": 4.9e-09,
        "f1:grad:fusion_nets_img.2.convz.point_transforms.0.weight": 5e-08,
        "f1:grad:fusion_nets_img.2.convz.point_transforms.0.bias": 7.1e-10,
        "f1:grad:fusion_nets_img.2.convr.net.kernel": 1.6e-08,
        "f1:grad:fusion_nets_img.2.convr.point_transforms.0.weight": 1.8e-07,
        "f1:grad:fusion_nets_img.2.convr.point_transforms.0.bias": 3.8e-08,
        "f1:grad:fusion_nets_img.2.convq.net.kernel": 1.8e-08,
        "f1:grad:fusion_nets_img.2.convq.point_transforms.0.weight": 1.5e-07,
        "f1:grad:fusion_nets_img.2.convq.point_transforms.0.bias": 2.2e-08, "f2:out": 2.1e-07, "f2:grad:values_in":
        2.6e-07, "f2:grad:fusion_nets_voxel.2.convz.net.kernel": 1.4e-08,
        "f2:grad:fusion_nets_voxel.2.convz.point_transforms.0.weight": 2.4e-08,
        "f2:grad:fusion_nets_voxel.2.convz.point_transforms.0.bias": 1.8e-07,
        "f2:grad:fusion_nets_voxel.2.convr.net.kernel": 3e-08,
        "f2:grad:fusion_nets_voxel.2.convr.point_transforms.0.weight": 1.8e-08,
        "f2:grad:fusion_nets_voxel.2.convr.point_transforms.0.bias": 4e-08,
        "f2:grad:fusion_nets_voxel.2.convq.net.kernel": 4.8e-08,
        "f2:grad:fusion_nets_voxel.2.convq.point_transforms.0.weight": 2.4e-07,
        "f2:grad:fusion_nets_voxel.2.convq.point_transforms.0.bias": 7.8e-09,
        "f2:grad:fusion_nets_img.2.convz.net.kernel": 2.3e-08,
        "f2:grad:fusion_nets_img.2.convz.point_transforms.0.weight": 2.8e-07,
        "f2:grad:fusion_nets_img.2.convz.point_transforms.0.bias": 1.3e-07,
        "f2:grad:fusion_nets_img.2.convr.net.kernel": 1.8e-08,
        "f2:grad:fusion_nets_img.2.convr.point_transforms.0.weight": 2.1e-07,
        "f2:grad:fusion_nets_img.2.convr.point_transforms.0.bias": 9.8e-08,
        "f2:grad:fusion_nets_img.2.convq.net.kernel": 1.5e-08,
        "f2:grad:fusion_nets_img.2.convq.point_transforms.0.weight": 1.2e-07,
        "f2:grad:fusion_nets_img.2.convq.point_transforms.0.bias": 9.6e-08
    },
}

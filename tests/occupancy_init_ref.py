"""Plain torch restatement of the occupancy-initialisation branch (Occupancy_Initialization.forward), written from the module
docstrings of eprecon_amd/modules.py and eprecon_amd/occupancy_initialization.py: the 2D fusion stack, the view-variance volume,
then norm0 / sparse ELAN / 3 x LN(x + ReLU(SubM(x))) / SubM(32 -> 1) / norm4.  It calls none of those modules and nothing of
oracle/.

Every function is pure, takes a `dtype` (torch.float64: the witness; torch.float32 on one CPU thread: its "twin") and reads
weights by their state_dict() names.  The variance volume is NOT restated: it is back_project_ref.forward / adjoint (float64
numpy, merged with the back-projection witness), whatever `dtype` the two torch segments run in.

branch_gradients joins THREE SEGMENTS by the chain rule: torch autograd through the sparse stack (every parameter of it, and
d var), back_project_ref.adjoint in its deterministic form from d var to d fused, torch autograd through the 2D stack with
that cotangent (every parameter of it and the three input maps).  The loss is sum(logit * dout) for a fixed cotangent dout.

`perturb` names ONE deliberate mistake (test_occupancy_init_witness_host.py shows that each moves a compared quantity by
>= 10 x its GPU bound):
  "norm0_unbiased"   norm0 divides by rows - 1
  "den_views"        the variance divides by V instead of the visible count
  "level_order"      the concat of the levels is [1/8, 1/16, 1/4]
  "align_corners"    the bilinear x2 of the 1/16 level with align_corners=True
  "elan2d_swap"      the 2D ELAN concatenates [x1, x2, x4, x3, x5, x6]
  "elan3d_swap"      the sparse ELAN concatenates [x1, x2, x4, x3, x5, x6]
  "ln_of_relu"       LN(ReLU(x + conv(x))) in place of LN(x + ReLU(conv(x)))
  "residual2d_form"  the 2D residual block as ReLU(BN(conv(x))) + x in place of BN(x + ReLU(conv(x)))"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import back_project_ref as BR
import dense_ref as DR

BN_EPS = 1e-5        # nn.BatchNorm1d / 2d default; eps is no state_dict entry (the GPU tests assert the modules carry it)
LN_EPS = 1e-5        # nn.LayerNorm default
PERTURBATIONS = ("norm0_unbiased", "den_views", "level_order", "align_corners", "elan2d_swap", "elan3d_swap", "ln_of_relu",
                 "residual2d_form")
PREFIXES_2D = ("self_fusion_", "fusion_down.", "post_fusion_")
PREFIXES_3D = ("norm", "similary_1.", "subm")


def tens(a, dtype):
    return DR._t64(a, dtype)


def leaves(sd, dtype, prefixes):
    """the floating-point parameters of a state_dict under `prefixes` as fresh leaves of `dtype` that require a gradient
    (running statistics and counters left out: train-mode BatchNorm never reads them)"""
    out = {}
    for k, v in sd.items():
        if k.startswith(prefixes) and not k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out[k] = tens(v.detach().cpu() if torch.is_tensor(v) else v, dtype).clone().requires_grad_()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the 2D fusion stack (the V views are the batch dimension)

def bn2d(sd, p, x):
    """train-mode BatchNorm2d written out: per channel over V H W, biased variance"""
    mean = x.mean((0, 2, 3), keepdim=True)
    d = x - mean
    var = (d * d).sum((0, 2, 3), keepdim=True) / (x.shape[0] * x.shape[2] * x.shape[3])
    w, b = (tens(sd[p + s], x.dtype).reshape(1, -1, 1, 1) for s in (".weight", ".bias"))
    return d / torch.sqrt(var + BN_EPS) * w + b


def conv2d(sd, p, x):
    """k x k convolution, stride 1, zero padding k // 2 ("same")"""
    w = tens(sd[p + ".weight"], x.dtype)
    return F.conv2d(x, w, tens(sd[p + ".bias"], x.dtype), padding=w.shape[-1] // 2)


def conv_block(sd, p, x):
    """ReLU(BN(conv(x))) with the names of Conv2d_Block (p.conv, p.bn)"""
    return torch.relu(bn2d(sd, p + ".bn", conv2d(sd, p + ".conv", x)))


def elan2d(sd, p, x, perturb=None):
    """two 1x1 branches x1, x2; a chain of four 3x3 layers at half width from x2; concat [x1 .. x6]; 1x1 back to full width"""
    parts = [conv_block(sd, p + ".conv1", x), conv_block(sd, p + ".conv2", x)]
    for name in ("conv3", "conv4", "conv5", "conv6"):
        parts.append(conv_block(sd, f"{p}.{name}", parts[-1]))
    if perturb == "elan2d_swap":
        parts[2], parts[3] = parts[3], parts[2]
    return conv_block(sd, p + ".conv7", torch.cat(parts, 1))


def fusion_block(sd, p, x, perturb=None):
    """conv3x3-BN-ReLU, conv1x1-BN-ReLU, ELAN"""
    x = torch.relu(bn2d(sd, p + ".bn1", conv2d(sd, p + ".conv1", x)))
    x = torch.relu(bn2d(sd, p + ".bn2", conv2d(sd, p + ".conv2", x)))
    return elan2d(sd, p + ".ELAN", x, perturb)


def residual2d(sd, p, x, perturb=None):
    """BN(x + ReLU(conv(x)))"""
    if perturb == "residual2d_form":
        return torch.relu(bn2d(sd, p + ".bn", conv2d(sd, p + ".conv", x))) + x
    return bn2d(sd, p + ".bn", x + torch.relu(conv2d(sd, p + ".conv", x)))


def fusion2d(sd, f16, f8, f4, dtype, perturb=None):
    """[V,80,h,w] (1/16), [V,40,2h,2w] (1/8), [V,24,4h,4w] (1/4) of ONE batch element -> fused [V,32,2h,2w]: a Fusion_Block
    per level; the 1/16 level bilinear x2 (align_corners=False), the 1/4 level 2x2 mean; concat [1/16, 1/8, 1/4]; fusion_down
    1x1; four residual blocks"""
    f16, f8, f4 = (tens(t, dtype) for t in (f16, f8, f4))
    a = fusion_block(sd, "self_fusion_1x", f16, perturb)
    b = fusion_block(sd, "self_fusion_2x", f8, perturb)
    c = fusion_block(sd, "self_fusion_4x", f4, perturb)
    a = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=perturb == "align_corners")
    c = F.avg_pool2d(c, 2)
    x = conv_block(sd, "fusion_down", torch.cat([b, a, c] if perturb == "level_order" else [a, b, c], 1))
    for k in (1, 2, 3, 4):
        x = residual2d(sd, f"post_fusion_{k}", x, perturb)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the variance volume: back_project_ref, float64

def geometry(coords, origin, voxel_size, kr, h8, w8):
    """back_project_ref.geometry of ONE batch element: coords int[N,4] (the batch column is ignored), origin f32[3],
    kr f32[V,4,4]"""
    c = np.asarray(coords).copy()
    c[:, 0] = 0
    return BR.geometry(c, np.asarray(origin, np.float32).reshape(1, 3), voxel_size, np.asarray(kr, np.float32)[:, None], h8, w8)


def variance(G, fused, min_view, vis=None, perturb=None):
    """fused [V,32,H,W] (tensor of any float dtype, or array) -> back_project_ref.forward's result in variance mode: .y
    float64 [N,32] on every row, .valid, .cnt; vis: the visibility to evaluate with (default: the witness's own)"""
    f = fused.detach().cpu().numpy() if torch.is_tensor(fused) else np.asarray(fused)
    return BR.forward(G, f[:, None], BR.MODE_VARIANCE, min_view, vis=vis, den_views=perturb == "den_views")


def variance_adjoint(G, fused, vis, valid, dvar):
    """d fused [V,32,H,W] float64 from d var [n_valid,32] on the kept rows: back_project_ref.adjoint, deterministic form"""
    f = fused.detach().cpu().numpy() if torch.is_tensor(fused) else np.asarray(fused)
    per_view = ("u", "v", "pz", "gx", "gy", "margin", "eu", "ev", "epz")
    Gv = SimpleNamespace(**{k: getattr(G, k)[:, valid] for k in per_view}, vis=(G.vis if vis is None else vis)[:, valid],
                         in_batch=G.in_batch[valid], batch=G.batch[valid], coords=G.coords[valid], H=G.H, W=G.W, V=G.V, B=G.B)
    df, _ = BR.adjoint(Gv, f[:, None], BR.MODE_VARIANCE, np.asarray(dvar, np.float64), None, det=True)
    return np.ascontiguousarray(df[:, 0].transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the sparse stack

def batchnorm_rows(sd, p, x, unbiased=False):
    """train-mode BatchNorm over the rows, written out: biased variance"""
    mean = x.mean(0, keepdim=True)
    d = x - mean
    var = (d * d).sum(0, keepdim=True) / (x.shape[0] - (1 if unbiased else 0))
    return d / torch.sqrt(var + BN_EPS) * tens(sd[p + ".weight"], x.dtype) + tens(sd[p + ".bias"], x.dtype)


def layernorm(sd, p, x):
    return F.layer_norm(x, (x.shape[1],), tens(sd[p + ".weight"], x.dtype), tens(sd[p + ".bias"], x.dtype), LN_EPS)


class Voxels:
    """the valid voxels of one batch element (rows (b, x, y, z) on the lattice of `interval`) in a dense_ref.Frame"""

    def __init__(self, coords, interval):
        self.coords = np.asarray(coords, np.int64).reshape(-1, 4).copy()
        self.coords[:, 0] = 0
        self.interval = int(interval)
        self.frame = DR.Frame([self.coords], self.interval)


def subm(sd, p, x, vox):
    """SubM convolution with bias; weights [27, C_in, C_out] in the x-fastest offset order dense_ref.dense_weight takes, or
    [1, C_in, C_out] for a 1x1x1 layer"""
    w = sd[p + ".weight"]
    if w.shape[0] == 1:
        return x @ tens(w, x.dtype)[0] + tens(sd[p + ".bias"], x.dtype)
    return DR.subm_conv3(vox.frame, vox.coords, x, w, vox.interval, bias=sd[p + ".bias"], dtype=x.dtype)


def elan_block(sd, p, x, vox):
    """conv -> LN -> ReLU"""
    return torch.relu(layernorm(sd, p + ".ln", subm(sd, p + ".conv", x, vox)))


def sparse_stack(sd, var, coords, dtype, interval=2, perturb=None, vox=None):
    """variance rows [N,32] of ONE batch element on coords [N,4] -> logit [N,1]"""
    vox = vox or Voxels(coords, interval)
    x = batchnorm_rows(sd, "norm0", tens(var, dtype), unbiased=perturb == "norm0_unbiased")
    parts = [elan_block(sd, "similary_1.conv1", x, vox), elan_block(sd, "similary_1.conv2", x, vox)]
    for name in ("conv3", "conv4", "conv5", "conv6"):
        parts.append(elan_block(sd, "similary_1." + name, parts[-1], vox))
    if perturb == "elan3d_swap":
        parts[2], parts[3] = parts[3], parts[2]
    x = elan_block(sd, "similary_1.conv7", torch.cat(parts, 1), vox)
    for k in (1, 2, 3):
        y = subm(sd, f"subm{k}", x, vox)
        x = layernorm(sd, f"norm{k}", torch.relu(x + y) if perturb == "ln_of_relu" else x + torch.relu(y))
    return batchnorm_rows(sd, "norm4", subm(sd, "subm4", x, vox))


# ---------------------------------------------------------------------------------------------------------------------
# the branch

def branch(sd, f16, f8, f4, G, coords, min_view, dtype, vis=None, interval=2, perturb=None):
    """one batch element, forward: -> dict(out [n_valid,1], fused [V,32,H,W], var [n_valid,32] tensors of `dtype`;
    valid bool[N], cnt int[N]); no graph is kept"""
    with torch.no_grad():
        fused = fusion2d(sd, f16, f8, f4, dtype, perturb)
        fw = variance(G, fused, min_view, vis, perturb)
        var = tens(fw.y[fw.valid], dtype)
        out = sparse_stack(sd, var, np.asarray(coords)[fw.valid], dtype, interval, perturb)
    return dict(out=out, fused=fused, var=var, valid=fw.valid, cnt=fw.cnt)


def branch_gradients(sd, f16, f8, f4, G, coords, min_view, dout_rows, dtype, vis=None, interval=2, perturb=None):
    """one batch element, forward and backward of sum(logit * dout), dout = dout_rows[valid] (dout_rows: one value per input
    row, so that the cotangent of a voxel does not depend on which other voxels are valid).  Three segments joined by the
    chain rule (module docstring).  -> branch()'s dict plus "grad:<state_dict name>" for every parameter and "grad:feat16" /
    "grad:feat8" / "grad:feat4" """
    assert perturb != "den_views", "back_project_ref.adjoint has no such variant"
    p2, p3 = leaves(sd, dtype, PREFIXES_2D), leaves(sd, dtype, PREFIXES_3D)
    maps = {n: tens(t, dtype).clone().requires_grad_() for n, t in (("feat16", f16), ("feat8", f8), ("feat4", f4))}
    fused = fusion2d(p2, maps["feat16"], maps["feat8"], maps["feat4"], dtype, perturb)
    fw = variance(G, fused, min_view, vis)
    valid = fw.valid
    var = tens(fw.y[valid], dtype).requires_grad_()
    out = sparse_stack(p3, var, np.asarray(coords)[valid], dtype, interval, perturb)
    dout = tens(np.asarray(dout_rows, np.float64)[valid].reshape(-1, 1), dtype)
    g3 = torch.autograd.grad((out * dout).sum(), [var] + list(p3.values()))
    dfused = variance_adjoint(G, fused, vis, valid, g3[0].detach().numpy())
    named = {**maps, **p2}
    g2 = torch.autograd.grad(fused, list(named.values()), grad_outputs=tens(dfused, dtype))
    res = dict(out=out.detach(), fused=fused.detach(), var=var.detach(), valid=valid, cnt=fw.cnt)
    res.update({"grad:" + k: g.detach() for k, g in zip(p3, g3[1:])})
    res.update({"grad:" + k: g.detach() for k, g in zip(named, g2)})
    return res

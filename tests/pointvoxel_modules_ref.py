"""Plain, differentiable torch restatement of the three point-voxel modules that train under autograd — SPVCNN, ConvGRU and
the ConvGRU pair of one GRUFusion level — composed from the dense blocks of tests/dense_ref.py, written from what the modules
are documented to compute (eprecon_amd/modules.py, eprecon_amd/gru_fusion.py docstrings).

Every function is pure (no in-place edit of its arguments), takes a `dtype` (torch.float64: the witness; torch.float32 on the
CPU: its "twin", the same arithmetic at the precision of the code under test) and reads weights by their state_dict() names.
All integer geometry — voxel sets, point -> voxel ids, strided parents, corner indices, trilinear weights, torchsparse's hash
order — is numpy from dense_ref / oracle/pointvoxel.py, never from the HIP path.

`perturb` names ONE deliberate composition mistake (test_pointvoxel_modules_host.py shows that each moves a compared quantity
by >= 10 x its bound):
  "unbiased_var"   the stem's BatchNorm divides by rows - 1
  "drop_up1_skip"  up1 concatenates zeros instead of the stage-1 features
  "swap_concat"    up2 concatenates [skip, up-sampled] instead of [up-sampled, skip]
  "swap_z"         the GRU mix is z h + (1 - z) q
  "no_r"           convq reads [h, x] instead of [r h, x]
  "map_grad"       (fuse_walk) the map rows keep their graph from one fragment to the next"""
import numpy as np
import torch

import dense_ref as DR
from oracle import pointvoxel as PV

BN_EPS = 1e-5        # nn.BatchNorm1d's default: eps is no state_dict entry (the GPU tests assert the modules use it)


def tens(a, dtype):
    """array / tensor -> tensor of `dtype`; a tensor of that dtype passes through with its graph"""
    return DR._t64(a, dtype)


def leaves(sd, dtype, prefix=""):
    """the floating-point parameters of a state_dict under `prefix` as fresh leaf tensors of `dtype` that require a gradient
    (running statistics and counters left out: train-mode BatchNorm never reads them)"""
    out = {}
    for k, v in sd.items():
        if k.startswith(prefix) and not k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out[k] = tens(v.detach().cpu() if torch.is_tensor(v) else v, dtype).clone().requires_grad_()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# layers

def batchnorm(sd, p, x, residual=None, relu=False, unbiased=False):
    """train-mode BatchNorm over the rows: (x - mean) / sqrt(biased variance + eps) * weight + bias [+ residual] [ReLU]"""
    mean = x.mean(0, keepdim=True)
    d = x - mean
    var = (d * d).sum(0, keepdim=True) / (x.shape[0] - (1 if unbiased else 0))
    y = d / torch.sqrt(var + BN_EPS) * tens(sd[p + ".weight"], x.dtype) + tens(sd[p + ".bias"], x.dtype)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def residual_block(sd, p, x, frame, coords, stride):
    """ReLU(BN(conv3(ReLU(BN(conv3(x))))) + skip), skip = x or BN(x W) when the block changes the channel count"""
    dt = x.dtype
    y = DR.subm_conv3(frame, coords, x, sd[p + ".net.0.kernel"], stride, dtype=dt)
    y = batchnorm(sd, p + ".net.1", y, relu=True)
    y = DR.subm_conv3(frame, coords, y, sd[p + ".net.3.kernel"], stride, dtype=dt)
    skip = x
    if p + ".downsample.0.kernel" in sd:
        skip = batchnorm(sd, p + ".downsample.1", x @ tens(sd[p + ".downsample.0.kernel"], dt))
    return batchnorm(sd, p + ".net.4", y, residual=skip, relu=True)


def point_mlp(sd, p, f):
    """ReLU(BN(Linear(f)))"""
    y = f @ tens(sd[p + ".0.weight"], f.dtype).t() + tens(sd[p + ".0.bias"], f.dtype)
    return batchnorm(sd, p + ".1", y, relu=True)


# ---------------------------------------------------------------------------------------------------------------------
# SPVCNN

class SpvcnnGeometry:
    """the three voxel sets (strides 1, 2, 4) of a point cloud, its point -> voxel ids and corner tables at strides 1 and 4"""

    def __init__(self, pts, pres, vres):
        res = float(vres) / float(pres) if pres != 1 else float(vres)
        self.scaled, self.vox = DR.quantise_points(pts, res)
        self.c1, self.inv1 = DR.number_first(self.vox)
        self.c2, _ = DR.number_first(DR.quantise_coords(self.c1, 2))
        self.c4, _ = DR.number_first(DR.quantise_coords(self.c2, 4))
        self.inv4 = DR.lookup(self.c4, DR.quantise_coords(self.vox, 4))
        self.idx1, self.w1 = DR.corner_tables(self.c1, 1, self.scaled)
        self.idx4, self.w4 = DR.corner_tables(self.c4, 4, self.scaled)
        self.frame = DR.Frame([self.c1], 4)


def spvcnn(sd, feat, pts, pres, vres, dtype, perturb=None, geometry=None):
    """point features [N, C_in] at the metric points pts [N, 4] (x, y, z, batch) -> point features [N, cs[4]]:
    voxelise (scatter-mean), stem, point branch z0; two k2s2 down stages with residual blocks; point branch z1 = devoxelise
    (stride 4) + MLP(z0); two transposed up stages, each concatenated with the features of its resolution, then residual
    blocks; output = devoxelise (stride 1) + MLP(z1)"""
    g = geometry or SpvcnnGeometry(pts, pres, vres)
    fr, c1, c2, c4 = g.frame, g.c1, g.c2, g.c4
    feat = tens(feat, dtype)
    kw = dict(dtype=dtype)
    x0 = DR.scatter_mean(feat, g.inv1, len(c1), **kw)
    f0 = batchnorm(sd, "stem.1", DR.subm_conv3(fr, c1, x0, sd["stem.0.kernel"], 1, **kw), relu=True,
                   unbiased=perturb == "unbiased_var")
    z0 = DR.devoxelize(f0, g.idx1, g.w1, **kw)
    x1 = DR.scatter_mean(z0, g.inv1, len(c1), **kw)
    f = batchnorm(sd, "stage1.0.net.1", DR.down_conv(fr, c1, x1, c2, sd["stage1.0.net.0.kernel"], 1, **kw), relu=True)
    f1 = residual_block(sd, "stage1.2", residual_block(sd, "stage1.1", f, fr, c2, 2), fr, c2, 2)
    f = batchnorm(sd, "stage2.0.net.1", DR.down_conv(fr, c2, f1, c4, sd["stage2.0.net.0.kernel"], 2, **kw), relu=True)
    f2 = residual_block(sd, "stage2.2", residual_block(sd, "stage2.1", f, fr, c4, 4), fr, c4, 4)
    z1 = DR.devoxelize(f2, g.idx4, g.w4, **kw) + point_mlp(sd, "point_transforms.0", z0)
    y3 = DR.scatter_mean(z1, g.inv4, len(c4), **kw)
    u = batchnorm(sd, "up1.0.net.1", DR.up_conv(fr, c4, y3, c2, sd["up1.0.net.0.kernel"], 2, **kw), relu=True)
    f = torch.cat([u, torch.zeros_like(f1) if perturb == "drop_up1_skip" else f1], 1)
    f = residual_block(sd, "up1.1.1", residual_block(sd, "up1.1.0", f, fr, c2, 2), fr, c2, 2)
    u = batchnorm(sd, "up2.0.net.1", DR.up_conv(fr, c2, f, c1, sd["up2.0.net.0.kernel"], 1, **kw), relu=True)
    f = torch.cat([f0, u] if perturb == "swap_concat" else [u, f0], 1)
    f = residual_block(sd, "up2.1.1", residual_block(sd, "up2.1.0", f, fr, c1, 1), fr, c1, 1)
    return DR.devoxelize(f, g.idx1, g.w1, **kw) + point_mlp(sd, "point_transforms.1", z1)


# ---------------------------------------------------------------------------------------------------------------------
# ConvGRU

class PackedFrame:
    """A dense volume for a voxel set that is far too spread out to embed as it lies (the second voxelisation of a ConvGRU
    divides voxel-unit coordinates by the resolution AGAIN: at 0.04 m every voxel lands ~25 cells from the next one).

    The set is split into its clusters — voxels linked through the 3 x 3 x 3 neighbourhood, the batch index part of the
    identity — and the clusters are laid side by side (shelves along z, then y, then x) with one empty cell between them.
    Inside a cluster every relative position is kept and no two clusters touch, so each voxel has exactly the neighbours,
    at exactly the offsets, it has in the original set: a padded conv3d on this volume read at the active sites IS the
    submanifold convolution.  Same embed / read interface as dense_ref.Frame at stride 1."""

    def __init__(self, coords):
        c = np.asarray(coords, np.int64).reshape(-1, 4)
        rows = [tuple(r) for r in c.tolist()]
        ids = {r: i for i, r in enumerate(rows)}
        assert len(ids) == len(rows), "voxel rows must be unique"
        root = list(range(len(rows)))

        def find(i):
            while root[i] != i:
                root[i] = root[root[i]]
                i = root[i]
            return i

        offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) > (0, 0, 0)]
        for i, (b, x, y, z) in enumerate(rows):
            for dx, dy, dz in offs:
                j = ids.get((b, x + dx, y + dy, z + dz))
                if j is not None:
                    root[find(j)] = find(i)
        label = np.array([find(i) for i in range(len(rows))])
        members = [np.nonzero(label == r)[0] for r in np.unique(label)]
        lo = [c[m, 1:].min(0) for m in members]
        ext = [c[m, 1:].max(0) - l + 1 for m, l in zip(members, lo)]
        side = max(int(max(e.max() for e in ext)), int(np.ceil(sum(float(np.prod(e + 1)) for e in ext) ** (1 / 3))))
        packed = np.zeros((len(rows), 3), np.int64)
        x0 = y0 = z0 = 0          # the corner the next cluster goes to
        dx_slab = dy_row = 0      # thickness of the current x slab / y row
        for m, l, e in zip(members, lo, ext):
            if z0 + e[2] > side:
                y0, z0, dy_row = y0 + dy_row + 1, 0, 0
            if y0 + e[1] > side:
                x0, y0, z0, dx_slab, dy_row = x0 + dx_slab + 1, 0, 0, 0, 0
            packed[m] = c[m, 1:] - l + (x0, y0, z0)
            z0 += e[2] + 1
            dy_row, dx_slab = max(dy_row, int(e[1])), max(dx_slab, int(e[0]))
        self.shape = tuple(int(v) + 1 for v in packed.max(0))
        self.index = torch.from_numpy((packed[:, 0] * self.shape[1] + packed[:, 1]) * self.shape[2] + packed[:, 2])
        self.rows = ids
        assert len(np.unique(self.index.numpy())) == len(rows)

    def flat(self, coords, stride=1):
        assert stride == 1
        return self.index[[self.rows[tuple(r)] for r in np.asarray(coords, np.int64).reshape(-1, 4).tolist()]]

    def embed(self, coords, feat, stride=1, dtype=DR.F64):
        feat = DR._t64(feat, dtype)
        x, y, z = self.shape
        vol = torch.zeros((x * y * z, feat.shape[1]), dtype=dtype).index_add(0, self.flat(coords, stride), feat)
        return vol.reshape(1, x, y, z, -1).permute(0, 4, 1, 2, 3)

    def read(self, vol, coords, stride=1):
        return vol.permute(0, 2, 3, 4, 1).reshape(-1, vol.shape[1])[self.flat(coords, stride)]


def _hash_ordered(coords, inverse):
    """a voxel set renumbered by ascending torchsparse hash (ties keep their first-occurrence order)"""
    perm = np.argsort(PV.sphash(coords), kind="stable")
    rank = np.empty_like(perm)
    rank[perm] = np.arange(len(perm))
    return coords[perm], rank[inverse]


class GruGeometry:
    """the two voxelisations the three gate convolutions of a cell see: `first` of the metric points (convz, convq), `second`
    of the points convz already divided by the resolution (convr).  Each is (frame, coords, point -> voxel ids, corner
    indices, corner weights).  literal: both sets numbered in hash order and convr devoxelising with the FIRST set's corner
    indices and weights applied to the second set (indices past its end dropped) — what the reference's cached tables do."""

    def __init__(self, pts, pres, vres, literal):
        res = float(vres) / float(pres) if pres != 1 else float(vres)
        sc1, vox1 = DR.quantise_points(pts, res)
        sc2, vox2 = DR.quantise_points(sc1, res)
        c1, inv1 = DR.number_first(vox1)
        c2, inv2 = DR.number_first(vox2)
        if literal:
            c1, inv1 = _hash_ordered(c1, inv1)
            c2, inv2 = _hash_ordered(c2, inv2)
        idx1, w1 = DR.corner_tables(c1, 1, sc1)
        if literal:
            idx2, w2 = np.where(idx1 < len(c2), idx1, -1), w1
        else:
            idx2, w2 = DR.corner_tables(c2, 1, sc2)
        self.first = (PackedFrame(c1), c1, inv1, idx1, w1)
        self.second = (PackedFrame(c2), c2, inv2, idx2, w2)


def sconv3d(sd, p, f, vox):
    """devoxelise(conv3(scatter-mean(f))) + Linear(f) on one voxelisation"""
    frame, coords, inv, idx, w = vox
    dt = f.dtype
    y = DR.subm_conv3(frame, coords, DR.scatter_mean(f, inv, len(coords), dtype=dt), sd[p + ".net.kernel"], 1, dtype=dt)
    lin = f @ tens(sd[p + ".point_transforms.0.weight"], dt).t() + tens(sd[p + ".point_transforms.0.bias"], dt)
    return DR.devoxelize(y, idx, w, dtype=dt) + lin


def convgru(sd, prefix, h, x, pts, pres, vres, literal, dtype, perturb=None, geometry=None):
    """z = sigmoid(convz([h, x])), r = sigmoid(convr([h, x])), q = convq([r h, x]), h' = (1 - z) h + z tanh(q)"""
    g = geometry or GruGeometry(pts, pres, vres, literal)
    p = prefix + "." if prefix else ""
    h, x = tens(h, dtype), tens(x, dtype)
    hx = torch.cat([h, x], 1)
    z = DR.gate(sconv3d(sd, p + "convz", hx, g.first), 1, dtype=dtype)
    rh = h if perturb == "no_r" else DR.gate(sconv3d(sd, p + "convr", hx, g.second), 2, h, dtype=dtype)
    q = sconv3d(sd, p + "convq", torch.cat([rh, x], 1), g.first)
    return DR.gate(q, 3, h, 1 - z if perturb == "swap_z" else z, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# one GRUFusion level

def fuse_level(sd, scale, h_rows, cur_rows, src_cur, pts, pres, vres, ch_voxel, literal, dtype, perturb=None, geometry=None):
    """the voxel-channel and image-channel ConvGRU of one fusion level over a union of N' voxels at the points pts [N', 4]:
    h_rows [N', C] the map's rows (constant: state), x_rows = cur_rows[src_cur] with zero rows where src_cur < 0 (the union
    holds a voxel the fragment does not); -> fused rows [N', C] = [voxel cell | image cell]"""
    g = geometry or GruGeometry(pts, pres, vres, literal)
    h = tens(h_rows, dtype)
    if perturb != "map_grad":
        h = h.detach()
    cur = tens(cur_rows, dtype)
    src = torch.as_tensor(np.asarray(src_cur), dtype=torch.int64)
    pad = torch.cat([cur, cur.new_zeros(1, cur.shape[1])])
    x = pad[torch.where(src >= 0, src, torch.full_like(src, cur.shape[0]))]
    cells = []
    for name, cols in (("fusion_nets_voxel", slice(0, ch_voxel)), ("fusion_nets_img", slice(ch_voxel, None))):
        cells.append(convgru(sd, f"{name}.{scale}", h[:, cols], x[:, cols], pts, pres, vres, literal, dtype, perturb, g))
    return torch.cat(cells, 1)

"""float64 dense formulations of the point-voxel layers (SPVCNN, SConv3d / ConvGRU, the strided sparse convolutions) — test
helpers, written from the reference's call sites (ops/torchsparse_utils.py:15-105, models/modules.py:15-222) and the closed
forms of SURVEY.md appendix A.2, independently of oracle/ and eprecon_amd/: no kernel map, no hash, no CSR list.

A sparse set of (b, x, y, z) rows is embedded in a dense [B, C, X, Y, Z] volume (absent voxels hold 0), the convolutions are
F.conv3d / F.conv_transpose3d on that volume read back at the active sites, voxels are numbered by a Python dict in
first-occurrence order, and every sum is float64.  (The differentiable blocks take a `dtype`, float64 unless said otherwise:
tests/pointvoxel_modules_ref.py runs the same formulation in float32 to measure what that precision alone costs.)"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _t64(a, dtype=F64):
    """a as a tensor of `dtype` (float64 unless a caller asks for the same formulation in another precision)"""
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64)).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# dense embedding

class Frame:
    """A cubic dense volume that holds every row of the coordinate sets it is built from.

    Coordinates are shifted by `shift`, a non-negative MULTIPLE OF `quantum` (the coarsest tensor stride involved, e.g.
    2^levels), so that negative coordinates land inside the volume while each coordinate keeps its residue modulo every
    stride up to `quantum`: a voxel floors to the same parent in the shifted frame as in the original one, and a conv3d
    with stride 2 on the shifted volume pairs exactly the children a floor division pairs.  An odd shift would move -1 to an
    even index and make a truncating division (-1 / 2 = 0 instead of -1) look correct.  The side is a multiple of `quantum`
    so that the volume subsampled at every stride s <= quantum tiles it exactly."""

    def __init__(self, coords_list, quantum):
        rows = np.concatenate([np.asarray(c, np.int64).reshape(-1, 4) for c in coords_list])
        self.quantum = int(quantum)
        lo, hi = int(rows[:, 1:].min()), int(rows[:, 1:].max())
        self.shift = self.quantum * max(0, math.ceil(-lo / self.quantum))
        self.side = self.quantum * math.ceil((hi + self.shift + 1) / self.quantum)
        self.batch = int(rows[:, 0].max()) + 1
        assert self.shift % self.quantum == 0 and lo + self.shift >= 0 and hi + self.shift < self.side

    def flat(self, coords, stride=1):
        """row index of each (b, x, y, z) in the [B * D^3] cells of the volume subsampled at `stride`"""
        c = np.asarray(coords, np.int64).reshape(-1, 4)
        xyz = c[:, 1:] + self.shift
        assert self.side % stride == 0 and (xyz % stride == 0).all(), "coordinates not on the stride's lattice"
        xyz = xyz // stride
        d = self.side // stride
        return torch.from_numpy(((c[:, 0] * d + xyz[:, 0]) * d + xyz[:, 1]) * d + xyz[:, 2])

    def embed(self, coords, feat, stride=1, dtype=F64):
        """feat [N, C] at the rows `coords` -> float64 volume [B, C, D, D, D] (D = side / stride), differentiable in feat"""
        feat = _t64(feat, dtype)
        d = self.side // stride
        vol = torch.zeros((self.batch * d ** 3, feat.shape[1]), dtype=dtype).index_add(0, self.flat(coords, stride), feat)
        return vol.reshape(self.batch, d, d, d, -1).permute(0, 4, 1, 2, 3)

    def read(self, vol, coords, stride=1):
        """the [N, C] rows of a volume embedded at `stride`, read at `coords`"""
        c = vol.shape[1]
        return vol.permute(0, 2, 3, 4, 1).reshape(-1, c)[self.flat(coords, stride)]


# ---------------------------------------------------------------------------------------------------------------------
# convolutions (weights in this project's [K, C_in, C_out] layout)

def dense_weight(w, ksize, dtype=F64):
    """[K, C_in, C_out] -> F.conv3d's [C_out, C_in, kx, ky, kz] on a volume indexed (x, y, z).
    k = 3: offset k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) (x fastest); k = 2: k = 4 bx + 2 by + bz (z fastest)."""
    w = _t64(w, dtype)
    cin, cout = w.shape[1], w.shape[2]
    if ksize == 3:
        return w.reshape(3, 3, 3, cin, cout).permute(4, 3, 2, 1, 0)       # (dz, dy, dx, ci, co) -> (co, ci, dx, dy, dz)
    assert ksize == 2
    return w.reshape(2, 2, 2, cin, cout).permute(4, 3, 0, 1, 2)           # (bx, by, bz, ci, co) -> (co, ci, bx, by, bz)


def _bias(bias, dtype=F64):
    return None if bias is None else _t64(bias, dtype)


def subm_conv3(frame, coords, x, w, stride=1, bias=None, dtype=F64):
    """submanifold k=3 convolution at tensor stride s: out[i] = bias + sum over the 27 offsets o of x[coords[i] + o s] W[o]
    = conv3d (padding 1) on the volume subsampled by s, read at the active sites"""
    vol = frame.embed(coords, x, stride, dtype)
    return frame.read(F.conv3d(vol, dense_weight(w, 3, dtype), _bias(bias, dtype), padding=1), coords, stride)


def down_conv(frame, fine, x, coarse, w, stride=1, bias=None, dtype=F64):
    """k2s2 convolution from the fine set at tensor stride s to the coarse set at 2s: out[j] = sum over b in {0,1}^3 of
    x[coarse[j] + b s] W[4 bx + 2 by + bz] = conv3d (stride 2) read at the coarse sites"""
    vol = frame.embed(fine, x, stride, dtype)
    return frame.read(F.conv3d(vol, dense_weight(w, 2, dtype), _bias(bias, dtype), stride=2), coarse, 2 * stride)


def up_conv(frame, coarse, x, fine, w, stride=1, bias=None, dtype=F64):
    """transposed k2s2 convolution from the coarse set at 2s back to the fine set at s: fine voxel i, child b of its parent
    p, gets x[p] W[4 bx + 2 by + bz] = conv_transpose3d (stride 2) from the coarse set, restricted to the fine set"""
    vol = frame.embed(coarse, x, 2 * stride, dtype)
    wt = dense_weight(w, 2, dtype).transpose(0, 1)                                # conv_transpose3d: [C_in, C_out, kx, ky, kz]
    return frame.read(F.conv_transpose3d(vol, wt, _bias(bias, dtype), stride=2), fine, stride)


# ---------------------------------------------------------------------------------------------------------------------
# voxelisation

def quantise_points(pts_xyzb, res):
    """ops/torchsparse_utils.py:16-17: the quotient p / res is a FLOAT32 division there (a float tensor divided by a Python
    scalar), then floored.  A float64 quotient can floor to another integer for a point within an ulp of a voxel face, so
    the quotient is formed in float32 and only the floor is exact.
    -> scaled f32[N, 4] (x / res, y / res, z / res, b), voxel int64[N, 4] (b, floor x, floor y, floor z)"""
    p = np.asarray(pts_xyzb, np.float32)
    scaled = p.copy()
    scaled[:, :3] = p[:, :3] / np.float32(res)
    vox = np.concatenate([p[:, 3:4].astype(np.int64), np.floor(scaled[:, :3].astype(np.float64)).astype(np.int64)], 1)
    return scaled, vox


def quantise_coords(coords, q):
    """(b, x, y, z) -> (b, floor(x / q) q, ...): floor toward -inf, in exact float64 arithmetic on small integers"""
    c = np.asarray(coords, np.int64).reshape(-1, 4).copy()
    c[:, 1:] = np.floor(c[:, 1:].astype(np.float64) / q).astype(np.int64) * q
    return c


def number_first(rows):
    """unique rows numbered by first occurrence -> (unique int64[M, 4], inverse int64[N])"""
    ids, inverse, uniq = {}, [], []
    for r in map(tuple, np.asarray(rows, np.int64).reshape(-1, 4).tolist()):
        if r not in ids:
            ids[r] = len(uniq)
            uniq.append(r)
        inverse.append(ids[r])
    return np.array(uniq, np.int64).reshape(-1, 4), np.array(inverse, np.int64)


def lookup(table_rows, query_rows):
    """row of each query in table_rows (first occurrence), -1 when absent"""
    ids = {}
    for i, r in enumerate(map(tuple, np.asarray(table_rows, np.int64).reshape(-1, 4).tolist())):
        ids.setdefault(r, i)
    return np.array([ids.get(r, -1) for r in map(tuple, np.asarray(query_rows, np.int64).reshape(-1, 4).tolist())], np.int64)


def scatter_mean(feat, inverse, m, dtype=F64):
    """float64 mean of the rows of feat per target (index_add_ + counts); rows with target -1 are dropped, empty targets 0"""
    feat = _t64(feat, dtype)
    inv = torch.as_tensor(np.asarray(inverse), dtype=torch.int64)
    live = inv >= 0
    s = torch.zeros((m, feat.shape[1]), dtype=dtype).index_add(0, inv[live], feat[live])
    n = torch.zeros(m, dtype=dtype).index_add_(0, inv[live], torch.ones(int(live.sum()), dtype=dtype))
    return s / n.clamp(min=1)[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# trilinear corner tables and devoxelisation

def corner_tables(vox_coords, stride, scaled_xyzb):
    """SURVEY.md appendix A.2 in closed form, float64: base pf = floor(p / s) s, pc = pf + s; corner k = 4 bx + 2 by + bz at
    pf + (bx, by, bz) s; w_k = prod over the axes of (bit ? p - pf : pc - p) / s^3, 0 for an absent corner, then
    w /= (sum w + 1e-8).  -> idx int64[N, 8] (row in vox_coords or -1), w float64[N, 8].
    The quotient p / s is a float32 division in the reference (ops/torchsparse_utils.py:75-76, torchsparse's calc_ti_weights on
    float tensors), exact for a power-of-two s except for a subnormal p, whose half rounds to -0.0 / 0.0: formed in float32."""
    p32 = np.asarray(scaled_xyzb, np.float32)
    p = p32.astype(np.float64)
    s = float(stride)
    pf = np.floor((p32[:, :3] / np.float32(stride)).astype(np.float64)) * s
    pc = pf + s
    base = pf.astype(np.int64)
    b = p[:, 3].astype(np.int64)
    ids = {}
    for i, r in enumerate(map(tuple, np.asarray(vox_coords, np.int64).reshape(-1, 4).tolist())):
        ids.setdefault(r, i)
    n = len(p)
    idx = np.full((n, 8), -1, np.int64)
    w = np.zeros((n, 8))
    for k in range(8):
        o = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
        corner = base + o[None] * stride
        idx[:, k] = [ids.get((bb, x, y, z), -1) for bb, (x, y, z) in zip(b.tolist(), corner.tolist())]
        f = np.prod([np.where(o[a], p[:, a] - pf[:, a], pc[:, a] - p[:, a]) for a in range(3)], 0) / s ** 3
        w[:, k] = np.where(idx[:, k] >= 0, f, 0.0)
    return idx, w / (w.sum(1, keepdims=True) + 1e-8)


def devoxelize(vfeat, idx, w, dtype=F64):
    """out[p] = sum_k w[p, k] vfeat[idx[p, k]] over the present corners, float64, differentiable in vfeat"""
    vfeat = _t64(vfeat, dtype)
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    w = _t64(w, dtype)
    pad = torch.cat([vfeat, vfeat.new_zeros(1, vfeat.shape[1])])
    rows = torch.where(idx >= 0, idx, torch.full_like(idx, vfeat.shape[0]))
    return (pad[rows] * torch.where(idx >= 0, w, torch.zeros_like(w))[:, :, None]).sum(1)


# ---------------------------------------------------------------------------------------------------------------------
# ConvGRU gates (models/modules.py:214-221)

def gate(v, mode, h=None, zg=None, dtype=F64):
    """mode 1 sigmoid(v) (update gate z), 2 sigmoid(v) h (r h), 3 (1 - z) h + z tanh(v) (new hidden state), float64"""
    v = _t64(v, dtype)
    if mode == 3:
        h, zg = _t64(h, dtype), _t64(zg, dtype)
        return (1 - zg) * h + zg * torch.tanh(v)
    r = torch.sigmoid(v)
    return r * _t64(h, dtype) if mode == 2 else r

"""Float64 reference of the convolution family (csrc/sparse_conv.hip and the family units csrc/sparse_conv_*.hip it dispatches to), in plain torch.

Independent of oracle/: every function works on torch tensors (on the GPU when the operands are there, so the references of
long lists stay cheap) and computes in float64.  Each result comes with S = sum |a| |w| + |b| + |residual| (+ |out| for
`accumulate`) per output element, the scale a per-element tolerance is taken relative to.

    y[i] = [LN]( [ReLU]( sum_k a[nbr[k, i]] @ W[k] + b [+ out] ) [+ res] )     a = [ReLU](x * scale + shift) for live rows

A missing neighbour (nbr = -1, a cell outside the grid or the image) contributes 0, never ReLU(shift).  Maps are used as
given: the caller builds them (in numpy) and hands the same table to the kernel.
"""
import torch
import torch.nn.functional as F

D = torch.float64


def prologue(x, in_affine=None):
    """the producer's pending BatchNorm applied on load: x float64 [n, C] -> a"""
    x = x.to(D)
    if in_affine is None:
        return x
    scale, shift, relu = in_affine
    a = x * scale.to(D) + shift.to(D)
    return a.clamp_min(0.0) if relu else a


def gather_conv(x, w, nbr, in_affine=None):
    """sum_k a[nbr[k, i]] @ W[k] over an explicit table (nbr None: identity, K = 1) -> (acc, S) float64 [n_out, C_out]"""
    a = prologue(x, in_affine)
    w = w.to(D)
    if w.dim() == 2:
        w = w.unsqueeze(0)
    if nbr is None:
        return a @ w[0], a.abs() @ w[0].abs()
    nbr = nbr.to(a.device).long()
    kvol, n_out = nbr.shape
    acc = torch.zeros((n_out, w.shape[2]), dtype=D, device=a.device)
    s = torch.zeros_like(acc)
    for k in range(kvol):
        live = nbr[k] >= 0
        if not bool(live.any()):
            continue
        rows = a[nbr[k][live]]
        acc[live] += rows @ w[k]
        s[live] += rows.abs() @ w[k].abs()
    return acc, s


def image_conv(x, w, maps, height, width, in_affine=None):
    """3x3 'same' convolution over [maps][height][width] channels-last pixel rows (offset k = 3 ky + kx), zero padding"""
    a = prologue(x, in_affine)
    cin, cout = w.shape[1], w.shape[2]
    img = a.view(maps, height, width, cin).permute(0, 3, 1, 2)
    w4 = w.to(D).view(3, 3, cin, cout).permute(3, 2, 0, 1)
    acc = F.conv2d(img, w4, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    s = F.conv2d(img.abs(), w4.abs(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    return acc, s


def grid_conv(x, w, cells, dims, in_affine=None):
    """3x3x3 stride-1 convolution of the rows of a set living on a dense grid: cells int64 [n, 3] (x, y, z in grid cells),
    offset k = (k % 3 - 1, k / 3 % 3 - 1, k / 9 - 1) in (x, y, z); empty cells and cells off the grid contribute 0"""
    a = prologue(x, in_affine)
    cin, cout = w.shape[1], w.shape[2]
    gx, gy, gz = dims
    cells = cells.to(a.device).long()
    vol = torch.zeros((1, cin, gx, gy, gz), dtype=D, device=a.device)
    vol[0, :, cells[:, 0], cells[:, 1], cells[:, 2]] = a.t()
    w5 = w.to(D).view(3, 3, 3, cin, cout).permute(4, 3, 2, 1, 0)      # [co][ci][dx][dy][dz]
    pick = lambda v: v[0][:, cells[:, 0], cells[:, 1], cells[:, 2]].t()
    return pick(F.conv3d(vol, w5, padding=1)), pick(F.conv3d(vol.abs(), w5.abs(), padding=1))


def epilogue(acc, s, bias=None, relu=False, residual=None, res_affine=None, out=None, ln=None):
    """v = acc + b [+ out]; [ReLU]; [+ residual] (res_affine = (scale, shift, relu): the residual's own pending BatchNorm);
    ln = (gamma, beta, eps, post_relu): row-wise LayerNorm over the output channels -> (y, S)"""
    v, s = acc.clone(), s.clone()
    if bias is not None:
        v += bias.to(D)
        s += bias.to(D).abs()
    if out is not None:
        v += out.to(D)
        s += out.to(D).abs()
    if relu:
        v = v.clamp_min(0.0)
    if residual is not None:
        r = prologue(residual, res_affine)
        v += r
        s += r.abs()
    if ln is not None:
        gamma, beta, eps, post_relu = ln
        mean = v.mean(1, keepdim=True)
        var = ((v - mean) ** 2).mean(1, keepdim=True)
        v = (v - mean) / torch.sqrt(var + eps)
        if gamma is not None:
            v = v * gamma.to(D)
        if beta is not None:
            v = v + beta.to(D)
        if post_relu:
            v = v.clamp_min(0.0)
    return v, s


def column_stats(y):
    """(count, mean, M2) per column of rows y, float64"""
    y = y.to(D)
    n = y.shape[0]
    mean = y.mean(0) if n else torch.zeros(y.shape[1], dtype=D, device=y.device)
    return n, mean, ((y - mean) ** 2).sum(0)


def merge_summaries(partial):
    """Chan merge, in float64, of per-workgroup (count, mean, M2) summaries [rows, 3, C] -> (count [C], mean [C], M2 [C])"""
    p = partial.to(D)
    n, m, q = p[:, 0], p[:, 1], p[:, 2]
    tot = n.sum(0)
    mean = (n * m).sum(0) / tot.clamp_min(1.0)
    return tot, mean, (q + n * (m - mean) ** 2).sum(0)


def bn_affine(y, gamma, beta, eps):
    """train-mode BatchNorm of rows y in affine form (biased variance): (scale, shift) float64"""
    n, mean, m2 = column_stats(y)
    scale = gamma.to(D) / torch.sqrt(m2 / n + eps)
    return scale, beta.to(D) - mean * scale


def weight_grad(x, dy, nbr, kvol):
    """dW[k] = sum_i x[nbr[k, i]]^T dy[i] (nbr None: identity) -> float64 [K, C_in, C_out]"""
    x, dy = x.to(D), dy.to(D)
    dw = torch.zeros((kvol, x.shape[1], dy.shape[1]), dtype=D, device=x.device)
    if nbr is None:
        dw[0] = x.t() @ dy
        return dw
    nbr = nbr.to(x.device).long()
    for k in range(kvol):
        live = nbr[k] >= 0
        if bool(live.any()):
            dw[k] = x[nbr[k][live]].t() @ dy[live]
    return dw

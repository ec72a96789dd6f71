"""Float64 references of the normalisation, head and decoder kernels (csrc/norm.hip, heads.hip, backbone2d.hip, decoder.hip),
in plain torch, with a first-order bound on the error of the fp32 kernel.

Independent of oracle/: every function works on torch tensors (on the GPU when the operands are there) and computes in
float64.  Each returns (y, E): y the exact result of the operation on the given fp32 inputs, E >= 0 per element, a
first-order bound on |y_fp32 - y| for a kernel that rounds each operation once (u = 2^-24) and sums m terms in some fixed
order (gamma_m = m u).  E is built op by op; m is stated per kernel from its own summation structure (the M_* helpers).

    matmul / GEMV   y = a W + b               E_y = E_a |W| + gamma_K (|a| |W| + |b|)
    ReLU                                      E passes unchanged
    residual add    s = a + b                 E_s = E_a + E_b + u |s|
    normalisation   y = (t - mu) / s_e g + b  over the reduced axis, s_e = sqrt(var + eps), d = t - mu, z = |d| / s_e:
                    E_y = |g| / s_e (E_t + mean E_t + gamma_m (|d| + mean |t|) + z (mean(z E_t) + gamma_m mean |t|))
                          + 2 u (|g| z + |b|)
                    (the first terms are the error of t and of the mean, the z-term that of the variance: its deviations
                    and the means of the sub-blocks it was merged from; the last the affine's two roundings)
    softmax-weighted sum  A = sum_j p_j V_j, p = softmax(s) over the allowed keys:
                    rho_j = 2 u + u |s_j - M| (+ u (M - min s) for v_exp_f32 with running rescales), M = max s,
                    e_j = E_s,j + rho_j,  E_p,j = p_j (e_j + sum_k p_k e_k + gamma_m)
                    E_A = sum_j (E_p,j |V_j| + p_j E_V,j) + gamma_m sum_j p_j |V_j|
    sin / cos       E = |cos p| E_p + 2 u   (resp. |sin p|): the libm error of sinf / cosf after range reduction
    row-wise chain  (heads, query-side blocks) E = |J_0| E_in + sum_s |J_s| e_s: each stage's own rounding e_s (the rules
                    above with an exact input) carried to the output by the float64 Jacobian J_s of the rest of the chain

A test passes when |y_kernel - y| <= C_SAFE * E for every element.
"""
import math

import torch
import torch.nn.functional as F

D = torch.float64
U = 2.0 ** -24
C_SAFE = 4.0


def gam(m):
    return float(m) * U


def f64(t):
    return t.detach().to(D)


# ---- the rules --------------------------------------------------------------------------------------------------------
def linear(a, ea, w, b=None, m=None):
    """a [.., K] @ w [K, N] + b: m defaults to K + 2 (a k-ordered chain and the bias)"""
    w = f64(w)
    m = w.shape[0] + 2 if m is None else m
    y = a @ w
    s = a.abs() @ w.abs()
    if b is not None:
        y = y + f64(b)
        s = s + f64(b).abs()
    return y, ea @ w.abs() + gam(m) * s


def add(a, ea, b, eb):
    s = a + b
    return s, ea + eb + U * s.abs()


def normalise(t, et, g, b, eps, dim, m):
    """(t - mean) / sqrt(biased var + eps) * g + b over `dim`; g / b broadcast (None: 1 / 0)"""
    mu = t.mean(dim, keepdim=True)
    d = t - mu
    var = (d * d).mean(dim, keepdim=True)
    se = torch.sqrt(var + eps)
    g = torch.ones((), dtype=D, device=t.device) if g is None else g
    b = torch.zeros((), dtype=D, device=t.device) if b is None else b
    y = d / se * g + b
    z = d.abs() / se
    mabs = t.abs().mean(dim, keepdim=True)
    e = g.abs() / se * (et + et.mean(dim, keepdim=True) + gam(m) * (d.abs() + mabs)
                        + z * ((z * et).mean(dim, keepdim=True) + gam(m) * mabs)) + 2 * U * (g.abs() * z + b.abs())
    return y, e


def softmax_av(s, es, v, ev, allowed, m, fast_exp):
    """A = softmax(s over the allowed keys) @ v; s / es [.., Nk], v / ev [Nk, Dv] (or [.., Nk, Dv]), allowed bool [.., Nk]"""
    neg = torch.tensor(-math.inf, dtype=D, device=s.device)
    sm = torch.where(allowed, s, neg)
    mx = sm.amax(-1, keepdim=True)
    p = torch.softmax(sm, -1)
    rho = 2 * U + U * (s - mx).abs()
    if fast_exp:
        mn = torch.where(allowed, s, torch.full_like(s, math.inf)).amin(-1, keepdim=True)
        rho = rho + U * (mx - mn)
    e = torch.where(allowed, es + rho, torch.zeros_like(s))
    ep = p * (e + (p * e).sum(-1, keepdim=True) + gam(m))
    a = p @ v
    return a, ep @ v.abs() + p @ ev + gam(m) * (p @ v.abs())


# ---- the kernels' sum lengths ------------------------------------------------------------------------------------------
CHAN = 5    # roundings of one Chan merge, counted against the magnitude of the merged mean / M2


def m_bn_train(n, C, nblk=None):
    """bn_stats_kernel: 8 rows per thread, a tree over 256 / C row groups; bn_finalize: ceil(nblk / 256) merges per thread,
    an 8-level tree; then the division, sqrt and reciprocal"""
    rpi = 256 // C
    nblk = -(-max(n, 1) // (8 * rpi)) if nblk is None else nblk
    return 8 + CHAN * (math.ceil(math.log2(max(rpi, 1))) + 1 + -(-nblk // 256) + 8) + 4


def m_bn_views(rows, C, chunks):
    """bn_views_stats_kernel: a lane merges ceil(per / R) rows four at a time (two-pass over the four), the R lanes merged in
    order, the chunks merged in order by the finalize"""
    r = 256 // (C // 4)
    per = -(-rows // chunks)
    return 4 + CHAN * (-(-per // (4 * r)) + 3 + r + chunks) + 8


def m_rowwise_ln(C):
    """rowwise_ln_kernel: 8 lanes per row, ceil(C / 8) terms each, three xor adds"""
    return -(-C // 8) + 3 + 4


def m_qs_ln():
    """qs_layernorm: one wave per row, a 64-lane xor tree"""
    return 6 + 4


def bn_train(x, gamma, beta, eps, m):
    """train-mode BatchNorm of rows x [n, C]: batch statistics, biased variance"""
    x = f64(x)
    return normalise(x, torch.zeros_like(x), None if gamma is None else f64(gamma), None if beta is None else f64(beta), eps, 0, m)


def bn_views(x, views, gamma, beta, eps, m, relu=False):
    """per-view train-mode BatchNorm2d of [V * B, C, H, W] (statistics over (B, H, W) of each view) -> NCHW (y, E)"""
    x = f64(x)
    n, c, h, w = x.shape
    t = x.reshape(views, n // views, c, h * w).transpose(1, 2).reshape(views, c, -1)
    y, e = normalise(t, torch.zeros_like(t), f64(gamma)[None, :, None], f64(beta)[None, :, None], eps, 2, m)
    back = lambda a: a.reshape(views, c, n // views, h * w).transpose(1, 2).reshape(n, c, h, w)
    y, e = back(y), back(e)
    return (y.clamp_min(0.0), e) if relu else (y, e)


def dwconv(a, ea, weight, stride):
    """depthwise k x k convolution (zero padding k // 2) of NCHW a with E_a; weight [C, 1, k, k]"""
    w = f64(weight)
    k = w.shape[-1]
    conv = lambda t, ww: F.conv2d(t, ww, stride=stride, padding=k // 2, groups=w.shape[0])
    return conv(a, w), conv(ea, w.abs()) + gam(k * k + 1) * conv(a.abs(), w.abs())


# ---- row-wise chains: the inherited error through the exact linearisation ----------------------------------------------
# A chain of stages on independent rows.  The elementwise rule E_out = |W|^T E_in compounds |W_n| ... |W_1| where the error
# really travels through |W_n ... W_1|: over three products and two LayerNorms that overstates it by more than |y| itself.
# Here each stage s contributes only its OWN rounding e_s (the rules above with an exact input), carried to the output by the
# exact float64 Jacobian J_s of the rest of the chain:  E = |J_0| E_in + sum_s |J_s| e_s  (first order, as tight as the
# linearisation).  Stages:  ("lin", W [K, N], b, m)   ("ln", g, b, eps, m)   ("relu",)   ("add", c [n, N]: an exact operand)
#                           ("res", [stages]): y = x + sub(x)
def _forward(x, stages):
    recs = []
    for st in stages:
        kind = st[0]
        if kind == "lin":
            w = f64(st[1])
            y, e = linear(x, torch.zeros_like(x), w, st[2], st[3])
            recs.append((kind, w, e))
        elif kind == "ln":
            g, b = f64(st[1]), f64(st[2])
            y, e = normalise(x, torch.zeros_like(x), g, b, st[3], 1, st[4])
            mu = x.mean(1, keepdim=True)
            se = torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + st[3])
            recs.append((kind, (g / se, (x - mu) / se), e))
        elif kind == "relu":
            y = x.clamp_min(0.0)
            recs.append((kind, (x > 0).to(D), torch.zeros_like(y)))
        elif kind == "add":
            y = x + f64(st[1])
            recs.append((kind, None, U * y.abs()))
        else:
            sub, inner = _forward(x, st[1])
            y = x + sub
            recs.append((kind, inner, U * y.abs()))
        x = y
    return x, recs


def _backward(m, recs):
    """m [n, N_out, N_last] -> (sum_s |J_s| e_s [n, N_out], the Jacobian to the chain's input)"""
    tot = 0.0
    for kind, data, e in reversed(recs):
        tot = tot + (m.abs() @ e.unsqueeze(-1)).squeeze(-1)
        if kind == "lin":
            m = m @ data.t()
        elif kind == "ln":
            gs, zh = data
            m1 = m * gs.unsqueeze(1)
            n = zh.shape[1]
            m = m1 - m1.sum(-1, keepdim=True) / n - (m1 @ zh.unsqueeze(-1)) * zh.unsqueeze(1) / n
        elif kind == "relu":
            m = m * data.unsqueeze(1)
        elif kind == "res":
            t, mj = _backward(m, data)
            tot = tot + t
            m = m + mj
    return tot, m


def chain(x, stages, e_in=None, rows=4096):
    """(y, E) of a row-wise chain on x [n, K] float64 (exact, or with the bound e_in of its own error)"""
    ys, es = [], []
    for r0 in range(0, x.shape[0], rows):
        xs = x[r0:r0 + rows]
        y, recs = _forward(xs, stages)
        m = torch.eye(y.shape[1], dtype=D, device=x.device).expand(y.shape[0], -1, -1)
        e, m = _backward(m, recs)
        if e_in is not None:
            e = e + (m.abs() @ e_in[r0:r0 + rows].unsqueeze(-1)).squeeze(-1)
        ys.append(y)
        es.append(e)
    return torch.cat(ys), torch.cat(es)


def linear4x(mod, x):
    """Linear4xTrans (eprecon_amd.modules): Linear(C, 4C) - LN - ReLU - Linear(4C, C) - LN - ReLU - Linear(C, C_out) [+ h].
    Sum lengths of csrc/heads.hip: the MFMA chains run over the inputs padded to 16 (k ascending, the split kernel adds four
    wave partials); LN1 sums 4 registers x T1 tiles per lane and two xor adds (+ four wave partials), LN2 4 x T2 + 2."""
    x = f64(x)
    c = mod.linear1.in_features
    kc = -(-c // 16)
    t1 = 4 * c // 16
    lin = lambda layer, m: ("lin", layer.weight.t(), layer.bias, m)
    tail = [lin(mod.linear2, 4 * c + 6), ("ln", mod.norm2.weight, mod.norm2.bias, mod.norm2.eps, 4 * kc + 6), ("relu",)]
    head = [lin(mod.linear1, 16 * kc + 6), ("ln", mod.norm1.weight, mod.norm1.bias, mod.norm1.eps, 4 * t1 + 10), ("relu",)] + tail
    if mod.use_residual:       # y = W3 h + b3 + h: the skip is the chain's last stage
        return chain(x, head + [("res", [lin(mod.linear3, 16 * kc + 6)])])
    return chain(x, head + [lin(mod.linear3, 16 * kc + 6)])


def level_keys(coords, feats, level_embed, gauss_b, extent):
    """src = feats + level_embed, keys = src + [sin p | cos p], p = (2 pi coords / extent) @ gauss_B (PositionEmbeddingCoordsSine
    with normalize=True) -> (src, E_src), (keys, E_keys).  p's error: coords / extent and * 2 pi (with 2 pi rounded to fp32)
    three roundings, the three-term fma chain gamma_3."""
    f, le, gb = f64(feats), f64(level_embed), f64(gauss_b)
    src = f + le
    esrc = U * src.abs()
    x = f64(coords) / torch.tensor([float(v) for v in extent], dtype=D, device=f.device) * (2 * math.pi)
    p = x @ gb
    ep = (3 * U * x.abs()) @ gb.abs() + gam(3) * (x.abs() @ gb.abs())
    pe = torch.cat([p.sin(), p.cos()], 1)
    epe = torch.cat([p.cos().abs() * ep, p.sin().abs() * ep], 1) + 2 * U
    keys, ekeys = add(src, esrc, pe, epe)
    return (src, esrc), (keys, ekeys)


def att_groups(n_keys):
    """csrc/decoder.hip att_groups: (keys per workgroup, workgroups)"""
    per = max(-(-(-(-n_keys // 768)) // 64) * 64, 64)
    return per, -(-n_keys // per)


def blocked_mask(logits_t, rows, n_keys):
    """bool [Q, N]: torch's own fp32 sigmoid(...) < 0.5 on the logits' device (rows None: identity)"""
    lg = logits_t[:n_keys] if rows is None else logits_t[rows.long()]
    return (torch.sigmoid(lg.float()) < 0.5).t()


def masked_attention(q, k, v, scale, blocked=None):
    """out [1, H, Q, Dh] of the split-K kernel: q [1, H, Q, Dh], k / v [N, H * Dh]; blocked bool [Q, N] (True = masked, a query
    with every key blocked attends to all).  Sum length: a workgroup's keys in order with a rescale per 8 keys, then the
    workgroups merged by a lane each (ceil(G / 64)) and a 6-level butterfly, every merge with two rescales."""
    _, h, nq, dh = q.shape
    n = k.shape[0]
    qq = f64(q)[0]                                               # [H, Q, Dh]
    kk = f64(k).view(n, h, dh).transpose(0, 1)                   # [H, N, Dh]
    vv = f64(v).view(n, h, dh).transpose(0, 1)
    s = scale * qq @ kk.transpose(1, 2)                          # [H, Q, N]
    es = gam(dh + 3) * scale * (qq.abs() @ kk.abs().transpose(1, 2))
    allowed = torch.ones((nq, n), dtype=torch.bool, device=s.device) if blocked is None else ~blocked.to(s.device)
    allowed = torch.where(allowed.any(1, keepdim=True), allowed, torch.ones_like(allowed))
    per, g = att_groups(n)
    m = per + 2 * (per // 8) + 3 * (-(-g // 64)) + 3 * 6 + 8
    return softmax_av(s, es, vv, torch.zeros_like(vv), allowed.expand(h, nq, n), m, True)


def query_side(dec, j, o_attn, state, qpos, inter=None):
    """MultiScaleMaskedTransformerDecoder._query_side of layer j on the queries state [Q, C] (o_attn [1, H, Q, Dh]) -> dict
    name -> (y, E): t1 (cross-attention out-projection + residual + LayerNorm), Qs / Ks / Vs (the self-attention's
    projections), state (self-attention block + FFN block), cls, me (decoder norm, class / mask-embed heads), q_next (None on
    the last layer).  The kernel publishes t1 / Qs / Ks / Vs (query_side_a's workspace) and state; each output is witnessed
    from the kernel's OWN values of the step before (`inter`: t1, Qs, Ks, Vs, state; None: the exact float64 ones), so a
    comparison spans at most one block and its bound keeps its power.  Sum lengths of query_side_a / _b: GEMVs k-ordered over K
    (parts added in order: K + 8), LayerNorms a 64-lane tree, the scores a Dh-term chain, the softmax one wave per (row,
    head) (ceil(Q / 64) + 6 adds)."""
    ca = dec.transformer_cross_attention_layers[j]
    sa = dec.transformer_self_attention_layers[j].self_attn
    sl = dec.transformer_self_attention_layers[j]
    ff = dec.transformer_ffn_layers[j]
    mha = ca.multihead_attn
    c, h = mha.embed_dim, mha.num_heads
    dh = c // h
    nq = state.shape[0]
    lin = lambda w, b: ("lin", w.t(), b, w.shape[1] + 8)
    ln = lambda mod: ("ln", mod.weight, mod.bias, mod.eps, m_qs_ln())
    o = f64(o_attn)[0].transpose(0, 1).reshape(nq, c)
    pos = f64(qpos)
    w, b = sa.in_proj_weight, sa.in_proj_bias
    out = {"t1": chain(o, [lin(mha.out_proj.weight, mha.out_proj.bias), ("add", state), ln(ca.norm)])}
    given = lambda name: out[name][0] if inter is None else f64(inter[name])
    t1 = given("t1")
    out["Qs"] = chain(t1, [("add", pos), lin(w[:c], b[:c])])
    out["Ks"] = chain(t1, [("add", pos), lin(w[c:2 * c], b[c:2 * c])])
    out["Vs"] = chain(t1, [lin(w[2 * c:], b[2 * c:])])
    split = lambda a: a.view(nq, h, dh).transpose(0, 1)          # [H, Q, Dh]
    qs, ks, vs = split(given("Qs")), split(given("Ks")), split(given("Vs"))
    scale = 1.0 / math.sqrt(dh)
    s = scale * qs @ ks.transpose(1, 2)
    es = gam(dh + 4) * scale * (qs.abs() @ ks.abs().transpose(1, 2))
    a, ea = softmax_av(s, es, vs, torch.zeros_like(vs), torch.ones_like(s, dtype=torch.bool), nq + -(-nq // 64) + 6 + 4, False)
    a, ea = a.transpose(0, 1).reshape(nq, c), ea.transpose(0, 1).reshape(nq, c)
    out["state"] = chain(a, [lin(sa.out_proj.weight, sa.out_proj.bias), ("add", t1), ln(sl.norm),
                             ("res", [lin(ff.linear1.weight, ff.linear1.bias), ("relu",), lin(ff.linear2.weight, ff.linear2.bias)]),
                             ln(ff.norm)], e_in=ea)
    t3 = given("state")
    out["cls"] = chain(t3, [ln(dec.decoder_norm), lin(dec.class_embed.weight, dec.class_embed.bias)])
    mlp = []
    for i, layer in enumerate(dec.mask_embed.layers):
        mlp += [lin(layer.weight, layer.bias)] + ([("relu",)] if i + 1 < len(dec.mask_embed.layers) else [])
    out["me"] = chain(t3, [ln(dec.decoder_norm)] + mlp)
    out["q_next"] = None
    if j + 1 < dec.num_layers:
        nxt = dec.transformer_cross_attention_layers[j + 1].multihead_attn
        out["q_next"] = chain(t3, [("add", pos), lin(nxt.in_proj_weight[:c], nxt.in_proj_bias[:c])])
    return out

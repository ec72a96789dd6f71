"""The float64 witness of tests/norm_ref.py, checked on the CPU: its values against torch's own float64 modules, and its error
bounds E against what fp32 torch computes on random inputs (a bound that fp32 torch breaks would not bound a kernel either)."""
import math

import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

import norm_ref as R  # noqa: E402
from eprecon_amd import mask3dformer as M  # noqa: E402
from eprecon_amd import modules as MO  # noqa: E402


def close(a, b, tol=1e-10):
    assert torch.allclose(a, b.to(a.dtype), rtol=tol, atol=tol), float((a - b).abs().max())


def within(y32, ref):
    y, e = ref
    err = (y32.double() - y).abs()
    assert bool(torch.isfinite(e).all())
    ratio = float((err / e).max())
    assert ratio <= R.C_SAFE, ratio
    return ratio


@pytest.mark.parametrize("n,c,offset", [(2, 3, 0.0), (5000, 24, 0.0), (777, 40, 1e3), (70001, 1, 0.0), (4097, 8, -3.0)])
def test_bn_train(n, c, offset):
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, generator=g) + offset
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    ref = R.bn_train(x, gamma, beta, 1e-5, R.m_bn_train(n, c))
    close(ref[0], F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), training=True, eps=1e-5))
    within(F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5), ref)


def test_bn_views_and_dwconv():
    g = torch.Generator().manual_seed(3)
    v, b, c, h, w = 3, 2, 16, 9, 11
    x = torch.randn(v * b, c, h, w, generator=g) * 2 + 0.5
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.normal_(generator=g), bn.bias.normal_(generator=g)
    y, e = R.bn_views(x, v, bn.weight, bn.bias, bn.eps, R.m_bn_views(b * h * w, c, 1), relu=True)
    want = torch.cat([F.batch_norm(x[i * b:(i + 1) * b].double(), None, None, bn.weight.double(), bn.bias.double(), training=True,
                                   eps=bn.eps) for i in range(v)]).clamp_min(0)
    close(y, want)
    y32 = torch.cat([F.batch_norm(x[i * b:(i + 1) * b], None, None, bn.weight, bn.bias, training=True) for i in range(v)]).relu()
    within(y32, (y, e))
    for k, s in ((3, 1), (5, 2)):
        conv = torch.nn.Conv2d(c, c, k, s, k // 2, groups=c, bias=False)
        ref = R.dwconv(y, e, conv.weight, s)
        close(ref[0], F.conv2d(want, conv.weight.double(), stride=s, padding=k // 2, groups=c))
        with torch.no_grad():
            within(conv(y32), ref)


@pytest.mark.parametrize("c", [5, 48, 61])
def test_layernorm(c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(300, c, generator=g) * torch.logspace(-3, 3, 300).unsqueeze(1) + 7.0
    ln = torch.nn.LayerNorm(c)
    with torch.no_grad():
        ln.weight.normal_(generator=g), ln.bias.normal_(generator=g)
    ref = R.normalise(x.double(), torch.zeros(300, c, dtype=torch.float64), ln.weight.double(), ln.bias.double(), ln.eps, 1,
                      R.m_rowwise_ln(c))
    with torch.no_grad():
        close(ref[0], ln.double()(x.double()))
        within(ln.float()(x), ref)


@pytest.mark.parametrize("cin,cout", [(24, 7), (48, 48), (88, 40), (176, 33)])
def test_linear4x(cin, cout):
    torch.manual_seed(cin)
    mod = MO.Linear4xTrans(cin, cout)
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(200, cin) * 3
    ref = R.linear4x(mod, x)
    with torch.no_grad():
        close(ref[0], mod.double()(x.double()))
        within(mod.float()(x), ref)
    powerful(ref, 5e-2)


def powerful(ref, tol):
    """the bound keeps its power: an error of `tol` |y| exceeds C_SAFE E on most elements, an all-zero output on some"""
    y, e = ref
    assert float((R.C_SAFE * e / y.abs()).median()) < tol
    assert float((y.abs() / e).max()) > 100 * R.C_SAFE


def _decoder(c, h, ffn, q, layers=3, seed=0):
    torch.manual_seed(seed)
    dec = M.MultiScaleMaskedTransformerDecoder(num_classes=11, hidden_dim=c, num_queries=q, nheads=h, dim_feedforward=ffn,
                                               dec_layers=layers, pre_norm=False, mask_dim=c)
    with torch.no_grad():
        for p in dec.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return dec.eval()


def _query_side_fp32(dec, j, o, state, qpos):
    """the query side step by step in fp32 torch, the same blocks the kernel publishes"""
    ca, sl, ff = dec.transformer_cross_attention_layers[j], dec.transformer_self_attention_layers[j], dec.transformer_ffn_layers[j]
    sa = sl.self_attn
    c, h = ca.multihead_attn.embed_dim, ca.multihead_attn.num_heads
    q, dh = state.shape[0], c // h
    t1 = ca.norm(state + F.linear(o[0].transpose(0, 1).reshape(q, c), ca.multihead_attn.out_proj.weight, ca.multihead_attn.out_proj.bias))
    w, b = sa.in_proj_weight, sa.in_proj_bias
    qs, ks, vs = F.linear(t1 + qpos, w[:c], b[:c]), F.linear(t1 + qpos, w[c:2 * c], b[c:2 * c]), F.linear(t1, w[2 * c:], b[2 * c:])
    sp = lambda a: a.view(q, h, dh).transpose(0, 1)
    a = (torch.softmax(sp(qs) / math.sqrt(dh) @ sp(ks).transpose(1, 2), -1) @ sp(vs)).transpose(0, 1).reshape(q, c)
    t2 = sl.norm(t1 + F.linear(a, sa.out_proj.weight, sa.out_proj.bias))
    t3 = ff.norm(t2 + ff.linear2(F.relu(ff.linear1(t2))))
    dn = dec.decoder_norm(t3)
    out = {"t1": t1, "Qs": qs, "Ks": ks, "Vs": vs, "state": t3, "cls": dec.class_embed(dn), "me": dec.mask_embed(dn), "q_next": None}
    if j + 1 < dec.num_layers:
        nxt = dec.transformer_cross_attention_layers[j + 1].multihead_attn
        out["q_next"] = F.linear(t3 + qpos, nxt.in_proj_weight[:c], nxt.in_proj_bias[:c])
    return out


@pytest.mark.parametrize("c,h,ffn,q,j", [(48, 8, 192, 80, 0), (16, 2, 64, 7, 2), (64, 4, 192, 33, 0), (48, 8, 256, 9, 1)])
def test_query_side(c, h, ffn, q, j):
    dec = _decoder(c, h, ffn, q)
    o = torch.randn(1, h, q, c // h)
    state, qpos = torch.randn(q, c), dec.query_embed.weight.detach()
    ref = R.query_side(dec, j, o, state, qpos)
    with torch.no_grad():
        d64 = _decoder(c, h, ffn, q).double()
        out, cls, me, q_next = d64._query_side(j, o.double(), state.double().unsqueeze(1), qpos.double().unsqueeze(1))
        close(ref["state"][0], out.squeeze(1))
        close(ref["cls"][0], cls.squeeze(0))
        close(ref["me"][0], me.squeeze(0))
        if j + 1 < dec.num_layers:
            close(ref["q_next"][0], q_next[0].transpose(0, 1).reshape(q, c))
        else:
            assert ref["q_next"] is None and q_next is None
        got = _query_side_fp32(dec.float(), j, o, state, qpos)
    ref = R.query_side(dec, j, o, state, qpos, got)
    for name, y in got.items():
        if y is not None:
            within(y, ref[name])
            powerful(ref[name], 1e-2)


@pytest.mark.parametrize("n,h,q,spread", [(200, 2, 5, 3.0), (1500, 8, 16, 80.0)])
def test_masked_attention(n, h, q, spread):
    g = torch.Generator().manual_seed(n)
    dh = 6
    qq = torch.randn(1, h, q, dh, generator=g)
    k, v = torch.randn(n, h * dh, generator=g), torch.randn(n, h * dh, generator=g)
    scale = 1.0 / math.sqrt(dh)
    k = k * (spread / (qq.abs().max() * k.abs().max() * scale * dh))
    logits = torch.randn(n, q, generator=g) * 2
    logits[:, 0] = -5.0                                   # query 0: every key blocked -> attends to all
    blocked = R.blocked_mask(logits, None, n)
    y, e = R.masked_attention(qq, k, v, scale, blocked)
    allowed = ~blocked
    allowed[allowed.sum(1) == 0] = True
    kk, vv = k.view(n, h, dh).transpose(0, 1)[None], v.view(n, h, dh).transpose(0, 1)[None]
    close(y[None], F.scaled_dot_product_attention(qq.double(), kk.double(), vv.double(), attn_mask=allowed, scale=scale))
    close(y[:, :1], F.scaled_dot_product_attention(qq[:, :, :1].double(), kk.double(), vv.double(), scale=scale)[0])
    within(F.scaled_dot_product_attention(qq, kk, vv, attn_mask=allowed, scale=scale)[0], (y, e))


def test_level_keys():
    g = torch.Generator().manual_seed(5)
    n, c = 500, 48
    coords = torch.randint(0, 96, (n, 3), generator=g, dtype=torch.int32)
    feats, le = torch.randn(n, c, generator=g), torch.randn(c, generator=g)
    pe = M.PositionEmbeddingCoordsSine(pos_type="fourier", d_pos=c, normalize=True)
    for scale in (1.0, 10.0):
        gb = pe.gauss_B * scale
        (src, esrc), (keys, ekeys) = R.level_keys(coords, feats, le, gb, (96, 96, 48))
        p = coords.double() / torch.tensor([96.0, 96.0, 48.0], dtype=torch.float64) * (2 * math.pi) @ gb.double()
        close(keys, feats.double() + le.double() + torch.cat([p.sin(), p.cos()], 1))
        close(src, feats.double() + le.double())
        pe.gauss_B.copy_(gb)
        lo, hi = torch.zeros(1, 3), torch.tensor([[96.0, 96.0, 48.0]])
        pos32 = pe(coords[None].float(), input_range=[lo, hi])[0].t()
        within(feats + le + pos32, (keys, ekeys))
        pe.gauss_B.copy_(gb / scale)

"""The kernels that normalise by a statistic (csrc/norm.hip, heads.hip, backbone2d.hip, decoder.hip) against the float64
witness of tests/norm_ref.py, through the project's own wrappers (the raw C ABI only where none exists).

Every comparison is |y - ref| <= C_SAFE * E per element (norm_ref.py states E and C_SAFE), an exact equality (counts, mask
decisions, refusals) or a bit-for-bit repeat: every case runs twice and must give the same bits.  Outputs sit in buffers
whose guard rows below and columns beside them start as NaN and must stay NaN.  A NaN in one row (LayerNorm, heads) or one
channel (BatchNorm) of the input may only make that row or channel non-finite.
"""
import math

import pytest

torch = pytest.importorskip("torch")

import norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 129
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def lib():
    from eprecon_amd import _lib
    return _lib


class Out:
    """an output view out = buf[:n, off:off + c] of a NaN buffer [n + GUARD, ld]"""

    def __init__(self, n, c, dev, ld=None, off=0):
        self.n, self.c, self.off = n, c, off
        self.buf = torch.full((n + GUARD, ld or c + off), NAN, device=dev)
        self.t = self.buf[:n, off:off + c]

    def untouched(self):
        b = self.buf
        assert bool(b[self.n:].isnan().all()), "rows past n written"
        assert bool(b[:, :self.off].isnan().all()) and bool(b[:, self.off + self.c:].isnan().all()), "columns beside written"


def within(name, y, ref, finite=None):
    """|y - ref| <= C_SAFE E where `finite` (bool mask broadcasting to y, default: everywhere); y must be finite there"""
    yr, e = ref
    y = y.double()
    if finite is None:
        finite = torch.ones_like(y, dtype=torch.bool)
    finite = finite.expand_as(y)
    assert bool(torch.isfinite(y[finite]).all()), f"{name}: non-finite output"
    ratio = float(((y - yr).abs() / e)[finite].max()) if bool(finite.any()) else 0.0
    print(f"RATIO {name} {ratio:.3f}")
    assert ratio <= R.C_SAFE, f"{name}: |err| / E = {ratio}"
    return ratio


def twice(fn):
    """fn() -> tensor or tuple of tensors; runs it twice and demands the same bits"""
    a = fn()
    a = a if isinstance(a, tuple) else (a,)
    a = tuple(t.clone() for t in a)
    b = fn()
    b = b if isinstance(b, tuple) else (b,)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.contiguous().view(torch.int32)), "not deterministic"
    return a if len(a) > 1 else a[0]


def data(n, c, dev, kind="normal", seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, c, generator=g)
    if kind == "offset":
        x = x + 1e3
    elif kind == "relu90":
        x = (x - 1.2816).clamp_min(0.0)          # ~90 % zeros
    elif kind == "tiny":
        x = x * math.sqrt(1e-5)                  # var ~ eps
    elif kind == "const":
        x[:, ::2] = 0.37
    return x.to(dev)


# ---- BatchNorm, train mode ---------------------------------------------------------------------------------------------
def _bn_case(dev, n, c, kind="normal", ld=None, off=0, residual=False, relu=False, alias=False, nan_ch=None, seed=0):
    from eprecon_amd import sparse as SP
    x0 = data(n, c, dev, kind, seed)
    if nan_ch is not None:
        x0[n // 2, nan_ch] = NAN
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    gamma, beta = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    res = data(n, c, dev, "normal", seed + 2) if residual else None
    xin = Out(n, c, dev, ld, off)
    out = xin if alias else Out(n, c, dev, ld, off)

    def run():
        xin.t.copy_(x0)
        SP.batchnorm_train(xin.t, gamma, beta, 1e-5, residual=res, relu=relu, out=out.t)
        return out.t.clone()
    y = twice(run)
    out.untouched()
    ref = R.bn_train(x0, gamma, beta, 1e-5, R.m_bn_train(n, c))
    if res is not None:
        ref = R.add(ref[0], ref[1], R.f64(res), torch.zeros_like(ref[1]))
    if relu:
        ref = (ref[0].clamp_min(0.0), ref[1])
    ok = torch.ones(1, c, dtype=torch.bool, device=dev)
    if nan_ch is not None:
        ok[0, nan_ch] = False
        assert not bool(torch.isfinite(y[:, nan_ch]).all())
    within(f"bn_train n={n} C={c} {kind}", y, ref, ok)


BN_C = (1, 8, 24, 40, 96, 128, 176, 200, 256)


@pytest.mark.parametrize("c", BN_C)
def test_bn_train_rows_per_block(dev, c):
    r = 8 * (256 // c)
    for n in (r - 1, r, r + 1):
        if n >= 1:
            _bn_case(dev, n, c, seed=n)


@pytest.mark.parametrize("nblk", (256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097))
def test_bn_train_finalize_boundaries(dev, nblk):
    c = 16
    _bn_case(dev, nblk * 8 * (256 // c), c, kind="relu90" if nblk % 2 else "normal", seed=nblk)


@pytest.mark.parametrize("kind", ("const", "tiny", "offset", "relu90"))
def test_bn_train_statistics_edges(dev, kind):
    _bn_case(dev, 5000, 24, kind)
    _bn_case(dev, 70001, 40, kind, residual=True, relu=True)


def test_bn_train_layouts(dev):
    _bn_case(dev, 1, 8)                                              # var = 0: y = beta
    _bn_case(dev, 3001, 13, ld=20, off=3)                            # row pitch > C, unaligned column slice
    _bn_case(dev, 3001, 40, ld=48, off=5, alias=True, residual=True, relu=True)
    _bn_case(dev, 3001, 24, nan_ch=7)


def _summaries(x, rows_per_block):
    """exact per-block (count, mean, M2) of x [n, C] in the channel-major layout sparse.bn_summaries hands out"""
    from eprecon_amd import sparse as SP
    n, c = x.shape
    nblk = -(-n // rows_per_block)
    part = SP.bn_summaries(nblk, c, x.device)
    xd = x.double()
    for b in range(nblk):
        blk = xd[b * rows_per_block:(b + 1) * rows_per_block]
        mu = blk.mean(0)
        part[b, 0] = blk.shape[0]
        part[b, 1] = mu.float()
        part[b, 2] = ((blk - mu) ** 2).sum(0).float()
    return part


@pytest.mark.parametrize("n,c,rpb", [(4000, 24, 37), (20011, 48, 64), (777, 256, 5)])
def test_bn_apply_partials_residual_affine(dev, n, c, rpb):
    """eprecon_batchnorm_apply_partials_async with res_scale / res_shift: a residual with its own pitch and its own pending BatchNorm"""
    from eprecon_amd import sparse as SP
    x = data(n, c, dev, "offset" if c == 48 else "normal", seed=n)
    part = _summaries(x, rpb)
    g = torch.Generator(device="cpu").manual_seed(c)
    gamma, beta = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    rs, rsh = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    rbuf = torch.randn(n, c + 7, generator=g).to(dev)
    res = rbuf[:, 3:3 + c]
    out = Out(n, c, dev, c + 9, 2)
    y = twice(lambda: SP.batchnorm_apply_partials(x, part, gamma, beta, 1e-5, residual=res, relu=True, out=out.t,
                                                  res_affine=(rs, rsh)).clone())
    out.untouched()
    nblk = part.shape[0]
    yb, eb = R.bn_train(x, gamma, beta, 1e-5, R.m_bn_train(n, c, nblk) + 4)   # (+ the rounding of the stored summaries)
    rv = R.f64(res) * R.f64(rs) + R.f64(rsh)
    yr, er = R.add(yb, eb, rv, R.U * rv.abs())
    within(f"bn_apply_partials_res n={n} C={c}", y, (yr.clamp_min(0.0), er))


@pytest.mark.parametrize("n,c", [(4000, 24), (999, 200)])
def test_bn_affine_and_affine_rows(dev, n, c):
    """finalize in affine form, then both affine-row kernels (with and without a residual: the raw eprecon_affine_rows_async)"""
    from eprecon_amd import sparse as SP
    _lib = lib()
    x = data(n, c, dev, "relu90", seed=c)
    part = _summaries(x, 41)
    g = torch.Generator(device="cpu").manual_seed(n)
    gamma, beta = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    sc, sh = twice(lambda: SP.bn_affine(part, gamma, beta, 1e-5))
    yb, eb = R.bn_train(x, gamma, beta, 1e-5, R.m_bn_train(n, c, part.shape[0]) + 4)
    res = data(n, c, dev, seed=7)
    out = Out(n, c, dev, c + 4, 1)
    y = twice(lambda: SP.affine_rows(x, sc, sh, residual=res, relu=True, out=out.t).clone())
    out.untouched()
    yr, er = R.add(yb, eb, R.f64(res), torch.zeros_like(eb))
    within(f"affine_rows_res n={n} C={c}", y, (yr.clamp_min(0.0), er))
    out2 = Out(n, c, dev, c + 3, 3)

    def raw():
        _lib.check(_lib.load().eprecon_affine_rows_async(x.data_ptr(), n, c, c, sc.data_ptr(), sh.data_ptr(), None, 0, 0,
                                                         out2.t.data_ptr(), out2.buf.stride(0), _lib.current_stream()), "eprecon_affine_rows_async")
        return out2.t.clone()
    y2 = twice(raw)
    out2.untouched()
    within(f"affine_rows n={n} C={c}", y2, (yb, eb))


@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("n,c,pitch", [(1, 1, 1), (5, 3, 7), (86, 3, 3), (257, 24, 40)])
def test_affine_rows_one_entry(dev, n, c, pitch, residual):
    """the one affine-rows kernel with and without a residual (its own pitch), n * c on both sides of a 256-thread workgroup:
    one rounding of the fma (norm_ref's GEMV rule with K = 1), one of the add; the same bits when `out` is `x`"""
    from eprecon_amd import sparse as SP
    g = torch.Generator(device="cpu").manual_seed(n + c)
    x0 = data(n, c, dev, seed=n)
    sc, sh = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    res = torch.randn(n, c + 2, generator=g).to(dev)[:, 1:1 + c] if residual else None
    xin = Out(n, c, dev, pitch, pitch - c)
    out = Out(n, c, dev, pitch + 3, 2)
    xin.t.copy_(x0)
    y = twice(lambda: SP.affine_rows(xin.t, sc, sh, residual=res, relu=True, out=out.t).clone())
    out.untouched()
    yr = R.f64(x0) * R.f64(sc) + R.f64(sh)
    er = R.gam(1) * ((R.f64(x0) * R.f64(sc)).abs() + R.f64(sh).abs())
    if residual:
        yr, er = R.add(yr, er, R.f64(res), torch.zeros_like(er))
    within(f"affine_rows n={n} C={c} pitch={pitch} res={residual}", y, (yr.clamp_min(0.0), er))
    assert SP.affine_rows(xin.t, sc, sh, residual=res, relu=True, out=xin.t) is xin.t
    xin.untouched()
    assert torch.equal(xin.t.contiguous().view(torch.int32), y.view(torch.int32)), "out aliasing x changes the bits"


@pytest.mark.parametrize("nblk", (1, 257))
@pytest.mark.parametrize("c", (4, 5))
def test_bn_apply_partials_one_entry(dev, c, nblk):
    """the one apply-partials entry on both sides of the one-launch limit (C <= 4) and with one and two summary rows per thread:
    no residual, a plain residual, a residual with its pending BatchNorm, and mean_out / var_out given -- then the same rows,
    and the statistics in the bits of the documented merge order of the same summaries"""
    import ctypes

    import test_bn_summary_layout_gpu as LAYOUT
    from eprecon_amd import sparse as SP
    _lib = lib()
    rpb = 3
    n = nblk * rpb - 1
    x = data(n, c, dev, seed=nblk + c)
    part = _summaries(x, rpb)
    assert part.shape[0] == nblk
    g = torch.Generator(device="cpu").manual_seed(c)
    gamma, beta = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    rs, rsh = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    res = torch.randn(n, c + 3, generator=g).to(dev)[:, 2:2 + c]
    yb, eb = R.bn_train(x, gamma, beta, 1e-5, R.m_bn_train(n, c, nblk) + 4)   # (+ the rounding of the stored summaries)
    rv = R.f64(res) * R.f64(rs) + R.f64(rsh)
    plain = None
    for name, kw, ref in (("none", {}, (yb, eb)),
                          ("res", {"residual": res}, R.add(yb, eb, R.f64(res), torch.zeros_like(eb))),
                          ("res_affine", {"residual": res, "res_affine": (rs, rsh)}, R.add(yb, eb, rv, R.U * rv.abs()))):
        out = Out(n, c, dev, c + 5, 1)
        y = twice(lambda: SP.batchnorm_apply_partials(x, part, gamma, beta, 1e-5, relu=True, out=out.t, **kw).clone())
        out.untouched()
        within(f"bn_apply_partials {name} C={c} nblk={nblk}", y, (ref[0].clamp_min(0.0), ref[1]))
        plain = y if plain is None else plain
    out = Out(n, c, dev, c + 5, 1)
    stats = torch.full((2, c + GUARD), NAN, device=dev)
    L = _lib.load()
    ws = torch.empty((L.eprecon_batchnorm_apply_workspace_bytes(c),), dtype=torch.uint8, device=dev)
    nb, ld = SP.summary_layout(part)

    def raw():
        _lib.check(L.eprecon_batchnorm_apply_partials_async(
            x.data_ptr(), n, c, c, part.data_ptr(), nb, ld, gamma.data_ptr(), beta.data_ptr(), ctypes.c_float(1e-5), None, 0, None,
            None, 1, out.t.data_ptr(), out.buf.stride(0), stats[0].data_ptr(), stats[1].data_ptr(), ws.data_ptr(), ws.numel(),
            _lib.current_stream()), "eprecon_batchnorm_apply_partials_async")
        return out.t.clone(), stats.clone()
    y, st = twice(raw)
    out.untouched()
    assert torch.equal(y.view(torch.int32), plain.view(torch.int32)), "asking for the statistics changes the rows"
    assert bool(st[:, c:].isnan().all()), "statistics past C written"
    want_mean, want_var = LAYOUT._stats_reference(part.cpu().numpy())
    got = st[:, :c].cpu().numpy()
    assert (got[0].view("uint32") == want_mean.view("uint32")).all(), (got[0], want_mean)
    assert (got[1].view("uint32") == want_var.view("uint32")).all(), (got[1], want_var)


# ---- row-wise LayerNorm ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", [(5, 33), (13, 1000), (48, 4001), (61, 257), (96, 31)])
def test_rowwise_layernorm(dev, c, n):
    from eprecon_amd import sparse as SP
    g = torch.Generator(device="cpu").manual_seed(c)
    x = (torch.randn(n, c, generator=g) * torch.logspace(-3, 2, n).unsqueeze(1) + 10 * torch.randn(n, 1, generator=g)).to(dev)
    x[n // 3] = 0.25                                                  # a constant row: var = 0
    x[n // 2, c // 2] = NAN
    res = torch.randn(n, c + 5, generator=g).to(dev)[:, 2:2 + c]
    gamma, beta = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    ok = torch.ones(n, 1, dtype=torch.bool, device=dev)
    ok[n // 2] = False
    for pre, post, use_res, alias in ((False, False, False, False), (True, True, True, False), (False, True, True, True)):
        xin = Out(n, c, dev, c + 6, 1)
        out = xin if alias else Out(n, c, dev, c + 3, 2)

        def run():
            xin.t.copy_(x)
            SP.rowwise_layernorm(xin.t, gamma, beta, 1e-5, residual=res if use_res else None, pre_relu=pre, post_relu=post,
                                 out=out.t)
            return out.t.clone()
        y = twice(run)
        out.untouched()
        t = R.f64(x).clamp_min(0.0) if pre else R.f64(x)
        et = torch.zeros_like(t)
        if use_res:
            t, et = R.add(t, et, R.f64(res), et)
        yr, e = R.normalise(t, et, R.f64(gamma), R.f64(beta), 1e-5, 1, R.m_rowwise_ln(c))
        if post:
            yr = yr.clamp_min(0.0)
        within(f"rowwise_ln C={c} pre={pre} post={post} res={use_res}", y, (yr, e), ok)


# ---- per-view BatchNorm and the depthwise convolution behind it --------------------------------------------------------
@pytest.mark.parametrize("c,v,b,h,w,kind", [(16, 3, 1, 24, 32, "outlier"), (96, 2, 2, 15, 20, "offset"), (480, 2, 1, 9, 13, "normal"),
                                            (40, 9, 1, 30, 40, "const"), (8, 1, 1, 120, 160, "outlier"), (24, 3, 1, 12, 16, "nan")])
def test_bn_views_and_dwconv(dev, c, v, b, h, w, kind):
    from eprecon_amd import backbone as BB
    _lib = lib()
    g = torch.Generator(device="cpu").manual_seed(c + v)
    x = torch.randn(v * b, c, h, w, generator=g)
    rows = b * h * w
    chunks = _lib.load().eprecon_bn2d_views_chunks(rows, c)
    per = -(-rows // chunks)
    if kind == "outlier":                     # the first row of a chunk (the second chunk of view 0, or its first)
        r = per if chunks > 1 else 0
        x[r // (h * w), :, (r % (h * w)) // w, r % w] = 1e4
    elif kind == "offset":                  # 1e4 sigma: sums of squares of raw values lose the variance entirely
        x = x + 1e4
    elif kind == "const":
        x[:, 3] = -2.5
    elif kind == "nan":
        x[1, 5, 2, 3] = NAN
    x = x.to(dev).contiguous(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(c).to(dev)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g)), bn.bias.copy_(torch.randn(c, generator=g))
    aff = twice(lambda: BB.bn_views_stats(bn, x, v))
    ref = R.bn_views(x, v, bn.weight, bn.bias, bn.eps, R.m_bn_views(rows, c, chunks) + 2, relu=True)
    ok = torch.ones(1, c, 1, 1, dtype=torch.bool, device=dev)
    if kind == "nan":
        ok[0, 5] = False
    y = twice(lambda: BB.bn_views_apply(x.clone(memory_format=torch.channels_last), aff, v, True))
    within(f"bn_views C={c} {kind}", y, ref, ok)
    if kind == "nan":                         # only view 1's channel 5 loses its statistics
        assert bool(aff[1, :, 5].isnan().all()) and int(aff.isnan().sum()) == 2
    for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)):
        conv = torch.nn.Conv2d(c, c, k, s, k // 2, groups=c, bias=False).to(dev)
        yc = twice(lambda: BB.dwconv_nhwc(conv, x, v, pending=(aff, True)))
        rc = R.dwconv(ref[0], ref[1], conv.weight, s)
        within(f"dwconv k{k} s{s} C={c} {kind}", yc, rc, ok)


# ---- the heads ---------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(24, 1), (24, 7), (24, 16), (48, 1), (48, 7), (48, 16), (96, 1), (96, 7), (96, 16),
               (48, 33), (48, 48), (88, 33), (88, 48), (176, 33), (176, 48)]
HEAD_ROWS = (1, 15, 16, 17, 63, 64, 65, 39999, 40000, 40001, 100003)


def _head(cin, cout, dev, seed):
    from eprecon_amd import modules as MO
    torch.manual_seed(seed)
    mod = MO.Linear4xTrans(cin, cout)
    with torch.no_grad():
        for p_ in mod.parameters():
            p_.add_(0.1 * torch.randn_like(p_))
    return mod.to(dev)


@pytest.mark.parametrize("cin,cout", HEAD_SHAPES)
def test_mlp4x(dev, cin, cout):
    from eprecon_amd import modules as MO
    from eprecon_amd import sparse as SP
    assert SP.mlp4x_supported(cin, cout)
    ma, mb = _head(cin, cout, dev, cin), _head(cin, cout, dev, cin + 1)
    g = torch.Generator(device="cpu").manual_seed(cout)
    with torch.no_grad():
        for n in HEAD_ROWS:
            xb = torch.full((n, cin + 4), NAN)
            xb[:, 1:1 + cin] = torch.randn(n, cin, generator=g) * 2
            if n > 2:
                xb[n // 2, 1 + cin // 3] = NAN
            xb = xb.to(dev)
            x = xb[:, 1:1 + cin]                                     # unaligned rows with a pitch: the scalar-load path
            ok = torch.ones(n, 1, dtype=torch.bool, device=dev)
            if n > 2:
                ok[n // 2] = False
            outs = [Out(n, cout, dev, cout + 2, 1), Out(n, cout, dev, cout + 2, 1)]
            ya, yb = twice(lambda: tuple(t.clone() for t in SP.mlp4x([ma, mb], x, [o.t for o in outs])))
            for o in outs:
                o.untouched()
            within(f"mlp4x {cin}->{cout} n={n} head0", ya, R.linear4x(ma, x), ok)
            within(f"mlp4x {cin}->{cout} n={n} head1", yb, R.linear4x(mb, x), ok)
            if n in (17, 40000, 40001):
                xc = x.contiguous()
                pa, pb = twice(lambda: tuple(MO.linear4x_pair(ma, mb, xc)))
                within(f"linear4x_pair {cin}->{cout} n={n}", pa, R.linear4x(ma, xc), ok)
                within(f"linear4x_pair {cin}->{cout} n={n} b", pb, R.linear4x(mb, xc), ok)


# ---- decoder -----------------------------------------------------------------------------------------------------------
def _decoder(c, h, ffn, q, dev, seed=0, mask_hidden=None):
    from eprecon_amd import mask3dformer as M
    torch.manual_seed(seed)
    dec = M.MultiScaleMaskedTransformerDecoder(num_classes=11, hidden_dim=c, num_queries=q, nheads=h, dim_feedforward=ffn,
                                               dec_layers=3, pre_norm=False, mask_dim=c)
    if mask_hidden is not None:
        dec.mask_embed = M.MLP(c, mask_hidden, c, 3)
    with torch.no_grad():
        for p_ in dec.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    return dec.to(dev).eval()


def _query_side_run(dec, j, o, state, pack, dev):
    q, c = state.shape
    outs = torch.full((3, q + GUARD, c), NAN, device=dev)
    cls = torch.full((q + GUARD, pack["n_cls"]), NAN, device=dev)
    ws = torch.empty((4, q, c), device=dev)
    res = dec._query_side_hip(pack, j, o, state, [outs[0, :q], outs[1, :q], outs[2, :q]], cls[:q], ws)
    assert bool(outs[:, q:].isnan().all()) and bool(cls[q:].isnan().all()), "rows past Q written"
    if j + 1 >= dec.num_layers:
        assert bool(outs[2].isnan().all()) and res[3] is None
    # (the workspace holds query_side_a's results t1 / Qs / Ks / Vs, the values query_side_b reads)
    got = (outs[0, :q].clone(), cls[:q].clone(), outs[1, :q].clone(), ws.clone())
    return got if res[3] is None else got + (outs[2, :q].clone(),)


def _check_query_side(dec, j, q, c, h, dev, tag):
    """each published value against the witness started from the kernel's own values of the step before (norm_ref.query_side)"""
    g = torch.Generator(device="cpu").manual_seed(q * 7 + c)
    o = torch.randn(1, h, q, c // h, generator=g).to(dev)
    state = torch.randn(q, c, generator=g).to(dev)
    with torch.no_grad():
        pack = dec._query_side_pack(dev)
        got = twice(lambda: _query_side_run(dec, j, o, state, pack, dev))
        ws = got[3]
        inter = {"t1": ws[0], "Qs": ws[1], "Ks": ws[2], "Vs": ws[3], "state": got[0]}
        ref = R.query_side(dec, j, o, state, pack["qpos"], inter)
    assert (len(got) == 5) == (ref["q_next"] is not None)
    vals = dict(inter, cls=got[1], me=got[2], q_next=got[4] if len(got) == 5 else None)
    for name, y in vals.items():
        if y is not None:
            within(f"query_side {tag} {name}", y, ref[name])


QS = [(q, c) for q in (1, 7, 80, 81, 128) for c in (16, 48, 64)]


@pytest.mark.parametrize("i,q,c", [(i, q, c) for i, (q, c) in enumerate(QS)])
def test_query_side(dev, i, q, c):
    h, ffn = (2, 4, 8)[i % 3], (64, 192)[i % 2]
    dec = _decoder(c, h, ffn, q, dev, seed=i)
    for j in (0, 2):                                             # with next_q (j < last) and without (j = last)
        _check_query_side(dec, j, q, c, h, dev, f"Q={q} C={c} H={h} FFN={ffn} j={j}")


@pytest.mark.parametrize("width", (192, 193, 256, 257, 384))
def test_query_side_widths(dev, width):
    """ffn_dim and mask_hidden at the header's limit (256 = the LDS row pitch of the hidden layers) and past it"""
    _lib = lib()
    q, c, h = 9, 48, 8
    dec = _decoder(c, h, width, q, dev, seed=width, mask_hidden=width)
    if width <= 256:
        _check_query_side(dec, 0, q, c, h, dev, f"width={width}")
        return
    with torch.no_grad():
        pack = dec._query_side_pack(dev)
        assert pack["ffn_dim"] == pack["mask_hidden"] == width
        o, state = torch.randn(1, h, q, c // h, device=dev), torch.randn(q, c, device=dev)
        with pytest.raises(_lib.EpreconError, match="error -3 "):
            _query_side_run(dec, 0, o, state, pack, dev)


def _attention_case(dev, h, q, n, spread=5.0, logits=None, rows=None, n_fine=None, seed=0):
    from eprecon_amd import mask3dformer as M
    g = torch.Generator(device="cpu").manual_seed(seed)
    dh = 6
    qq = torch.randn(1, h, q, dh, generator=g)
    k = torch.randn(n, h * dh, generator=g)
    v = torch.randn(n, h * dh, generator=g)
    scale = 1.0 / math.sqrt(dh)
    s = scale * (qq[0] @ k.view(n, h, dh).permute(1, 2, 0))
    k = k * (spread / float(s.abs().max()))                  # scores span about +-spread after scaling
    qq, k, v = qq.to(dev), k.to(dev), v.to(dev)
    lt = None if logits is None else logits.to(dev)
    rw = None if rows is None else rows.to(dev)
    out = torch.full((1, h, q, dh), NAN, device=dev)
    y = twice(lambda: M.masked_attention(qq, k, v, lt, rw, out, scale).clone())
    blocked = None if lt is None else R.blocked_mask(lt, rw, n)
    within(f"masked_attention H={h} Q={q} N={n} spread={spread}", y, R.masked_attention(qq, k, v, scale, blocked))
    return y, blocked


@pytest.mark.parametrize("h,q", [(2, 1), (2, 80), (2, 128), (8, 1), (8, 80), (8, 128)])
def test_masked_attention_shapes(dev, h, q):
    per, _ = R.att_groups(1000)
    for n in (1, 37, per - 1, per, per + 1, 2 * per - 1, 2 * per + 1, 5000, 60001):
        g = torch.Generator(device="cpu").manual_seed(n)
        logits = torch.randn(n, q, generator=g) * 3
        logits[:, 0] = -4.0                                      # query 0 blocks every key: attends to all
        _attention_case(dev, h, q, n, 80.0 if n % 2 else 5.0, logits, seed=n + q)
    _attention_case(dev, h, q, 300, 80.0, None, seed=1)          # no mask at all


def test_masked_attention_decisions(dev):
    """mask logits at the sigmoid's edges, each key's decision = torch's fp32 sigmoid(x) < 0.5; query 1 may only attend to keys
    of one workgroup; every query has only a few allowed keys, so one wrong decision moves its output far outside E"""
    h, q = 2, 3
    per, _ = R.att_groups(5000)
    n = 5000
    special = torch.tensor([-1e-8, -0.0, 0.0, 1e-8, 17.0, -17.0, -89.0, -105.0])
    logits = torch.full((n, q), -30.0)
    idx = torch.arange(0, 8 * 611, 611)
    logits[idx, 0] = special                                      # query 0: the special values, spread over the groups
    logits[per + 3:per + 9, 1] = special[:6]                      # query 1: allowed keys inside the second workgroup only
    logits[idx, 2] = -special                                     # query 2: the mirrored values
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(torch.int32)
    fine = torch.empty_like(logits)
    fine[rows.long()] = logits                                    # key n reads fine row rows[n]
    y, blocked = _attention_case(dev, h, q, n, 20.0, fine, rows, seed=5)
    assert not bool(blocked[0, idx[0]]), "fp32 sigmoid(-1e-8) rounds to 0.5: allowed, where x < 0 would block it"
    assert int((~blocked[1]).sum()) == 5 and bool(blocked[1, :per].all()) and bool(blocked[1, 2 * per:].all())


@pytest.mark.parametrize("scale", (1.0, 10.0))
def test_decoder_level_inputs(dev, scale):
    from eprecon_amd import mask3dformer as M
    g = torch.Generator(device="cpu").manual_seed(int(scale))
    for n, c, ext in ((1, 48, (96, 96, 48)), (4099, 48, (96, 96, 48)), (777, 16, (200, 120, 64))):
        coords = torch.randint(0, max(ext), (n, 4), generator=g, dtype=torch.int32)
        coords[:, :3] = coords[:, :3] % torch.tensor(ext, dtype=torch.int32)
        feats = torch.randn(n, c + 3, generator=g)[:, 1:1 + c]
        le = torch.randn(c, generator=g)
        pe = M.PositionEmbeddingCoordsSine(pos_type="fourier", d_pos=c, normalize=True)
        gb = (pe.gauss_B * scale).to(dev)
        xyz = coords.to(dev)[:, :3]                              # a row pitch of 4
        f, le = feats.to(dev), le.to(dev)
        src, keys = twice(lambda: M.decoder_level_inputs(xyz, f, le, gb, ext))
        rs, rk = R.level_keys(xyz, f, le, gb, ext)
        within(f"level_src n={n} C={c} x{scale}", src, rs)
        within(f"level_keys n={n} C={c} x{scale}", keys, rk)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from eprecon_amd import sparse as SP
    _lib = lib()
    L = _lib.load()
    st = _lib.current_stream()
    x = torch.randn(64, 520, device=dev)
    with pytest.raises(_lib.EpreconError):
        SP.batchnorm_train(x[:, :257].contiguous())
    assert L.eprecon_batchnorm_workspace_bytes(64, 257) == 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    aff = torch.full((2, 2, 520), NAN, device=dev)
    for c in (484, 18):
        rc = L.eprecon_bn2d_views_stats_async(x.data_ptr(), 2, 8, c, None, None, 1e-5, aff.data_ptr(), ws.data_ptr(), ws.numel(), st)
        assert rc == -1, (c, rc)
    acc = torch.zeros(2 * 1024, dtype=torch.int64, device=dev)
    out = torch.full((64, 520), NAN, device=dev)
    rc = L.eprecon_affine_rows_acc_async(x.data_ptr(), 64, 513, 520, acc.data_ptr(), 1024, 0, 1e-5, 0, out.data_ptr(), 520, st)
    assert rc == -1, rc
    # the one apply-partials entry: res_scale without res_shift, res_scale / res_shift without a residual, a residual pitch
    # below C (the one affine-rows entry as well)
    import ctypes
    c = 8
    part = torch.ones((3, c, 4), device=dev)
    v = torch.ones(c, device=dev)
    aws = torch.empty((L.eprecon_batchnorm_apply_workspace_bytes(c),), dtype=torch.uint8, device=dev)
    for res, ld_res, rs, rsh in ((x, 520, v, None), (x, 520, None, v), (None, 0, v, v), (x, c - 1, None, None), (x, c - 1, v, v)):
        rc = L.eprecon_batchnorm_apply_partials_async(
            x.data_ptr(), 64, c, 520, part.data_ptr(), 4, 4, None, None, ctypes.c_float(1e-5), _lib.ptr(res), ld_res, _lib.ptr(rs),
            _lib.ptr(rsh), 0, out.data_ptr(), 520, None, None, aws.data_ptr(), aws.numel(), st)
        assert rc == -1, (ld_res, rs is None, rsh is None, rc)
    rc = L.eprecon_affine_rows_async(x.data_ptr(), 64, c, 520, v.data_ptr(), v.data_ptr(), x.data_ptr(), c - 1, 0, out.data_ptr(), 520, st)
    assert rc == -1, rc
    torch.cuda.synchronize()
    assert bool(aff.isnan().all()) and bool(out.isnan().all())

"""The short-list image-tile kernel of the 2D fusion stack's 3x3 layers (csrc/sparse_conv_tile2d_short.hip: conv2d_tile_short_kernel)
against float64 F.conv2d + train-mode BatchNorm, against the kernels of the previous rule (EPRECON_CONV_TILE2D_SHORT=0), and
against itself (run-to-run bits).  The shapes are the 3x3 layers of the 1/16 level of Occupancy_Initialization (9 x 30 x 40:
80 -> 80, 80 -> 40, 40 -> 40) plus ragged images (H, W not multiples of the 16-pixel tile; V = 1 and V = 9)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-3          # against float64 (north_star: fp32 features within 1e-3)
TOL_PREV = 1e-4     # against the previous kernel: the same products summed in another order
KERNEL = "conv2d_tile_short_kernel"


def _dev():
    return torch.device("cuda:0")


# (V, H, W, C_in, C_out, features)
CASES = [
    (9, 30, 40, 80, 80, dict()),                                                            # Fusion_Block conv1 (raw input)
    (9, 30, 40, 80, 80, dict(bn_in=True, in_relu=True, residual=True, res_relu=True)),
    (9, 30, 40, 80, 40, dict(bn_in=True, in_relu=True, slice_out=True)),                    # ELAN conv3
    (9, 30, 40, 40, 40, dict(bn_in=True, in_relu=True, slice_in=True, slice_out=True)),     # ELAN conv4..6
    (9, 30, 40, 40, 40, dict(bn_in=True, pre_relu=True)),
    (1, 23, 37, 80, 80, dict(bn_in=True, in_relu=True)),                                    # ragged, one view
    (9, 13, 21, 40, 40, dict(bn_in=True, residual=True)),                                   # ragged, nine views
    (9, 17, 9, 72, 36, dict(bn_in=True, in_relu=True, slice_in=True)),                      # an 8-channel last chunk of five
    (1, 7, 50, 44, 48, dict(pre_relu=True)),                                                # three full-width chunks
]
IDS = ["%dx%dx%d_%d_%d_%d" % (v, h, w, ci, co, i) for i, (v, h, w, ci, co, _) in enumerate(CASES)]


class Layer:
    """one 3x3 layer's operands: input / residual as Acts with pending BatchNorms, output rows (possibly a channel slice)"""

    def __init__(self, v, h, w, ci, co, f, seed):
        from eprecon_amd import dense2d as D2
        dev = _dev()
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.v, self.h, self.w, self.ci, self.co, self.f = v, h, w, ci, co, f
        n = self.n = v * h * w
        conv = torch.nn.Conv2d(ci, co, 3, padding="same")
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * ci ** 0.5))
            conv.bias.copy_(torch.randn(co, generator=g) * 0.1)
        self.weight, self.bias = conv.weight.to(dev), conv.bias.to(dev)
        self.wk = D2.packed_weight(conv.to(dev))
        if f.get("slice_in"):   # a channel slice [4, 4 + ci) of a wider buffer (ELAN concat buffers)
            self.xbuf = torch.randn(n, ci + 8, generator=g).to(dev)
            rows = self.xbuf[:, 4:4 + ci]
        else:
            rows = self.xbuf = torch.randn(n, ci, generator=g).to(dev)
        sc = sh = None
        if f.get("bn_in"):
            sc = (torch.rand(ci, generator=g) + 0.5).to(dev)
            sh = (torch.randn(ci, generator=g) * 0.3).to(dev)
        self.x = D2.Act(rows, sc, sh, bool(f.get("in_relu")))
        self.res = None
        if f.get("residual"):
            self.res = D2.Act(torch.randn(n, co, generator=g).to(dev), (torch.rand(co, generator=g) + 0.5).to(dev),
                              (torch.randn(co, generator=g) * 0.3).to(dev), bool(f.get("res_relu")))
        self.gamma = (torch.rand(co, generator=g) + 0.5).to(dev)
        self.beta = (torch.randn(co, generator=g) * 0.1).to(dev)
        self.grid = D2.PixelGrid.get(v, h, w, dev)

    def run(self):
        """-> (raw output rows, scale, shift, kernel name), on fresh output memory"""
        from eprecon_amd import dense2d as D2, _lib
        if self.f.get("slice_out"):
            obuf = torch.full((self.n, self.co + 12), float("nan"), device=_dev())
            out = obuf[:, 8:8 + self.co]
        else:
            obuf = out = torch.full((self.n, self.co), float("nan"), device=_dev())
        y = D2.conv_bn_launch(self.wk, self.bias, self.gamma, self.beta, 1e-5, 3, self.x, self.grid, out=out,
                              relu=True, pre_relu=bool(self.f.get("pre_relu")), residual=self.res)
        kernel = _lib.last_conv_kernel()
        torch.cuda.synchronize()
        if self.f.get("slice_out"):   # the columns around the slice are not touched
            assert torch.isnan(obuf[:, :8]).all() and torch.isnan(obuf[:, 8 + self.co:]).all()
        return y.rows.clone(), y.scale.clone(), y.shift.clone(), kernel

    def reference(self):
        """float64: conv(BN_in(x)) + b, [ReLU], + BN_res(res); the train-mode BatchNorm's (scale, shift) of that"""
        a = self.x.rows.double()
        if self.x.scale is not None:
            a = a * self.x.scale.double() + self.x.shift.double()
            if self.x.relu:
                a = a.clamp_min(0.0)
        img = a.view(self.v, self.h, self.w, self.ci).permute(0, 3, 1, 2)
        y = F.conv2d(img, self.weight.double(), self.bias.double(), padding=1).permute(0, 2, 3, 1).reshape(self.n, self.co)
        if self.f.get("pre_relu"):
            y = y.clamp_min(0.0)
        if self.res is not None:
            r = self.res.rows.double() * self.res.scale.double() + self.res.shift.double()
            if self.res.relu:
                r = r.clamp_min(0.0)
            y = y + r
        mean, var = y.mean(0), y.var(0, unbiased=False)
        scale = self.gamma.double() / torch.sqrt(var + 1e-5)
        return y, scale, self.beta.double() - mean * scale


@pytest.fixture(autouse=True)
def short_on(monkeypatch):
    monkeypatch.delenv("EPRECON_CONV_TILE2D_SHORT", raising=False)


@pytest.mark.parametrize("v,h,w,ci,co,f", CASES, ids=IDS)
def test_short_against_float64(v, h, w, ci, co, f):
    L = Layer(v, h, w, ci, co, f, seed=7 + ci + co + h)
    out, scale, shift, kernel = L.run()
    assert kernel == KERNEL
    ref, rscale, rshift = L.reference()
    assert torch.isfinite(out).all()
    assert (out.double() - ref).abs().max().item() < TOL
    assert (scale.double() - rscale).abs().max().item() < TOL * rscale.abs().max().item()
    assert (shift.double() - rshift).abs().max().item() < TOL * (1.0 + rshift.abs().max().item())


@pytest.mark.parametrize("v,h,w,ci,co,f", CASES, ids=IDS)
def test_short_against_previous_kernel_and_switch(v, h, w, ci, co, f, monkeypatch):
    L = Layer(v, h, w, ci, co, f, seed=11 + ci + co + w)
    out, scale, shift, kernel = L.run()
    assert kernel == KERNEL
    monkeypatch.setenv("EPRECON_CONV_TILE2D_SHORT", "0")
    out0, scale0, shift0, kernel0 = L.run()
    assert kernel0 != KERNEL
    if (v, h, w) == (9, 30, 40):
        assert kernel0 == "spconv_splitk_kernel"     # the previous rule's choice on the 1/16 level
    mag = out0.abs().max().item()
    assert (out - out0).abs().max().item() <= TOL_PREV * max(mag, 1.0)
    assert (scale - scale0).abs().max().item() <= TOL_PREV * scale0.abs().max().item()
    assert (shift - shift0).abs().max().item() <= TOL_PREV * max(shift0.abs().max().item(), 1.0)
    monkeypatch.setenv("EPRECON_CONV_TILE2D_SHORT", "1")
    assert L.run()[3] == KERNEL


@pytest.mark.parametrize("v,h,w,ci,co,f", [CASES[i] for i in (1, 2, 3, 5, 7)], ids=[IDS[i] for i in (1, 2, 3, 5, 7)])
def test_short_same_bits_every_run(v, h, w, ci, co, f):
    L = Layer(v, h, w, ci, co, f, seed=3)
    a, b = L.run(), L.run()
    assert a[3] == b[3] == KERNEL
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_short_declines_accumulator_inputs_and_long_lists():
    """BatchNorm form (c) (EPRECON_BN_ACC): the kernel produces into an accumulator block, with the rows of the finalize form; a
    consumer of such a block (in_acc) keeps the previous kernel; a long list stays on conv2d_tile16_kernel"""
    from eprecon_amd import dense2d as D2, _lib
    L = Layer(9, 30, 40, 40, 40, dict(bn_in=True, in_relu=True), seed=5)
    rows, _, _, _ = L.run()
    with D2.bn_pass(D2.BnArena(_dev())):
        a = D2.conv_bn_launch(L.wk, L.bias, L.gamma, L.beta, 1e-5, 3, L.x, L.grid)
        assert _lib.last_conv_kernel() == KERNEL and a.acc is not None
        assert torch.equal(a.rows, rows)
        D2.conv_bn_launch(L.wk, L.bias, L.gamma, L.beta, 1e-5, 3, a, L.grid)
        assert _lib.last_conv_kernel() == "spconv_splitk_kernel"
    S = Layer(9, 60, 80, 40, 40, dict(bn_in=True), seed=6)
    assert S.run()[3] == "conv2d_tile16_kernel"

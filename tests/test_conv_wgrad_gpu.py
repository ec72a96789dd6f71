"""Weight gradient of the sparse convolution (autograd.conv_weight_grad -> spconv_wgrad_kernel, csrc/backward.hip) against
float64 dW[k] = sum_i x[nbr[k, i]]^T dy[i], |dW - ref| <= 2^-16 S with S = sum_i |x[nbr[k, i]]|^T |dy[i]|.

Every (ti, tj) tile of wgrad_tile() (seven instantiations), kvol 1 / 8 / 27, n_out 1 / 255 / 256 / 257 and a multi-chunk list
with a ragged last chunk, one of them long enough for several compaction sub-chunks per chunk; x and dy both as misaligned
column slices of wider NaN-filled buffers and as the contiguous tensors autograd hands over; an offset without entries
(dW[k] exactly 0);
n_out = 0 (zeros); the same bits on a second run."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402

BOUND = 2.0 ** -16

# (C_in, C_out) -> the (ti, tj) tile wgrad_tile() picks: tj = 32 / 64 / 128 by C_out, ti = 32 for C_in <= 32, else 64 unless
# C_in > 64 and tj = 128
TILES = {
    "32x32": (16, 24),
    "64x32": (48, 32),
    "32x64": (32, 64),
    "64x64": (64, 40),
    "32x128": (8, 96),
    "64x128": (48, 128),     # 32 < C_in <= 64, C_out > 64
    "128x128": (96, 129),
}


def _slice(rng, n, c, off):
    """f32 [n, c]: columns [off, off + c) of a NaN-filled buffer (rows misaligned), or with off None a plain contiguous
    tensor (16-byte aligned rows for C % 4 == 0: what autograd hands over)"""
    v = torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)).cuda()
    if off is None:
        return v
    buf = torch.full((max(n, 1), c + off + 3), float("nan"), dtype=torch.float32, device="cuda")[:n]
    buf[:, off:off + c] = v
    return buf[:, off:off + c]


def _map(rng, kvol, n_out, n_in):
    if kvol == 1:
        return None
    nbr = np.where(rng.random((kvol, n_out)) < 0.6, rng.integers(0, n_in, (kvol, n_out)), -1).astype(np.int32)
    nbr[kvol - 1] = -1          # an offset with no entries
    return torch.from_numpy(nbr).cuda()


def _check(x, dy, nbr, kvol, what):
    from eprecon_amd.autograd import conv_weight_grad
    cin, cout = x.shape[1], dy.shape[1]
    dw = conv_weight_grad(x, dy, nbr, kvol, cin, cout)
    torch.cuda.synchronize()
    ref = R.weight_grad(x, dy, nbr, kvol)
    s = R.weight_grad(x.abs(), dy.abs(), nbr, kvol)
    assert bool(torch.isfinite(dw).all()), f"{what}: non-finite dW"
    ratio = float(((dw.to(torch.float64) - ref).abs() / (s * BOUND).clamp_min(1e-30)).max())
    assert ratio <= 1.0, f"{what}: |dW - ref| / (2^-16 S) = {ratio:.3g}"
    if nbr is not None:
        assert bool((dw[kvol - 1] == 0).all()), f"{what}: an offset without entries got a non-zero gradient"
    return dw, ratio


@pytest.mark.parametrize("kvol", [1, 8, 27])
@pytest.mark.parametrize("tile", list(TILES))
def test_weight_gradient_tiles(record_property, tile, kvol):
    cin, cout = TILES[tile]
    rng = np.random.default_rng(zlib.crc32(f"{tile}-{kvol}".encode()))
    worst = 0.0
    for n_out in (1, 255, 256, 257):
        for layout, (xo, do) in {"sliced": (1, 2), "contiguous": (None, None)}.items():
            n_in = n_out if kvol != 8 else max(1, 2 * n_out)
            x = _slice(rng, n_in if kvol > 1 else n_out, cin, xo)
            dy = _slice(rng, n_out, cout, do)
            nbr = _map(rng, kvol, n_out, x.shape[0])
            worst = max(worst, _check(x, dy, nbr, kvol, f"{tile} K={kvol} n={n_out} {layout}")[1])
    record_property("err_over_S", worst * BOUND)


# (the 70,000-row list: 29 chunks of 2,560 rows, each walked in more than one 2,048-row compaction sub-chunk)
@pytest.mark.parametrize("kvol,n_out,tile", [(1, 5000, "32x32"), (8, 3000, "64x128"), (27, 9000, "128x128"),
                                             (27, 4097, "32x64"), (27, 70000, "64x128")])
def test_weight_gradient_multi_chunk_and_same_bits(record_property, kvol, n_out, tile):
    """several row chunks (partial sums reduced by a second launch), the last one ragged; a second run gives the same bits"""
    cin, cout = TILES[tile]
    rng = np.random.default_rng(n_out)
    n_in = n_out
    x = _slice(rng, n_in, cin, 3)
    dy = _slice(rng, n_out, cout, 1)
    nbr = _map(rng, kvol, n_out, n_in)
    dw, ratio = _check(x, dy, nbr, kvol, f"{tile} K={kvol} n={n_out}")
    from eprecon_amd.autograd import conv_weight_grad
    assert torch.equal(conv_weight_grad(x, dy, nbr, kvol, cin, cout), dw)
    record_property("err_over_S", ratio * BOUND)


@pytest.mark.parametrize("kvol", [1, 27])
def test_weight_gradient_of_an_empty_list_is_zero(kvol):
    from eprecon_amd.autograd import conv_weight_grad
    x = torch.randn(5, 32, device="cuda")
    dy = torch.empty((0, 48), device="cuda")
    nbr = None if kvol == 1 else torch.empty((kvol, 0), dtype=torch.int32, device="cuda")
    dw = conv_weight_grad(x, dy, nbr, kvol, 32, 48)
    assert dw.shape == (kvol, 32, 48) and bool((dw == 0).all())

"""BatchNorm summaries in their channel-major storage ([3, C, ld], handed out as the logical [rows, 3, C] view): the finalize
launches merge them in the documented fixed order, bit for bit as a float32 numpy re-enactment of that order, for lists from
one row to past the 16 rows per thread a loop trip holds; the convolutions hand back views whose values are the summaries of
their output."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _dev():
    return torch.device("cuda:0")


def _summaries(nblk, c, seed):
    """random (count, mean, M2) rows as producers leave them: integer counts up to 128 (some rows and columns empty)"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 129, size=(nblk, c)).astype(np.float32)
    n[rng.random((nblk, c)) < 0.05] = 0.0
    mean = np.where(n > 0, rng.normal(0.0, 2.0, size=(nblk, c)), 0.0).astype(np.float32)
    m2 = np.where(n > 0, n * rng.random((nblk, c)), 0.0).astype(np.float32)
    return np.stack([n, mean, m2], axis=1)                              # [nblk, 3, c]


def _merge(a, b):
    """chan_merge (csrc/conv_common.hpp) element-wise in float32, the same operations in the same order"""
    na, ma, qa = a
    nb, mb, qb = b
    with np.errstate(divide="ignore", invalid="ignore"):
        n = na + nb
        d = mb - ma
        mean = ma + d * (nb / n)
        m2 = (qa + qb) + (d * d) * ((na * nb) / n)
    pick_a, pick_b = nb == 0, (nb != 0) & (na == 0)
    return tuple(np.where(pick_a, x, np.where(pick_b, y, z)).astype(np.float32)
                 for x, y, z in ((na, nb, n), (ma, mb, mean), (qa, qb, m2)))


def _thread_merge(s):
    """thread t of a channel's workgroup merges rows t, t + 256, ... in order -> three float32[256, c]"""
    nblk, _, c = s.shape
    acc = tuple(np.zeros((256, c), np.float32) for _ in range(3))
    for b0 in range(0, nblk, 256):
        blk = np.zeros((256, 3, c), np.float32)
        blk[:min(256, nblk - b0)] = s[b0:b0 + 256]
        acc = _merge(acc, (blk[:, 0], blk[:, 1], blk[:, 2]))
    return acc


def _affine_reference(s, gamma, beta):
    """bn_finalize_affine_kernel: thread merges, xor butterfly inside each wave (lower lane left), waves 0..3 in order"""
    acc = _thread_merge(s)
    lane = np.arange(256)
    m = 1
    while m < 64:
        lo, hi = lane & ~m, lane | m
        acc = _merge(tuple(x[lo] for x in acc), tuple(x[hi] for x in acc))
        m <<= 1
    tot = tuple(x[0] for x in acc)
    for w in range(1, 4):
        tot = _merge(tot, tuple(x[64 * w] for x in acc))
    n, mean, m2 = tot
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n > 0, m2 / n, np.float32(0)).astype(np.float32)
    sc = (gamma / np.sqrt(var + np.float32(EPS))).astype(np.float32)
    return sc, (beta - mean * sc).astype(np.float32)


def _stats_reference(s):
    """bn_finalize_kernel: thread merges, then the LDS tree (tid merges tid + s for s = 128, 64, ..., 1)"""
    acc = _thread_merge(s)
    st = 128
    while st > 0:
        left = _merge(tuple(x[:st] for x in acc), tuple(x[st:2 * st] for x in acc))
        acc = tuple(np.concatenate([l, x[st:]]) for l, x in zip(left, acc))
        st >>= 1
    n, mean, m2 = (x[0] for x in acc)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n > 0, m2 / n, np.float32(0)).astype(np.float32)
    return mean, var


def _device_view(s, ld=None):
    """the logical [nblk, 3, c] summaries in channel-major storage with row stride ld (>= nblk)"""
    from eprecon_amd import sparse as SP
    nblk, _, c = s.shape
    if ld is None:
        p = SP.bn_summaries(nblk, c, _dev())
    else:
        p = torch.full((3, c, ld), float("nan"), dtype=torch.float32, device=_dev())[:, :, :nblk].permute(2, 0, 1)
    p.copy_(torch.from_numpy(s))
    assert SP.summary_layout(p) == (nblk, p.stride(2))
    return p


NBLKS = [1, 7, 85, 256, 257, 1000, 4096, 4097, 9001]   # one row per thread .. past 16 rows per thread (a second loop trip)
CHANNELS = [1, 3, 12, 40, 96]


@pytest.mark.parametrize("nblk", NBLKS)
def test_finalize_affine_is_the_documented_merge_order(nblk):
    from eprecon_amd import sparse as SP
    for i, c in enumerate(CHANNELS):
        s = _summaries(nblk, c, seed=1000 * nblk + i)
        rng = np.random.default_rng(i)
        gamma = (0.5 + rng.random(c)).astype(np.float32)
        beta = (rng.random(c) - 0.5).astype(np.float32)
        want_sc, want_sh = _affine_reference(s, gamma, beta)
        for ld in (None, nblk + 13):
            p = _device_view(s, ld)
            sc, sh = SP.bn_affine(p, torch.from_numpy(gamma).to(_dev()), torch.from_numpy(beta).to(_dev()), EPS)
            assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32)), (nblk, c, ld)
            assert np.array_equal(sh.cpu().numpy().view(np.uint32), want_sh.view(np.uint32)), (nblk, c, ld)


@pytest.mark.parametrize("nblk", [1, 257, 4097])
def test_finalize_statistics_is_the_documented_merge_order(nblk):
    """the two-launch form (bn_finalize_kernel + apply): mean / biased variance out of eprecon_batchnorm_apply_partials_async"""
    from eprecon_amd import _lib
    lib = _lib.load()
    for i, c in enumerate([1, 12, 96]):
        s = _summaries(nblk, c, seed=7 + i)
        want_mean, want_var = _stats_reference(s)
        p = _device_view(s, nblk + 5)
        x = torch.zeros((1, c), dtype=torch.float32, device=_dev())
        out = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=_dev())
        var = torch.empty(c, dtype=torch.float32, device=_dev())
        ws = torch.empty((lib.eprecon_batchnorm_apply_workspace_bytes(c),), dtype=torch.uint8, device=_dev())
        _lib.check(lib.eprecon_batchnorm_apply_partials_async(
            x.data_ptr(), 1, c, c, p.data_ptr(), nblk, p.stride(2), None, None, ctypes.c_float(EPS), None, 0, None, None, 0,
            out.data_ptr(), c, mean.data_ptr(), var.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream()),
            "eprecon_batchnorm_apply_partials_async")
        assert np.array_equal(mean.cpu().numpy().view(np.uint32), want_mean.view(np.uint32)), (nblk, c)
        assert np.array_equal(var.cpu().numpy().view(np.uint32), want_var.view(np.uint32)), (nblk, c)


def test_a_stride_shorter_than_the_list_is_refused():
    from eprecon_amd import _lib
    lib = _lib.load()
    p = torch.zeros((3, 4, 10), dtype=torch.float32, device=_dev())
    aff = torch.empty((2, 4), dtype=torch.float32, device=_dev())
    rc = lib.eprecon_batchnorm_finalize_affine_async(p.data_ptr(), 10, 9, 4, None, None, ctypes.c_float(EPS), aff[0].data_ptr(),
                                                     aff[1].data_ptr(), _lib.current_stream())
    assert rc != 0


@pytest.mark.parametrize("n,cin,cout,k", [(5000, 16, 24, 1), (20000, 32, 40, 1), (3000, 16, 8, 27)])
def test_conv_summaries_describe_the_output(n, cin, cout, k):
    """the partial a convolution returns is the channel-major view; its counts add up to n and its merge is the batch
    statistics of the stored output"""
    from eprecon_amd import sparse as SP
    g = torch.Generator().manual_seed(n + cout)
    x = torch.randn((n, cin), generator=g).to(_dev())
    w = (torch.randn((k, cin, cout), generator=g) * 0.2).to(_dev())
    nbr = None
    if k == 27:
        nbr = torch.randint(-1, n, (27, n), generator=g, dtype=torch.int32)
        nbr[13] = torch.arange(n, dtype=torch.int32)
        nbr = nbr.to(_dev())
    out, partial = SP.sparse_conv_fused(x, w if k > 1 else w[0], nbr, None, bn_partial=True)
    nblk, ld = SP.summary_layout(partial)
    assert partial.shape == (nblk, 3, cout) and partial.stride() == (1, cout * ld, ld)
    assert torch.equal(partial[:, 0, :].sum(0), torch.full((cout,), float(n), device=_dev()))
    y = SP.batchnorm_apply_partials(out, partial)
    ref = (out.double() - out.double().mean(0)) / torch.sqrt(out.double().var(0, unbiased=False) + EPS)
    assert torch.allclose(y.double(), ref, atol=1e-3, rtol=1e-3)

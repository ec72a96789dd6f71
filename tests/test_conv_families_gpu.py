"""Conformance of every kernel family of the convolution dispatcher (select_conv, csrc/sparse_conv.hip) against the
float64 reference of tests/conv_ref.py.

FAMILIES maps each name the dispatcher can report (_lib.last_conv_kernel) to the cases built to reach it, each with the
instantiation the dispatcher's rules should pick for it (derived from the rules, not observed).  Every case goes through the
wrappers the project itself uses (sparse.sparse_conv / sparse_conv_fused / sparse_conv_ln / conv_stats, dense2d.conv_bn_launch,
DenseMap) and checks:
  - the family that took the launch;
  - a finite output, |y - ref| <= 2^-16 S per element (S = sum |a||w| + |b| + |res|; 2^-14 S under EPRECON_CONV_BF16X3=1),
    LayerNorm outputs within 1e-3; the 129 guard rows below every output (NaN, or a finite sentinel for `accumulate`) and
    the NaN columns around an output slice stay untouched;
  - BatchNorm summaries: exact counts, the merged mean / M2 against float64 statistics of the kernel's own stored output
    (1e-6 relative);
    BatchNorm in affine form (finalize or accumulator blocks, EPRECON_BN_ACC's form) against the same statistics;
  - for some cases, the same bits on a second run.
Maps are built in numpy and handed to the kernel and the reference alike (every gather map holds rows with only their centre,
an offset dead for every row and a 32-row group without a live entry at the first offsets).

(family, epilogue) pairs no wrapper produces:
  - pending BatchNorm on load + fused ReLU / residual on the gather kernels: conv_stats (the only gather wrapper with an
    in_affine) has neither; dense2d.conv_bn_launch has both, on K = 1 / 9 pixel rows (pending BatchNorms held as accumulator
    blocks, in_acc, included: the image tile16 / short kernels decline those);
  - the residual's own pending BatchNorm: only dense2d.conv_bn_launch (image families, and the gather kernels it falls back to);
  - accumulate: declined by every family but resident, resident(wide) and mfma (and with LayerNorm by all);
  - BatchNorm summaries with LayerNorm: refused (EPRECON_ERR_UNSUPPORTED), tested below;
  - conv3d_tile*: no accumulator (EPRECON_BN_ACC) form, no accumulate; spconv_wide_kernel: no LayerNorm / accumulate.
"""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT, BF16X3 = 2.0 ** -16, 2.0 ** -14
LN_TOL = 1e-3


def case(cid, inst, n, k, cin, cout, via="stats", **kw):
    c = dict(id=cid, inst=inst, n=n, k=k, cin=cin, cout=cout, via=via, map="mixed", xoff=0, xld=None, oslice=False, bias=True,
             relu=False, res=False, res_aff=False, acc=False, aff=False, ln=None, env={}, img=None, dims=None, fill=0.6,
             arena=False, bound=EXACT, rep=False, post_relu=False, stats=False, pre_relu=False, in_acc=False)
    c.update(kw)
    return c


ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129)

FAMILIES = {
    "spconv_splitk_kernel": [
        *[case(f"rows{n}", "splitk<VEC4, RT=1, NW=8, FAST, AFF>", n, 27, 32, 32, aff=n % 2 == 0) if n % 2 == 0 else
          case(f"rows{n}", "splitk<VEC4, RT=1, NW=8, FAST>", n, 27, 32, 32, via="fused", relu=True, res=True, oslice=True,
               stats=True, rep=n == 129) for n in ROWS],
        case("rows32768_last_short_list", "splitk<VEC4, RT=2, NW=8, FAST, AFF> (256 blocks of 128 rows)", 32768, 27, 16, 16,
             aff=True),
        case("unaligned_slice", "splitk<VEC4=false, RT=1, NW=8> (x offset by one float)", 300, 27, 30, 24, xoff=1, aff=True,
             rep=True),
        case("cin13_nan_pitch", "splitk<VEC4, RT=1, NW=4, FAST>", 200, 27, 13, 17, via="fused", xld=16, relu=True),
        case("cin36_chunk4", "splitk<VEC4, RT=1, NW=8, FAST, AFF>", 150, 27, 36, 9, aff=True),
        case("cin40_chunk8_cout65", "splitk<VEC4, RT=1, NW=8, FAST>", 100, 27, 40, 65, via="fused", res=True, oslice=True,
             stats=True),
        case("cout1", "splitk<VEC4, RT=1, NW=8, FAST>", 100, 27, 16, 1),
        case("cout192", "splitk<VEC4, RT=1, NW=8, FAST> (6 column blocks)", 60, 27, 32, 192, via="fused", relu=True),
        case("general_form", "splitk<VEC4, RT=1, NW=8, ACC=false, FAST=false> (EPRECON_CONV_SPLITK_FAST=0)", 129, 27, 32, 32,
             aff=True, env={"EPRECON_CONV_SPLITK_FAST": "0"}),
        case("layernorm", "splitk<VEC4, RT=1, NW=8, FAST>", 129, 27, 32, 32, via="ln", relu=True, res=True, ln=True,
             post_relu=True),
        case("layernorm_relu_before_residual", "splitk<VEC4, RT=1, NW=8, FAST>", 33, 27, 32, 17, via="ln", relu=True, res=True,
             ln=True),
        case("down_k8", "splitk<VEC4, RT=1, NW=4> (no packing: K = 8)", 500, 8, 16, 8, via="conv", map="down"),
        case("up_k8", "splitk<VEC4, RT=1, NW=4>", 700, 8, 32, 16, via="conv", map="up"),
        case("wide_below_4096_rows", "splitk<VEC4, RT=1, NW=4, FAST>", 4095, 27, 96, 65, via="fused", relu=True, stats=True),
        case("image_short_bn_acc", "splitk<VEC4, RT=1, NW=4, ACC> (accumulator blocks)", 1200, 9, 24, 24, via="d2",
             img=(1, 30, 40), aff=True, arena=True),
        case("image_short_in_acc", "splitk<VEC4, RT=1, NW=4, ACC> finishing its input's accumulator block", 1200, 9, 24, 24,
             via="d2", img=(1, 30, 40), in_acc=True, arena=True, pre_relu=True),
    ],
    "spconv_direct16_kernel": [
        case("rows32769_first_long_list", "direct16 ct1 (K = 27)", 32769, 27, 16, 16, aff=True),
        case("k1_20000_rows", "direct16 ct4 (K = 1, identity map; K1_DIRECT_MIN_ROWS)", 20000, 1, 32, 64, via="fused", map=None,
             relu=True, res=True, stats=True),
        case("cin13_nan_pitch_slice", "direct16 ct3", 40000, 27, 13, 33, via="fused", xld=16, oslice=True),
        case("bf16x3", "direct16 ct3, EPRECON_CONV_BF16X3=1", 35000, 27, 32, 48, aff=True, bound=BF16X3,
             env={"EPRECON_CONV_BF16X3": "1"}),
        case("cin24_chunk8_cout8", "direct16 ct1", 34000, 27, 24, 8, rep=True),
        case("cout1", "direct16 ct1", 33000, 27, 16, 1, aff=True),
        case("image_cout64", "direct16 ct4 (K = 9 pixel map)", 40000, 9, 32, 64, via="d2", img=(1, 200, 200), aff=True,
             pre_relu=True),
        case("image_cout64_bn_acc", "direct16 ct4, accumulator blocks", 40000, 9, 32, 64, via="d2", img=(1, 200, 200),
             aff=True, arena=True),
        case("image_in_acc", "direct16 ct2 finishing its input's accumulator block (tile16 declines in_acc)", 40000, 9, 16, 32,
             via="d2", img=(1, 200, 200), in_acc=True, arena=True, rep=True),
    ],
    "spconv_resident_kernel": [
        *[case(f"accumulate_rows{n}", "resident<1, VEC4, NCH=4, PIPE>", n, 27, 32, 32, via="fused", acc=True, relu=True,
               oslice=n % 2 == 1, rep=n == 129) for n in ROWS],
        case("accumulate_nt2", "resident<2, VEC4, NCH=3, PIPE> (258 blocks: no column split)", 33000, 27, 24, 64, via="fused",
             acc=True),
        case("accumulate_unaligned", "resident<1, VEC4=false, NCH=2, PIPE=false> over blockIdx.y", 300, 27, 13, 40, via="fused",
             acc=True, xoff=1),
        case("accumulate_cin13_nan_pitch", "resident<1, VEC4, NCH=2, PIPE>", 200, 27, 13, 17, via="fused", acc=True, xld=16),
        case("accumulate_cout96_split", "resident<1, VEC4, NCH=4, PIPE> over 3 column blocks", 500, 27, 32, 96, via="fused",
             acc=True, oslice=True),
        case("down_k8_summaries128", "resident<1, VEC4, NCH=4, PIPE> (128-row summaries: split-K declines)", 1000, 8, 32, 32,
             via="fused", map="down", stats=True),
        case("k1_19999_rows", "resident<1, VEC4, NCH=4, PIPE> over blockIdx.y (one row under K1_DIRECT_MIN_ROWS)", 19999, 1, 32,
             64, via="fused", map=None, res=True),
        case("direct_off", "resident<1, VEC4, NCH=2, PIPE> (EPRECON_CONV_DIRECT=0)", 33000, 27, 16, 16, aff=True,
             env={"EPRECON_CONV_DIRECT": "0"}),
        case("layernorm_k8", "resident<2, VEC4, NCH=4, PIPE>", 500, 8, 32, 64, via="ln", map="down", ln=True, relu=True,
             res=True, post_relu=True),
        case("image_20000_rows", "resident<1, VEC4, NCH=5, PIPE> over blockIdx.y (kT2ShortMaxRows)", 20000, 9, 40, 40,
             via="d2", img=(1, 100, 200), aff=True, res=True, res_aff=True),
        case("image_in_acc", "resident<1, VEC4, NCH=5, PIPE> finishing its input's accumulator block", 20000, 9, 40, 40,
             via="d2", img=(1, 100, 200), in_acc=True, arena=True, res=True),
    ],
    "spconv_resident_kernel(wide)": [
        case("down_k8_cin96_summaries128", "resident<1, VEC4, NCH=6, PIPE> over blockIdx.y, 2 slabs", 600, 8, 96, 48,
             via="fused", map="down", stats=True),
        case("accumulate_cin96", "resident<1, VEC4, NCH=6, PIPE> over blockIdx.y, 2 slabs", 300, 27, 96, 64, via="fused",
             acc=True, relu=True, rep=True),
        case("accumulate_cin72", "resident<1, VEC4, NCH=5, PIPE>, 2 slabs", 129, 27, 72, 33, via="fused", acc=True),
        case("accumulate_cin98_nan_pitch", "resident<1, VEC4, NCH=7, PIPE>, 2 slabs", 200, 27, 98, 16, via="fused", acc=True,
             xld=100),
        case("layernorm_k8", "resident<2, VEC4, NCH=6, PIPE>, 2 slabs", 400, 8, 96, 64, via="ln", map="down", ln=True,
             post_relu=True),
        case("rows40001_past_wide", "resident<2, VEC4, NCH=6, PIPE>, 2 slabs", 40001, 27, 96, 65, via="fused", stats=True),
    ],
    "spconv_mfma_kernel": [
        *[case(f"k1_accumulate_rows{n}", "mfma<1, VEC4>", n, 1, 96, 32, via="fused", map=None, acc=True, relu=n % 2 == 0)
          if n % 2 == 0 else
          case(f"unaligned_accumulate_rows{n}", "mfma<1, VEC4=false>", n, 27, 94, 40, via="fused", acc=True, xoff=1,
               oslice=True, rep=n == 129) for n in ROWS],
        case("accumulate_unaligned_cin94", "mfma<1, VEC4=false>", 300, 27, 94, 32, via="fused", acc=True, xoff=1, relu=True),
        case("k1_cout129_long", "mfma<4, VEC4> over blockIdx.y", 33000, 1, 96, 129, via="fused", map=None, relu=True),
        case("k1_cout33_short", "mfma<1, VEC4> over blockIdx.y", 129, 1, 96, 33, via="conv", map=None),
        case("layernorm_k1_cout128", "mfma<4, VEC4>", 300, 1, 96, 128, via="ln", map=None, ln=True, res=True, relu=True),
        case("pending_bn_unaligned", "mfma<1, VEC4=false> (EPRECON_CONV_SPLITK=0)", 300, 27, 96, 32, xoff=1, aff=True,
             env={"EPRECON_CONV_SPLITK": "0"}, rep=True),
        case("pending_bn_unaligned_long", "mfma<1, VEC4=false> over 3 column blocks", 11000, 27, 96, 80, xoff=1, aff=True),
        case("k1_accumulate_cout192", "mfma<1, VEC4> over 6 column blocks", 200, 1, 80, 192, via="fused", map=None, acc=True),
        case("k1_cin100_slice", "mfma<1, VEC4>", 127, 1, 100, 24, via="fused", map=None, oslice=True),
        case("up_k8_unaligned", "mfma<1, VEC4=false>", 800, 8, 96, 16, via="fused", map="up", acc=True, xoff=1),
    ],
    "spconv_wide_kernel": [
        case("rows4096", "wide<3>", 4096, 27, 96, 65, via="fused", relu=True, res=True),
        case("rows40000", "wide<4>", 40000, 27, 128, 128, aff=True),
        case("rows9415_slice", "wide<3>", 9415, 27, 192, 96, via="fused", oslice=True, stats=True, rep=True),
    ],
    "conv2d_tile_kernel": [
        case("ragged_tiles", "conv2d_tile<1, NCH=3> over 2 column blocks", 31200, 9, 24, 40, via="d2", img=(4, 60, 130),
             aff=True, pre_relu=True, res=True, res_aff=True, rep=True),
        case("rows39999", "conv2d_tile<1, NCH=2> (kT2MinRows - 1)", 39999, 9, 16, 16, via="d2", img=(1, 3, 13333)),
        case("cin36_nch5", "conv2d_tile<1, NCH=5>", 32000, 9, 36, 8, via="d2", img=(2, 100, 160), aff=True),
        case("bn_acc_cout1", "conv2d_tile<1, NCH=1>, accumulator blocks", 31200, 9, 8, 1, via="d2", img=(4, 60, 130), aff=True,
             arena=True),
        case("in_acc", "conv2d_tile<1, NCH=3> finishing its input's accumulator block", 31200, 9, 24, 24, via="d2",
             img=(4, 60, 130), in_acc=True, arena=True, oslice=True),
        case("cin4_cout33", "conv2d_tile<1, NCH=1> over 2 column blocks", 31200, 9, 4, 33, via="d2", img=(4, 60, 130),
             oslice=True),
    ],
    "conv2d_tile16_kernel": [
        case("rows40000", "tile16 ct1 kch1 (kT2MinRows)", 40000, 9, 16, 16, via="d2", img=(1, 200, 200), aff=True),
        case("cin48_cout17_residual", "tile16 ct2 kch3", 51000, 9, 48, 17, via="d2", img=(2, 150, 170), pre_relu=True, res=True,
             res_aff=True, rep=True),
        case("cin12_cout48_bn_acc", "tile16 ct3 kch1, accumulator blocks", 40803, 9, 12, 48, via="d2", img=(1, 203, 201),
             aff=True, arena=True),
        case("cin40_cout33_slice", "tile16 ct3 kch3", 43200, 9, 40, 33, via="d2", img=(1, 120, 360), oslice=True),
    ],
    "conv2d_tile_short_kernel": [
        case("cin40_cout40", "tile_short CT=3 KCH=3", 1200, 9, 40, 40, via="d2", img=(1, 30, 40), aff=True, rep=True),
        case("cin80_cout80_residual", "tile_short CT=5 KCH=5", 5400, 9, 80, 80, via="d2", img=(2, 45, 60), pre_relu=True,
             res=True),
        case("rows19999", "tile_short CT=5 KCH=3 (kT2ShortMaxRows - 1)", 19999, 9, 36, 65, via="d2", img=(1, 7, 2857),
             aff=True),
        case("cin80_cout40_bn_acc", "tile_short CT=3 KCH=5, accumulator blocks", 10800, 9, 80, 40, via="d2", img=(1, 60, 180),
             aff=True, arena=True),
    ],
    "conv3d_tile16_kernel": [
        case("cin16_cout16", "conv3d_tile16<CT=1, KCH=1>", 0, 27, 16, 16, map="grid", dims=(12, 10, 16), fill=0.7, aff=True,
             rep=True),
        case("cin32_cout17_residual_slice", "conv3d_tile16<CT=2, KCH=2>", 0, 27, 32, 17, via="fused", map="grid",
             dims=(9, 13, 17), fill=0.9, relu=True, res=True, oslice=True, stats=True),
        case("cin64_cout32", "conv3d_tile16<CT=2, KCH=4>", 0, 27, 64, 32, map="grid", dims=(8, 8, 8), fill=0.5),
        case("layernorm", "conv3d_tile16<CT=2, KCH=1>", 0, 27, 16, 32, via="ln", map="grid", dims=(10, 10, 10), ln=True,
             relu=True, res=True, post_relu=True),
    ],
    "conv3d_tile_narrow_kernel": [
        case("cin16", "conv3d_tile_narrow<NCH=2>", 0, 27, 16, 1, map="grid", dims=(12, 10, 16), fill=0.7, aff=True, rep=True),
        case("cin4_fused", "conv3d_tile_narrow<NCH=1>", 0, 27, 4, 1, via="fused", map="grid", dims=(9, 13, 17), fill=0.9,
             relu=True),
        case("cin64", "conv3d_tile_narrow<NCH=8>", 0, 27, 64, 1, map="grid", dims=(8, 9, 10), fill=0.5),
    ],
}

CASES = [pytest.param(fam, c, id=f"{fam}-{c['id']}") for fam, cs in FAMILIES.items() for c in cs]


def test_table_names_exactly_the_dispatched_families():
    """CPU: the names the dispatcher can report are exactly the table's keys (a family added or removed fails here)"""
    with open(os.path.join(ROOT, "eprecon_amd", "csrc", "sparse_conv.hip")) as f:
        table = re.search(r"\bkConvFamilyNames\[\]\s*=\s*\{(.*?)\};", f.read(), re.S)     # the dispatcher's one table of names
    assert table
    names = set(re.findall(r'"([^"]*)"', table.group(1)))
    assert names == set(FAMILIES), (sorted(names - set(FAMILIES)), sorted(set(FAMILIES) - names))
    for fam, cs in FAMILIES.items():
        assert cs, fam
        assert len({c["id"] for c in cs}) == len(cs), fam


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def mixed_map(rng, n, kvol, fill):
    """int32 [K, n] over n input rows: random live entries, the centre offset = the row itself, every 7th row with only its
    centre, one offset dead for every row, and rows 32..63 without a live entry at the first K // 2 offsets"""
    nbr = np.where(rng.random((kvol, n)) < fill, rng.integers(0, n, (kvol, n)), -1).astype(np.int32)
    centre = kvol // 2
    nbr[centre] = np.arange(n)
    only = np.arange(0, n, 7)
    nbr[:, only] = -1
    nbr[centre, only] = only
    if kvol > 2:
        nbr[kvol - 2] = -1
    if n > 64:
        nbr[:kvol // 2, 32:64] = -1
    return nbr


def down_map(rng, n):
    """k2s2 down map: each of n coarse rows has 1..8 of its 8 children (missing children -1); -> (map [8, n], n_in)"""
    live = rng.random((8, n)) < 0.5
    live[rng.integers(0, 8, n), np.arange(n)] = True
    nbr = np.full((8, n), -1, np.int32)
    nbr[live] = rng.permutation(int(live.sum()))
    return nbr, int(live.sum())


def up_map(rng, n):
    """transposed map: each of n fine rows has its one parent at the offset of its position; -> (map [8, n], n_in)"""
    n_in = max(1, n // 3)
    nbr = np.full((8, n), -1, np.int32)
    nbr[rng.integers(0, 8, n), np.arange(n)] = rng.integers(0, n_in, n)
    return nbr, n_in


def features(rng, n, c, xoff=0, ld=None):
    """f32 [n, c], possibly a column slice (offset xoff, pitch ld) of a NaN-filled buffer"""
    ld = ld or xoff + ((c + 3) & ~3)
    buf = torch.full((max(n, 1), ld + (4 if xoff else 0)), float("nan"), dtype=torch.float32, device="cuda")[:n]
    x = buf[:, xoff:xoff + c]
    x.copy_(torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)))
    return x


GUARD_ROWS = 129     # (a 128-row workgroup's tail past the last row, and one more)
GUARD_ACC = -4096.5  # guard rows of an `accumulate` output: finite, so that out += v past n_out changes them (NaN + v stays NaN)


def out_buffer(n, c, oslice, accumulate=False):
    """rows [0, n) of a NaN-filled buffer with GUARD_ROWS rows below them; with oslice, columns [3, 3 + c) of a wider one"""
    buf = torch.full((n + GUARD_ROWS, c + 7 if oslice else c), float("nan"), dtype=torch.float32, device="cuda")
    if accumulate:
        buf[n:] = GUARD_ACC
    return buf, (buf[:n, 3:3 + c] if oslice else buf[:n])


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------
# checks

def check_close(y, ref, s, bound, what):
    y64 = y.to(torch.float64)
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
    err = (y64 - ref).abs()
    ratio = float((err / (s * bound).clamp_min(1e-30)).max()) if err.numel() else 0.0
    assert ratio <= 1.0, f"{what}: |y - ref| / ({bound:g} S) = {ratio:.3g}"
    return ratio * bound


def check_summaries(partial, y, what):
    """counts exact; merged mean / M2 against float64 statistics of the kernel's own stored rows"""
    cnt = partial[:, 0].to(torch.float64)
    assert bool((cnt == cnt.round()).all() and (cnt >= 0).all()), f"{what}: non-integral summary counts"
    n, mean, m2 = R.merge_summaries(partial)
    rn, rmean, rm2 = R.column_stats(y)
    assert bool((n == rn).all()), f"{what}: counts {n.unique().tolist()} != {rn}"
    sd = torch.sqrt(rm2 / max(rn, 1))
    e_mean = float(((mean - rmean).abs() / (rmean.abs() + sd).clamp_min(1e-30)).max())
    e_m2 = float(((m2 - rm2).abs() / rm2.clamp_min(1e-30)).max())
    assert e_mean <= 1e-6 and e_m2 <= 1e-6, f"{what}: summaries mean {e_mean:.3g} M2 {e_m2:.3g}"
    return max(e_mean, e_m2)


def check_affine(scale, shift, y, gamma, beta, eps, what):
    rs, rb = R.bn_affine(y, gamma, beta, eps)
    e_s = float(((scale.to(torch.float64) - rs).abs() / rs.abs().clamp_min(1e-30)).max())
    b64 = beta.to(torch.float64)
    e_b = float(((shift.to(torch.float64) - rb).abs() / (b64.abs() + (rb - b64).abs()).clamp_min(1e-30)).max())
    assert e_s <= 1e-5 and e_b <= 1e-5, f"{what}: BatchNorm affine scale {e_s:.3g} shift {e_b:.3g}"
    return max(e_s, e_b)


# ---------------------------------------------------------------------------------------------------------------------------
# one case

def run_case(c, rng):
    """issue the case once through its wrapper -> dict(y, ref, s, partial, affine, buf, family)"""
    from eprecon_amd import _lib
    from eprecon_amd import dense2d as D2
    from eprecon_amd import sparse as SP
    k, cin, cout = c["k"], c["cin"], c["cout"]
    nbr = cells = None
    n = c["n"]
    if c["map"] == "grid":
        from test_dense_conv3d_gpu import grid_set
        coords = grid_set(rng, c["dims"], 1, c["fill"])
        vs = SP.VoxelSet(torch.from_numpy(coords).cuda(), 1, dims=c["dims"])
        nbr = SP.DenseMap(vs, c["dims"])
        cells = torch.from_numpy(coords[:, 1:].astype(np.int64)).cuda()
        n = n_in = len(coords)
    elif c["map"] == "mixed" and c["via"] != "d2":
        nbr_np, n_in = mixed_map(rng, n, k, c["fill"]), n
    elif c["map"] == "down":
        nbr_np, n_in = down_map(rng, n)
    elif c["map"] == "up":
        nbr_np, n_in = up_map(rng, n)
    else:
        nbr_np, n_in = None, n
    if c["map"] in ("mixed", "down", "up") and c["via"] != "d2":
        nbr = torch.from_numpy(nbr_np).cuda()
    x = features(rng, n_in, cin, c["xoff"], c["xld"])
    w = t32(rng.normal(0, 1, (k, cin, cout)) / np.sqrt(k * cin))
    bias = t32(rng.normal(0, 0.5, cout)) if c["bias"] else None
    aff = (t32(rng.uniform(0.5, 1.5, cin)), t32(rng.uniform(0.2, 1.0, cin)), True) if c["aff"] else None
    res = t32(rng.uniform(-1, 1, (n, cout))) if c["res"] else None
    res_aff = (t32(rng.uniform(0.5, 1.5, cout)), t32(rng.uniform(-0.5, 0.5, cout)), True) if c["res_aff"] else None
    lnp = (t32(rng.uniform(0.5, 1.5, cout)), t32(rng.normal(0, 0.3, cout)), 1e-5, c["post_relu"]) if c["ln"] else None
    buf, out = out_buffer(n, cout, c["oslice"], c["acc"])
    prior = None
    if c["acc"]:
        prior = t32(rng.uniform(-1, 1, (n, cout)))
        out.copy_(prior)
    r = dict(buf=buf, partial=None, affine=None)
    gamma, beta = t32(rng.uniform(0.5, 1.5, cout)), t32(rng.normal(0, 0.3, cout))
    via = c["via"]
    if via == "stats":
        y, r["partial"] = SP.conv_stats(x, w, nbr, in_affine=aff, out=out, bias=bias)
    elif via == "fused":
        y, r["partial"] = SP.sparse_conv_fused(x, w, nbr, bias, out, c["relu"], res, c["acc"], bn_partial=c["stats"])
    elif via == "conv":
        y = SP.sparse_conv(x, w, nbr, bias, out, c["relu"], c["acc"])
    elif via == "ln":
        y = SP.sparse_conv_ln(x, w, nbr, bias, lnp[0], lnp[1], lnp[2], out=out, relu=c["relu"], residual=res,
                              post_relu=lnp[3])
    else:   # dense2d.conv_bn_launch on a pixel grid: BN([ReLU](conv(a) + b) [+ BN_res(res)]) left pending
        maps, h, wd = c["img"]
        grid = D2.PixelGrid(maps, h, wd, x.device)
        xa = D2.Act(x, aff[0], aff[1], True) if aff else D2.Act(x)
        ra = D2.Act(res, res_aff[0], res_aff[1], True) if res_aff else (D2.Act(res) if res is not None else None)
        if c["arena"]:
            with D2.bn_pass(D2.BnArena(x.device, words=1 << 14)):
                if c["in_acc"]:
                    # a producer layer first: its BatchNorm stays pending as an accumulator block, which the case's launch
                    # finishes in its prologue while gathering; the reference applies the float64 BatchNorm of the rows it stored
                    gp, bp = t32(rng.uniform(0.5, 1.5, cin)), t32(rng.normal(0, 0.3, cin))
                    wp = t32(rng.normal(0, 1, (9, 8, cin)) / np.sqrt(72))
                    xa = D2.conv_bn_launch(wp, None, gp, bp, 1e-5, 3, D2.Act(features(rng, n, 8)), grid, relu=True)
                    assert xa.acc is not None and xa.scale is None, "the producer did not take the accumulator form"
                    x = xa.rows
                    sc, sh = R.bn_affine(x, gp, bp, 1e-5)
                    aff = (sc, sh, True)
                act = D2.conv_bn_launch(w, bias, gamma, beta, 1e-5, 3, xa, grid, out=out, pre_relu=c["pre_relu"],
                                        residual=ra)
            assert act.acc is not None, "the launch did not take the accumulator form"
        else:
            act = D2.conv_bn_launch(w, bias, gamma, beta, 1e-5, 3, xa, grid, out=out, pre_relu=c["pre_relu"],
                                    residual=ra)
        y = act.rows
        r["affine"] = act.affine()
        r["gamma_beta"] = (gamma, beta)
    r["family"] = _lib.last_conv_kernel()
    torch.cuda.synchronize()
    # float64 reference
    if via == "d2":
        acc, s = R.image_conv(x, w, *c["img"], in_affine=aff)
        ref, s = R.epilogue(acc, s, bias, c["pre_relu"], res, res_aff)
    else:
        if c["map"] == "grid":
            acc, s = R.grid_conv(x, w, cells, c["dims"], in_affine=aff)
        else:
            acc, s = R.gather_conv(x, w, nbr, in_affine=aff)
        ref, s = R.epilogue(acc, s, bias, c["relu"], res, out=prior, ln=lnp)
    r.update(y=y, ref=ref, s=s)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("family,c", CASES)
def test_family_case(monkeypatch, record_property, family, c):
    for key, v in c["env"].items():
        monkeypatch.setenv(key, v)
    rng = np.random.default_rng(zlib.crc32(f"{family}-{c['id']}".encode()))
    state = rng.bit_generator.state
    r = run_case(c, rng)
    what = f"{family}-{c['id']} [{c['inst']}]"
    assert r["family"] == family, f"{what}: the launch went to {r['family']}"
    y = r["y"]
    assert y.shape[1] == c["cout"]
    if c["ln"]:
        assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
        err = float((y.to(torch.float64) - r["ref"]).abs().max())
        assert err <= LN_TOL, f"{what}: LayerNorm output off by {err:.3g}"
        record_property("ln_err", err)
    else:
        worst = check_close(y, r["ref"], r["s"], c["bound"], what)
        record_property("err_over_S", worst)
    buf, n = r["buf"], y.shape[0]
    guard = buf[n:] == GUARD_ACC if c["acc"] else torch.isnan(buf[n:])
    assert bool(guard.all()), f"{what}: wrote rows past n_out"
    if c["oslice"]:
        edges = torch.cat([buf[:n, :3], buf[:n, 3 + c["cout"]:]], 1)
        assert bool(torch.isnan(edges).all()), f"{what}: wrote outside its output slice"
    if r["partial"] is not None:
        record_property("summary_err", check_summaries(r["partial"], y, what))
    if r["affine"] is not None:
        record_property("affine_err", check_affine(*r["affine"], y, *r["gamma_beta"], 1e-5, what))
    if c["rep"]:
        rng2 = np.random.default_rng()
        rng2.bit_generator.state = state
        r2 = run_case(c, rng2)
        assert torch.equal(r2["y"], y), f"{what}: a second run gave other bits"
        if r["partial"] is not None:
            assert torch.equal(r2["partial"], r["partial"]), f"{what}: a second run gave other summaries"


# ---------------------------------------------------------------------------------------------------------------------------
# combinations the dispatcher must refuse

def _ln_desc(x, w, nbr, out, cout, **kw):
    from eprecon_amd import _lib
    d = _lib.ConvDesc()
    d.x, d.n_in, d.ld_x = x.data_ptr(), x.shape[0], x.stride(0)
    d.nbr, d.kvol, d.n_out = nbr.data_ptr(), nbr.shape[0], nbr.shape[1]
    d.weight, d.cin, d.cout = w.data_ptr(), w.shape[1], cout
    d.out, d.ld_out = out.data_ptr(), out.stride(0)
    d.ln, d.ln_eps = 1, 1e-5
    for key, v in kw.items():
        setattr(d, key, v)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("cout,extra", [(129, {}), (192, {}), (32, {"accumulate": 1}), (64, "bn_partial")],
                         ids=["cout129", "cout192", "accumulate", "summaries"])
def test_layernorm_refusals(cout, extra):
    """LayerNorm needs every column of a row in one workgroup (nt_full <= 4) and takes neither accumulate nor summaries:
    EPRECON_ERR_UNSUPPORTED, and the output is left alone"""
    from eprecon_amd import _lib
    rng = np.random.default_rng(cout)
    n = 300
    x = features(rng, n, 32)
    w = t32(rng.normal(0, 0.1, (27, 32, cout)))
    nbr = torch.from_numpy(mixed_map(rng, n, 27, 0.5)).cuda()
    out = torch.full((n, cout), 7.0, dtype=torch.float32, device="cuda")
    keep = []
    if extra == "bn_partial":
        part = torch.zeros((3 * cout * 3,), dtype=torch.float32, device="cuda")
        keep.append(part)
        extra = {"bn_partial": part.data_ptr(), "bn_ld": 3}
    d = _ln_desc(x, w, nbr, out, cout, **extra)
    rc = _lib.load().eprecon_conv_desc_async(ctypes.byref(d), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -3, rc       # EPRECON_ERR_UNSUPPORTED
    assert bool((out == 7.0).all())

"""Host-side layout logic of the round-4 entry points (no GPU): the operand order the one-launch heads kernel expects from
sparse._pack_mlp_weight (include/eprecon_hip.h: eprecon_mlp4x_async), the tap-major depthwise weights, and the sizing
functions of the library that do not touch a device."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("k,m", [(24, 96), (96, 24), (88, 352), (48, 1), (176, 48)])
def test_mlp_weight_packing_matches_the_header(k, m):
    """block (t, c), lane 16 q + j, component i = Wt[16 c + 4 q + i][16 t + j], zero outside the matrix"""
    from eprecon_amd.sparse import _pack_mlp_weight
    torch.manual_seed(k + m)
    wt = torch.randn(k, m)
    packed = _pack_mlp_weight(wt).numpy()
    kc, mt = (k + 15) // 16, (m + 15) // 16
    assert packed.shape == (mt * kc * 64 * 4,)
    p = packed.reshape(mt, kc, 4, 16, 4)            # [t][c][q][j][i]
    w = np.zeros((16 * kc, 16 * mt), np.float32)
    w[:k, :m] = wt.numpy()
    rng = np.random.default_rng(0)
    for _ in range(200):
        t, c, q, j, i = rng.integers(mt), rng.integers(kc), rng.integers(4), rng.integers(16), rng.integers(4)
        assert p[t, c, q, j, i] == w[16 * c + 4 * q + i, 16 * t + j]
    assert np.count_nonzero(packed) == np.count_nonzero(wt.numpy())


def test_pack_mlp4x_views_are_aligned_and_cached():
    from eprecon_amd.modules import Linear4xTrans
    from eprecon_amd.sparse import clear_packed_weights, pack_mlp4x
    m = Linear4xTrans(24, 1)
    a = pack_mlp4x(m)
    assert set(a) == {"w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3"}
    assert all(v.data_ptr() % 16 == 0 and v.numel() % 16 == 0 for v in a.values())
    assert a["b3"].numel() == 16 and float(a["b3"][1:].abs().sum()) == 0.0          # C_out = 1 padded to a tile
    assert a["g2"].numel() == 32 and float(a["g2"][24:].abs().sum()) == 0.0         # C = 24 padded to two tiles, zeros behind
    assert pack_mlp4x(m) is a                        # cached per parameter version
    with torch.no_grad():
        m.linear3.weight.add_(1.0)                   # an in-place write bumps the version
    assert pack_mlp4x(m) is not a
    b = pack_mlp4x(m)
    m.linear3.weight.data.mul_(2.0)                  # a write through .data does not: clear_packed_weights is the contract
    assert pack_mlp4x(m) is b
    clear_packed_weights(m)
    assert pack_mlp4x(m) is not b


def test_depthwise_taps_are_tap_major():
    import torch.nn as nn
    from eprecon_amd.backbone import _dw_taps, _is_depthwise
    conv = nn.Conv2d(8, 8, 5, padding=2, stride=2, groups=8, bias=False)
    taps = _dw_taps(conv)
    assert taps.shape == (25, 8) and taps.is_contiguous()
    assert torch.equal(taps[7], conv.weight.detach()[:, 0, 1, 2])        # tap (dy, dx) = (1, 2) -> row 5 * 1 + 2
    assert _is_depthwise(conv)
    assert not _is_depthwise(nn.Conv2d(8, 8, 3, padding=1))              # dense
    assert not _is_depthwise(nn.Conv2d(8, 8, 3, padding=0, groups=8, bias=False))    # not 'same' padded
    assert not _is_depthwise(nn.Conv2d(6, 6, 3, padding=1, groups=6, bias=False))    # channels not a multiple of 4


def test_sizing_functions_of_the_library():
    from eprecon_amd import _lib
    lib = _lib.load()
    # per-view BatchNorm: ~16 rows per row lane, between 1 and 128 ranges per view
    assert lib.eprecon_bn2d_views_chunks(76800, 32) == 128 and lib.eprecon_bn2d_views_chunks(1200, 480) == 38
    assert lib.eprecon_bn2d_views_chunks(10, 16) == 1
    assert lib.eprecon_bn2d_views_workspace_bytes(9, 1200, 480) == 9 * 38 * 3 * 480 * 4
    # shapes the one-launch heads take
    assert lib.eprecon_mlp4x_supported(96, 1) and lib.eprecon_mlp4x_supported(176, 48) and lib.eprecon_mlp4x_supported(48, 48)
    assert not lib.eprecon_mlp4x_supported(96, 48) and not lib.eprecon_mlp4x_supported(50, 1)
    # workspaces grow with their arguments and are 0 for nothing to do
    assert lib.eprecon_sphash_order_workspace_bytes(0) == 0
    assert lib.eprecon_sphash_order_workspace_bytes(400000) > lib.eprecon_sphash_order_workspace_bytes(1000) > 0
    assert lib.eprecon_gru_stage_finish_workspace_bytes(1000, 900, 1000) >= lib.eprecon_sphash_order_workspace_bytes(1000)
    assert lib.eprecon_spvcnn_geometry_workspace_bytes(1000, 900, 100) > 0


def test_backbone_walker_on_the_pytorch_fallbacks():
    """MnasMulti._run_hip (one module of look-ahead: pending BatchNorm in front of a depthwise layer, the block's skip added by
    the last BatchNorm's apply pass) walks the trunk correctly: on CPU tensors every HIP piece falls back to its PyTorch
    expression, and the result must equal the plain per-view route"""
    import eprecon_amd.backbone as BB
    torch.manual_seed(0)
    net = BB.MnasMulti(1.0).train()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.7, 1.3)
                m.bias.uniform_(-0.2, 0.2)
        x = torch.randn(4, 3, 32, 48).contiguous(memory_format=torch.channels_last)     # two views of two images
        v = 2
        for stage in (net.conv0, net.conv1):
            a = net._run(stage, x, v)
            b = net._run_hip(stage, x, v)
            assert a.shape == b.shape
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), float((a - b).abs().max())
            x = a


def _conv_desc(n_out, kvol, cin, cout, **kw):
    """a ConvDesc with made-up 16-byte aligned addresses: the two sizing entry points below are host arithmetic and
    dereference nothing.  Rows of cin / cout floats, as many input rows as output rows, a kernel map unless nbr=0 is given."""
    from eprecon_amd import _lib
    d = _lib.ConvDesc()
    d.x, d.n_in, d.ld_x = 0x10000, n_out, cin
    d.nbr, d.kvol, d.n_out = 0x20000, kvol, n_out
    d.weight, d.cin, d.cout = 0x30000, cin, cout
    d.out, d.ld_out = 0x40000, cout
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _cdiv(a, b):
    return -(-a // b)


def test_summary_rows_and_workspace_per_convolution_family(monkeypatch):
    """eprecon_conv_desc_partial_rows / eprecon_conv_desc_workspace_bytes against each family's documented workgroup, at the
    smallest shapes on either side of a selection boundary (the direct gather kernel is left out: its block rows depend on the
    device, so the shapes that would reach it run with EPRECON_CONV_DIRECT=0)"""
    import ctypes
    import os
    from eprecon_amd import _lib
    lib = _lib.load()
    for name in [k for k in os.environ if k.startswith("EPRECON_CONV_") or k == "EPRECON_BN_ACC"]:
        monkeypatch.delenv(name)

    def rows(d):
        return lib.eprecon_conv_desc_partial_rows(ctypes.byref(d))

    def ws(d):
        return lib.eprecon_conv_desc_workspace_bytes(ctypes.byref(d))

    PACK, PACK16, RANK = 0x50000, 0x60000, 0x70000
    # ---- gather forms on a kernel map: 128-row workgroups (resident, resident on wide inputs, the slab kernel) ----
    for kvol, cin, cout, n in [(27, 32, 32, 100000), (27, 64, 64, 40000), (27, 72, 64, 40000), (9, 72, 64, 40001), (27, 20, 130, 33333)]:
        d = _conv_desc(n, kvol, cin, cout)
        assert rows(d) == _cdiv(n, 128) and ws(d) == 0, (kvol, cin, cout, n)
    # ---- split-K: 32-row summary blocks while the 128-row blocks x column tiles number 256 at most ----
    assert rows(_conv_desc(256 * 128, 27, 32, 32)) == 256 * 4
    assert rows(_conv_desc(256 * 128 + 1, 27, 32, 32)) == 257                      # one block more: resident
    assert rows(_conv_desc(128 * 128, 27, 72, 64)) == 128 * 4                      # two column tiles: 256 blocks
    assert rows(_conv_desc(128 * 128 + 1, 27, 72, 64)) == 129
    assert rows(_conv_desc(1000, 27, 32, 32, accumulate=1)) == 8                   # accumulate: never split-K
    monkeypatch.setenv("EPRECON_CONV_SPLITK", "0")
    assert rows(_conv_desc(1000, 27, 32, 32)) == 8
    monkeypatch.delenv("EPRECON_CONV_SPLITK")
    # ---- wide (cross-workgroup split of the offsets): 4,096..40,000 rows, C_in >= 96, 64 < C_out <= 128, packed weights, and
    # only with the workspace the library asks for; otherwise the shape is split-K's ----
    for n, cin, cout, wide in [(4096, 96, 65, True), (4095, 96, 65, False), (4096, 96, 64, False), (4096, 92, 65, False),
                               (40000, 128, 128, True), (40001, 128, 128, False), (4096, 96, 129, False)]:
        d = _conv_desc(n, 27, cin, cout, packed_weight=PACK)
        need = ws(d)
        assert (need > 0) == wide, (n, cin, cout)
        short = _cdiv(n, 128) * _cdiv(cout, 32) <= 256
        other = _cdiv(n, 32) if short else _cdiv(n, 128)
        assert rows(d) == other, (n, cin, cout)                                    # no workspace given
        if wide:
            d.workspace, d.workspace_bytes = 0x80000, need
            assert rows(d) == _cdiv(n, 128), (n, cin, cout)
            d.workspace_bytes = need - 1
            assert rows(d) == other, (n, cin, cout)
    assert ws(_conv_desc(4096, 27, 96, 65)) == 0                                   # no packed weights: not wide
    monkeypatch.setenv("EPRECON_CONV_WIDEK", "0")
    assert ws(_conv_desc(4096, 27, 96, 65, packed_weight=PACK)) == 0
    monkeypatch.delenv("EPRECON_CONV_WIDEK")
    # ---- conv2d_tile: 8 x 16 pixel tiles, from 256 tiles on ----
    img = dict(img_h=30, img_w=40)                                                 # 4 x 3 tiles per map, neither edge a multiple
    assert rows(_conv_desc(22 * 1200, 9, 24, 24, img_maps=22, **img)) == 22 * 12
    assert rows(_conv_desc(21 * 1200, 9, 24, 24, img_maps=21, **img)) == _cdiv(21 * 1200, 32)     # 252 tiles: split-K
    assert rows(_conv_desc(30 * 1200, 9, 44, 24, img_maps=30, **img)) == _cdiv(30 * 1200, 128)    # six 8-channel chunks: resident
    # ---- the 16-row image-tile kernel: 4 x 16 pixel tiles, lists of kT2MinRows = 40,000 rows and more, wq16 packing ----
    monkeypatch.setenv("EPRECON_CONV_DIRECT", "0")
    assert rows(_conv_desc(40000, 9, 24, 24, img_maps=1, img_h=200, img_w=200, packed_weight16=PACK16)) == 50 * 13
    assert rows(_conv_desc(39999, 9, 24, 24, img_maps=1, img_h=199, img_w=201, packed_weight16=PACK16)) == 25 * 13   # conv2d_tile
    assert rows(_conv_desc(40000, 9, 52, 24, img_maps=1, img_h=200, img_w=200, packed_weight16=PACK16)) == _cdiv(40000, 128)
    # ---- the short-list image kernel: one 16-pixel segment of a row per workgroup, lists below kT2ShortMaxRows = 20,000 ----
    assert rows(_conv_desc(10800, 9, 80, 40, img_maps=9, img_h=30, img_w=40, packed_weight16=PACK16)) == 9 * 30 * 3
    assert rows(_conv_desc(19999, 9, 80, 40, img_maps=1, img_h=2857, img_w=7, packed_weight16=PACK16)) == 2857
    assert rows(_conv_desc(20006, 9, 80, 40, img_maps=1, img_h=2858, img_w=7, packed_weight16=PACK16)) == _cdiv(20006, 128)
    assert rows(_conv_desc(10800, 9, 80, 40, img_maps=9, img_h=30, img_w=40)) == _cdiv(10800, 32)   # no packing: split-K
    # ---- dense-grid 3D: tiles of 4 x 4 x 8 cells (single column) or 2 x 4 x 8 (16-row MFMA kernel) over the whole grid ----
    grid = dict(vox_rank=RANK, grid_x=9, grid_y=10, grid_z=11)
    assert rows(_conv_desc(700, 27, 32, 1, **grid)) == 3 * 3 * 2
    assert rows(_conv_desc(700, 27, 32, 16, packed_weight16=PACK16, **grid)) == 5 * 3 * 2
    assert rows(_conv_desc(700, 27, 32, 16, **grid)) == _cdiv(700, 32)             # no packing: the kernel map (split-K)
    monkeypatch.setenv("EPRECON_CONV_DENSE3D", "1")
    assert rows(_conv_desc(700, 27, 32, 1, **grid)) == 18
    assert rows(_conv_desc(700, 27, 32, 16, packed_weight16=PACK16, **grid)) == _cdiv(700, 32)
    monkeypatch.setenv("EPRECON_CONV_DENSE3D", "0")
    assert rows(_conv_desc(700, 27, 32, 1, **grid)) == _cdiv(700, 32)
    assert rows(_conv_desc(0, 27, 32, 32)) == 0 and ws(_conv_desc(0, 27, 96, 65, packed_weight=PACK)) == 0


def test_dense_grid_kind_is_the_shape_rule_of_the_library(monkeypatch):
    """eprecon_conv_dense3d_kind (what DenseMap asks before it packs weights or drops the kernel map) on both sides of every
    clause of the rule, and its agreement with eprecon_conv_desc_partial_rows: kind 2 becomes the 16-row kernel's tile count
    only with a packed_weight16"""
    import ctypes
    import os
    from eprecon_amd import _lib
    lib = _lib.load()
    for name in [k for k in os.environ if k.startswith("EPRECON_CONV_")]:
        monkeypatch.delenv(name)
    monkeypatch.setenv("EPRECON_CONV_DIRECT", "0")       # (its summary rows depend on the device; no shape here is meant for it)
    PACK16, RANK, AFF = 0x60000, 0x70000, 0x90000

    def kind(cin=32, cout=16, n=700, kvol=27, **kw):
        grid = dict(vox_rank=RANK, grid_x=9, grid_y=10, grid_z=11)
        grid.update(kw)
        return lib.eprecon_conv_dense3d_kind(ctypes.byref(_conv_desc(n, kvol, cin, cout, **grid)))

    def rows(cin, cout, **kw):
        d = _conv_desc(700, 27, cin, cout, vox_rank=RANK, grid_x=9, grid_y=10, grid_z=11, **kw)
        return lib.eprecon_conv_desc_partial_rows(ctypes.byref(d))

    assert lib.eprecon_conv_dense3d_kind(None) == 0
    # C_in: a multiple of 4 up to 64 for either kernel, of 16 for the 16-row kernel
    assert kind(cin=32, cout=1) == 1 and kind(cin=30, cout=1) == 0 and kind(cin=36, cout=1) == 1
    assert kind(cin=64, cout=1) == 1 and kind(cin=68, cout=1) == 0
    assert kind(cin=64) == 2 and kind(cin=68) == 0 and kind(cin=80) == 0
    assert kind(cin=16) == 2 and kind(cin=36) == 0 and kind(cin=48) == 2
    # C_out: one column (without LayerNorm), or up to 32 columns
    assert kind(cout=1) == 1 and kind(cout=1, ln=1) == 2 and kind(cin=36, cout=1, ln=1) == 0
    assert kind(cout=2) == 2 and kind(cout=32) == 2 and kind(cout=33) == 0
    # LayerNorm with summaries and accumulate: not the 16-row kernel; the single-column kernel takes accumulate
    assert kind(ln=1) == 2 and kind(bn_partial=0xa0000) == 2 and kind(ln=1, bn_partial=0xa0000) == 0
    assert kind(accumulate=1) == 0 and kind(cout=1, accumulate=1) == 1
    # alignment of x, its pitch and the pending BatchNorm's vectors
    assert kind(ld_x=36) == 2 and kind(ld_x=34) == 0 and kind(cout=1, ld_x=34) == 0
    assert kind(x=0x10004) == 0 and kind(cout=1, x=0x10004) == 0 and kind(x=0x10010) == 2
    assert kind(in_scale=AFF, in_shift=AFF + 128) == 2 and kind(cout=1, in_scale=AFF, in_shift=AFF + 128) == 1
    assert kind(in_scale=AFF + 4, in_shift=AFF + 128) == 0 and kind(in_scale=AFF, in_shift=AFF + 132) == 0
    assert kind(cout=1, in_scale=AFF + 4, in_shift=AFF + 132) == 0
    # no grid, an empty grid, another kernel volume, no rows
    assert kind(vox_rank=None) == 0 and kind(grid_x=0) == 0 and kind(grid_y=0) == 0 and kind(grid_z=0) == 0
    assert kind(kvol=8) == 0 and kind(kvol=1) == 0 and kind(n=0) == 0 and kind(n=1) == 2
    # the packing is not part of the answer ...
    assert kind(packed_weight16=PACK16) == 2 and kind(packed_weight16=PACK16 + 4) == 2
    # ... it decides whether the launch gets the kernel: the 16-row kernel's 2 x 4 x 8 tiles, else the kernel-map family's rows
    assert rows(32, 16, packed_weight16=PACK16) == 5 * 3 * 2
    assert rows(32, 16) == _cdiv(700, 32) and rows(32, 16, packed_weight16=PACK16 + 4) == _cdiv(700, 32)
    assert rows(32, 1) == 3 * 3 * 2                                                # the single-column kernel needs none
    assert kind(cin=40, cout=32) == 0 and rows(40, 32, packed_weight16=PACK16) == _cdiv(700, 32)
    # the levels of EPRECON_CONV_DENSE3D, read per call
    monkeypatch.setenv("EPRECON_CONV_DENSE3D", "1")
    assert kind(cout=1) == 1 and kind() == 0 and rows(32, 16, packed_weight16=PACK16) == _cdiv(700, 32)
    monkeypatch.setenv("EPRECON_CONV_DENSE3D", "0")
    assert kind(cout=1) == 0 and kind() == 0
    monkeypatch.setenv("EPRECON_CONV_DENSE3D", "2")
    assert kind(cout=1) == 1 and kind() == 2


# lengths that straddle a scan tile (2,048) and the lengths at which the device scan changes its form (32,768; 4,096 tiles)
_SCAN_EDGES = [0, 1, 2047, 2048, 2049, 32768, 32769, 8388608, 8388609]
# the same products as three dimensions (2047 = 23 * 89, 2049 = 3 * 683, 32769 = 9 * 3641, 8388609 = 3 * 2796203)
_SCAN_EDGE_DIMS = [(0, 1, 1), (1, 1, 1), (23, 89, 1), (16, 16, 8), (3, 683, 1), (32, 32, 32), (9, 3641, 1), (256, 256, 128),
                   (3, 2796203, 1)]
_SCAN_EDGE_CUBES = [0, 1, 12, 13, 16, 32, 33, 203, 204]        # dim^3 around 2,048, 32,768 and 8,388,608


def _size_calls():
    """(function, arguments) of every sizing call the golden file records"""
    pairs = [(n, m) for n in _SCAN_EDGES for m in _SCAN_EDGES]
    calls = {
        "eprecon_hash_table_bytes": [(c,) for c in _SCAN_EDGES + [1024, 1 << 20, 1 << 31]],
        "eprecon_unique_workspace_bytes": [(n,) for n in [-1] + _SCAN_EDGES],
        "eprecon_gru_stage_workspace_bytes": [(n,) for n in _SCAN_EDGES],
        "eprecon_sphash_order_workspace_bytes": [(n,) for n in _SCAN_EDGES],
        "eprecon_marching_cubes_workspace_bytes": _SCAN_EDGE_DIMS,
        "eprecon_fbv_union_workspace_bytes": [(d,) for d in _SCAN_EDGE_CUBES],
        "eprecon_voxel_down_sample_workspace_bytes": pairs,
        "eprecon_nn_search_workspace_bytes": pairs,
        "eprecon_segment_workspace_bytes": pairs,
        "eprecon_label_volumes_workspace_bytes": pairs,
    }
    return [(name, args) for name, arglist in calls.items() for args in arglist]


def test_workspace_sizes_are_the_recorded_ones():
    """Every sizing function that counts a scan scratch or a hash table returns what tests/golden/workspace_sizes.json
    records (values taken from the build before the scratch size and the table layout got one definition each)."""
    import json
    import os
    from eprecon_amd import _lib
    lib = _lib.load()
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "workspace_sizes.json")))
    calls = _size_calls()
    assert sorted(golden) == sorted({name for name, _ in calls})
    assert sum(len(v) for v in golden.values()) == len(calls)
    for name, args in calls:
        want = golden[name][",".join(map(str, args))]
        got = getattr(lib, name)(*args)
        assert got == want, (name, args, got, want)


def test_scan_scratch_query_is_the_documented_rule():
    """eprecon_exclusive_scan_scratch_ints, the contract of the scan's scratch: one int32 per tile of 2,048 elements, one rule
    for every length; nothing where there is no scan"""
    from eprecon_amd import _lib
    lib = _lib.load()
    for n in _SCAN_EDGES + [100003, 320868, 2 ** 31 - 1]:
        assert lib.eprecon_exclusive_scan_scratch_ints(n) == (n + 2047) // 2048, n
    assert lib.eprecon_exclusive_scan_scratch_ints(-1) == 0 and lib.eprecon_exclusive_scan_scratch_ints(2 ** 31) == 0

"""GPU: the level-transition helpers (csrc/grid_ops.hip, and the join of csrc/norm.hip that shares its arithmetic) at their edges.

  init_select   list form on D = 1 .. 32 (D = 32: all 1,024 threads live, bit 31 of a column word shifted out; D < 3: nothing can
                survive), cells 1 / 2 / 4, batches 1 and 3, the patterns of tests/grid_cases.py; dense form against the list form on
                grids that are no multiple of the ratio.  Model: oracle/grid_ops.py, integer throughout, so bit exact.
  upsample      0 / 1 / 32 / 33 parents, 1 / 7 / 64 channels, negative coordinates, features as a column slice, features only and
                coordinates only, inside guard-filled buffers
  upsample2x    eprecon_upsample2x_nhwc_async and eprecon_affine_up2_rows_async against F.interpolate in float64 on the host.
                The weights (0, 1/4, 3/4, 1 and their products) are exact in fp32, so a result is four rounded products and three
                additions: |y - y64| <= 8 U S, U = 2^-24, S the same interpolation of |x|.  The join applies y = fma(x, scale, shift)
                first (one rounding, <= U A with A = |x scale| + |shift| >= |y|): |out - out64| <= U I(A) + 8 U (I(|y64|) + U I(A)).
  sparsify      the scan's 1,024-tile pass boundary, 63 / 64 / 65 channels, occ == thr, non-finite occupancy, pitched columns, the
                32-batch limit, rows of no batch element.  Model: the torch sequence of tests/test_sparsify_gpu.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import grid_cases as G
from oracle import grid_ops as OG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# init_select, list form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", G.CELLS)
@pytest.mark.parametrize("D", G.DIMS)
def test_init_select_list_form(D, cell):
    from eprecon_amd.grid_ops import init_select
    for names in G.calls(D):
        logit, coords = G.voxel_list(names, D, cell)
        with np.errstate(over="ignore", invalid="ignore"):
            want = OG.init_select(logit, coords, len(names), dim=D, cell=cell, thr=G.THRESHOLD)
        per = [int((want[:, 0] == b).sum()) for b in range(len(names))]
        for b, name in enumerate(names):                     # the oracle's own counts first
            if G.expected_rows(name, D) is not None:
                assert per[b] == G.expected_rows(name, D), (name, D, cell)
        got, counts = init_select(dev(logit).reshape(-1, 1), dev(coords), len(names), dim=D, cell=cell, threshold=G.THRESHOLD)
        assert list(counts) == per, (names, D, cell)
        assert np.array_equal(got.cpu().numpy(), want), (names, D, cell)      # per element, raster order, scaled by the cell


def test_init_select_without_rows_and_refusals():
    from eprecon_amd import _lib
    from eprecon_amd.grid_ops import init_select
    empty_l, empty_c = torch.zeros((0, 1), device="cuda"), torch.zeros((0, 4), dtype=torch.int32, device="cuda")
    got, counts = init_select(empty_l, empty_c, 2, dim=32, cell=4)
    assert got.shape == (0, 4) and list(counts) == [0, 0]
    for kw in (dict(dim=33), dict(dim=0), dict(cell=0)):
        with pytest.raises(_lib.EpreconError):
            init_select(empty_l, empty_c, 1, **{"dim": 24, "cell": 4, **kw})


# ---------------------------------------------------------------------------------------------------------------------
# init_select, dense form
# ---------------------------------------------------------------------------------------------------------------------
def _voxel_set(grid, stride, keep):
    from eprecon_amd import sparse as SP
    cells = np.argwhere(np.ones(grid, bool))
    coords = np.concatenate([np.zeros((cells.shape[0], 1), np.int64), stride * cells], 1).astype(np.int32)[keep]
    vset = SP.VoxelSet(dev(coords), stride, dims=grid)
    return coords, vset, SP.DenseMap(vset, grid)


@pytest.mark.parametrize("grid,stride,cell,D", [
    ((9, 7, 10), 2, 4, 5),        # ratio 2, no side a multiple of it
    ((9, 7, 10), 2, 4, 8),        # the grid is smaller than D * ratio
    ((9, 7, 10), 2, 4, 4),        # ... and larger: the cells beyond D are dropped
    ((5, 4, 6), 2, 2, 6),         # ratio 1 (cell == stride)
    ((9, 7, 10), 1, 4, 3),        # ratio 4
    ((63, 40, 64), 2, 4, 32),     # D = 32
    ((3, 5, 2), 1, 2, 2),         # D < 3
])
def test_init_select_dense_form_equals_the_list_form(grid, stride, cell, D):
    from eprecon_amd.grid_ops import init_select
    rng = np.random.default_rng(grid[0] * 100 + D)
    n_cells = grid[0] * grid[1] * grid[2]
    for fill in ("blobs", "all", "none", "nonfinite"):
        keep = rng.random(n_cells) < (1.0 if fill == "all" else 0.8)      # holes in the rank volume
        coords, vset, dense = _voxel_set(grid, stride, keep)
        centre = (np.array(grid) - 1.0) / 2.0
        dist = np.abs(coords[:, 1:] / stride - centre).max(axis=1) / (centre.max() + 1.0)
        logit = (3.0 - 6.0 * dist + rng.normal(0.0, 0.7, coords.shape[0])).astype(np.float32)       # a cube-ish blob with a ragged rim
        if fill == "all":
            logit[:] = 4.0
        elif fill == "none":
            logit[:] = -4.0
        elif fill == "nonfinite":
            logit[logit > 0] = np.inf
            logit[logit < -2] = -np.inf
            logit[(logit > -1) & (logit < 0)] = np.nan
        inside = (coords[:, 1:] // cell < D).all(axis=1)      # the list kernel drops the rest; the oracle would index past its volume
        with np.errstate(over="ignore", invalid="ignore"):
            want = OG.init_select(logit[inside], coords[inside], 1, dim=D, cell=cell, thr=G.THRESHOLD)
        listed, n_listed = init_select(dev(logit).reshape(-1, 1), vset.coords, 1, dim=D, cell=cell, threshold=G.THRESHOLD)
        got, n_got = init_select(dev(logit).reshape(-1, 1), vset.coords, 1, dim=D, cell=cell, threshold=G.THRESHOLD, dense=dense)
        assert list(n_listed) == list(n_got) == [want.shape[0]], (fill, grid, D)
        assert np.array_equal(listed.cpu().numpy(), want) and np.array_equal(got.cpu().numpy(), want), (fill, grid, D)
        if fill == "all" and D >= 3 and min(-(-g * stride // cell) for g in grid) >= 3:
            assert want.shape[0] > 0
        if fill == "none":
            assert want.shape[0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# upsample
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(shape, guard, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, guard):
    return bool((buf[:GUARD] == guard).all()) and bool((buf[-GUARD:] == guard).all())


def _parents(n, c, seed):
    rng = np.random.default_rng(seed)
    coords = rng.integers(-40, 96, size=(n, 4)).astype(np.int32)           # negative coordinates too
    coords[:, 0] = rng.integers(0, 3, size=n)
    wide = rng.standard_normal((n, c + 5)).astype(np.float32)
    return coords, wide


@pytest.mark.parametrize("interval", [1, 2, 4])
@pytest.mark.parametrize("c", [1, 7, 64])
@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_upsample_through_the_c_abi(n, c, interval):
    from eprecon_amd import _lib
    lib = _lib.load()
    coords, wide = _parents(n, c, 1000 * n + 10 * c + interval)
    feat = wide[:, 2:2 + c]
    want_f, want_c = OG.upsample(feat, coords, interval)
    d_coords, d_wide = dev(coords), dev(wide)
    d_feat = d_wide[:, 2:2 + c]                                             # a column slice: ld = c + 5
    st = _lib.current_stream()
    # both outputs in one call
    fbuf, up_f = _guarded((8 * n, c), -7.0, torch.float32)
    cbuf, up_c = _guarded((8 * n, 4), -7, torch.int32)
    assert lib.eprecon_upsample_async(_lib.ptr(d_feat), d_wide.stride(0), _lib.ptr(d_coords), n, c, interval, _lib.ptr(up_f),
                                      _lib.ptr(up_c), st) == 0
    assert np.array_equal(up_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32).reshape(8 * n, c))
    assert np.array_equal(up_c.cpu().numpy(), want_c.astype(np.int32))
    assert _guards_intact(fbuf, -7.0) and _guards_intact(cbuf, -7)
    # features only (the children were written by an earlier call)
    fbuf, up_f = _guarded((8 * n, c), -7.0, torch.float32)
    assert lib.eprecon_upsample_async(_lib.ptr(d_feat), d_wide.stride(0), _lib.ptr(d_coords), n, c, interval, _lib.ptr(up_f), None,
                                      st) == 0
    assert np.array_equal(up_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32).reshape(8 * n, c)) and _guards_intact(fbuf, -7.0)
    # coordinates only (the training path)
    cbuf, up_c = _guarded((8 * n, 4), -7, torch.int32)
    assert lib.eprecon_upsample_async(None, 0, _lib.ptr(d_coords), n, 0, interval, None, _lib.ptr(up_c), st) == 0
    assert np.array_equal(up_c.cpu().numpy(), want_c.astype(np.int32)) and _guards_intact(cbuf, -7)
    if n > 0:
        # refusals (nothing is launched): a row pitch below the channel count, no output at all, interval 0
        assert lib.eprecon_upsample_async(_lib.ptr(d_feat), c - 1, _lib.ptr(d_coords), n, c, interval, _lib.ptr(up_f), None, st) == -1
        assert lib.eprecon_upsample_async(None, 0, _lib.ptr(d_coords), n, 0, interval, None, None, st) == -1
        assert lib.eprecon_upsample_async(None, 0, _lib.ptr(d_coords), n, 0, 0, None, _lib.ptr(up_c), st) == -1


@pytest.mark.parametrize("n,c,interval", [(0, 7, 2), (1, 1, 1), (33, 64, 4), (32, 7, 2)])
def test_upsample_wrapper_forms(n, c, interval):
    from eprecon_amd.grid_ops import upsample
    coords, wide = _parents(n, c, 77 + n)
    feat = wide[:, 1:1 + c]
    want_f, want_c = OG.upsample(feat, coords, interval)
    d_feat, d_coords = dev(wide)[:, 1:1 + c], dev(coords)
    with torch.no_grad():
        uf, uc = upsample(d_feat, d_coords, interval)
        assert np.array_equal(uf.cpu().numpy(), want_f) and np.array_equal(uc.cpu().numpy(), want_c)
        given = uc.clone()
        uf2, uc2 = upsample(d_feat, d_coords, interval, up_coords=given)    # features only
        assert uc2 is given and torch.equal(uf2, uf) and torch.equal(given, uc)
    leaf = d_feat.clone().requires_grad_(True)                             # training: coordinates from the kernel, features by autograd
    uf3, uc3 = upsample(leaf, d_coords, interval)
    assert np.array_equal(uf3.detach().cpu().numpy(), want_f) and np.array_equal(uc3.cpu().numpy(), want_c)
    uf3.sum().backward()
    assert torch.equal(leaf.grad, torch.full_like(leaf, 8.0))


# ---------------------------------------------------------------------------------------------------------------------
# upsample2x
# ---------------------------------------------------------------------------------------------------------------------
def _interp64(x_nhwc):
    """float64 [n, h, w, c] on the host -> F.interpolate(scale_factor=2, mode="bilinear") of it, channels last"""
    import torch.nn.functional as F
    return F.interpolate(x_nhwc.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear").permute(0, 2, 3, 1).contiguous()


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


H2, W2 = [1, 2, 3, 30], [1, 2, 5, 40]


@pytest.mark.parametrize("w", W2)
@pytest.mark.parametrize("h", H2)
def test_upsample2x_against_float64(h, w, record_property):
    from eprecon_amd import _lib
    from eprecon_amd.modules import upsample2x_bilinear
    lib = _lib.load()
    worst = 0.0
    for n in (1, 9):
        for c in (4, 12, 80):
            g = torch.Generator().manual_seed(1000 * h + 10 * w + n + c)
            x = torch.randn((n, h, w, c), generator=g) * torch.rand((1, 1, 1, c), generator=g) * 4.0
            want, scale = _interp64(x.double()), _interp64(x.double().abs())
            dx = x.cuda()
            buf, out = _guarded((n, 2 * h, 2 * w, c), -7.0, torch.float32)
            assert lib.eprecon_upsample2x_nhwc_async(_lib.ptr(dx), _lib.ptr(out), n, h, w, c, _lib.current_stream()) == 0
            got = out.cpu()
            assert _guards_intact(buf, -7.0)
            r = _ratio((got.double() - want).abs(), 8 * U * scale)
            assert r <= 1.0, (n, h, w, c, r)
            worst = max(worst, r)
            # the module function takes this kernel for channels-last maps outside autograd: the same bits
            with torch.no_grad():
                y = upsample2x_bilinear(dx.permute(0, 3, 1, 2))
            assert y.shape == (n, c, 2 * h, 2 * w) and y.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(y.permute(0, 2, 3, 1).cpu(), got)
    print(f"upsample2x h={h} w={w}: max |y - y64| / (8 U S) = {worst:.3f}")
    record_property("observed_over_bound", worst)
    assert lib.eprecon_upsample2x_nhwc_async(_lib.ptr(dx), _lib.ptr(out), n, h, w, 6, _lib.current_stream()) == -1     # C % 4


def test_upsample2x_leaves_other_maps_to_the_framework():
    import torch.nn.functional as F
    from eprecon_amd.modules import upsample2x_bilinear
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        six = torch.randn((2, 6, 3, 5), generator=g).cuda().contiguous(memory_format=torch.channels_last)      # C % 4 != 0
        plain = torch.randn((2, 8, 3, 5), generator=g).cuda()                                                  # not channels-last
        for x in (six, plain):
            assert torch.equal(upsample2x_bilinear(x), F.interpolate(x, scale_factor=2, mode="bilinear"))
    grad = torch.randn((1, 4, 2, 2), generator=g).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = upsample2x_bilinear(grad)                                                                              # under autograd
    assert y.requires_grad and torch.equal(y, F.interpolate(grad, scale_factor=2, mode="bilinear"))


@pytest.mark.parametrize("w", W2)
@pytest.mark.parametrize("h", H2)
def test_affine_up2_rows_against_float64(h, w, record_property):
    from eprecon_amd import dense2d as D2
    from eprecon_amd.occupancy_initialization import Occupancy_Initialization as OI
    net = SimpleNamespace(pool4x=torch.nn.AvgPool2d(2))
    worst = 0.0
    for maps in (1, 9):
        for c in (4, 12, 80):
            g = torch.Generator().manual_seed(2000 * h + 10 * w + maps + c)
            x = torch.randn((maps, h, w, c), generator=g) * 3.0
            grid = D2.PixelGrid.get(maps, h, w, torch.device("cuda:0"))
            framed = torch.full((grid.n, c + 3), float("nan")).cuda()[:, 1:1 + c]              # a column slice, NaN around it
            framed.copy_(x.reshape(grid.n, c))
            for affine, rows, off in (("identity", x.reshape(grid.n, c).cuda(), 4), ("identity", framed, 1), ("bn", framed, 4),
                                      ("bn_relu", x.reshape(grid.n, c).cuda(), 4), ("bn_relu", framed, 1)):
                if affine == "identity":
                    scale, shift, relu = torch.ones(c), torch.zeros(c), False
                else:
                    scale, shift, relu = 0.5 + torch.rand(c, generator=g), torch.randn(c, generator=g), affine == "bn_relu"
                y = x.double() * scale.double() + shift.double()
                A = _interp64((x.double() * scale.double()).abs() + shift.double().abs())
                if relu:
                    y = y.clamp_min(0.0)
                want, S = _interp64(y), _interp64(y.abs())
                bound = 8 * U * S if affine == "identity" else U * A + 8 * U * (S + U * A)
                dst = torch.full((maps * 4 * h * w, c + 8), -3.0, device="cuda")
                with torch.no_grad():
                    OI._join(net, D2.Act(rows, scale.cuda(), shift.cuda(), relu), grid, dst[:, off:off + c], False)
                got = dst.cpu()
                assert bool((got[:, :off] == -3.0).all()) and bool((got[:, off + c:] == -3.0).all())     # the columns around the slice
                r = _ratio((got[:, off:off + c].double() - want.reshape(-1, c)).abs(), bound.reshape(-1, c))
                assert r <= 1.0, (maps, h, w, c, affine, r)
                worst = max(worst, r)
    print(f"affine_up2_rows h={h} w={w}: max error / bound = {worst:.3f}")
    record_property("observed_over_bound", worst)


# ---------------------------------------------------------------------------------------------------------------------
# sparsify
# ---------------------------------------------------------------------------------------------------------------------
THR = float(np.float32(0.3))


def _sparsify_inputs(n, c_all, bs, seed, stray=False):
    """occ and tsdf as columns of wider tensors, features as a column slice, batch indices unsorted"""
    g = torch.Generator().manual_seed(seed)
    wide_o = torch.randn((n, 3), generator=g)
    wide_t = torch.randn((n, 2), generator=g)
    wide_f = torch.randn((n, c_all + 3), generator=g)
    coords = torch.randint(0, 96, (n, 4), generator=g, dtype=torch.int32)
    coords[:, 0] = torch.randint(-1 if stray else 0, bs + 1 if stray else bs, (n,), generator=g, dtype=torch.int32)
    target = torch.rand((n, 1), generator=g) > 0.3
    return wide_o.cuda()[:, 1:2], wide_t.cuda()[:, 1:2], wide_f.cuda()[:, 2:2 + c_all], coords.cuda(), target.cuda()


def _check_sparsify(occ, tsdf, feat_all, coords, target, c_feat, bs, thr=THR):
    from eprecon_amd import grid_ops as GO
    assert occ.stride(0) > 1 and tsdf.stride(0) > 1 and feat_all.stride(0) > feat_all.shape[1]
    host, pc, pt, po, ka, pf = GO.sparsify(occ, thr, target, coords, tsdf, feat_all, c_feat, bs)
    occupancy = occ.squeeze(1) > thr
    keep = torch.nonzero(occupancy).squeeze(1)
    assert host[0] == keep.numel()
    tgt = target.reshape(-1) if target is not None else torch.ones_like(occupancy)
    for b in range(bs):
        rows = coords[:, 0] == b
        assert host[1 + b] == int((occupancy & rows).sum()), b
        assert host[1 + bs + b] == int((occupancy & tgt & rows).sum()), b
    assert len(host) == 1 + 2 * bs
    assert torch.equal(pc, coords.index_select(0, keep))
    assert torch.equal(pt, tsdf.index_select(0, keep)) and torch.equal(po, occ.index_select(0, keep))
    kept = feat_all.index_select(0, keep)
    assert torch.equal(ka, kept)
    assert pf.shape == (keep.numel(), c_feat + 2) and torch.equal(pf, torch.cat([kept[:, :c_feat], pt, po], dim=1))
    return host, keep


@pytest.mark.parametrize("c_feat", [0, 1])
@pytest.mark.parametrize("n", [256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1])
def test_sparsify_at_the_pass_boundary_of_the_scan(n, c_feat):
    occ, tsdf, feat, coords, target = _sparsify_inputs(n, 1, 2, n + c_feat)
    host, keep = _check_sparsify(occ, tsdf, feat, coords, target, c_feat, 2)
    assert 0.3 * n < host[0] < 0.5 * n
    pitched = lambda col: torch.cat([col, col], 1)[:, 1:2]
    last = torch.full((n, 1), -1.0, device="cuda")          # only the last row kept: every tile offset in front of it is 0
    last[-1] = 1.0
    host, keep = _check_sparsify(pitched(last), tsdf, feat, coords, None, c_feat, 2)
    assert host[0] == 1 and keep.tolist() == [n - 1]
    host, keep = _check_sparsify(pitched(torch.ones((n, 1), device="cuda")), tsdf, feat, coords, target, c_feat, 2)      # every row
    assert host[0] == n


@pytest.mark.parametrize("c_all", [63, 64, 65])
def test_sparsify_channel_counts_around_a_wave(c_all):
    for c_feat in (0, c_all):
        occ, tsdf, feat, coords, target = _sparsify_inputs(1000, c_all, 3, c_all + c_feat)
        _check_sparsify(occ, tsdf, feat, coords, target, c_feat, 3)
        _check_sparsify(occ, tsdf, feat, coords, None, c_feat, 3)


def test_sparsify_threshold_and_non_finite_occupancy():
    n = 700
    occ, tsdf, feat, coords, target = _sparsify_inputs(n, 5, 2, 9)
    thr = np.float32(THR)
    special = np.array([thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), np.nan, -np.inf, np.inf, -thr, 0.0],
                       np.float32)
    kept_by_hand = np.array([False, True, False, False, False, True, False, False])        # > thr is strict; NaN compares false
    idx = torch.arange(n, device="cuda") % len(special)
    occ.copy_(torch.from_numpy(special).cuda()[idx].reshape(n, 1))
    host, keep = _check_sparsify(occ, tsdf, feat, coords, target, 3, 2)
    assert torch.equal(keep, torch.nonzero(torch.from_numpy(kept_by_hand).cuda()[idx]).squeeze(1))
    assert host[0] == int(kept_by_hand[np.arange(n) % len(special)].sum()) > 0


def test_sparsify_batch_limit_and_rows_of_no_element():
    from eprecon_amd import _lib
    from eprecon_amd import grid_ops as GO
    n = 5000
    occ, tsdf, feat, coords, target = _sparsify_inputs(n, 9, 32, 3)
    host, keep = _check_sparsify(occ, tsdf, feat, coords, target, 4, 32)
    assert all(host[1 + b] > 0 and host[1 + 32 + b] > 0 for b in range(32))                 # rows in every element
    with pytest.raises(_lib.EpreconError):
        GO.sparsify(occ, THR, target, coords, tsdf, feat, 4, 33)
    with pytest.raises(_lib.EpreconError):
        GO.sparsify(occ, THR, target, coords, tsdf, feat, 4, 0)
    # rows with the batch index -1 or `batch`: kept and compacted, in no per-batch count
    occ, tsdf, feat, coords, target = _sparsify_inputs(n, 9, 3, 4, stray=True)
    stray = (coords[:, 0] < 0) | (coords[:, 0] >= 3)
    host, keep = _check_sparsify(occ, tsdf, feat, coords, target, 4, 3)
    n_stray = int((stray & (occ.squeeze(1) > THR)).sum())
    assert n_stray > 100 and sum(host[1:4]) == host[0] - n_stray

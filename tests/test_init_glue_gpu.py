"""GPU: the glue launches of the occupancy-initialisation branch that EPRECON_INIT_GLUE folds away ("Switches")
give the bits of the launches they replace.  Every test runs the default path and the path under EPRECON_INIT_GLUE=0 on the same
inputs and compares byte for byte.

  rank        the rank volume the back-projection of a dense raster writes against eprecon_grid_rank_async on its rows
  count       the variance call as count half (on a side stream) + gather half against the one-call form
  joins       the outer levels of the 2D stack onto the 1/8 grid (BatchNorm -> 2x2 mean / bilinear x2 -> concat slice) in one
              launch against the three launches
  norm4       the C <= 4 BatchNorm from producer-side summaries in one launch against finalize + apply
  selection   the stage-0 selection through the rank volume against the list form (clear + mark over the list)
  forward     a whole Cfg2Step (Occupancy_Initialization.forward + selection) on a 24^3 volume with 64x48 images, with and
              without the HIP graph of the 2D stack (the graphed one compared on its second replay)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------
# rank volume from the back-projection
# ------------------------------------------------------------------------------------------------
RANK_VIEWS = 3


def _raster_scene(dims, c):
    """the interval-2 raster of `dims` cells in front of three pinhole cameras (17 x 9 maps) placed so that the block leaves
    the frusta on two sides: cells seen by 0, 1, 2 and 3 views"""
    h, w = 9, 17
    kr = np.zeros((RANK_VIEWS, 1, 4, 4), np.float32)
    for v, (tx, ty, f) in enumerate([(0.0, 0.0, 8.0), (0.75, 0.0, 8.0), (0.0, -0.5, 4.0)]):
        k = np.array([[f, 0, (w - 1) / 2, 0], [0, f, (h - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        m = np.eye(4)
        m[:3, 3] = (tx, ty, 0.0)
        kr[v, 0] = (k @ m).astype(np.float32)
    gx, gy, gz = np.meshgrid(*[2 * np.arange(d) for d in dims], indexing="ij")
    coords = np.stack([np.zeros(gx.size, np.int64), gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.int32)
    feats = np.random.default_rng(7 + c).standard_normal((RANK_VIEWS, 1, c, h, w), dtype=np.float32)
    return dict(coords=np.ascontiguousarray(coords), origin=np.array([[-1.25, -0.75, 0.5]], np.float32), voxel_size=0.125,
                feats=feats, kr=kr)


def _grid_rank(coords, dims):
    """eprecon_grid_rank_async on compacted rows -> the volume with its trailing word"""
    from eprecon_amd import sparse as SP
    return SP.DenseMap(SP.VoxelSet(coords, 2, dims=dims), dims).rank


@pytest.mark.parametrize("dims", [(6, 5, 7), (8, 8, 8)])
def test_rank_volume_from_the_gather_is_grid_rank_of_its_rows(dims):
    import back_project_ref as R
    from eprecon_amd import back_project as BP
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    for c in (8, 3):                                    # C % 4 == 0: bp_gather_mlp_kernel; else bp_gather_kernel
        sc = _raster_scene(dims, c)
        seen = R.geometry_of(sc).vis.sum(axis=0)
        assert (seen >= 2).any() and (seen < 2).any()       # min_view = 2 keeps some cells and drops some
        coords = BP.mark_dense(t(sc["coords"]), dims, 2)
        nchw = t(sc["feats"])
        nhwc = nchw.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        for mode in (BP.MODE_VARIANCE, BP.MODE_MEAN):
            for feats in (nchw, nhwc):
                for min_view in (2, 0, RANK_VIEWS + 1):     # some cells, every cell, no cell
                    rank = BP.dense_rank_buffer(coords, dims, 2)
                    assert rank is not None
                    rank.fill_(-7)
                    res = BP.run(coords, t(sc["origin"]), sc["voxel_size"], feats, t(sc["kr"]), min_view, mode,
                                 min_valid_per_batch=0, rank_out=rank)
                    want = _grid_rank(res["coords"], dims)
                    assert torch.equal(rank, want), (c, mode, min_view)
                    assert int(rank[-1]) == 0
                    nv = {2: int((seen >= 2).sum()), 0: seen.size, RANK_VIEWS + 1: 0}[min_view]
                    if min_view != 2:       # (at 2 a cell within rounding of a frustum face may fall either way)
                        assert res["n_valid"] == nv
                    assert int((rank[:-1] >= 0).sum()) == res["n_valid"]
                    # the rows themselves are what a call without the rank volume returns
                    ref = BP.run(coords, t(sc["origin"]), sc["voxel_size"], feats, t(sc["kr"]), min_view, mode, min_valid_per_batch=0)
                    assert torch.equal(res["coords"], ref["coords"]) and np.array_equal(_bits(res["feats"]), _bits(ref["feats"]))


def test_rank_volume_is_for_tagged_rasters_only(monkeypatch):
    from eprecon_amd import back_project as BP
    dims = (6, 5, 7)
    sc = _raster_scene(dims, 8)
    coords = torch.from_numpy(sc["coords"]).to(_dev())
    assert BP.dense_rank_buffer(coords, dims, 2) is None                                    # no tag
    assert BP.dense_rank_buffer(BP.mark_dense(coords.clone(), dims, 2), (6, 5, 8), 2) is None      # another grid
    assert BP.dense_rank_buffer(BP.mark_dense(coords.clone(), dims, 2), dims, 1) is None           # another spacing
    assert BP.dense_rank_buffer(BP.mark_dense(coords[:-1].clone(), dims, 2), dims, 2) is None      # not the whole raster
    monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
    assert BP.dense_rank_buffer(BP.mark_dense(coords.clone(), dims, 2), dims, 2) is None           # switched off
    monkeypatch.delenv("EPRECON_INIT_GLUE")
    # the setter is one-shot: the call after the armed one writes nothing
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    tagged = BP.mark_dense(coords.clone(), dims, 2)
    rank = BP.dense_rank_buffer(tagged, dims, 2)
    args = (t(sc["origin"]), sc["voxel_size"], t(sc["feats"]), t(sc["kr"]), 2, BP.MODE_MEAN)
    BP.run(tagged, *args, rank_out=rank)
    keep = rank.clone()
    rank.fill_(-7)
    BP.run(tagged, *args)
    assert bool((rank == -7).all()) and bool((keep[:-1] >= -1).all())


# ------------------------------------------------------------------------------------------------
# count half beside the maps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vox,interval", [(32, 2), (96, 2)])     # 4,096 rows: 16-voxel tiles; 110,592 rows: 64-voxel tiles
def test_count_half_on_a_side_stream_then_gather_is_the_one_call_form(n_vox, interval):
    from eprecon_amd import _lib
    from eprecon_amd import back_project as BP
    from eprecon_amd import synthetic as S
    w = S.make_window(seed=2, width=320, height=240, n_vox=(n_vox,) * 3)
    _, h, wd = S.pyramid_shapes(240, 320)[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    feats = t(S.make_features(11, 9, (32, h, wd))).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)     # channels-last
    dims = (n_vox // interval,) * 3
    coords = BP.mark_dense(t(S.dense_coords((n_vox,) * 3, interval)), dims, interval)
    origin, kr = t(w["vol_origin_partial"][None]), t(w["proj_matrices"][:, 1][:, None])
    want = BP.run_async(coords, origin, w["voxel_size"], feats, kr, 2, BP.MODE_VARIANCE).result()
    side = _lib.side_stream(_dev(), _lib.SIDE_SETUP)
    for stream in (None, side):
        rank = BP.dense_rank_buffer(coords, dims, interval)
        counted = BP.count_async(coords, origin, w["voxel_size"], tuple(feats.shape), kr, 2, BP.MODE_VARIANCE, stream=stream)
        got = BP.run_async(coords, origin, w["voxel_size"], feats, kr, 2, BP.MODE_VARIANCE, counted=counted, rank_out=rank).result()
        assert got["n_valid"] == want["n_valid"] > 0 and got["n_valid_per_batch"] == want["n_valid_per_batch"]
        for k in ("feats", "count"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        assert torch.equal(got["coords"], want["coords"])
        assert torch.equal(rank, _grid_rank(got["coords"], dims))


# ------------------------------------------------------------------------------------------------
# joins of the 2D stack
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [12, 24, 80])
@pytest.mark.parametrize("h,w", [(4, 6), (6, 10), (5, 7)])      # (odd sizes: the 2x2 mean drops a row and a column)
@pytest.mark.parametrize("maps", [1, 2])
def test_joins_in_one_launch_have_the_bits_of_the_three_launches(maps, h, w, c, monkeypatch):
    from types import SimpleNamespace
    from eprecon_amd import dense2d as D2
    from eprecon_amd.occupancy_initialization import Occupancy_Initialization as OI
    net = SimpleNamespace(pool4x=torch.nn.AvgPool2d(2))        # (all of the module that _join reads)
    g = torch.Generator().manual_seed(maps * 1000 + h * 10 + c)
    grid = D2.PixelGrid.get(maps, h, w, _dev())
    x = torch.randn((grid.n, c), generator=g).to(_dev())
    scale = (0.5 + torch.rand(c, generator=g)).to(_dev())
    shift = torch.randn(c, generator=g).to(_dev())
    with torch.no_grad():
        for pool in (True, False):
            n_out = maps * (h // 2) * (w // 2) if pool else maps * 4 * h * w
            for relu in (False, True):
                for off in (4, 1):          # a 16-byte aligned slice of a wider buffer, and one that is not
                    got, want = (torch.full((n_out, c + 8), -3.0, device=_dev()) for _ in range(2))
                    monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
                    OI._join(net, D2.Act(x, scale, shift, relu), grid, want[:, off:off + c], pool)
                    monkeypatch.delenv("EPRECON_INIT_GLUE")
                    OI._join(net, D2.Act(x, scale, shift, relu), grid, got[:, off:off + c], pool)
                    assert np.array_equal(_bits(got), _bits(want)), (pool, relu, off)       # (the columns around the slice too)
                    assert bool((got[:, off:off + c] != -3.0).any())


# ------------------------------------------------------------------------------------------------
# norm4
# ------------------------------------------------------------------------------------------------
def _summaries(nblk, c, ld, seed):
    """(count, mean, M2) rows as a convolution leaves them (counts up to 128, some rows empty), channel-major with row stride
    ld > nblk and NaN in the padding -> the logical [nblk, 3, c] view"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 129, size=(nblk, c)).astype(np.float32)
    n[rng.random((nblk, c)) < 0.05] = 0.0
    mean = np.where(n > 0, rng.normal(0.0, 2.0, size=(nblk, c)), 0.0).astype(np.float32)
    m2 = np.where(n > 0, n * rng.random((nblk, c)), 0.0).astype(np.float32)
    p = torch.full((3, c, ld), float("nan"), dtype=torch.float32, device=_dev())[:, :, :nblk].permute(2, 0, 1)
    p.copy_(torch.from_numpy(np.stack([n, mean, m2], axis=1)))
    return p


@pytest.mark.parametrize("nblk", [1, 255, 256, 257, 864])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_norm4_one_launch_has_the_bits_of_finalize_and_apply(nblk, c, monkeypatch):
    from eprecon_amd import sparse as SP
    g = torch.Generator().manual_seed(17 * nblk + c)
    rows = 128 * nblk - 37 if nblk > 1 else 91        # (more than one grid stride of the 256 workgroups at nblk = 864)
    # x and the residual are column slices of wider buffers: row strides above C
    x = (torch.randn((rows, c + 2), generator=g) * 3.0).to(_dev())[:, 1:1 + c]
    res = torch.randn((rows, c + 1), generator=g).to(_dev())[:, :c]
    gamma = (0.5 + torch.rand(c, generator=g)).to(_dev())
    beta = (torch.rand(c, generator=g) - 0.5).to(_dev())
    partial = _summaries(nblk, c, nblk + 13, seed=1000 * nblk + c)
    for residual, relu in ((None, False), (None, True), (res, False), (res, True)):
        monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
        want = SP.batchnorm_apply_partials(x, partial, gamma, beta, EPS, residual, relu)
        monkeypatch.delenv("EPRECON_INIT_GLUE")
        got = SP.batchnorm_apply_partials(x, partial, gamma, beta, EPS, residual, relu)
        assert np.array_equal(_bits(got), _bits(want)), (nblk, c, residual is not None, relu)
        # in place, as the logit layer calls it (out = x)
        xi = x.clone()
        SP.batchnorm_apply_partials(xi, partial, gamma, beta, EPS, residual, relu, out=xi)
        assert np.array_equal(_bits(xi), _bits(want)), (nblk, c, "in place")


def test_norm4_without_affine_parameters(monkeypatch):
    from eprecon_amd import sparse as SP
    x = torch.randn((5000, 1), generator=torch.Generator().manual_seed(3)).to(_dev())
    partial = _summaries(40, 1, 41, seed=5)
    monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
    want = SP.batchnorm_apply_partials(x, partial)
    monkeypatch.delenv("EPRECON_INIT_GLUE")
    assert np.array_equal(_bits(SP.batchnorm_apply_partials(x, partial)), _bits(want))


# ------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------
THRESHOLD = 0.3


def _logit_at_threshold():
    """the float32 logits within 8 ulps of logit(THRESHOLD): their sigmoids, as init_mark_kernel computes them, lie on both
    sides of the comparison's edge"""
    x = np.float32(np.log(THRESHOLD / (1.0 - THRESHOLD)))
    return (x.view(np.int32) + np.arange(-8, 9, dtype=np.int32)).view(np.float32)


def _voxel_set(dims, keep):
    """the voxels of the interval-2 raster of `dims` cells for which keep is set, in raster order -> VoxelSet with its DenseMap"""
    from eprecon_amd import sparse as SP
    gx, gy, gz = dims
    cells = np.stack(np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij"), -1).reshape(-1, 3)
    coords = np.concatenate([np.zeros((cells.shape[0], 1), np.int64), 2 * cells], 1).astype(np.int32)[keep.reshape(-1)]
    vset = SP.VoxelSet(torch.from_numpy(coords).to(_dev()), 2, dims=dims)
    return vset, SP.DenseMap(vset, dims)


def _both_selections(logit, vset, dense, dim, monkeypatch):
    from eprecon_amd import grid_ops as GO
    monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
    want = GO.init_select(logit, vset.coords, 1, dim=dim, cell=4, threshold=THRESHOLD, dense=dense)
    monkeypatch.delenv("EPRECON_INIT_GLUE")
    listed = GO.init_select(logit, vset.coords, 1, dim=dim, cell=4, threshold=THRESHOLD)
    got = GO.init_select(logit, vset.coords, 1, dim=dim, cell=4, threshold=THRESHOLD, dense=dense)
    for other in (listed, got):
        assert torch.equal(other[0], want[0]) and list(other[1]) == list(want[1])
    return got


@pytest.mark.parametrize("dims,dim", [((8, 8, 8), 4), ((12, 8, 8), 6)])
def test_dense_selection_equals_the_list_form(dims, dim, monkeypatch):
    rng = np.random.default_rng(dims[0])
    cells = dims[0] * dims[1] * dims[2]
    edge = _logit_at_threshold()
    for name in ("random", "holes", "edge", "none", "all"):
        keep = np.ones(cells, bool) if name != "holes" else rng.random(cells) < 0.6      # holes in the rank volume
        vset, dense = _voxel_set(dims, keep)
        n = vset.n
        if name in ("random", "holes"):
            # blobs, so that something survives the erosion
            d = np.linalg.norm(vset.coords.cpu().numpy()[:, 1:] / 2.0 - (np.array(dims) - 1.0) / 2.0, axis=1)
            logit = (2.0 - d + rng.normal(0.0, 0.5, n)).astype(np.float32)
        elif name == "edge":
            logit = edge[rng.integers(0, edge.shape[0], n)]       # every logit at the comparison's edge, on either side
        else:
            logit = np.full(n, -4.0 if name == "none" else 4.0, np.float32)
        sel, counts = _both_selections(torch.from_numpy(logit).to(_dev()).reshape(-1, 1), vset, dense, dim, monkeypatch)
        assert counts[0] == sel.shape[0]
        if name == "none":
            assert sel.shape[0] == 0
        if name == "all":
            assert sel.shape[0] > 0


def test_edge_logits_fall_on_both_sides():
    """the logits of the `edge` case are on both sides of init_mark_kernel's comparison (float32 sigmoid > threshold)"""
    x = _logit_at_threshold()
    sig = np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))
    hits = sig > np.float32(THRESHOLD)
    assert hits.any() and not hits.all()


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def _same_step(a, b):
    assert torch.equal(a["stage0_coords"], b["stage0_coords"])
    assert len(a["init"]) == len(b["init"]) == 3        # occupancy logit, coordinates, view count
    for x, y in zip(a["init"], b["init"]):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("graph", [False, True])
def test_forward_and_selection_on_a_small_volume(graph, monkeypatch):
    from eprecon_amd import occupancy_initialization as OI
    from eprecon_amd import sparse as SP
    from eprecon_amd.fragment_step import Cfg2Step
    # 12^3 cells of which ~340 are seen by two of the nine 64x48 views: below the guard of the reference's volume (1000 valid
    # voxels) and below the fill at which a set takes the dense-grid path, so both constants are lowered for this volume
    monkeypatch.setattr(OI, "INIT_MIN_VALID", 100)
    monkeypatch.setattr(SP, "DENSE_MIN_FILL", 0.1)
    step = Cfg2Step(seed=0, height=48, width=64, n_vox=(24, 24, 24))
    step.init_net.use_hip_graph = graph
    monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
    want = dict(step.run())
    assert want["init"] is not None and want["init"][0].shape[0] >= 100
    monkeypatch.delenv("EPRECON_INIT_GLUE")
    step.run()
    got = step.run()                       # (graphed: the second replay under the default path)
    assert step.init_net.dense_map is not None          # the selection went through the rank volume
    _same_step(got, want)

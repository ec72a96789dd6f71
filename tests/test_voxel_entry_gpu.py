"""GPU: every route that publishes a voxelisation (torchsparse_utils._VoxEntry) leaves a COMPLETE entry under the points tensor:
_voxelize_points at one and at three levels, SpvcnnPrefetch.finish, register_voxelization and register_voxelization_pair.
A hit costs no blocking read; an SPVCNN entry hands the native pass its 15 geometry tensors and initial_voxelize the same
storage; the ConvGRU pair is found complete in both LITERAL_CONVR modes.  Tables are NOT compared across routes (the hash-probe
and the map-based trilinear kernels are pinned to each other at 1e-6 only: test_corner_tables_native_pass owns that).

The scene: 595 points in 179 voxels (32 at stride 2, 12 at stride 4: pairwise different, a swapped table shows in its shape),
negative coordinates on every axis, one voxel that holds 125 points."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RES = 0.2
VOXEL_SIZE = 0.04
ROUTES = ["points1", "points3", "prefetch", "register", "pair"]
GEOMETRY = ["offsets1", "order1", "offsets4", "order4", "k1", "k2", "k4", "down12", "up21", "down24", "up42",
            "idx8_1", "weight8_1", "idx8_4", "weight8_4"]
_SCENE = {}


def scene():
    """(coords int32[N,4], origin f32[1,3], world_to_aligned_camera f32[1,4,4]) on the device; a 5x5x5 block of source voxels
    that falls into ONE voxel at RES plus 470 scattered ones, shuffled"""
    if not _SCENE:
        rng = np.random.default_rng(7)
        block = np.stack(np.meshgrid(np.arange(10, 15), np.arange(21, 26), np.arange(3, 8), indexing="ij"), -1).reshape(-1, 3)
        cells = rng.choice(32 * 32 * 18, 475, replace=False)
        scattered = np.stack([cells // (32 * 18), cells // 18 % 32, cells % 18], 1)
        xyz = np.unique(np.concatenate([block, scattered]), axis=0)
        xyz = xyz[rng.permutation(len(xyz))]
        coords = np.concatenate([np.zeros((len(xyz), 1)), xyz], 1).astype(np.int32)
        w2ac = np.eye(4, dtype=np.float32)[None].copy()
        w2ac[0, :3, 3] = [0.013, -0.021, 0.007]
        _SCENE.update(coords=torch.from_numpy(coords).cuda(), origin=torch.tensor([[-1.01, -0.59, -0.31]], device="cuda"),
                      w2ac=torch.from_numpy(w2ac).cuda())
    return _SCENE["coords"], _SCENE["origin"], _SCENE["w2ac"]


def points():
    """a fresh tensor of the scene's aligned-camera points"""
    from eprecon_amd import torchsparse_utils as TU
    coords, origin, w2ac = scene()
    return TU.aligned_camera_coords(coords, origin, VOXEL_SIZE, w2ac)


def pair_parts(pts):
    """first / second = (scaled, vox, inverse, uniq, grid) of `pts` and of the once-scaled points, as the GRU-fusion stage call
    hands them over; the cache is left empty"""
    from eprecon_amd import torchsparse_utils as TU
    e1 = TU._voxelize_points(pts, RES)
    e2 = TU._voxelize_points(e1.scaled, RES)
    TU.clear_voxelization_cache()
    return tuple((e.scaled, e.vox, e.inverse, e.vset.coords, e.vset.grid) for e in (e1, e2))


def publish(route):
    """-> (points tensor, the entry the route published under it)"""
    from eprecon_amd import _lib
    from eprecon_amd import torchsparse_utils as TU
    TU.clear_voxelization_cache()
    if route == "prefetch":
        coords, origin, w2ac = scene()
        n = coords.shape[0]
        pf = TU.SpvcnnPrefetch(coords, torch.tensor([n], dtype=torch.int32, device="cuda"), False, 1, origin, VOXEL_SIZE, w2ac, RES)
        up, pts = pf.finish(n, _lib.read_counts(pf.headers()))
        assert up is None and pts.shape == (n, 4)
        (e,) = TU.VOXELIZATIONS.values()
        return pts, e
    pts = points()
    if route == "points1":
        return pts, TU._voxelize_points(pts, RES, levels=1)
    if route == "points3":
        return pts, TU._voxelize_points(pts, RES, levels=3)
    first, second = pair_parts(pts)
    if route == "register":
        return pts, TU.register_voxelization(pts, RES, *first)
    return pts, TU.register_voxelization_pair(pts, RES, first, second)[0]


def strided_sizes(vox):
    """the number of distinct voxels of int32[N,4] (b,x,y,z) rows at tensor strides 1, 2, 4"""
    v = vox.cpu().numpy()
    return [len(np.unique(np.concatenate([v[:, :1], v[:, 1:] // s], 1), axis=0)) for s in (1, 2, 4)]


@pytest.mark.parametrize("route", ROUTES)
def test_every_route_publishes_a_complete_entry(route):
    from eprecon_amd import _lib
    from eprecon_amd import sparse as SP
    from eprecon_amd import torchsparse_utils as TU
    pts, e = publish(route)
    n = pts.shape[0]
    for name in type(e).__slots__:                      # every field is set, whoever published the entry
        getattr(e, name)
    assert e.pts is pts and e.scaled.shape == (n, 4) and e.vox.shape == (n, 4) and e.inverse.shape == (n,)
    n1, n2, n4 = strided_sizes(e.vox)
    assert len({n1, n2, n4}) == 3 and n1 < n                                          # the scene is what the docstring says
    assert (e.vox[:, 1:] < 0).any(0).all() and int(torch.bincount(e.inverse.long()).max()) > 64
    assert e.vset.n == n1 and e.vset.stride == 1
    offsets, order = e.lists
    assert offsets.shape == (n1 + 1,) and order.shape == (n,)
    assert (e.idx8 is None) == (e.w8 is None) and (e.idx8 is None or (e.idx8.shape == (n, 8) and e.w8.shape == (n, 8)))
    assert e._stale == {} and (e.tables is None) == (route not in ("points3", "prefetch"))
    if route == "pair":
        assert e.vset.built_kernel_map().shape == (27, n1) and e.idx8 is not None
    # a hit: the same entry object, at no blocking read, for every levels argument
    reads = _lib.HOST_READS
    assert TU._voxelize_points(pts, RES) is e and TU._voxelize_points(pts, RES, levels=3) is e
    assert _lib.HOST_READS == reads
    # a producer's kernel map is the set's kernel map: nothing is launched, nothing else is there yet
    nbr = torch.empty((27, n1), dtype=torch.int32, device="cuda")
    vs = SP.VoxelSet(e.vset.coords, kernel_map=nbr)
    assert vs.built_kernel_map() is nbr and vs.kernel_map(3) is nbr and vs.built_downsample() is None
    assert SP.VoxelSet(e.vset.coords).built_kernel_map() is None


@pytest.mark.parametrize("route", ["points3", "prefetch"])
def test_spvcnn_entry_hands_out_its_geometry(route):
    from eprecon_amd import torchsparse_utils as TU
    from eprecon_amd.tensor import PointTensor
    pts, e = publish(route)
    n = pts.shape[0]
    n1, n2, n4 = strided_sizes(e.vox)
    g = e.spvcnn_geometry()
    assert sorted(g) == sorted(GEOMETRY)
    shapes = {"offsets1": (n1 + 1,), "order1": (n,), "offsets4": (n4 + 1,), "order4": (n,), "k1": (27, n1), "k2": (27, n2),
              "k4": (27, n4), "down12": (8, n2), "up21": (8, n1), "down24": (8, n4), "up42": (8, n2), "idx8_1": (n, 8),
              "weight8_1": (n, 8), "idx8_4": (n, 8), "weight8_4": (n, 8)}
    for name in GEOMETRY:
        assert g[name].is_cuda and tuple(g[name].shape) == shapes[name], name
        assert g[name].dtype == (torch.float32 if name.startswith("weight") else torch.int32), name
    # the same tensors the voxel sets answer with, launching nothing
    s1 = e.vset
    s2, down12, up21 = s1.built_downsample()
    s4, down24, up42 = s2.built_downsample()
    assert (s1.n, s2.n, s4.n) == (n1, n2, n4) and (s2.stride, s4.stride) == (2, 4) and s4.built_downsample() is None
    assert g["k1"] is s1.built_kernel_map() and g["k2"] is s2.built_kernel_map() and g["k4"] is s4.built_kernel_map()
    assert g["down12"] is down12 and g["up21"] is up21 and g["down24"] is down24 and g["up42"] is up42
    assert e.lists[0] is g["offsets1"] and e.lists[1] is g["order1"] and e.idx8 is g["idx8_1"] and e.w8 is g["weight8_1"]
    # initial_voxelize fills the PointTensor's tables at strides 1 and 4 from the same storage
    z = PointTensor(torch.randn((n, 8), device="cuda"), pts)
    with torch.no_grad():
        x = TU.initial_voxelize(z, 1, RES, levels=3)
    assert x.vset is s1 and z._vox_entry is e and x.F.shape == (n1, 8)
    same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape
    assert same(z.idx_query[1], g["idx8_1"]) and same(z.weights[1], g["weight8_1"])
    assert same(z.idx_query[4], g["idx8_4"]) and same(z.weights[4], g["weight8_4"])
    lists = z.additional_features["lists"]
    assert same(lists[1][0], g["offsets1"]) and same(lists[1][1], g["order1"])
    assert same(lists[4][0], g["offsets4"]) and same(lists[4][1], g["order4"])
    assert same(z.additional_features["idx_query"][1], e.inverse) and same(z.additional_features["idx_query"][4], e.tables["idx4"])


@pytest.mark.parametrize("route", ["points1", "register", "pair"])
def test_convgru_entries_have_no_spvcnn_geometry(route):
    _, e = publish(route)
    assert e.spvcnn_geometry() is None


@pytest.mark.parametrize("literal", [True, False])
def test_registered_pair_is_found_complete(literal, monkeypatch):
    """after register_voxelization_pair, prepare_convgru_voxelizations only finds: the same two entries, no blocking read"""
    from eprecon_amd import _lib
    from eprecon_amd import torchsparse_utils as TU
    monkeypatch.setattr(TU, "LITERAL_CONVR", literal)
    TU.clear_voxelization_cache()
    pts = points()
    first, second = pair_parts(pts)
    e1, e2 = TU.register_voxelization_pair(pts, RES, first, second)
    for e in (e1, e2):
        for name in type(e).__slots__:
            getattr(e, name)
    maps = (e1.vset.built_kernel_map(), e2.vset.built_kernel_map())
    assert maps[0].shape == (27, e1.vset.n) and maps[1].shape == (27, e2.vset.n) and e2.pts is e1.scaled
    reads = _lib.HOST_READS
    found = TU.prepare_convgru_voxelizations(pts, 1, RES)
    assert _lib.HOST_READS == reads
    assert found[0] is e1 and found[1] is e2
    assert e1.vset.kernel_map(3) is maps[0] and e2.vset.kernel_map(3) is maps[1]
    n = pts.shape[0]
    assert e1.idx8.shape == (n, 8) and e1.w8.shape == (n, 8)
    if literal:
        idx2, w2 = e2.stale_from(e1)
        assert idx2.shape == (n, 8) and w2 is e1.w8 and e2.idx8 is None
        assert all(t.shape == (e.vset.n,) for e in (e1, e2) for t in e.sphash_order())
    else:
        assert e2.idx8.shape == (n, 8) and e2.w8.shape == (n, 8) and e2._stale == {}
    assert _lib.HOST_READS == reads
    torch.cuda.synchronize()

"""GPU: eprecon_amd.distance_field (csrc/distance_field.hip) against the brute force of tests/distance_field_ref.py.  dist2, site
and state must be EQUAL to it: the rule is integer arithmetic and there are no tolerances.  Scenes of tests/raycast_fixtures.py
with their rows in a seeded shuffled order (so that "smallest row" is not "smallest coordinate"), box extents around the lane
width and the tile of the passes, radii around the cut, ties, boundary rows, empty input, split boxes, two runs, the derived
outputs, the errors, the file and the command line."""
import ctypes
import functools
import os
import struct
import zlib

import numpy as np
import pytest

import distance_field_ref as D
import raycast_fixtures as FX

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FAR = D.FAR
VOXEL = FX.VOXEL
SCENES = ("sphere", "sphere_shifted", "slab_box")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def metres(radius):
    """a max_distance whose floor(max_distance / voxel) is `radius` whatever the rounding of the quotient"""
    return None if radius is None else (radius + 0.25) * VOXEL


@functools.lru_cache(None)
def shuffled(scene):
    s = FX.SCENES[scene]()
    order = np.random.default_rng(11).permutation(len(s["coords"]))
    return {"coords": s["coords"][order], "tsdf": s["tsdf"][order], "semantic": s["semantic"][order], "instance": s["instance"][order],
            "origin": s["origin"], "voxel_size": s["voxel_size"], "lo": tuple(int(v) - 8 for v in s["coords"].min(0)),
            "hi": tuple(int(v) + 9 for v in s["coords"].max(0))}


@functools.lru_cache(None)
def scene_reference(scene):
    """the unbounded answer over the scene's box (its rows' box and 8 cells around it: about 40^3), computed once"""
    s = shuffled(scene)
    out = D.distance_field(s["coords"], s["tsdf"], s["lo"], s["hi"])
    for a in out:
        a.setflags(write=False)
    return out


def cut(dist2, site, radius):
    if radius is None:
        return dist2, site
    far = dist2 > radius * radius
    return np.where(far, FAR, dist2).astype(np.int32), np.where(far, -1, site).astype(np.int32)


def field_of(coords, tsdf, lo=None, hi=None, radius=None, origin=FX.ORIGIN, **kw):
    from eprecon_amd import _lib
    from eprecon_amd.distance_field import distance_field
    field = distance_field((dev(coords, torch.int32).reshape(-1, 3), dev(tsdf, torch.float32).reshape(-1), origin, VOXEL), lo, hi,
                           metres(radius), **kw)
    _lib.drain_deferred()              # the kernel's status word: raises when it is set
    return field


def assert_field(field, want, radius):
    dist2, site = cut(want[0], want[1], radius)
    assert field.dist2.dtype == torch.int32 and field.site.dtype == torch.int32 and field.state.dtype == torch.uint8
    assert np.array_equal(host(field.state), want[2])
    assert np.array_equal(host(field.dist2), dist2)
    assert np.array_equal(host(field.site), site)


def raw(coords, tsdf, lo, hi, radius, workspace_bytes=None):
    """the C entry itself: -> (return code, dist2, site, state, status) with only the sites inside [lo, hi) counting"""
    from eprecon_amd import _lib
    lib = _lib.load()
    coords, tsdf = np.asarray(coords, np.int32).reshape(-1, 3), np.asarray(tsdf, np.float32).reshape(-1)
    m = len(coords)
    c, t = (dev(coords), dev(tsdf)) if m else (None, None)
    c_lo, c_hi = (ctypes.c_int32 * 3)(*lo), (ctypes.c_int32 * 3)(*hi)
    shape = tuple(max(int(h - l), 1) for l, h in zip(lo, hi))
    nbytes = int(lib.eprecon_distance_field_workspace_bytes(m, c_lo, c_hi))
    mem = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    dist2 = torch.full(shape, 12345, dtype=torch.int32, device="cuda")
    site = torch.full(shape, 12345, dtype=torch.int32, device="cuda")
    state = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    rc = lib.eprecon_distance_field_async(_lib.ptr(c), _lib.ptr(t), m, c_lo, c_hi, int(radius), _lib.ptr(dist2), _lib.ptr(site),
                                          _lib.ptr(state), _lib.ptr(status), _lib.ptr(mem), nbytes if workspace_bytes is None else workspace_bytes,
                                          _lib.current_stream())
    torch.cuda.synchronize()
    return rc, host(dist2), host(site), host(state), int(status.item())


def raw_reference(coords, tsdf, lo, hi, radius):
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    sites = D.site_rows(coords, tsdf)
    inside = ((coords[sites] >= np.array(lo)) & (coords[sites] < np.array(hi))).all(1) if len(sites) else np.zeros(0, bool)
    shape = tuple(int(h - l) for l, h in zip(lo, hi))
    dist2, site = D.nearest_sites(D.box_cells(lo, hi), coords, sites[inside], radius)
    return dist2.astype(np.int32).reshape(shape), site.astype(np.int32).reshape(shape), D.states(coords, tsdf, lo, hi)


def scattered(lo, hi, n, seed):
    """n rows (coordinates may repeat), half of them scattered over the box and half over the box and one cell around it, a
    third of them inside, the first one for certain: most are sites"""
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.integers(l - 1, h + 1, n) for l, h in zip(lo, hi)], 1).astype(np.int32)
    coords[:(n + 1) // 2] = np.stack([rng.integers(l, h, (n + 1) // 2) for l, h in zip(lo, hi)], 1)
    tsdf = np.where(rng.random(n) < 0.34, -0.5, 0.5).astype(np.float32)
    tsdf[rng.random(n) < 0.1] = 0.0
    tsdf[0] = -0.5
    return coords, tsdf


# ------------------------------------------------------------------------------------------------------------------- scenes

@pytest.mark.parametrize("radius", [0, 1, 5, 100, None])
@pytest.mark.parametrize("scene", SCENES)
def test_scenes_are_the_reference(scene, radius):
    """R = 0 keeps the sites only, R = 100 is larger than the box, None is unbounded"""
    s = shuffled(scene)
    field = field_of(s["coords"], s["tsdf"], s["lo"], s["hi"], radius, origin=s["origin"])
    assert field.lo == s["lo"] and field.shape == tuple(h - l for l, h in zip(s["lo"], s["hi"]))
    assert_field(field, scene_reference(scene), radius)
    near = host(field.dist2) != FAR
    assert near.any() and (radius in (100, None)) == bool(near.all())
    if radius == 0:
        assert int(near.sum()) == len(D.site_rows(s["coords"], s["tsdf"]))


def test_the_default_box_is_the_rows_box_dilated():
    s = shuffled("sphere")
    lo, hi = s["coords"].min(0), s["coords"].max(0) + 1
    bounded = field_of(s["coords"], s["tsdf"], radius=3)
    assert bounded.lo == tuple(int(v) - 3 for v in lo) and bounded.hi == tuple(int(v) + 3 for v in hi) and bounded.radius == 3
    unbounded = field_of(s["coords"], s["tsdf"])
    assert unbounded.lo == s["lo"] and unbounded.hi == s["hi"]
    assert_field(unbounded, scene_reference("sphere"), None)
    inner = tuple(slice(5, n - 5) for n in unbounded.shape)
    want = cut(scene_reference("sphere")[0][inner], scene_reference("sphere")[1][inner], 3)
    assert np.array_equal(host(bounded.dist2), want[0]) and np.array_equal(host(bounded.site), want[1])


def test_a_scene_grid_is_accepted_and_only_its_rows_are_used():
    from types import SimpleNamespace
    s = shuffled("sphere")
    grid = SimpleNamespace(coords=dev(s["coords"]), tsdf=dev(s["tsdf"]), origin=s["origin"], voxel_size=s["voxel_size"])
    from eprecon_amd.distance_field import distance_field
    field = distance_field(grid, s["lo"], s["hi"], metres(5))
    assert_field(field, scene_reference("sphere"), 5)
    from eprecon_amd.raycast import SceneGrid
    field = distance_field(SceneGrid(grid.coords, grid.tsdf, s["origin"], s["voxel_size"]), s["lo"], s["hi"], metres(5))
    assert_field(field, scene_reference("sphere"), 5)
    assert np.array_equal(field.origin, np.asarray(s["origin"], np.float64)) and field.voxel_size == s["voxel_size"]


# ------------------------------------------------------------------------------------------------------------- box extents

EXTENTS = [(7, 9, 1), (7, 9, 63), (7, 9, 64), (7, 9, 65), (3, 4, 200),      # z, the lane axis: one wave, its edge, two, four
           (1, 9, 20), (7, 1, 20), (130, 5, 9), (5, 130, 9),                # a scanned axis of 1 and of more than one tile
           (1, 70, 1), (1, 1, 1)]


@pytest.mark.parametrize("radius", [3, 300])
@pytest.mark.parametrize("shape", EXTENTS)
def test_box_extents_at_the_entry_itself(shape, radius):
    lo = (-3, 5, -60)
    hi = tuple(l + n for l, n in zip(lo, shape))
    coords, tsdf = scattered(lo, hi, 6 + shape[0] * shape[1] * shape[2] // 40, seed=sum(shape))
    rc, dist2, site, state, status = raw(coords, tsdf, lo, hi, radius)
    assert (rc, status) == (0, 0)
    want = raw_reference(coords, tsdf, lo, hi, radius)
    assert np.array_equal(state, want[2])
    assert np.array_equal(dist2, want[0])
    assert np.array_equal(site, want[1])
    assert (dist2 != FAR).any()


@pytest.mark.parametrize("shape", [(7, 9, 65), (130, 5, 9), (1, 70, 1)])
def test_box_extents_through_the_module(shape):
    """... where every site counts, those outside the box too"""
    lo = (-3, 5, -60)
    hi = tuple(l + n for l, n in zip(lo, shape))
    coords, tsdf = scattered(tuple(v - 4 for v in lo), tuple(v + 4 for v in hi), 40 + shape[0] * shape[1] * shape[2] // 40, seed=sum(shape))
    for radius in (3, None):
        assert_field(field_of(coords, tsdf, lo, hi, radius), D.distance_field(coords, tsdf, lo, hi), radius)


# ------------------------------------------------------------------------------------------------------------------ radius

def test_the_cut_keeps_r_squared_and_drops_r_squared_plus_one():
    coords, tsdf = np.array([[0, 0, 0]], np.int32), np.array([-0.3], np.float32)        # one inside row in empty space: a site
    field = field_of(coords, tsdf, (-6, -6, -6), (7, 7, 7), 5)
    dist2, site = host(field.dist2), host(field.site)
    at = lambda x, y, z: (x + 6, y + 6, z + 6)
    assert dist2[at(3, 4, 0)] == 25 and site[at(3, 4, 0)] == 0 and dist2[at(5, 0, 0)] == 25 and dist2[at(0, -4, 3)] == 25
    assert dist2[at(3, 4, 1)] == FAR and site[at(3, 4, 1)] == -1 and dist2[at(5, 1, 0)] == FAR and dist2[at(-6, 0, 0)] == FAR
    assert_field(field, D.distance_field(coords, tsdf, (-6, -6, -6), (7, 7, 7)), 5)
    assert int((dist2 != FAR).sum()) == 515                                             # the lattice points of a ball of radius 5


# -------------------------------------------------------------------------------------------------------------------- ties

@pytest.mark.parametrize("axes,ways", [((0,), 2), ((0, 1), 4), ((0, 1, 2), 8)])
def test_ties_go_to_the_smallest_row(axes, ways):
    """sites mirrored about a plane, an edge and a corner; the rows in a shuffled order, every coordinate repeated by a later
    row of the other sign, which must not count"""
    base = np.array([3, 2, 4])
    signs = np.stack(np.meshgrid(*[(-1, 1) if a in axes else (1,) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    cells = signs * base
    assert len(cells) == ways
    order = np.random.default_rng(ways).permutation(ways)
    coords = np.concatenate([cells[order], cells]).astype(np.int32)
    tsdf = np.concatenate([np.full(ways, -0.5), np.full(ways, 0.5)]).astype(np.float32)
    lo, hi = (-7, -6, -8), (8, 7, 9)
    want = D.distance_field(coords, tsdf, lo, hi)
    centre = tuple(0 if a in axes else int(base[a]) for a in range(3))
    k = tuple(c - l for c, l in zip(centre, lo))
    assert want[1][k] == 0 and want[0][k] == sum(int(base[a]) ** 2 for a in axes)       # all `ways` sites tie there: row 0 wins
    for radius in (None, 6):
        field = field_of(coords, tsdf, lo, hi, radius)
        assert_field(field, want, radius)
        assert host(field.site).max() < ways                                           # never a repeated coordinate's later row


# ----------------------------------------------------------------------------------------------------------- boundary rows

def test_boundary_rows():
    lo, hi = (-3, -3, -3), (6, 5, 4)
    # an inside row beside an empty coordinate; a row with tsdf == 0, which is inside; an outside row none of whose neighbours
    # is inside, which is no site
    coords = np.array([[0, 0, 0], [1, 0, 0], [3, 1, 0], [3, 2, 0], [4, 3, 2]], np.int32)
    tsdf = np.array([-0.5, 0.5, 0.0, 0.5, 0.5], np.float32)
    assert D.site_rows(coords, tsdf).tolist() == [0, 1, 2, 3]
    field = field_of(coords, tsdf, lo, hi)
    assert_field(field, D.distance_field(coords, tsdf, lo, hi), None)
    assert host(field.state)[3, 3, 3] == 2 and host(field.state)[6, 4, 3] == 2 and host(field.state)[7, 6, 5] == 1
    assert host(field.dist2)[7, 6, 5] == 6                                              # (4,3,2) is no site: (3,2,0) is nearest


def test_rows_that_are_all_outside_give_all_far():
    coords, tsdf = scattered((0, 0, 0), (9, 9, 9), 60, seed=5)
    field = field_of(coords, np.abs(tsdf) + 0.1, (-2, -2, -2), (11, 11, 11))
    assert (host(field.dist2) == FAR).all() and (host(field.site) == -1).all()
    assert np.array_equal(host(field.state), D.states(coords, tsdf * 0 + 1, (-2, -2, -2), (11, 11, 11))) and host(field.state).any()


def test_no_rows():
    from eprecon_amd import _lib
    reads = _lib.HOST_READS
    field = field_of(np.zeros((0, 3), np.int32), np.zeros(0, np.float32), (1, 2, 3), (4, 7, 5), 2)
    assert _lib.HOST_READS == reads
    assert field.shape == (3, 5, 2) and (host(field.dist2) == FAR).all() and (host(field.site) == -1).all() and not host(field.state).any()
    rc, dist2, site, state, status = raw(np.zeros((0, 3)), np.zeros(0), (1, 2, 3), (4, 7, 5), 2)
    assert (rc, status) == (0, 0) and (dist2 == FAR).all() and (site == -1).all() and not state.any()
    with pytest.raises(ValueError):
        field_of(np.zeros((0, 3), np.int32), np.zeros(0, np.float32))


# -------------------------------------------------------------------------------------------- split boxes, runs, host reads

@pytest.mark.parametrize("radius", [5, None])
def test_a_box_in_parts_is_the_box_whole(radius):
    """halves and octants: sites outside a part, within R of it, count as they do for the whole"""
    s = shuffled("sphere_shifted")
    lo, hi = s["lo"], s["hi"]
    mid = tuple((l + h) // 2 + 1 for l, h in zip(lo, hi))
    whole = field_of(s["coords"], s["tsdf"], lo, hi, radius)
    assert_field(whole, scene_reference("sphere_shifted"), radius)
    halves = [((lo[0], lo[1], lo[2]), (mid[0], hi[1], hi[2])), ((mid[0], lo[1], lo[2]), hi)]
    octants = [(tuple((lo, mid)[b][a] for a, b in enumerate(bits)), tuple((mid, hi)[b][a] for a, b in enumerate(bits)))
               for bits in np.ndindex(2, 2, 2)]
    for parts in (halves, octants):
        for plo, phi in parts:
            part = field_of(s["coords"], s["tsdf"], plo, phi, radius)
            where = tuple(slice(a - l, b - l) for a, b, l in zip(plo, phi, lo))
            for name in ("dist2", "site", "state"):
                assert torch.equal(getattr(part, name), getattr(whole, name)[where]), (name, plo, phi)


def test_a_box_beyond_reach_of_the_rows_is_all_far_without_a_launch():
    s = shuffled("sphere")
    field = field_of(s["coords"], s["tsdf"], (40, 0, 0), (45, 6, 7), 5)
    assert field.shape == (5, 6, 7) and (host(field.dist2) == FAR).all() and (host(field.site) == -1).all() and not host(field.state).any()
    # ... and one step closer the nearest site is exactly R away
    s2 = (np.array([[0, 0, 0]], np.int32), np.array([-1.0], np.float32))
    assert (host(field_of(*s2, (6, 0, 0), (8, 1, 1), 5).dist2) == FAR).all()
    assert host(field_of(*s2, (5, 0, 0), (8, 1, 1), 5).dist2).reshape(-1).tolist() == [25, FAR, FAR]


def test_two_runs_are_bit_equal_and_a_call_reads_once():
    from eprecon_amd import _lib
    s = shuffled("slab_box")
    reads = _lib.HOST_READS
    from eprecon_amd.distance_field import distance_field
    rows = (dev(s["coords"]), dev(s["tsdf"]), s["origin"], s["voxel_size"])
    first = distance_field(rows, s["lo"], s["hi"], metres(5))
    assert _lib.HOST_READS == reads + 1 and _lib.has_deferred()
    _lib.drain_deferred()
    second = distance_field(rows, s["lo"], s["hi"], metres(5))
    for name in ("dist2", "site", "state"):
        assert torch.equal(getattr(first, name), getattr(second, name)), name


# ---------------------------------------------------------------------------------------------------------- derived outputs

def test_labels_are_the_sites_ids():
    s = shuffled("slab_box")
    field = field_of(s["coords"], s["tsdf"], s["lo"], s["hi"], 5)
    sem, ins = field.labels(dev(s["semantic"]), dev(s["instance"]), backgrounds=(0, 255))
    _, site = cut(*scene_reference("slab_box")[:2], 5)
    assert np.array_equal(host(sem), np.where(site >= 0, s["semantic"][site.clip(0)], 0))
    assert np.array_equal(host(ins), np.where(site >= 0, s["instance"][site.clip(0)], 255))
    assert sem.dtype == torch.int32 and len(np.unique(host(sem))) == 3


def test_metres_and_at():
    s = shuffled("sphere")
    field = field_of(s["coords"], s["tsdf"], s["lo"], s["hi"], 5, origin=s["origin"])
    dist2, site = cut(*scene_reference("sphere")[:2], 5)
    state = scene_reference("sphere")[2]
    with np.errstate(over="ignore"):
        want = np.where(dist2 == FAR, np.inf, np.sqrt(dist2.astype(np.float64)) * VOXEL)
    assert np.array_equal(host(field.metres(signed=False)), want.astype(np.float32))
    assert np.array_equal(host(field.metres()), np.where(state == 2, -want, want).astype(np.float32))
    assert (host(field.metres()) < 0).any()
    lo, hi, origin = np.array(s["lo"]), np.array(s["hi"]), np.asarray(s["origin"], np.float64)
    # inside the box off a cell's centre, on it, the box's two corner cells; one cell below the box and one above it
    a = np.argwhere((dist2[:-1] > 0) & (dist2[:-1] != FAR) & (dist2[1:] != dist2[:-1]))[0]       # a cell unlike its upper x neighbour
    cells = np.array([lo + a, lo + a, hi - 1, lo, lo - (1, 0, 0), (lo[0], lo[1], hi[2])])
    offsets = np.array([[0.3, -0.4, 0.1], [0.0, 0.0, 0.0], [0.2, 0.2, 0.49], [-0.49, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    inside = np.array([True, True, True, True, False, False])
    k = (cells - lo).clip(0, np.array(field.shape) - 1)
    want_d2, want_site = np.where(inside, dist2[k[:, 0], k[:, 1], k[:, 2]], FAR), np.where(inside, site[k[:, 0], k[:, 1], k[:, 2]], -1)
    assert want_d2[0] not in (0, FAR) and want_d2[2] == FAR
    got_d2, got_site = field.at(origin + (cells + offsets) * VOXEL)
    assert host(got_d2).tolist() == want_d2.tolist() and host(got_site).tolist() == want_site.tolist()
    got_d2, got_site = field.at(dev(origin + (cells + offsets) * VOXEL))             # a device tensor as well as an array
    assert host(got_d2).tolist() == want_d2.tolist() and host(got_site).tolist() == want_site.tolist()
    # exactly on the boundary between two cells (a lattice whose arithmetic is exact): the upper one
    from eprecon_amd.distance_field import DistanceField
    exact = DistanceField(field.dist2, field.site, field.state, field.lo, (0.0, 0.0, 0.0), 0.25, 5)
    c = lo + a
    got_d2, _ = exact.at(np.array([(c + (-0.5, 0.0, 0.0)) * 0.25, (c + (0.5, 0.0, 0.0)) * 0.25, (c + (0.0, 0.0, -0.5)) * 0.25]))
    here = dist2[a[0]:a[0] + 2, a[1], a[2]].tolist() + [int(dist2[tuple(a)])]
    assert host(got_d2).tolist() == here and here[0] != here[1]


def test_clearance_is_the_minimum_over_the_slab():
    s = shuffled("slab_box")
    field = field_of(s["coords"], s["tsdf"], s["lo"], s["hi"], 5)
    dist2, _ = cut(*scene_reference("slab_box")[:2], 5)
    z = np.arange(s["lo"][2], s["hi"][2])
    for z_lo, z_hi in ((0.1, 0.6), (9 * VOXEL, 9 * VOXEL), (-5.0, 5.0), (0.41, 0.43)):
        keep = (z * VOXEL >= z_lo - 1e-9) & (z * VOXEL <= z_hi + 1e-9)
        want = dist2[:, :, keep].min(2) if keep.any() else np.full(dist2.shape[:2], FAR)
        got = field.clearance(z_lo, z_hi)
        assert got.dtype == torch.int32 and np.array_equal(host(got), want), (z_lo, z_hi)
    assert (host(field.clearance(0.41, 0.43)) == FAR).all() and (host(field.clearance(0.1, 0.6)) != FAR).any()


# ------------------------------------------------------------------------------------------------------------------ errors

def test_errors():
    from eprecon_amd import _lib
    from eprecon_amd.distance_field import distance_field
    s = shuffled("sphere")
    cpu = (torch.from_numpy(s["coords"]), torch.from_numpy(s["tsdf"]), s["origin"], VOXEL)
    with pytest.raises(_lib.EpreconError):
        distance_field(cpu)
    rows = (dev(s["coords"]), dev(s["tsdf"]), s["origin"], VOXEL)
    reads = _lib.HOST_READS
    with pytest.raises(ValueError, match="inverted"):
        distance_field(rows, (0, 0, 5), (4, 4, 5))
    with pytest.raises(ValueError, match="inverted"):
        distance_field(rows, (0, 6, 0), (4, 4, 5))
    with pytest.raises(ValueError, match=r"1025 x 2 x 2 = 4100 cells exceeds max_cells = 134217728 cells or 1024 cells per axis"):
        distance_field(rows, (0, 0, 0), (1025, 2, 2))
    ext = tuple(h - l for l, h in zip(s["lo"], s["hi"]))
    cells = ext[0] * ext[1] * ext[2]
    with pytest.raises(ValueError, match=f"{ext[0]} x {ext[1]} x {ext[2]} = {cells} cells exceeds max_cells = {cells - 1} cells"):
        distance_field(rows, s["lo"], s["hi"], max_cells=cells - 1)
    assert _lib.HOST_READS == reads and not _lib.has_deferred()           # refused before the read and before any launch
    assert distance_field(rows, s["lo"], s["hi"], max_cells=cells).shape == ext
    _lib.drain_deferred()
    # the working box is what counts: the request's 24 x 24 x 8 cells grow by 8 towards the rows above them
    with pytest.raises(ValueError, match=r"24 x 24 x 16 = 9216 cells exceeds max_cells = 9215"):
        distance_field(rows, (0, 0, 0), (24, 24, 8), metres(8), max_cells=9215)
    assert not _lib.has_deferred()
    assert distance_field(rows, (0, 0, 0), (24, 24, 8), metres(8), max_cells=9216).shape == (24, 24, 8)


def test_a_coordinate_at_the_key_limit():
    from eprecon_amd import _lib
    limit = (1 << 19) - 2
    coords = np.array([[0, 0, 0], [0, limit, 0]], np.int32)
    tsdf = np.array([-0.5, -0.5], np.float32)
    with pytest.raises(_lib.EpreconError, match="range"):
        field_of(coords, tsdf, (-2, -2, -2), (3, 3, 3))
    rc, dist2, site, state, status = raw(coords, tsdf, (-2, -2, -2), (3, 3, 3), 9)
    assert rc == 0 and status == 1
    coords[1, 1] = 1 - limit
    assert raw(coords, tsdf, (-2, -2, -2), (3, 3, 3), 9)[4] == 0
    coords[1, 1] = -limit
    assert raw(coords, tsdf, (-2, -2, -2), (3, 3, 3), 9)[4] == 1


def test_the_entry_refuses_bad_arguments():
    from eprecon_amd import _lib
    lib = _lib.load()
    coords, tsdf = np.array([[0, 0, 0]], np.int32), np.array([-0.5], np.float32)
    bad = _lib.EPRECON_ERR_ARG if hasattr(_lib, "EPRECON_ERR_ARG") else -1
    assert bad == -1
    assert raw(coords, tsdf, (0, 0, 0), (0, 4, 4), 1)[0] == bad             # empty
    assert raw(coords, tsdf, (0, 5, 0), (4, 4, 4), 1)[0] == bad             # inverted
    assert raw(coords, tsdf, (0, 0, 0), (4, 4, 4), -1)[0] == bad            # radius
    assert raw(coords, tsdf, (0, 0, 0), (4, 4, 4), 1, workspace_bytes=255)[0] == bad
    c_lo, c_big = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(1025, 1, 1)
    assert lib.eprecon_distance_field_workspace_bytes(1, c_lo, c_big) == 0  # an extent above 2^10
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    mem = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.empty(1025, dtype=torch.int32, device="cuda")
    assert lib.eprecon_distance_field_async(None, None, 0, c_lo, c_big, 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(mem), _lib.ptr(status),
                                            _lib.ptr(mem), mem.numel(), _lib.current_stream()) == bad
    c_ok = (ctypes.c_int32 * 3)(1024, 1, 1)
    want = 256 + 1024 * 12 + 2 * 1024 * 8                                   # the row table of one row and two volumes of keys
    assert lib.eprecon_distance_field_workspace_bytes(1, c_lo, c_ok) == want
    assert raw(coords, tsdf, (0, 0, 0), (4, 4, 4), 1)[0] == 0


# -------------------------------------------------------------------------------------------------- file and command line

def read_png16(path):
    """a 16-bit greyscale PNG whose rows all use filter 0 (raycast.write_png16 writes those) -> uint16 [H,W]"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, {}
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        chunks[tag] = chunks.get(tag, b"") + data[at + 8:at + 8 + n]
        at += 12 + n
    w, h, depth, colour = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, colour) == (16, 0)
    raw_rows = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + 2 * w)
    assert not raw_rows[:, 0].any()
    return raw_rows[:, 1:].copy().view(">u2").astype(np.uint16)


def test_the_file_round_trip(tmp_path):
    from eprecon_amd.distance_field import FILE_KEYS, read_distance, write_distance
    s = shuffled("sphere_shifted")
    field = field_of(s["coords"], s["tsdf"], s["lo"], s["hi"], 5, origin=s["origin"])
    path = write_distance(field, str(tmp_path / "deep" / "scene_distance.npz"))
    with np.load(path) as z:
        assert sorted(z.files) == sorted(FILE_KEYS)
        assert z["dist2"].dtype == np.int32 and z["site"].dtype == np.int32 and z["state"].dtype == np.uint8
    back = read_distance(path)
    assert back.lo == field.lo and back.radius == 5 and back.voxel_size == field.voxel_size and np.array_equal(back.origin, field.origin)
    for name in ("dist2", "site", "state"):
        assert torch.equal(getattr(back, name), getattr(field, name).cpu()), name
    assert torch.equal(read_distance(path, "cuda").clearance(-1.0, 0.0), field.clearance(-1.0, 0.0))


def test_the_command_line(tmp_path, capsys):
    from eprecon_amd import distance_field as DF
    from eprecon_amd.scene_io import write_scene
    s = FX.slab_box()                                                     # in raster order, as a saved scene's rows are read
    pred, out = tmp_path / "pred", tmp_path / "out"
    pred.mkdir()
    write_scene(str(pred / "scene0000_00.npz"), s["tsdf"], s["semantic"], s["instance"], coords=s["coords"],
                origin=np.asarray(s["origin"], np.float32), voxel_size=np.float32(VOXEL), dims=np.array(s["dims"]))
    (tmp_path / "scenes.txt").write_text("scene0000_00\n")
    args = ["--pred", str(pred), "--scenes", str(tmp_path / "scenes.txt"), "--out", str(out), "--max_distance", "0.2", "--slab", "0.1", "0.6"]
    assert DF.main(args) == 0
    assert sorted(os.listdir(out)) == ["scene0000_00_clearance.png", "scene0000_00_distance.npz"]
    lo, hi = tuple(int(v) - 5 for v in s["coords"].min(0)), tuple(int(v) + 6 for v in s["coords"].max(0))
    assert "scene0000_00: {} x {} x {} cells from {}, R = 5 cells".format(*(h - l for l, h in zip(lo, hi)), lo) in capsys.readouterr().out
    field = DF.read_distance(str(out / "scene0000_00_distance.npz"))
    assert field.lo == lo and field.radius == 5
    want = D.distance_field(s["coords"], s["tsdf"], lo, hi, 5)
    for got, ref in zip((field.dist2, field.site, field.state), want):
        assert np.array_equal(host(got), ref)
    z = np.arange(lo[2], hi[2])
    slab = want[0][:, :, (z * VOXEL >= 0.1 - 1e-9) & (z * VOXEL <= 0.6 + 1e-9)].min(2)
    mm = np.where(slab == FAR, 65535, np.floor(np.sqrt(slab.astype(np.float64)) * VOXEL * 1000.0 + 0.5)).astype(np.uint16)
    assert np.array_equal(read_png16(str(out / "scene0000_00_clearance.png")), mm) and len(np.unique(mm)) > 3

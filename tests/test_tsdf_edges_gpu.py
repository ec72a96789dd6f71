"""GPU: the TSDF integration (csrc/tsdf_fusion.hip) at its edges.

  sweep        both variants on three volumes that are no cubes / no multiple of the workgroup, fx != fy, H != W, observation
               weights 0.5, 1 and 2, one call against frame by frame (equal bits), against the float64 witness (tests/tsdf_ref.py)
  views        1 .. 33 views: the 16-view chunks of one call, the occupancy written by the last chunk only
  cells        volumes of 1, 255, 256, 257 and 105 cells inside guard-filled buffers
  constructed  identity pose and power-of-two sizes, every fp32 quantity exact: each decision of the kernel (pixel ties, the camera
               plane, diff == -trunc, depth 0 / -1 / Inf / NaN) bit exact against oracle/tsdf_fusion.py and against the result
               written out by hand (CONSTRUCTED below; tests/test_tsdf_ref.py checks the hand results against the oracle on the host)
  occupancy    weight 1 against 2, tsdf one fp32 step either side of +-0.999: the device byte and the Python fallback
  refusals     the C entry point's argument checks, which write nothing
"""
import ctypes

import numpy as np
import pytest

import tsdf_ref as R
from oracle import tsdf_fusion as OT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
EYE = np.eye(4, dtype=F32)
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# constructed cases (host data only: shared with tests/test_tsdf_ref.py)
# ---------------------------------------------------------------------------------------------------------------------
def _ramp(h, w, z):
    """depth increasing by column and by row: d - z = (1 + column + w * row) / 64, distinct per pixel, inside (0, 1)"""
    return (z + (1.0 + np.arange(w)[None, :] + w * np.arange(h)[:, None]) / 64.0).astype(F32)


def _case(dims, origin, voxel_size, margin, depth, f, cx, cy, want):
    """want: variant -> (tsdf, weight) nested lists over [X][Y][Z]"""
    intr = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], F32)
    return dict(dims=dims, origin=np.array(origin, F32), voxel_size=voxel_size, margin=margin, depths=np.asarray(depth, F32)[None],
                intrs=intr[None], want={k: (np.array(t, F32).reshape(dims), np.array(w, F32).reshape(dims)) for k, (t, w) in want.items()})


def _from_pixels(px, py, w):
    """the ramp's value at the pixel each voxel picks (-1: not integrated), voxels [X][Y][1]"""
    t = [[[(1.0 + a + w * b) / 64.0 if a >= 0 and b >= 0 else 1.0] for b in py] for a in px]
    wt = [[[1.0 if a >= 0 and b >= 0 else 0.0] for b in py] for a in px]
    return t, wt


def _constructed():
    c = {}
    # Pixel ties in u: voxel size 1/4, focal length 4, layer z = 1, origin x = -1/4, cx = 1/2: u = ix - 1/2 for ix = 0 .. 5, on a
    # 5 x 3 image, so u = -1/2 and u = W - 1/2 are among them; v = iy.  "torch" rounds to even (-1/2 -> -0 -> pixel 0; 9/2 -> 4),
    # "cuda" away from zero (-1/2 -> -1 and 9/2 -> 5: both outside).
    even, away = [0, 0, 2, 2, 4, 4], [-1, 1, 2, 3, 4, -1]
    c["tie_u"] = _case((6, 3, 1), (-0.25, 0, 1), 0.25, 4, _ramp(3, 5, 1.0), 4, 0.5, 0,
                       {"torch": _from_pixels(even, [0, 1, 2], 5), "cuda": _from_pixels(away, [0, 1, 2], 5)})
    # the same in v, on a 3 x 5 image
    c["tie_v"] = _case((3, 6, 1), (0, -0.25, 1), 0.25, 4, _ramp(5, 3, 1.0), 4, 0, 0.5,
                       {"torch": _from_pixels([0, 1, 2], even, 3), "cuda": _from_pixels([0, 1, 2], away, 3)})
    # Camera plane: layers at z = -1/4, 0 and 1/4.  Only the last is integrated: u = 4 (ix / 4) / (1 / 4) = 4 ix, v = 4 iy on a
    # 9 x 5 image, so ix <= 2 and iy <= 1 are inside.  At z = 0 "torch" fails the front test and "cuda" divides by zero (Inf / NaN
    # pixel); at z < 0 "cuda" without its front test would find u = -4 ix, i.e. pixel 0 for ix = 0.
    t = [[[1.0, 1.0, (1.0 + 4 * ix + 9 * 4 * iy) / 64.0 if ix <= 2 and iy <= 1 else 1.0] for iy in range(3)] for ix in range(4)]
    w = [[[0.0, 0.0, 1.0 if ix <= 2 and iy <= 1 else 0.0] for iy in range(3)] for ix in range(4)]
    c["plane"] = _case((4, 3, 3), (0, 0, -0.25), 0.25, 4, _ramp(5, 9, 0.25), 4, 0, 0, {"torch": (t, w), "cuda": (t, w)})
    # Truncation: layer z = 2, trunc = 1, u = 8 (ix / 4) / 2 = ix.  d = 1: diff = -1 = -trunc, integrated with dist = -1; d = 1 - 2^-23:
    # diff = -1 - 2^-23, the next fp32 below -1, skipped; d = 1 + 2^-23: dist = -1 + 2^-23; d = 3: dist = 1; d = 3 - 2^-22: the last fp32
    # below 1; d = 3 + 2^-22 and d = 5: clipped to 1; d = 2.5: 0.5
    e23, e22 = 2.0 ** -23, 2.0 ** -22
    depth = [[1.0, 1.0 - e23, 1.0 + e23, 3.0, 3.0 - e22, 3.0 + e22, 5.0, 2.5], [9.0] * 8]
    t = [[[v]] for v in (-1.0, 1.0, -1.0 + e23, 1.0, 1.0 - e22, 1.0, 1.0, 0.5)]
    w = [[[v]] for v in (1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)]
    c["trunc"] = _case((8, 1, 1), (0, 0, 2), 0.25, 4, depth, 8, 0, 0, {"torch": (t, w), "cuda": (t, w)})
    # Depth values: voxel size 1, layer z = 1, trunc = 4, focal length 1: u = ix.  d = 2 gives dist = 1/4 in both; d = -1 gives
    # diff = -2 >= -trunc, dist = -1/2 where it is let through
    depth = [[0.0, -1.0, INF, NAN, 2.0, -0.0, -INF]]
    c["depth_values"] = _case((7, 1, 1), (0, 0, 1), 1.0, 4, depth, 1, 0, 0, {
        "torch": ([[[v]] for v in (1.0, 1.0, 1.0, 1.0, 0.25, 1.0, 1.0)], [[[v]] for v in (0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)]),
        "cuda": ([[[v]] for v in (1.0, -0.5, 1.0, 1.0, 0.25, 1.0, 1.0)], [[[v]] for v in (0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0)])})
    return c


CONSTRUCTED = _constructed()


def oracle_of_constructed(case, variant):
    tsdf, weight = np.ones(case["dims"], F32), np.zeros(case["dims"], F32)
    OT.integrate(tsdf, weight, case["origin"], case["voxel_size"], case["depths"][0], case["intrs"][0], EYE,
                 case["margin"] * case["voxel_size"], 1.0, variant)
    return tsdf, weight


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
def _volume(dims, origin, voxel_size, variant, margin=R.MARGIN):
    from eprecon_amd.tsdf_fusion import TSDFVolumeHIP
    return TSDFVolumeHIP(torch.tensor(list(dims)), torch.from_numpy(np.asarray(origin, F32)), voxel_size, margin=margin,
                         variant=variant)


def _host(vol):
    t, w = (x.cpu().numpy() for x in vol.get_volume())
    return t, w, vol.occupancy().cpu().numpy()


def _rule(tsdf, weight):
    return (tsdf < F32(0.999)) & (tsdf > F32(-0.999)) & (weight > 1)


def _run_both_forms(case, variant, obs, idx=None):
    """one call with all views, and integrate() frame by frame -> (tsdf, weight, occ) of the call, after asserting equal bits; the
    matrices the kernel got"""
    idx = np.arange(len(case["depths"])) if idx is None else idx
    depths = torch.from_numpy(case["depths"][idx]).cuda()
    intrs, poses = torch.from_numpy(case["intrs"][idx]), torch.from_numpy(case["poses"][idx])
    a = _volume(case["dims"], case["origin"], case["voxel_size"], variant)
    b = _volume(case["dims"], case["origin"], case["voxel_size"], variant)
    a.integrate_views(depths, intrs, poses, obs_weight=obs)
    for v in range(len(idx)):
        b.integrate(depths[v], intrs[v], poses[v], obs_weight=obs)
    ta, wa, oa = _host(a)
    tb, wb, ob = _host(b)
    assert same_bits(ta, tb) and same_bits(wa, wb) and np.array_equal(oa, ob)
    assert np.array_equal(a._occ.cpu().numpy(), _rule(ta, wa).astype(np.uint8))      # the device byte itself: 0 or 1
    mats = torch.inverse(poses).numpy() if variant == "torch" else poses.numpy()
    return (ta, wa, oa), mats


# ---------------------------------------------------------------------------------------------------------------------
# sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["torch", "cuda"])
@pytest.mark.parametrize("name", list(R.SWEEP))
def test_sweep_against_the_float64_witness(name, variant, record_property):
    case = R.sweep_case(name)
    worst = 0.0
    for obs in (1.0, 0.5, 2.0):
        (tsdf, weight, occ), mats = _run_both_forms(case, variant, obs)
        wit = R.fuse(case["dims"], case["origin"], case["voxel_size"], case["depths"], case["intrs"], mats, case["trunc"], obs, variant)
        undecided = 1.0 - float(wit.decided.mean())
        assert undecided <= 0.10
        ratio = R.check(wit, tsdf, weight, occ)
        print(f"{name} {variant} obs {obs}: undecided share {undecided:.4f}, max |tsdf - tsdf64| / E = {ratio:.3f}")
        worst = max(worst, ratio)
        if obs == 0.5:      # two views do not make a cell occupied
            assert not occ[weight == 1.0].any() and (weight == 1.0).any() and occ[weight == 1.5].any()
        record_property(f"undecided_share_obs{obs}", undecided)
    record_property("observed_over_bound", worst)


# ---------------------------------------------------------------------------------------------------------------------
# view-count boundary
# ---------------------------------------------------------------------------------------------------------------------
VIEWS_CASE = dict(dims=(12, 9, 7), voxel_size=0.3, views=9, width=80, height=60)


@pytest.mark.parametrize("variant", ["torch", "cuda"])
@pytest.mark.parametrize("n_views", [1, 15, 16, 17, 32, 33])
def test_view_chunks(n_views, variant):
    """the 9 rendered views wrapped round (view k is view k % 9, pose and all).  With obs = 1/16 (1/32) a cell is occupied only once
    17 (33) views have reached it: an occupancy written after the first chunk of 16 would be empty."""
    case = R.window_case(**VIEWS_CASE)
    idx = np.arange(n_views) % 9
    for obs in (1.0, 1.0 / 16, 1.0 / 32):
        (tsdf, weight, occ), mats = _run_both_forms(case, variant, obs, idx)
        assert np.array_equal(occ, _rule(tsdf, weight))
        wit = R.fuse(case["dims"], case["origin"], case["voxel_size"], case["depths"][idx], case["intrs"][idx], mats, case["trunc"],
                     obs, variant)
        assert wit.decided.mean() >= 0.9
        R.check(wit, tsdf, weight, occ)
        occ64, sure = R.occupancy(wit)
        total = obs * n_views
        if total <= 1.0:
            assert not occ.any()
        elif obs == 1.0:
            assert (occ64 & sure & wit.decided).any() and occ.any()
        elif obs * (n_views - 1) <= 1.0:      # 17 views at 1/16, 33 at 1/32: only the cells every view reaches
            assert (occ64 & sure & wit.decided).any() and occ.any() and (weight[occ] == F32(total)).all()


# ---------------------------------------------------------------------------------------------------------------------
# cell counts, through the C ABI on slices of guard-filled buffers
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 1024


def _guarded(n, fill, guard, dtype):
    buf = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, guard):
    return bool((buf[:GUARD] == guard).all()) and bool((buf[GUARD + n:] == guard).all())


def _raw_integrate(tsdf, weight, occ, dims, origin, voxel_size, depths, intrs, mats, trunc, obs, variant, n_views=None):
    from eprecon_amd import _lib
    lib = _lib.load()
    cdims = (ctypes.c_int32 * 3)(*dims)
    origin = np.ascontiguousarray(origin, F32)
    intrs, mats = np.ascontiguousarray(intrs, F32), np.ascontiguousarray(mats, F32)
    v, h, w = depths.shape
    return lib.eprecon_tsdf_integrate_async(
        _lib.ptr(tsdf), _lib.ptr(weight), ctypes.cast(cdims, ctypes.c_void_p), origin.ctypes.data_as(ctypes.c_void_p), float(voxel_size),
        _lib.ptr(depths), v if n_views is None else n_views, h, w, intrs.ctypes.data_as(ctypes.c_void_p), mats.ctypes.data_as(ctypes.c_void_p), float(trunc),
        float(obs), {"torch": 0, "cuda": 1}.get(variant, variant), _lib.ptr(occ), _lib.current_stream())


def _cells_scene(dims):
    """two views from the origin along +z onto a 64 x 48 image; the volume is centred in front of the camera, off every tie"""
    vs = 0.05
    origin = np.array([-(dims[0] - 1) * vs / 2 + 0.013, -(dims[1] - 1) * vs / 2 - 0.007, 1.03], F32)
    rng = np.random.default_rng(sum(dims))
    depths = rng.uniform(0.9, 1.3, size=(2, 48, 64)).astype(F32)
    depths[rng.random(depths.shape) < 0.1] = 0.0
    if dims[2] > 1:
        depths[1] += F32(0.25 * (dims[2] - 1) * vs)
    intr = np.array([[20.0, 0, 31.3], [0, 21.0, 23.4], [0, 0, 1]], F32)
    return vs, origin, depths, np.stack([intr, intr]), np.stack([EYE, EYE])


@pytest.mark.parametrize("variant", ["torch", "cuda"])
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 255), (1, 256, 1), (257, 1, 1), (3, 5, 7)])
def test_cell_counts_write_nothing_outside_the_volume(dims, variant):
    vs, origin, depths, intrs, mats = _cells_scene(dims)
    n = dims[0] * dims[1] * dims[2]
    tbuf, tsdf = _guarded(n, 1.0, -7.0, torch.float32)
    wbuf, weight = _guarded(n, 0.0, -7.0, torch.float32)
    obuf, occ = _guarded(n, 0x55, 0xAB, torch.uint8)
    trunc = 3 * vs
    assert _raw_integrate(tsdf, weight, occ, dims, origin, vs, torch.from_numpy(depths).cuda(), intrs, mats, trunc, 1.0, variant) == 0
    torch.cuda.synchronize()
    assert _guards_intact(tbuf, n, -7.0) and _guards_intact(wbuf, n, -7.0) and _guards_intact(obuf, n, 0xAB)
    wit = R.fuse(dims, origin, vs, depths, intrs, mats, trunc, 1.0, variant)
    assert wit.decided.mean() >= 0.9 and (wit.weight > 0).any()
    t, w, o = tsdf.cpu().numpy().reshape(dims), weight.cpu().numpy().reshape(dims), occ.cpu().numpy().reshape(dims)
    assert set(np.unique(o)) <= {0, 1}             # every byte of the volume written
    R.check(wit, t, w, o)
    assert np.array_equal(o.astype(bool), _rule(t, w))
    # without an occupancy buffer the volumes come out the same
    tbuf2, tsdf2 = _guarded(n, 1.0, -7.0, torch.float32)
    wbuf2, weight2 = _guarded(n, 0.0, -7.0, torch.float32)
    assert _raw_integrate(tsdf2, weight2, None, dims, origin, vs, torch.from_numpy(depths).cuda(), intrs, mats, trunc, 1.0, variant) == 0
    assert torch.equal(tbuf2, tbuf) and torch.equal(wbuf2, wbuf)


# ---------------------------------------------------------------------------------------------------------------------
# constructed decisions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["torch", "cuda"])
@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_constructed_decisions(name, variant):
    case = CONSTRUCTED[name]
    vol = _volume(case["dims"], case["origin"], case["voxel_size"], variant, margin=case["margin"])
    vol.integrate_views(torch.from_numpy(case["depths"]).cuda(), torch.from_numpy(case["intrs"]), torch.from_numpy(EYE[None]),
                        world2cam=EYE[None])
    tsdf, weight, occ = _host(vol)
    want_t, want_w = case["want"][variant]
    assert same_bits(tsdf, want_t), (tsdf.reshape(-1), want_t.reshape(-1))
    assert same_bits(weight, want_w), (weight.reshape(-1), want_w.reshape(-1))
    o_t, o_w = oracle_of_constructed(case, variant)
    assert same_bits(tsdf, o_t) and same_bits(weight, o_w)
    assert not occ.any()                                            # one view: weight 1
    # frame by frame through integrate(), with the pose inverted on the host (the inverse of the identity is the identity)
    two = _volume(case["dims"], case["origin"], case["voxel_size"], variant, margin=case["margin"])
    two.integrate(torch.from_numpy(case["depths"][0]).cuda(), torch.from_numpy(case["intrs"][0]), torch.from_numpy(EYE), 1.0)
    assert same_bits(two.get_volume()[0].cpu().numpy(), want_t) and same_bits(two.get_volume()[1].cpu().numpy(), want_w)


# ---------------------------------------------------------------------------------------------------------------------
# occupancy
# ---------------------------------------------------------------------------------------------------------------------
def test_occupancy_thresholds_device_byte_and_fallback():
    t999 = F32(0.999)
    below, above = np.nextafter(t999, F32(0)), np.nextafter(t999, F32(2))
    values = np.array([below, t999, above, -below, -t999, -above, 0.0, 1.0, -1.0], F32)
    inside = np.array([True, False, False, True, False, False, True, False, False])          # by hand: |t| < 0.999 is strict
    weights = np.array([0.0, 1.0, np.nextafter(F32(1), F32(2)), 2.0], F32)
    heavy = np.array([False, False, True, True])                                              # w > 1 is strict
    dims = (len(values), len(weights), 1)
    want = inside[:, None, None] & heavy[None, :, None]
    t0 = torch.from_numpy(np.broadcast_to(values[:, None, None], dims).copy()).cuda()
    w0 = torch.from_numpy(np.broadcast_to(weights[None, :, None], dims).copy()).cuda()
    nothing = torch.zeros((1, 2, 2), device="cuda")                                        # depth 0 everywhere: no cell is touched
    intr = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]])
    for variant in ("torch", "cuda"):
        vol = _volume(dims, (0, 0, 1), 0.25, variant, margin=4)
        vol.get_volume()[0].copy_(t0)
        vol.get_volume()[1].copy_(w0)
        vol.integrate_views(nothing, intr, torch.from_numpy(EYE[None]), world2cam=EYE[None])
        assert torch.equal(vol.get_volume()[0], t0) and torch.equal(vol.get_volume()[1], w0)
        assert np.array_equal(vol._occ.cpu().numpy(), want.astype(np.uint8))                 # the device byte
        assert np.array_equal(vol.occupancy().cpu().numpy(), want)
        vol.reset()
        assert vol._occ is None and not vol.occupancy().any()                                # fresh volume, Python fallback
        vol.get_volume()[0].copy_(t0)
        vol.get_volume()[1].copy_(w0)
        assert np.array_equal(vol.occupancy().cpu().numpy(), want)                           # the fallback on the same values


@pytest.mark.parametrize("variant", ["torch", "cuda"])
def test_weight_one_is_not_occupied_weight_two_is(variant):
    case = CONSTRUCTED["trunc"]
    vol = _volume(case["dims"], case["origin"], case["voxel_size"], variant, margin=case["margin"])
    args = (torch.from_numpy(case["depths"][0]).cuda(), torch.from_numpy(case["intrs"][0]), torch.from_numpy(EYE), 1.0)
    vol.integrate(*args)
    assert not vol.occupancy().any() and float(vol.get_volume()[1].max()) == 1.0
    vol.integrate(*args)
    tsdf, weight, occ = _host(vol)
    want_t, want_w = case["want"][variant]
    assert same_bits(tsdf, want_t) and same_bits(weight, 2 * want_w)      # (t + t) / 2 = t exactly
    # by hand: dist = -1, skipped, -1 + 2^-23, 1, 1 - 2^-22, 1, 1, 0.5 -> inside (-0.999, 0.999) is the last one only
    assert occ.reshape(-1).tolist() == [False] * 7 + [True]
    vol.reset()
    assert not vol.occupancy().any()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    case = CONSTRUCTED["tie_u"]
    dims = case["dims"]
    n = dims[0] * dims[1] * dims[2]
    depths = torch.from_numpy(case["depths"]).cuda()
    bufs = [_guarded(n, 1.0, -7.0, torch.float32), _guarded(n, 0.0, -7.0, torch.float32), _guarded(n, 0x55, 0xAB, torch.uint8)]
    before = [b.clone() for b, _ in bufs]
    tsdf, weight, occ = (s for _, s in bufs)

    def call(dims=dims, trunc=1.0, variant=0, n_views=None):
        return _raw_integrate(tsdf, weight, occ, dims, case["origin"], case["voxel_size"], depths, case["intrs"], EYE[None], trunc, 1.0,
                              variant, n_views)
    assert call(n_views=0) == ERR_ARG
    assert call(n_views=-1) == ERR_ARG
    assert call(trunc=0.0) == ERR_ARG
    assert call(trunc=-1.0) == ERR_ARG
    assert call(trunc=NAN) == ERR_ARG
    assert call(variant=2) == ERR_ARG
    assert call(variant=-1) == ERR_ARG
    for zero in ((0, 3, 1), (6, 0, 1), (6, 3, 0)):
        assert call(dims=zero) == ERR_UNSUPPORTED
    assert call(dims=(2048, 2048, 512)) == ERR_UNSUPPORTED   # 2^31 cells
    torch.cuda.synchronize()
    assert all(torch.equal(b, was) for (b, _), was in zip(bufs, before))
    assert call() == 0                                       # and the same arguments, valid, do run
    torch.cuda.synchronize()
    assert same_bits(tsdf.cpu().numpy().reshape(dims), case["want"]["torch"][0])
    assert all(_guards_intact(b, n, g) for (b, _), g in zip(bufs, (-7.0, -7.0, 0xAB)))

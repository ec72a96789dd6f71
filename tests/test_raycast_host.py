"""CPU, no library: tests/raycast_ref.py (the ray-cast rule of DESIGN.md §5b restated) held to cases worked out by hand, the
cap on the pixels it leaves out on every view the GPU tests use, and the measured distance of its float32 twin from float64,
which is where the GPU tolerances come from."""
import math

import numpy as np
import pytest

import raycast_fixtures as FX
import raycast_ref as R


def one_cell(shift=(0, 0, 0)):
    """samples of the cell `shift`: the face x = 0 reads 0.625 at y = 0 and 0.125 at y = 1, the face x = 1 reads -0.25
    (all exact in float32)"""
    coords, tsdf = [], []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                coords.append((shift[0] + dx, shift[1] + dy, shift[2] + dz))
                tsdf.append(-0.25 if dx else (0.125 if dy else 0.625))
    return R.row_dict(np.array(coords), np.array(tsdf, np.float32)), coords


def field(rows, p):
    """F at a lattice point p, straight from the definition (product weights, no shared expression with the reference)"""
    base = [math.floor(x) for x in p]
    total = 0.0
    for k in range(8):
        d = (k >> 2, (k >> 1) & 1, k & 1)
        w = 1.0
        for a in range(3):
            f = p[a] - base[a]
            w *= f if d[a] else 1.0 - f
        r = rows.get(tuple(base[a] + d[a] for a in range(3)))
        total += w * (1.0 if r is None else r[1])
    return total


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_single_cell_axis_parallel_ray(dtype):
    """The ray p = (-2 + t, 0.25, 0.75) enters the active box (cells 0 .. 1 in x) at t_0 = 2, where F = 0.625 * 0.75 + 0.125 *
    0.25 = 0.5; at the far plane x = 1 (t = 3) F = -0.25.  Along x the field is linear, 0.5 (1 - f) - 0.25 f, so the first
    interpolation is exact: f = 0.5 / 0.75 = 2/3 and depth = 2 + 2/3, and the refinement step changes nothing.  Gradient there:
    dF/dx = -0.25 - 0.5 = -0.75, dF/dy = (0.125 - 0.625) (1 - 2/3) = -1/6, dF/dz = 0; the normal is that vector normalised
    (it points back at the camera, towards positive F).  Nearest corner of (2/3, 0.25, 0.75): (1, 0, 1), row 5."""
    rows, coords = one_cell()
    hit = R.cast_ray(rows, R.active_box(rows), (-2.0, 0.25, 0.75), (1.0, 0.0, 0.0), dtype=dtype)
    tol = 1e-12 if dtype == np.float64 else 1e-6
    assert abs(hit.depth - (2.0 + 2.0 / 3.0)) < tol
    g = np.array([-0.75, -1.0 / 6.0, 0.0])
    assert np.allclose(hit.normal, g / np.linalg.norm(g), atol=tol)
    assert hit.row == coords.index((1, 0, 1)) == 5 and hit.cell == (0, 0, 0) and not hit.left_out
    assert R.active_box(rows) == ((0, -1, -1), (1, 1, 1))


def test_plus_minus_plus_inside_one_segment_is_not_seen():
    """Rows (0,0,z) = (1,1,z) = 0.2 and (1,0,z) = (0,1,z) = -1 for z = 0, 1; the ray p = (-1 + t, -1.1 + t, 0.3) crosses
    cell (0,0,0) between t = 1.1 (y = 0) and t = 2 (x = 1): F = 0.08 at both ends, negative in between (-0.406 at t = 1.55).
    Every other boundary sample of the ray is positive too: the rule sees no hit."""
    coords = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    rows = R.row_dict(np.array(coords), np.array([0.2 if x == y else -1.0 for x, y, _ in coords], np.float32))
    p0, d = (-1.0, -1.1, 0.3), (1.0, 1.0, 0.0)
    at = lambda t: [p0[a] + t * d[a] for a in range(3)]
    assert abs(field(rows, at(1.1 + 1e-12)) - 0.08) < 1e-6 and abs(field(rows, at(2.0 - 1e-12)) - 0.08) < 1e-6
    assert abs(field(rows, at(1.55)) + 0.406) < 1e-6
    for dtype in (np.float64, np.float32):
        hit = R.cast_ray(rows, R.active_box(rows), p0, d, dtype=dtype)
        assert hit.depth == 0.0 and hit.row == -1 and hit.normal == (0.0, 0.0, 0.0)


def test_start_inside_miss_and_far_plane():
    rows, _ = one_cell()
    box = R.active_box(rows)
    # znear = 2.9: F(t_0) = 0.5 * 0.1 - 0.25 * 0.9 < 0, the walk starts inside
    inside = R.cast_ray(rows, box, (-2.0, 0.25, 0.75), (1.0, 0.0, 0.0), znear=2.9)
    assert inside.depth == 0.0 and inside.row == -1
    # a ray beside the box, one that points away from it, and one cut short by zfar before the sign change
    for p0, d, far in (((-2.0, 5.25, 0.75), (1.0, 0.0, 0.0), 100.0), ((-2.0, 0.25, 0.75), (-1.0, 0.0, 0.0), 100.0),
                       ((-2.0, 0.25, 0.75), (1.0, 0.0, 0.0), 2.5)):
        miss = R.cast_ray(rows, box, p0, d, zfar=far)
        assert miss.depth == 0.0 and miss.row == -1 and miss.normal == (0.0, 0.0, 0.0)
    assert R.cast_ray(rows, None, (-2.0, 0.25, 0.75), (1.0, 0.0, 0.0)).row == -1        # no active cell at all


@pytest.mark.parametrize("d", [(1.0, 0.3, 0.0), (1.0, 0.0, -0.2), (0.8, 0.25, 0.1)])
def test_zero_direction_components_against_bisection(d):
    """one or no zero component: the depth is a root of the field along the ray, and the first one (bisection on `field`
    from a fine march); the normal is the field's numerical gradient there"""
    rows, _ = one_cell()
    p0 = (-2.0, 0.05, 0.8)
    at = lambda t: [p0[a] + t * d[a] for a in range(3)]
    hit = R.cast_ray(rows, R.active_box(rows), p0, d, refine=60)      # (regula falsi closes in from one side: linearly)
    ts = np.arange(0.05, 6.0, 1e-3)
    first = next(i for i, t in enumerate(ts) if field(rows, at(t)) <= 0.0)
    lo, hi = ts[first - 1], ts[first]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if field(rows, at(mid)) <= 0.0 else (mid, hi)
    assert abs(hit.depth - hi) < 1e-6
    p, h = at(hit.depth), 1e-6
    grad = np.array([(field(rows, [p[b] + (h if a == b else 0.0) for b in range(3)])
                      - field(rows, [p[b] - (h if a == b else 0.0) for b in range(3)])) / (2 * h) for a in range(3)])
    assert np.allclose(hit.normal, grad / np.linalg.norm(grad), atol=1e-5)


@pytest.mark.parametrize("shift", [(-7, -9, -4), (3, 7, -5), (-1, 0, 3)])
def test_negative_coordinates_and_brick_edges(shift):
    """the single cell moved: to negative coordinates, and to x = 3 | 4 (coordinates = 3 and 0 modulo 4: the positive and the
    negative face lie in different 4x4x4 bricks) — the same depth, normal and corner"""
    rows, coords = one_cell(shift)
    hit = R.cast_ray(rows, R.active_box(rows), (-2.0 + shift[0], 0.25 + shift[1], 0.75 + shift[2]), (1.0, 0.0, 0.0))
    assert abs(hit.depth - (2.0 + 2.0 / 3.0)) < 1e-12 and hit.cell == shift
    assert hit.row == coords.index((shift[0] + 1, shift[1], shift[2] + 1))
    g = np.array([-0.75, -1.0 / 6.0, 0.0])
    assert np.allclose(hit.normal, g / np.linalg.norm(g), atol=1e-12)


def test_view_rays_are_camera_z_depth():
    """t is the camera-z depth: a wall seen by a tilted camera has depth = z of the hit point in the camera frame"""
    coords = np.array([(x, y, z) for x in (10, 11) for y in range(-3, 27) for z in range(-3, 27)])
    tsdf = np.where(coords[:, 0] == 10, 0.5, -0.5).astype(np.float32)        # the wall x = 10.5
    rows = R.row_dict(coords, tsdf)
    pose = FX.look_at(FX.world([-12.3, 9.1, 14.2]), FX.world([10.5, 12.4, 11.3]))
    out = R.cast_view(rows, FX.intrinsics(9, 7), pose, 7, 9, FX.ORIGIN, FX.VOXEL)
    assert (out["row"] >= 0).all()
    p0, d = R.view_rays(FX.intrinsics(9, 7), pose, 7, 9, FX.ORIGIN, FX.VOXEL)
    hit_x = p0[0] + out["depth"] * d[..., 0]
    assert np.allclose(hit_x, 10.5, atol=1e-9)
    assert np.allclose(out["normal"], [-1.0, 0.0, 0.0], atol=1e-9)


def test_left_out_cap_and_float32_twin(capsys):
    """On every view the GPU tests compare, left_out (with the shading pixels within 1e-4 of a rounding step) covers at most
    2 %; outside it the float32 twin decides hit and row as float64 does, and its depth and normal differences are the figures
    the GPU tolerances are 4 x of (recorded in raycast_fixtures and DESIGN.md §7ao)."""
    worst_depth = worst_normal = 0.0
    for case, (scene, k, poses, h, w) in FX.CASES.items():
        s = FX.SCENES[scene]()
        for v, (a, b) in enumerate(zip(FX.reference(case), FX.reference(case, np.float32))):
            _, near = R.flat_shade(a["normal"], a["row"], k, poses[v])
            share = (a["left_out"] | near).mean()
            assert share <= FX.LEFT_OUT_CAP, (case, v, share)
            ok = ~a["left_out"]
            assert np.array_equal(a["row"][ok] >= 0, b["row"][ok] >= 0), (case, v)
            assert np.array_equal(a["row"][ok], b["row"][ok]), (case, v)
            worst_depth = max(worst_depth, float(np.abs(a["depth"] - b["depth"])[ok].max(initial=0.0)) / s["voxel_size"])
            worst_normal = max(worst_normal, float(np.abs(a["normal"] - b["normal"])[ok].max(initial=0.0)))
    with capsys.disabled():
        print(f"\n[raycast_ref] float32 twin against float64 outside left_out: depth {worst_depth:.3e} cells, "
              f"normal {worst_normal:.3e} per component")
    assert worst_depth <= FX.TWIN_DEPTH and worst_normal <= FX.TWIN_NORMAL
    assert 4 * FX.TWIN_DEPTH <= FX.DEPTH_CEILING and 4 * FX.TWIN_NORMAL <= FX.NORMAL_CEILING
    hits = sum(int((r["row"] >= 0).sum()) for case in FX.CASES for r in FX.reference(case))
    assert hits > 5000

"""The ray-cast rule of DESIGN.md §5b restated for the tests: numpy scalars and Python loops, a dict of rows, no code of the
package.  `dtype` carries the walk in float64 (Python floats) or in float32 (numpy.float32 scalars, every constant wrapped):
the float32 twin shows what the number format alone does to a result, which is where the GPU tolerances come from.

    rows = row_dict(coords, tsdf)                       # {(x, y, z): (row index, tsdf)}: of repeated coordinates the first
    cast_ray(rows, box, p0, d, znear, zfar, refine, dtype) -> Hit
    cast_view(rows, K, pose, height, width, origin, voxel_size, ...) -> {"depth", "normal", "row", "left_out"} arrays [H,W]

The rule.  F is the trilinear interpolation of the samples at the integer points of the lattice (world = origin + c *
voxel_size); a sample that is no row reads 1.  The ray of pixel (u, v) is p(t) = P0 + t D in lattice units with
D = R K^-1 (u + pixel_center, v + pixel_center, 1) / voxel_size, so t is the camera-z depth in metres.  It is cut at the
integer planes, t_plane(n) = (n - P0) * (1 / D) per axis, between t_0 = max(znear, entry into the box of the active cells) and
t_end = min(zfar, exit of that box); a cell is active when one of its corners is a row with tsdf <= 0.  F(t_0) <= 0: the walk
starts inside, nothing is hit.  Else the hit segment is the first whose far end has F <= 0; the depth is the regula-falsi point
of the two ends, refined `refine` times; the normal is the normalised gradient of the hit cell's trilinear polynomial there; the
row is the nearest corner of the hit cell that is a row (ties: the smallest (x, y, z)).

left_out marks the pixels float64 cannot decide: a boundary sample at or before the hit with |F| <= F_EPS, a hit segment with
g0 - g1 < SLOPE_EPS, two boundary parameters at or before the hit within a relative TIE_EPS, a fractional coordinate of the hit
point within HALF_EPS of 0.5, |grad F| < GRAD_EPS.
"""
import math
from collections import namedtuple

import numpy as np

F_EPS, SLOPE_EPS, TIE_EPS, HALF_EPS, GRAD_EPS = 1e-5, 1e-4, 1e-6, 1e-4, 1e-3

Hit = namedtuple("Hit", "depth normal row left_out cell")


def row_dict(coords, tsdf):
    rows = {}
    for i, (c, t) in enumerate(zip(np.asarray(coords).reshape(-1, 3).tolist(), np.asarray(tsdf, np.float32).tolist())):
        rows.setdefault(tuple(c), (i, t))
    return rows


def active_box(rows):
    """(lo, hi): the smallest and largest active cell per axis, or None"""
    neg = [c for c, (_, t) in rows.items() if t <= 0.0]
    if not neg:
        return None
    return tuple(min(c[k] for c in neg) - 1 for k in range(3)), tuple(max(c[k] for c in neg) for k in range(3))


def _corners(rows, cell, T):
    """values and row indices of the cell's corners, k = 4 dx + 2 dy + dz; None when no corner is a row (F = 1 there)"""
    vals, idx, any_row = [], [], False
    for k in range(8):
        r = rows.get((cell[0] + (k >> 2), cell[1] + ((k >> 1) & 1), cell[2] + (k & 1)))
        if r is None:
            vals.append(T(1.0))
            idx.append(-1)
        else:
            vals.append(T(r[1]))
            idx.append(r[0])
            any_row = True
    return (vals, idx) if any_row else None


def _trilinear(v, fx, fy, fz, one):
    ux, uy, uz = one - fx, one - fy, one - fz
    x00, x01 = v[0] * ux + v[4] * fx, v[1] * ux + v[5] * fx
    x10, x11 = v[2] * ux + v[6] * fx, v[3] * ux + v[7] * fx
    y0, y1 = x00 * uy + x10 * fy, x01 * uy + x11 * fy
    return y0 * uz + y1 * fz


def _gradient(v, fx, fy, fz, one):
    ux, uy, uz = one - fx, one - fy, one - fz
    gx = ((v[4] - v[0]) * uy + (v[6] - v[2]) * fy) * uz + ((v[5] - v[1]) * uy + (v[7] - v[3]) * fy) * fz
    gy = ((v[2] - v[0]) * ux + (v[6] - v[4]) * fx) * uz + ((v[3] - v[1]) * ux + (v[7] - v[5]) * fx) * fz
    gz = ((v[1] - v[0]) * ux + (v[5] - v[4]) * fx) * uy + ((v[3] - v[2]) * ux + (v[7] - v[6]) * fx) * fy
    return gx, gy, gz


def cast_ray(rows, box, p0, d, znear=0.05, zfar=100.0, refine=1, dtype=np.float64):
    """p0, d: the ray in lattice units (float64; cast to `dtype` here) -> Hit(depth or 0.0, normal (3 floats), row or -1,
    left_out, hit cell or None)"""
    T = float if dtype == np.float64 else dtype
    one, zero = T(1.0), T(0.0)
    miss = lambda left_out=False: Hit(0.0, (0.0, 0.0, 0.0), -1, left_out, None)
    if box is None:
        return miss()
    lo, hi = box
    P = [T(x) for x in p0]
    D = [T(x) for x in d]
    inv = [one / x if x != zero else None for x in D]
    plane = lambda n, k: (T(n) - P[k]) * inv[k]
    t0, t_end = T(znear), T(zfar)
    for k in range(3):
        if D[k] != zero:
            ta, tb = plane(lo[k], k), plane(hi[k] + 1, k)
            t0, t_end = max(t0, min(ta, tb)), min(t_end, max(ta, tb))
        elif not (T(lo[k]) <= P[k] <= T(hi[k] + 1)):
            return miss()
    if not t0 < t_end:
        return miss(abs(float(t0) - float(t_end)) <= TIE_EPS * abs(float(t_end)))
    # every plane crossing strictly between t_0 and t_end, by parameter
    cuts = []
    for k in range(3):
        if D[k] == zero:
            continue
        a, b = float(P[k]) + float(t0) * float(D[k]), float(P[k]) + float(t_end) * float(D[k])
        for n in range(math.floor(min(a, b)) - 1, math.ceil(max(a, b)) + 2):
            t = plane(n, k)
            if t0 < t < t_end:
                cuts.append(t)
    bounds = [t0] + sorted(cuts) + [t_end]
    left_out = False
    for k in range(1, len(bounds)):
        ta, tb = bounds[k - 1], bounds[k]
        if abs(float(tb) - float(ta)) <= TIE_EPS * abs(float(tb)):
            left_out = True
        mid = (float(ta) + float(tb)) * 0.5
        cell = tuple(math.floor(float(P[a]) + mid * float(D[a])) for a in range(3))
        corners = _corners(rows, cell, T)
        if corners is None:
            continue
        v, idx = corners
        off = [P[a] - T(cell[a]) for a in range(3)]
        F = lambda t: _trilinear(v, off[0] + t * D[0], off[1] + t * D[1], off[2] + t * D[2], one)
        a, ga = ta, F(ta)
        if abs(float(ga)) <= F_EPS:
            left_out = True
        x = None
        if ga <= zero:
            if k == 1:
                return miss(left_out)            # the walk starts inside
            x = a                                # (rounding between two cells' views of one face)
            left_out = True
        else:
            b, gb = tb, F(tb)
            if abs(float(gb)) <= F_EPS:
                left_out = True
            if gb <= zero:
                if float(ga) - float(gb) < SLOPE_EPS:
                    left_out = True
                x = a + (b - a) * (ga / (ga - gb))
                for _ in range(refine):
                    f = F(x)
                    if f <= zero:
                        b, gb = x, f
                    else:
                        a, ga = x, f
                    x = a + (b - a) * (ga / (ga - gb))
        if x is None:
            continue
        fx, fy, fz = off[0] + x * D[0], off[1] + x * D[1], off[2] + x * D[2]
        gx, gy, gz = _gradient(v, fx, fy, fz, one)
        length = T(math.sqrt(gx * gx + gy * gy + gz * gz)) if T is float else np.sqrt(gx * gx + gy * gy + gz * gz)
        normal = (float(gx / length), float(gy / length), float(gz / length)) if length > zero else (0.0, 0.0, 0.0)
        if float(length) < GRAD_EPS or any(abs(float(f) - 0.5) <= HALF_EPS for f in (fx, fy, fz)):
            left_out = True
        best, row = None, -1
        for c in range(8):
            if idx[c] < 0:
                continue
            ex, ey, ez = fx - T(c >> 2), fy - T((c >> 1) & 1), fz - T(c & 1)
            d2 = ex * ex + ey * ey + ez * ez
            if best is None or d2 < best:
                best, row = d2, idx[c]
        return Hit(float(x), normal, row, left_out, cell)
    return miss(left_out)


def view_rays(K, pose, height, width, origin, voxel_size, pixel_center=0.5):
    """-> (P0 float64[3], D float64[H,W,3]) in lattice units"""
    K, pose = np.asarray(K, np.float64).reshape(3, 3), np.asarray(pose, np.float64).reshape(4, 4)
    s = 1.0 / float(voxel_size)
    u, v = np.meshgrid(np.arange(width) + float(pixel_center), np.arange(height) + float(pixel_center))
    cam = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T
    return (pose[:3, 3] - np.asarray(origin, np.float64).reshape(3)) * s, (cam @ pose[:3, :3].T) * s


def cast_view(rows, K, pose, height, width, origin, voxel_size, znear=0.05, zfar=100.0, pixel_center=0.5, refine=1,
              dtype=np.float64, box="auto"):
    box = active_box(rows) if box == "auto" else box
    p0, d = view_rays(K, pose, height, width, origin, voxel_size, pixel_center)
    depth, normal = np.zeros((height, width)), np.zeros((height, width, 3))
    row, left_out = np.full((height, width), -1, np.int64), np.zeros((height, width), bool)
    for v in range(height):
        for u in range(width):
            h = cast_ray(rows, box, p0, d[v, u], znear, zfar, refine, dtype)
            depth[v, u], normal[v, u], row[v, u], left_out[v, u] = h.depth, h.normal, h.row, h.left_out
    return {"depth": depth, "normal": normal, "row": row, "left_out": left_out}


def flat_shade(normal, row, K, pose, colors=None, ambient=0.3, background=(255, 255, 255), pixel_center=0.5):
    """the flat rule on a cast_view result -> (uint8[H,W,3], near_half bool[H,W]: a channel's value before rounding is within
    1e-4 of x.5)"""
    h, w = row.shape
    K, pose = np.asarray(K, np.float64).reshape(3, 3), np.asarray(pose, np.float64).reshape(4, 4)
    u, v = np.meshgrid(np.arange(w) + float(pixel_center), np.arange(h) + float(pixel_center))
    d = (np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) @ pose[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    intensity = ambient + (1.0 - ambient) * np.abs((normal * d).sum(-1))
    c = np.full((h, w, 3), 153.0) if colors is None else np.asarray(colors, np.float64)[np.maximum(row, 0)]
    raw = c * intensity[..., None] + 0.5
    rgb = np.minimum(255.0, np.floor(raw)).astype(np.uint8)
    near = (np.abs(raw - np.round(raw)) <= 1e-4).any(-1) & (row >= 0)
    rgb[row < 0] = np.asarray(background, np.uint8)
    return rgb, near

"""Float64 witness of the TSDF integration (csrc/tsdf_fusion.hip), in plain numpy, written from the definition in the header of
oracle/tsdf_fusion.py (not from the kernel, and without calling the oracle).

Definition.  Voxel (ix, iy, iz) has the centre X = voxel_size * i + origin.  A view maps it to the camera point
    "torch":  c = M (X, 1), M = world->camera          "cuda":  c_j = sum_k P[k, j] (X_k - P[k, 3]), P = the camera pose
and to the pixel (u, v) = (fx c_x / c_z + cx, fy c_y / c_z + cy), rounded to the nearest integer (ties: to even in "torch", away
from zero in "cuda": only a tie tells them apart, and a tie is never decided here).  The view is integrated iff the point is in
front (c_z > 0; "cuda" c_z >= 0), the pixel lies in the image, its depth d is valid (d > 0; "cuda" d != 0) and
diff = d - c_z >= -trunc; then dist = min(1, diff / trunc), w' = w + obs, tsdf' = (w tsdf + obs dist) / w'.  A fresh volume is
tsdf = 1, w = 0.  Occupancy: |tsdf| < 0.999 and w > 1.
All inputs are the fp32 arrays the kernel gets, converted exactly, and the matrix is the one handed to the kernel; every
operation below is float64 (unit roundoff 2^-53, ignored against the fp32 terms).

Error bounds (U = 2^-24, the fp32 unit roundoff; nothing here is fitted to an observed error).  A running bound on sums of
absolute terms, one rounding per multiply / add / fma / division, as in the "Coordinates" paragraph of back_project_ref.py:
    t = i vs               e_t = U |t|
    X = t + o              e_X = e_t + U (|t| + |o| + e_t)
    "torch" c = fma chain  e_c = E + ((1+U)^4 - 1) (A + E),  A = sum_k |M_k| |X_k| + |M_3|,  E = sum_k |M_k| e_Xk  (mul + three fma)
    "cuda"  s = X - p      e_s = e_X + U (|X| + |p| + e_X)
            c = sum P s    e_c = E + ((1+U)^3 - 1) (A + E),  A = sum_k |P_k| |s_k|,  E = sum_k |P_k| e_sk  (three mul, two adds)
    "torch" a = fx c_x     e_a = fx e_x + U (|a| + fx e_x);   r = a / c_z: d = (e_a + |r| e_z) / (|c_z| - e_z), e_r = d + U (|r| + d)
            u = r + cx     e_u = e_r + U (|r| + |cx| + e_r)
    "cuda"  r = c_x / c_z  d = (e_x + |r| e_z) / (|c_z| - e_z), e_r = d + U (|r| + d);   a = fx r: e_a = fx e_r + U (|a| + fx e_r)
            u = a + cx     e_u = e_a + U (|a| + |cx| + e_a)
    diff = d - c_z         e_diff = e_z + U (|d| + |c_z|)
    dist = min(1, diff / trunc)    e_dist = e_diff / trunc + U |dist|;  0 where diff / trunc - e_diff / trunc >= 1 (clipped to 1
                                   on both sides of its band), and 0 for d = +Inf / NaN ("cuda": fminf), where dist = 1
e_u is evaluated where c_z > 2 e_z.

Decisions.  A (voxel, view) is DECIDED when no fp32 evaluation within these bounds can take another branch:
    c_z < -e_z                                                             (behind: skipped), or c_z > 2 e_z and then
    u < -1/2 - e_u, u > W - 1/2 + e_u, or the same for v                   (outside: skipped), or
    the distance of u (v) to the nearest k + 1/2 exceeds e_u (e_v)         (the pixel is certain; -1/2 and W - 1/2 are such k + 1/2)
    and: the pixel is outside, or its depth is invalid (the depth is read exactly), or is +-Inf / NaN, or |diff + trunc| > e_diff.
A voxel is decided when all its views are.

Values.  E is carried through the update (the two products, the sum and the division: four roundings):
    E' = (w E + obs e_dist) / w' + 4 U (|w tsdf| + |obs dist|) / w'.
On decided voxels: weight == weight64 exactly (w + obs is exact for the small dyadic weights in use), |tsdf - tsdf64| <= E, and the
occupancy agrees wherever ||tsdf64| - 0.999| > E.
"""
import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
F8 = np.float64
OCC_T = 0.999


def _f8(a):
    return np.asarray(a, np.float32).astype(F8)


def _centres(dims, origin, voxel_size):
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3).astype(F8)
    o = _f8(origin).reshape(3)
    t = g * float(np.float32(voxel_size))
    et = U * np.abs(t)
    return t + o, et + U * (np.abs(t) + np.abs(o) + et)


def _camera(X, eX, m, variant):
    """-> c, e_c float64[N, 3]"""
    if variant == "torch":
        R, p = m[:3, :3], m[:3, 3]
        c = X @ R.T + p
        A = np.abs(X) @ np.abs(R).T + np.abs(p)
        E = eX @ np.abs(R).T
        return c, E + ((1 + U) ** 4 - 1) * (A + E)
    R, p = m[:3, :3], m[:3, 3]
    s = X - p
    es = eX + U * (np.abs(X) + np.abs(p) + eX)
    c = s @ R                                               # c_j = sum_k P[k, j] s_k
    A = np.abs(s) @ np.abs(R)
    E = es @ np.abs(R)
    return c, E + ((1 + U) ** 3 - 1) * (A + E)


def _pixel(q, eq, z, ez, f, c, variant):
    """u = f q / z + c and its bound, where z > 2 e_z (NaN / inf elsewhere)"""
    f, ca = abs(f), abs(c)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ok = z > 2 * ez
        den = np.where(ok, np.abs(z) - ez, np.nan)
        if variant == "torch":
            a = f * q
            ea = f * eq + U * (np.abs(a) + f * eq)
            r = a / z
            d = (ea + np.abs(r) * ez) / den
            er = d + U * (np.abs(r) + d)
            return r + c, np.where(ok, er + U * (np.abs(r) + ca + er), np.inf)
        r = q / z
        d = (eq + np.abs(r) * ez) / den
        er = d + U * (np.abs(r) + d)
        a = f * r
        ea = f * er + U * (np.abs(a) + f * er)
        return a + c, np.where(ok, ea + U * (np.abs(a) + ca + ea), np.inf)


def _axis(u, eu, size):
    """-> pixel index (int64, -1 where off the image or not finite), certain (rounding decided), certainly outside"""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(u) & np.isfinite(eu)
        k = np.rint(np.where(fin, np.clip(u, -4.0, size + 4.0), -4.0))
        certain = fin & (0.5 - np.abs(np.where(fin, np.clip(u, -4.0, size + 4.0), -4.0) - k) > eu)
        outside = fin & ((u < -0.5 - eu) | (u > size - 0.5 + eu))
    k = k.astype(np.int64)
    return np.where((k >= 0) & (k < size), k, -1), certain, outside


def fuse(dims, origin, voxel_size, depths, intrs, mats, trunc, obs_weight=1.0, variant="torch"):
    """All views into a fresh volume.  depths f32[V, H, W]; intrs f32[V, 3, 3]; mats f32[V, 4, 4]: world->camera ("torch") or the
    camera poses ("cuda"); trunc as the kernel gets it (rounded to fp32).
    -> tsdf64, weight64, E float64[dims]; decided bool[dims]; views_undecided int[dims]"""
    dims = tuple(int(d) for d in dims)
    X, eX = _centres(dims, origin, voxel_size)
    n = X.shape[0]
    tr = float(np.float32(trunc))
    obs = float(np.float32(obs_weight))
    t, w, E = np.ones(n), np.zeros(n), np.zeros(n)
    undecided = np.zeros(n, np.int64)
    depths = np.asarray(depths, np.float32)
    V, H, W = depths.shape
    for v in range(V):
        m, K = _f8(mats[v]), _f8(intrs[v])
        c, ec = _camera(X, eX, m, variant)
        z, ez = c[:, 2], ec[:, 2]
        behind = z < -ez
        front = z > 2 * ez
        u, eu = _pixel(c[:, 0], ec[:, 0], z, ez, K[0, 0], K[0, 2], variant)
        vv, ev = _pixel(c[:, 1], ec[:, 1], z, ez, K[1, 1], K[1, 2], variant)
        px, cu, ou = _axis(u, eu, W)
        py, cv, ov = _axis(vv, ev, H)
        inside = front & (px >= 0) & (py >= 0)
        d = np.zeros(n)
        d[inside] = depths[v][py[inside], px[inside]].astype(F8)
        with np.errstate(invalid="ignore"):
            valid = (d > 0) if variant == "torch" else (d != 0)      # (NaN != 0: the "cuda" form lets NaN through)
            diff = d - z
            ediff = ez + U * (np.abs(d) + np.abs(z))
            fin = np.isfinite(d)
            keep = ~(diff < -tr)
            tdec = ~fin | (np.abs(diff + tr) > ediff)
            q = diff / tr
            dist = np.fmin(1.0, q)
            eq = ediff / tr
            edist = np.where(~fin | (q - eq >= 1.0), 0.0, eq + U * np.abs(dist))
        integ = inside & valid & keep
        decided = behind | (front & ((ou | ov) | (cu & cv & (~inside | ~valid | tdec))))
        undecided += ~decided
        wn = w + obs
        En = (w * E + obs * edist) / wn + 4 * U * (np.abs(w * t) + np.abs(obs * dist)) / wn
        tn = (w * t + obs * dist) / wn
        t, w, E = np.where(integ, tn, t), np.where(integ, wn, w), np.where(integ, En, E)
    r = lambda a: a.reshape(dims)
    return SimpleNamespace(tsdf=r(t), weight=r(w), E=r(E), decided=r(undecided == 0), views_undecided=r(undecided))


def occupancy(wit):
    """-> occ64, and where it is certain: ||tsdf64| - 0.999| > E (the weight is exact on decided voxels)"""
    return (np.abs(wit.tsdf) < OCC_T) & (wit.weight > 1), np.abs(np.abs(wit.tsdf) - OCC_T) > wit.E


def check(wit, tsdf, weight, occ=None):
    """The assertion on decided voxels -> the largest |tsdf - tsdf64| / E over them (0/0 = 0)"""
    dec = wit.decided
    tsdf, weight = np.asarray(tsdf), np.asarray(weight)
    assert tsdf.shape == wit.tsdf.shape and weight.shape == wit.tsdf.shape
    bad = dec & (weight.astype(F8) != wit.weight)
    assert not bad.any(), f"{int(bad.sum())} decided voxels with another weight, first at {np.argwhere(bad)[0]}"
    err = np.abs(tsdf.astype(F8) - wit.tsdf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(wit.E > 0, err / wit.E, np.where(err == 0, 0.0, np.inf))
    ratio = float(ratio[dec].max(initial=0.0))
    assert ratio <= 1.0, f"|tsdf - tsdf64| / E = {ratio}"
    if occ is not None:
        occ64, sure = occupancy(wit)
        sel = dec & sure
        assert np.array_equal(np.asarray(occ).astype(bool)[sel], occ64[sel])
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# The sweep cases the CPU and the GPU module share: eprecon_amd.synthetic windows (seed 3) with fy = 1.07 fx and H != W, on
# volumes that are not cubes, are no multiple of the workgroup, and (20 views) take two view chunks
# ---------------------------------------------------------------------------------------------------------------------
SWEEP = {
    "23x17x29": dict(dims=(23, 17, 29), voxel_size=0.16, views=9, width=160, height=120),
    "24x24x24": dict(dims=(24, 24, 24), voxel_size=0.16, views=9, width=97, height=61),
    "31x20x11": dict(dims=(31, 20, 11), voxel_size=0.12, views=20, width=160, height=120),
}
MARGIN = 3


@functools.lru_cache(maxsize=None)
def window_case(dims, voxel_size, views, width, height, seed=3):
    """-> dict(dims, origin f32[3], voxel_size, trunc, depths f32[V,H,W], intrs f32[V,3,3], poses f32[V,4,4], w2c f32[V,4,4])"""
    from eprecon_amd import synthetic as S
    window = S.make_window(seed=seed, width=width, height=height, n_views=views, n_vox=dims, voxel_size=voxel_size)
    k = window["intrinsics"].copy()
    k[1, 1] *= np.float32(1.07)
    window["intrinsics"] = k
    depths = np.stack([S.render_depth(window, v, holes_seed=100 + v) for v in range(views)])
    poses = window["poses"].astype(np.float32)
    w2c = np.stack([np.linalg.inv(p.astype(F8)).astype(np.float32) for p in poses])
    return dict(dims=tuple(dims), origin=window["vol_origin_partial"].astype(np.float32), voxel_size=voxel_size,
                trunc=MARGIN * float(voxel_size), depths=depths, intrs=np.repeat(k[None], views, 0).astype(np.float32),
                poses=poses, w2c=w2c)


def sweep_case(name):
    return window_case(**SWEEP[name])


def mats_of(case, variant):
    return case["w2c"] if variant == "torch" else case["poses"]

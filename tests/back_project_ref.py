"""Float64 witness of the multi-view back-projection (csrc/back_project.hip), in plain numpy, written from the definition of
the operation (not from the kernel and not from oracle/c/back_project_oracle.c).

Definition.  Voxel n = (b, cx, cy, cz) has the centre X = c * voxel_size + origin[b].  View v projects it with rows 0..2 of
its 4x4 matrix: (px, py, pz) = P[v, b] (X, 1); u = px / pz, v = py / pz (pixels); g = 2 u / (W - 1) - 1.  It is visible iff
|gx| <= 1, |gy| <= 1 and pz > 0.  s_v = the bilinear sample of map (v, b) at (u, v), align_corners=True, zero padding.
    mean      y = sum_vis s_v / max(cnt, 1)                  variance   y = sum_vis (s_v - m)^2 / max(cnt, 1), m = the mean
    depth     d = sum_vis pz / max(cnt, 1); per batch element over the kept rows with d > 0: mu = mean d,
              sigma = ||d - mu||_2 + 1e-5, channel C = (d - mu) / sigma, 0 where d <= 0
Rows with cnt >= min_view and 0 <= b < B are kept, in input order.  All inputs are the fp32 arrays the kernel gets, converted
exactly; every operation below is float64 (unit roundoff 2^-53, ignored against the fp32 terms).

Error bounds (U = 2^-24, the fp32 unit roundoff; nothing here is fitted to an observed error).

Coordinates.  A running first-order-plus analysis of the contract's fp32 chain, on sums of absolute terms:
    t = c vs            e_t = U |t|                                  (one rounding)
    X = t + o           e_X = e_t + U (|t| + |o| + e_t)
    p = fma chain       e_p = E + 4 U (A + E),  A = sum_k |P_k| |X_k| + |P_3|,  E = sum_k |P_k| e_Xk   (mul + three fma)
    u = px / pz         d = (e_px + |u| e_pz) / (|pz| - e_pz),  e_u = d + U (|u| + d)
    g = 2u/(W-1) - 1    e_g = k e_u + U (k|u| + k e_u) + U (k|u| + 1 + k e_u),  k = 2 / (W - 1)   (2u exact, division, subtraction)
    ix = (g+1)/2 (W-1)  e_ix = (e_g + U (2 + e_g)) / k;  e_ix += U ((W - 1) + e_ix)              (add, exact halving, multiply)
and the allowance the kernel documents for its reciprocal-and-Newton path, 1e-6 in normalised units:
    eu = e_ix + 1e-6 (W - 1) / 2      [pixels; ev likewise with H]
eu is evaluated where pz > 2 e_pz and is 0 elsewhere (such a view is never sampled).

Mean.  s_v is bilinear, so |s_v(u') - s_v(u)| <= |u' - u| Du + |v' - v| Dv with Du (Dv) the largest |difference of horizontal
(vertical) neighbours| over the 3 x 4 (4 x 3) cells around the sample point — the cell itself and its neighbours, so that a
fp32 coordinate that falls into the next cell is covered; the image is continued by zeros.  The arithmetic (weights, 4 fma,
cnt additions, one division) costs a few U of S = sum_vis sum_taps w |f| / cnt; the project's bound for such chains is
2^-16 S (tests/test_conv_families_gpu.py).  Hence
    |y - y64| <= 2^-16 S + sum_vis (eu Du + ev Dv) / cnt.
Variance.  d var / d s_v = 2 (s_v - m) / cnt (the mean's own variation cancels because sum (s_v - m) = 0), so with
delta_v = eu Du + ev Dv the coordinate term is sum_vis (2 |s_v - m| delta_v + (delta_v + mean delta)^2) / cnt; a rounding error
r_v <= a few U (S_v + M) in (s_v - m) (S_v, M the absolute forms of s_v and m) changes a square by <= 2 |s_v - m| r_v + r_v^2
<= a few U (S_v + M)^2, so the scale is S_var = sum_vis (S_v + M)^2 / cnt:   |var - var64| <= 2^-16 S_var + coordinate term.
Depth.  e_d = sum_vis e_pz / cnt + 2^-16 sum_vis |pz| / cnt per row.  With e_mu = mean e_d + 2^-16 mean |d| and
e_sigma = ||e_d + e_mu||_2 + 2^-16 sigma:   |z - z64| <= (e_d + e_mu) / sigma + |z| e_sigma / sigma + 2^-16 (|d| + |mu|) / sigma.
Adjoint (w.r.t. the maps; A^T of the sampling above).  Every (voxel, visible view, channel) adds w_tap * gv to its four taps,
    mean / depth  gv = dout / cnt             variance  gv = 2 (s_v - m) dvar / cnt + dmean / cnt.
Scale S_adj = sum w |gv|_abs with |gv|_abs = (2 (S_v + M) |dvar| + |dmean|) / cnt.  Each tap weight is 1-Lipschitz in u and in v,
and a coordinate that crosses a cell border moves weight <= (eu + ev) to a neighbouring element; so (eu + ev) |gv| is charged to
the 4 x 4 elements around the sample (box sum of the four taps' charge over 3 x 3).  In variance mode gv itself moves by
<= 2 (delta_v + mean delta) |dvar| / cnt, charged through the weights.  The deterministic form adds its fixed-point quantum, 2^-40
per contribution:   |df - df64| <= 2^-16 S_adj + position charge + value charge (+ 2^-40 * contributions).
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -16
BAND = 1e-4
MODE_MEAN, MODE_MEAN_DEPTH, MODE_VARIANCE = 0, 1, 2
F8 = np.float64


def geometry(coords, origin, voxel_size, kr, H, W, strict=False):
    """-> u, v, pz, gx, gy, vis, margin, eu, ev, epz: float64 / bool [V, N]; in_batch bool [N]"""
    c = np.asarray(coords).astype(np.int64)
    kr = np.asarray(kr, np.float32).astype(F8)
    V, B = kr.shape[:2]
    inb = (c[:, 0] >= 0) & (c[:, 0] < B)
    b = np.where(inb, c[:, 0], 0)
    vs = float(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(F8).reshape(-1, 3)[b]
    t = c[:, 1:4].astype(F8) * vs
    X = t + o
    eX = U * np.abs(t)
    eX = eX + U * (np.abs(t) + np.abs(o) + eX)
    P = kr[:, b, :3, :]                                               # [V, N, 3, 4]
    Xh = np.concatenate([X, np.ones((X.shape[0], 1))], axis=1)
    p = np.einsum("vnij,nj->ivn", P, Xh)
    A = np.einsum("vnij,nj->ivn", np.abs(P), np.abs(Xh))
    E = np.einsum("vnij,nj->ivn", np.abs(P[..., :3]), eX)
    ep = E + 4 * U * (A + E)
    px, py, pz = p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, v = px / pz, py / pz
        gx, gy = 2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1
        if strict:
            vis = (np.abs(gx) < 1) & (np.abs(gy) < 1) & (pz > 0)
        else:
            vis = (np.abs(gx) <= 1) & (np.abs(gy) <= 1) & (pz > 0)
        vis &= inb[None]
        margin = np.fmin(np.fmin(np.abs(np.abs(gx) - 1), np.abs(np.abs(gy) - 1)), np.abs(pz))
        margin = np.where(inb[None], margin, np.inf)
        ok = pz > 2 * ep[2]

        def pix_err(q, eq, size):
            k = 2.0 / (size - 1)
            d = (eq + np.abs(q) * ep[2]) / (np.abs(pz) - ep[2])
            e = d + U * (np.abs(q) + d)
            eg = k * e + U * (k * np.abs(q) + k * e) + U * (k * np.abs(q) + 1 + k * e)
            ei = (eg + U * (2 + eg)) / k
            ei = ei + U * ((size - 1) + ei)
            return np.where(ok, ei + 1e-6 * (size - 1) / 2, 0.0)
        eu, ev = pix_err(u, ep[0], W), pix_err(v, ep[1], H)
    return SimpleNamespace(u=u, v=v, pz=pz, gx=gx, gy=gy, vis=vis, margin=margin, eu=eu, ev=ev, epz=ep[2], in_batch=inb,
                           batch=b, H=H, W=W, V=V, B=B, coords=np.asarray(coords))


def in_band(G, band=BAND):
    """rows with a view whose decision lies within `band` of a frustum face"""
    return (G.margin <= band).any(axis=0)


def _maps(feats):
    """f32[V, B, C, H, W] -> float64 channels-last maps padded by 2 zeros, and the local Lipschitz tables"""
    F = np.asarray(feats).astype(F8).transpose(0, 1, 3, 4, 2)      # (fp32 maps convert exactly; float64 maps are taken as given)
    V, B, H, W, C = F.shape
    Fp = np.zeros((V, B, H + 4, W + 4, C))
    Fp[:, :, 2:-2, 2:-2] = F
    DX = np.abs(Fp[:, :, :, 1:] - Fp[:, :, :, :-1])                   # [H+4, W+3] edges
    DY = np.abs(Fp[:, :, 1:] - Fp[:, :, :-1])                         # [H+3, W+4]
    MX = np.zeros((V, B, H + 1, W + 1, C))
    MY = np.zeros((V, B, H + 1, W + 1, C))
    for r in range(4):
        for s in range(3):
            np.maximum(MX, DX[:, :, r:r + H + 1, s:s + W + 1], out=MX)
            np.maximum(MY, DY[:, :, s:s + H + 1, r:r + W + 1], out=MY)
    return Fp, MX, MY


def _taps(uu, vv, H, W):
    """cell, the four (padded y, padded x, weight) taps of a bilinear sample; taps off the image land in the zero border"""
    x0, y0 = np.floor(uu), np.floor(vv)
    fx, fy = uu - x0, vv - y0
    x0 = np.clip(x0, -2, W).astype(np.int64)
    y0 = np.clip(y0, -2, H).astype(np.int64)
    taps = [(y0 + 2, x0 + 2, (1 - fx) * (1 - fy)), (y0 + 2, x0 + 3, fx * (1 - fy)),
            (y0 + 3, x0 + 2, (1 - fx) * fy), (y0 + 3, x0 + 3, fx * fy)]
    return x0, y0, taps


def _sample_views(G, feats, vis, du=0.0):
    """per view: rows it is visible in, sample s, absolute form sa, coordinate sensitivity dl (all [rows, C])"""
    Fp, MX, MY = _maps(feats)
    H, W = G.H, G.W
    for v in range(G.V):
        rows = np.nonzero(vis[v])[0]
        if rows.size == 0:
            continue
        b = G.batch[rows]
        x0, y0, taps = _taps(G.u[v, rows] + du, G.v[v, rows], H, W)
        s = sa = 0.0
        for (yy, xx, w) in taps:
            f = Fp[v, b, yy, xx]
            s = s + w[:, None] * f
            sa = sa + w[:, None] * np.abs(f)
        xc, yc = np.clip(x0, -1, W - 1) + 1, np.clip(y0, -1, H - 1) + 1
        dl = G.eu[v, rows, None] * MX[v, b, yc, xc] + G.ev[v, rows, None] * MY[v, b, yc, xc]
        yield v, rows, s, sa, dl


def forward(G, feats, mode, min_view, vis=None, du=0.0, den_views=False):
    """The operation on every input row (callers index with `.valid`).  vis: visibility to evaluate with (default: the
    witness's own).  du / den_views: deliberately wrong variants for the sensitivity tests (u shifted by du pixels; the
    denominator V instead of the visible count).
    -> y, bound [N, C(+1)]; mean, mean_bound [N, C] (variance); cnt [N]; valid bool [N]; order = the kept rows"""
    vis = G.vis if vis is None else vis
    N, C = vis.shape[1], feats.shape[2]
    cnt = vis.sum(axis=0)
    den = np.full(N, float(G.V)) if den_views else np.maximum(cnt, 1).astype(F8)
    valid = G.in_batch & (cnt >= min_view)
    acc, accS, accD = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C))
    keep = []
    for v, rows, s, sa, dl in _sample_views(G, feats, vis, du):
        acc[rows] += s
        accS[rows] += sa
        accD[rows] += dl
        if mode == MODE_VARIANCE:
            keep.append((rows, s, sa, dl))
    m, M, Dm = acc / den[:, None], accS / den[:, None], accD / den[:, None]
    out = SimpleNamespace(cnt=cnt, valid=valid, order=np.nonzero(valid)[0], vis=vis)
    if mode == MODE_VARIANCE:
        var, Sv, Dv = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C))
        for rows, s, sa, dl in keep:
            d = s - m[rows]
            var[rows] += d * d
            Sv[rows] += (sa + M[rows]) ** 2
            Dv[rows] += 2 * np.abs(d) * dl + (dl + Dm[rows]) ** 2
        out.y, out.bound = var / den[:, None], (EPS * Sv + Dv) / den[:, None]
        out.mean, out.mean_bound = m, EPS * M + Dm
        return out
    out.y, out.bound = m, EPS * M + Dm
    if mode == MODE_MEAN_DEPTH:
        pz = np.where(vis, G.pz, 0.0)
        d = pz.sum(axis=0) / den
        ed = (np.where(vis, G.epz, 0.0).sum(axis=0) + EPS * np.abs(pz).sum(axis=0)) / den
        z, ez = np.zeros(N), np.zeros(N)
        for b in range(G.B):
            sel = valid & (G.batch == b) & (d > 0)
            if not sel.any():
                continue
            db, eb = d[sel], ed[sel]
            mu = db.mean()
            sigma = np.sqrt(((db - mu) ** 2).sum()) + 1e-5
            zb = (db - mu) / sigma
            emu = eb.mean() + EPS * np.abs(db).mean()
            esig = np.sqrt(((eb + emu) ** 2).sum()) + EPS * sigma
            z[sel] = zb
            ez[sel] = (eb + emu) / sigma + np.abs(zb) * esig / sigma + EPS * (np.abs(db) + abs(mu)) / sigma
        out.depth_raw = d
        out.y = np.concatenate([out.y, z[:, None]], axis=1)
        out.bound = np.concatenate([out.bound, ez[:, None]], axis=1)
    return out


def adjoint(G, feats, mode, dout, dmean=None, det=False):
    """A^T of forward() with respect to the maps, for the rows of G (the kept rows of a forward run): dout [N, >= C] (the
    first C columns are read), dmean [N, C] or None -> df, bound float64 [V, B, H, W, C] (channels-last, as the kernel's)"""
    V, B, H, W = G.V, G.B, G.H, G.W
    C = feats.shape[2]
    dout = np.asarray(dout).astype(F8)[:, :C]
    dmean = None if dmean is None else np.asarray(dmean).astype(F8)
    cnt = G.vis.sum(axis=0)
    den = np.maximum(cnt, 1).astype(F8)[:, None]
    df = np.zeros((V, B, H + 4, W + 4, C))
    bnd, pos = np.zeros_like(df), np.zeros_like(df)
    views = list(_sample_views(G, feats, G.vis))
    N = G.vis.shape[1]
    m, M, Dm = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C))
    for v, rows, s, sa, dl in views:
        m[rows] += s
        M[rows] += sa
        Dm[rows] += dl
    m, M, Dm = m / den, M / den, Dm / den
    for v, rows, s, sa, dl in views:
        g = dout[rows] / den[rows]
        if mode == MODE_VARIANCE:
            gm = 0.0 if dmean is None else dmean[rows] / den[rows]
            gv = 2 * (s - m[rows]) * g + gm
            ga = 2 * (sa + M[rows]) * np.abs(g) + np.abs(gm)
            gd = 2 * (dl + Dm[rows]) * np.abs(g)
        else:
            gv, ga, gd = g, np.abs(g), 0.0 * g
        b = G.batch[rows]
        x0, y0, taps = _taps(G.u[v, rows], G.v[v, rows], H, W)
        charge = (G.eu[v, rows] + G.ev[v, rows])[:, None] * ga
        for (yy, xx, w) in taps:
            np.add.at(df[v], (b, yy, xx), w[:, None] * gv)
            np.add.at(bnd[v], (b, yy, xx), w[:, None] * (EPS * ga + gd) + (2.0 ** -40 if det else 0.0) * (w[:, None] > 0))
            np.add.at(pos[v], (b, np.clip(yy, 2, H + 1), np.clip(xx, 2, W + 1)), charge)
    box = np.zeros_like(pos)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            box[:, :, 1:-1, 1:-1] += pos[:, :, 1 + dy:H + 3 + dy, 1 + dx:W + 3 + dx]
    inner = (slice(None), slice(None), slice(2, H + 2), slice(2, W + 2))
    return df[inner], (bnd + box)[inner]


# ---------------------------------------------------------------------------------------------------------------------
# The scenes the CPU and the GPU module share (eprecon_amd.synthetic windows at 320x240: 80x60 maps at level 0, 40x30 at 1)
# ---------------------------------------------------------------------------------------------------------------------
def _scene_table():
    t = {}
    for c in (24, 32, 40, 80, 4, 12, 44):
        t[f"mlp_c{c}"] = dict(seed=0, V=9, C=c)
    for v, b, c in ((21, 1, 24), (21, 1, 32), (32, 1, 40), (32, 1, 80), (32, 1, 12), (20, 2, 24), (20, 2, 44)):
        t[f"vec4_v{v}_b{b}_c{c}"] = dict(seed=3, lvl=1, V=v, B=b, C=c, n=(1000,) * b)
    for c in (1, 7, 13):
        t[f"vec1_c{c}"] = dict(seed=4, V=9, C=c)
    for n in (1, 15, 16, 17, 255, 256, 257, 16385, 49151, 49152):
        t[f"tile_n{n}"] = dict(seed=4, nvox=96, V=3, C=8, n=(n,))
    for n in (524287, 524288):
        t[f"tile_n{n}"] = dict(seed=0, nvox=96, interval=1, V=3, C=4, n=(n,))
    t["lds_v29"] = dict(seed=0, nvox=96, interval=1, V=29, C=4, n=(524288,))
    for v in (1, 2, 9, 20, 21, 31, 32):
        t[f"views_v{v}"] = dict(seed=3, V=v, C=8, n=(1500,))
    t["batch_b2"] = dict(seed=4, lvl=1, V=9, B=2, C=24, n=(70, 200))          # boundary inside a wave and a 16-row tile
    t["batch_b3"] = dict(seed=4, lvl=1, V=9, B=3, C=12, n=(100, 3, 300))       # one element of 3 rows
    t["bwd_c1"] = dict(seed=0, lvl=1, V=1, C=1, n=(700,))
    t["bwd_c7"] = dict(seed=3, lvl=1, V=9, C=7, n=(700,))
    t["bwd_c24"] = dict(seed=4, lvl=1, V=32, C=24, n=(300,))
    t["bwd_b2"] = dict(seed=4, lvl=1, V=9, B=2, C=7, n=(200, 333))
    return t


SCENES = _scene_table()


def scene(name=None, seed=0, nvox=32, interval=2, lvl=0, V=9, B=1, C=24, n=None, fseed=100, pick_seed=5):
    """-> dict(coords int32[N,4], origin f32[B,3], voxel_size, feats f32[V,B,C,H,W], kr f32[V,B,4,4]).  n: rows kept per batch
    element (a sorted random subset of the dense raster: a sparse list); batch element b sees the views rolled by b."""
    from eprecon_amd import synthetic as S
    if name is not None:
        return scene(**SCENES[name])
    window = S.make_window(seed=seed, width=320, height=240, n_views=V, n_vox=(nvox,) * 3)
    _, h, w = S.pyramid_shapes(240, 320)[lvl]
    feats = S.make_features(fseed + C, V, (C, h, w), batch=B)
    dense = S.dense_coords((nvox,) * 3, interval)
    rng = np.random.default_rng(pick_seed)
    parts = []
    for b in range(B):
        rows = dense if n is None else dense[np.sort(rng.choice(dense.shape[0], size=n[b], replace=False))]
        rows = rows.copy()
        rows[:, 0] = b
        parts.append(rows)
    proj = window["proj_matrices"][:, lvl]
    kr = np.ascontiguousarray(np.stack([np.roll(proj, b, axis=0) for b in range(B)], axis=1))
    origin = np.repeat(window["vol_origin_partial"][None], B, axis=0).copy()
    origin[:, 0] += 0.36 * np.arange(B, dtype=np.float32)
    return dict(coords=np.ascontiguousarray(np.concatenate(parts)), origin=origin, voxel_size=window["voxel_size"], feats=feats,
                kr=kr)


def geometry_of(sc, rows=None, strict=False):
    c = sc["coords"] if rows is None else sc["coords"][rows]
    return geometry(c, sc["origin"], sc["voxel_size"], sc["kr"], sc["feats"].shape[3], sc["feats"].shape[4], strict)


def band_stats(sc, chunk=65536):
    """(share of rows with a view inside the band, share of rows some view sees, the largest normalised coordinate error bound
    over the views that are visible or inside the band), evaluated in chunks of rows"""
    n = sc["coords"].shape[0]
    nb = nv = 0
    en = 0.0
    for i in range(0, n, chunk):
        G = geometry_of(sc, slice(i, i + chunk))
        near = G.margin <= BAND
        nb += int(near.any(axis=0).sum())
        nv += int(G.vis.any(axis=0).sum())
        with np.errstate(invalid="ignore"):   # views that can be sampled: visible, or undecided at a face in front of the camera
            face = np.abs(np.fmax(np.abs(G.gx), np.abs(G.gy)) - 1) <= BAND
        use = G.vis | (face & (G.pz > BAND))
        if use.any():
            en = max(en, float((G.eu * 2 / (G.W - 1))[use].max()), float((G.ev * 2 / (G.H - 1))[use].max()))
    return nb / max(n, 1), nv / max(n, 1), en


def exact_scene(C=8, V=3, fseed=77):
    """Pinhole views (focal lengths 8, 8 and 4 px, principal point at the map centre, 17 x 9 maps) of a 25 x 17 x 4 block of voxels
    of size 0.125 at depths -1, 0, 1 and 2: every product and sum of the fp32 chain is exact, so fp32 and float64 agree bit for
    bit and no decision lies in a band.  At depth 1 the voxels step through whole pixels from one step outside the left / top
    face (u = -4 .. 20, v = -4 .. 12) over u = 0, u = W - 1, v = 0, v = H - 1; at depth 2 through half pixels."""
    H, W = 9, 17
    shifts = [(0.0, 0.0, 0.0, 8.0), (0.5, 0.0, 0.0, 8.0), (0.0, -0.25, 0.0, 4.0)]
    shifts += [(0.125 * (k - 2) - 1.0, 0.125 * (k % 5 - 2), 0.0, 8.0 if k % 2 else 4.0) for k in range(3, V)]
    shifts = shifts[:V]
    kr = np.zeros((len(shifts), 1, 4, 4), np.float32)
    for v, (*t, f) in enumerate(shifts):
        k = np.array([[f, 0, (W - 1) / 2, 0], [0, f, (H - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        m = np.eye(4)
        m[:3, 3] = t
        kr[v, 0] = (k @ m).astype(np.float32)
    gx, gy, gz = np.meshgrid(np.arange(25), np.arange(17), np.array([0, 8, 16, 24]), indexing="ij")
    coords = np.stack([np.zeros(gx.size, np.int64), gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.int32)
    origin = np.array([[-1.5, -1.0, -1.0]], np.float32)
    feats = np.random.default_rng(fseed).standard_normal((len(shifts), 1, C, H, W), dtype=np.float32)
    return dict(coords=np.ascontiguousarray(coords), origin=origin, voxel_size=0.125, feats=feats, kr=kr)


def fp32_chain(sc):
    """u, v, pz of the contract's chain in fp32 (numpy float32: separate multiply and add; where every step is exact, as in
    exact_scene, this equals the fused form)"""
    f = np.float32
    c, kr = sc["coords"], sc["kr"].astype(f)
    X = [c[:, 1 + a].astype(f) * f(sc["voxel_size"]) + sc["origin"].astype(f)[c[:, 0], a] for a in range(3)]
    out = []
    for i in range(3):
        P = kr[:, c[:, 0], i, :]
        out.append(((P[..., 0] * X[0] + P[..., 1] * X[1]) + P[..., 2] * X[2]) + P[..., 3])
    with np.errstate(divide="ignore", invalid="ignore"):
        return out[0] / out[2], out[1] / out[2], out[2]

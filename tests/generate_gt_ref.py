"""Seeded inputs and float64 / brute-force restatements for the scene ground-truth tests (eprecon_amd/generate_gt.py), shared
by tests/golden/make_generate_gt_golden.py (build container, reference present) and tests/test_generate_gt_{host,gpu}.py.
numpy default_rng only; nothing here touches the reference tree.  tests/golden/generate_gt.npz stores OUTPUTS only."""
import numpy as np

from eprecon_amd import synthetic as S

VOXEL_SIZE = 0.04
NUM_LAYERS = 3


# ------------------------------------------------------------------------------------------------------------------
# bounds / level dimensions
# ------------------------------------------------------------------------------------------------------------------
def _pose(rng, yaw, pitch, eye):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, cp, -sp], [0, sp, cp]])
    p = np.eye(4)
    p[:3, :3] = rz @ rx
    p[:3, 3] = eye
    return p


# name -> (seed, frames, index of a frame with an infinite pose or None)
BOUNDS_CASES = {"many_frames": (11, 230, 57), "few_frames": (2, 12, None)}
BOUNDS_HW = (6, 8)


def bounds_case(name):
    """-> depths f32[n,6,8], cam_intr f64[3,3], poses f64[n,4,4]: a hand-held sweep whose extreme frames are NOT on the
    200-frame linspace subset in 'many_frames' (the generator asserts the subset changes the bounds)"""
    seed, n, bad = BOUNDS_CASES[name]
    rng = np.random.default_rng(seed)
    h, w = BOUNDS_HW
    intr = np.array([[7.3, 0, 3.4], [0, 7.1, 2.6], [0, 0, 1.0]])
    depths = rng.uniform(0.4, 3.0, (n, h, w)).astype(np.float32)
    poses = np.stack([_pose(rng, rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4), rng.uniform(-1.5, 1.5, 3)) for _ in range(n)])
    if bad is not None:
        poses[bad] = -np.inf
    return depths, intr, poses


def level_dims_f64(vol_bnds, voxel_size, num_layers):
    """float64 restatement of TSDFVolume.__init__'s dimension rule applied level after level to ONE array
    (tools/tsdf_fusion/fusion.py:44-47 as driven by generate_gt.py:148-149) -> [(dim int[3], origin f32[3])]"""
    b = np.array(vol_bnds, np.float64)
    out = []
    for l in range(num_layers):
        size = float(voxel_size * 2 ** l)
        dim = np.round((b[:, 1] - b[:, 0]) / size).astype(int)
        b[:, 1] = b[:, 0] + dim * size
        out.append((dim, b[:, 0].astype(np.float32)))
    return out


def naive_dims(vol_bnds, voxel_size, level):
    b = np.asarray(vol_bnds, np.float64)
    return np.round((b[:, 1] - b[:, 0]) / float(voxel_size * 2 ** level)).astype(int)


# ------------------------------------------------------------------------------------------------------------------
# fragment selection
# ------------------------------------------------------------------------------------------------------------------
FRAGMENT_ARGS = dict(window_size=3, min_angle=15, min_distance=0.1)
FRAGMENT_PITCH = -1.4          # the camera looks along the horizon: a yaw step turns the viewing direction by nearly as much


def fragment_case():
    """-> depths, cam_intr, poses, script: a scripted walk; script[i] names what frame i is meant to be
    ('first', 'inf', 'reject', 'angle', 'distance', 'both')"""
    rng = np.random.default_rng(21)
    script = ["first", "reject", "inf", "angle", "reject", "distance",            # window 0: frames 0, 3, 5
              "first", "reject", "reject", "both", "inf", "distance",             # window 1: frames 6, 9, 11
              "first", "angle", "reject", "distance",                             # window 2: frames 12, 13, 15
              "first", "reject", "angle", "reject"]                               # unfinished: dropped
    yaw, eye = 0.3, np.array([0.2, -0.1, 1.4])
    poses = []
    for kind in script:
        if kind == "inf":
            poses.append(np.full((4, 4), np.inf if len(poses) % 2 else -np.inf))
            continue
        if kind in ("angle", "both"):
            yaw += np.deg2rad(21.0)
        if kind in ("distance", "both"):
            eye = eye + np.array([0.13, 0.05, 0.0])
        if kind == "reject":      # a small wobble of the last taken pose, which itself stays the comparison base
            poses.append(_pose(rng, yaw + np.deg2rad(4.0), FRAGMENT_PITCH, eye + np.array([0.02, 0.01, 0.0])))
            continue
        poses.append(_pose(rng, yaw, FRAGMENT_PITCH, eye))
    h, w = BOUNDS_HW
    depths = rng.uniform(0.4, 3.0, (len(script), h, w)).astype(np.float32)
    intr = np.array([[7.3, 0, 3.4], [0, 7.1, 2.6], [0, 0, 1.0]])
    return depths, intr, np.stack(poses), script


# ------------------------------------------------------------------------------------------------------------------
# label volumes
# ------------------------------------------------------------------------------------------------------------------
LABEL_CASES = {"main": ((9, 7, 5), 31), "thin": ((6, 1, 4), 32)}
LABEL_VOL_MIN = np.array([-0.37, 0.125, -0.05])
# cells the 'main' case shapes by hand
CELL_EMPTY, CELL_ONE, CELL_64, CELL_256, CELL_TIE, CELL_TIE0 = (4, 3, 2), (1, 1, 1), (2, 5, 3), (6, 2, 1), (7, 4, 4), (3, 6, 0)


def cell_of(xyz, vol_min, voxel_size, dims):
    """generate_gt.py:199-202 restated: np.round (half to even) in float64, then the clip"""
    c = np.round((np.asarray(xyz, np.float64) - np.asarray(vol_min, np.float64)[None]) / voxel_size).astype(int)
    return np.stack([np.clip(c[:, k], 0, dims[k] - 1) for k in range(3)], 1)


def _points_in(rng, cell, n, vol_min, vs):
    return vol_min[None] + (np.asarray(cell)[None] + rng.uniform(-0.45, 0.45, (n, 3))) * vs


def label_case(name):
    """-> xyz f64[N,3], rgb f64[N,3], semantic int64[N], instance int64[N], vol_min f64[3], voxel_size, dims"""
    dims, seed = LABEL_CASES[name]
    rng = np.random.default_rng(seed)
    vs, vol_min = VOXEL_SIZE, LABEL_VOL_MIN
    ext = np.array(dims) * vs
    if name == "thin":
        n = 220
        xyz = vol_min[None] + rng.uniform(-0.2, 1.2, (n, 3)) * ext[None]
        sem, ins = rng.integers(0, 6, n), rng.integers(0, 300, n)
    else:
        n = 2600
        xyz = vol_min[None] + rng.uniform(-0.15, 1.08, (n, 3)) * ext[None]          # beyond every face
        sem, ins = rng.integers(0, 41, n), rng.integers(0, 400, n)
        shaped = [CELL_EMPTY, CELL_ONE, CELL_64, CELL_256, CELL_TIE, CELL_TIE0]
        cells = cell_of(xyz, vol_min, vs, dims)
        keep = ~np.any([np.all(cells == np.array(c)[None], 1) for c in shaped], 0)
        xyz, sem, ins = xyz[keep], sem[keep], ins[keep]
        extra = [(_points_in(rng, CELL_ONE, 1, vol_min, vs), [9], [301]),
                 (_points_in(rng, CELL_64, 100, vol_min, vs), rng.integers(1, 5, 100), rng.integers(250, 262, 100)),
                 (_points_in(rng, CELL_256, 300, vol_min, vs), rng.integers(0, 3, 300), rng.integers(0, 390, 300)),
                 (_points_in(rng, CELL_TIE, 2, vol_min, vs), [5, 3], [7, 7]),
                 (_points_in(rng, CELL_TIE0, 4, vol_min, vs), [7, 0, 0, 7], [300, 2, 300, 2])]
        # coordinates exactly on .5 of a cell (x axis): k + 0.5 for the k whose arithmetic gives the tie exactly
        half = []
        for k in range(dims[0] - 1):
            x = vol_min[0] + (k + 0.5) * vs
            if (x - vol_min[0]) / vs == k + 0.5:
                half.append([x, vol_min[1] + 2.2 * vs, vol_min[2] + 3.1 * vs])
        extra.append((np.array(half).reshape(-1, 3), np.full(len(half), 11), np.full(len(half), 333)))
        xyz = np.concatenate([xyz] + [e[0] for e in extra])
        sem = np.concatenate([sem] + [np.asarray(e[1]) for e in extra])
        ins = np.concatenate([ins] + [np.asarray(e[2]) for e in extra])
        perm = rng.permutation(len(xyz))           # the shaped cells' points are spread over the index range
        xyz, sem, ins = xyz[perm], sem[perm], ins[perm]
    rgb = rng.uniform(0, 255, (len(xyz), 3))
    return xyz, rgb, sem.astype(np.int64), ins.astype(np.int64), vol_min.copy(), vs, dims


# ------------------------------------------------------------------------------------------------------------------
# nearest-label fill
# ------------------------------------------------------------------------------------------------------------------
FILL_CASES = {"surface": ((40, 36, 28), 41), "odd": ((37, 29, 19), 42), "flat": ((5, 1, 64), 43)}


def fill_case(name):
    """int64[X,Y,Z]: a thinned surface — two planes and a box shell, 60 % kept, five labels (0 = no site)"""
    dims, seed = FILL_CASES[name]
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    vol = np.zeros(dims, np.int64)
    if name == "flat":
        vol[rng.random(dims) < 0.04] = 1
        vol[(rng.random(dims) < 0.04) & (z > 30)] = 4
        return vol
    vol[(z == 2) & (x < dims[0] * 0.7)] = 1                                     # a floor that stops short
    vol[(y == dims[1] - 3)] = 2                                                 # a wall
    lo, hi = np.array(dims) // 4, np.array(dims) * 5 // 8
    inside = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
    shell = inside & ((x == lo[0]) | (x == hi[0]) | (y == lo[1]) | (y == hi[1]) | (z == lo[2]) | (z == hi[2]))
    vol[shell & (x + y < lo[0] + lo[1] + 8)] = 3
    vol[shell & (x + y >= lo[0] + lo[1] + 8) & (z <= (lo[2] + hi[2]) // 2)] = 4
    vol[shell & (x + y >= lo[0] + lo[1] + 8) & (z > (lo[2] + hi[2]) // 2)] = 5
    vol[rng.random(dims) >= 0.6] = 0
    return vol


def fill_edge_case(name):
    dims = (13, 9, 21)
    rng = np.random.default_rng(47)
    vol = np.zeros(dims, np.int64)
    if name == "corner":
        vol[dims[0] - 1, 0, dims[2] - 1] = 6
    elif name == "face":
        vol[0] = rng.integers(0, 4, dims[1:])             # sites (and gaps) on the x = 0 face only
    elif name == "gaps":
        vol[:] = rng.integers(1, 6, dims) * (rng.random(dims) < 0.15)
        vol[4:7] = 0                                      # empty planes
        vol[:, 2] = 0
        vol[:, :, 10:15] = 0
        vol[9, 5, :] = 0                                  # an empty column beside full ones
    elif name != "zero":
        raise KeyError(name)
    return vol


def fill_bruteforce(vol, chunk=4096):
    """-> dmin int64[X,Y,Z] (exact squared distance to the nearest site), allowed bool[X,Y,Z,n_labels] (labels[k] has a site
    at that distance), labels int64[n_labels], rule int64[X,Y,Z] (the label the documented tie rule picks: among the
    nearest sites the smallest |dx|, the lower x, the smallest |dy|, the lower y, the smallest |dz|, the lower z).
    Every cell against every site: |c|^2 + |s|^2 - 2 c.s in float32, which is exact here (integers below 2^24)."""
    dims = vol.shape
    assert max(dims) <= 1024
    sites = np.argwhere(vol != 0).astype(np.int64)
    vals = vol[vol != 0].astype(np.int64)
    labels = np.unique(vals)
    lab_idx = np.searchsorted(labels, vals)
    cells = np.argwhere(np.ones(dims, bool)).astype(np.int64)
    cf, sf = cells.astype(np.float32), sites.astype(np.float32)
    cn, sn = (cf * cf).sum(1), (sf * sf).sum(1)
    dmin = np.zeros(len(cells), np.int64)
    allowed = np.zeros((len(cells), len(labels)), bool)
    rule = np.zeros(len(cells), np.int64)
    m = max(dims) + 1
    for c0 in range(0, len(cells), chunk):
        d = cn[c0:c0 + chunk, None] + sn[None, :] - 2.0 * (cf[c0:c0 + chunk] @ sf.T)
        dm = d.min(1)
        dmin[c0:c0 + chunk] = dm.astype(np.int64)
        rows, cols = np.nonzero(d == dm[:, None])                 # the nearest sites of every cell of the chunk
        allowed[c0 + rows, lab_idx[cols]] = True
        diff = np.abs(cells[c0 + rows] - sites[cols])
        assert np.array_equal((diff ** 2).sum(1), dmin[c0 + rows])
        key = np.zeros(len(rows), np.int64)
        for a in range(3):
            key = (key * m + diff[:, a]) * m + sites[cols, a]
        order = np.lexsort((key, rows))
        r_sorted = rows[order]
        first = np.r_[True, r_sorted[1:] != r_sorted[:-1]]
        rule[c0 + r_sorted[first]] = vals[cols[order][first]]
    return dmin.reshape(dims), allowed.reshape(dims + (len(labels),)), labels, rule.reshape(dims)


# ------------------------------------------------------------------------------------------------------------------
# a small scene: 20 frames at 60 x 80 of eprecon_amd.synthetic's room, 8 cm cells (level 0 about 48 x 40 x 24)
# ------------------------------------------------------------------------------------------------------------------
SCENE_VOXEL, SCENE_FRAMES, SCENE_HW, SCENE_MAX_DEPTH = 0.08, 20, (60, 80), 3.0


def scene_case():
    """-> depths f32[20,60,80] (values above 3 m zeroed, as the loader does), cam_intr f64[3,3], poses f64[20,4,4]: a slow
    arc (2.5 degrees and 6 cm per frame) through the room with a 60 degree lens"""
    h, w = SCENE_HW
    window = S.make_window(seed=3, width=w, height=h, n_views=SCENE_FRAMES)
    k = np.array([[70.0, 0, (w - 1) / 2.0], [0, 70.0, (h - 1) / 2.0], [0, 0, 1.0]])
    poses = []
    for v in range(SCENE_FRAMES):
        t = v - (SCENE_FRAMES - 1) / 2.0
        yaw, pitch = np.deg2rad(2.5 * t), np.deg2rad(-12.0)
        fwd = np.array([np.sin(yaw) * np.cos(pitch), np.cos(yaw) * np.cos(pitch), np.sin(pitch)])
        poses.append(S._look_at_pose(np.array([0.06 * t, -0.6, 1.5]), fwd))
    window = dict(window, intrinsics=k.astype(np.float32), poses=np.stack(poses).astype(np.float32))
    depths = np.stack([S.render_depth(window, v, holes_seed=300 + v) for v in range(SCENE_FRAMES)])
    depths[depths > SCENE_MAX_DEPTH] = 0
    return depths, window["intrinsics"].astype(np.float64), window["poses"].astype(np.float64)


def scene_cloud(depths, cam_intr, poses, every=4):
    """a labelled cloud sampled from the scene's surface: the valid pixels of every `every`-th frame back-projected, labelled
    with the nearest primitive of the analytic room (floor 2, walls 1, spheres 5 / 6 / 7; instance = primitive + 1)
    -> vertices f64[N,6] xyzrgb, semantic int64[N], instance int64[N]"""
    pts = []
    for v in range(0, len(depths), every):
        d = depths[v].astype(np.float64)
        vv, uu = np.nonzero(d > 0)
        z = d[vv, uu]
        cam = np.stack([(uu - cam_intr[0, 2]) / cam_intr[0, 0] * z, (vv - cam_intr[1, 2]) / cam_intr[1, 1] * z, z], 1)
        pts.append(cam @ poses[v][:3, :3].T + poses[v][:3, 3][None])
    p = np.concatenate(pts)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    prims = [z - 0.0, 3.4 - y, x + 1.7, 1.7 - x]
    prims += [np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r for cx, cy, cz, r in S.SCENE_SPHERES]
    nearest = np.argmin(np.abs(np.stack(prims)), axis=0)
    semantic = np.array([2, 1, 1, 1, 5, 6, 7], np.int64)[nearest]
    rgb = np.stack([40.0 + 30 * nearest, 128 + 100 * np.sin(3 * x), 128 + 100 * np.cos(2 * y)], 1)
    return np.concatenate([p, rgb], 1), semantic, (nearest + 1).astype(np.int64)

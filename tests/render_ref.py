"""float64 numpy restatement of view rendering (eprecon_amd/render.py, csrc/mesh_render.hip) — a test helper that shares no
code with the package: one face at a time over the whole image.

Per pixel: the nearest face by ray / plane depth among the faces that cover it, the corner of that face with the largest
perspective-correct weight, the labels and colour of that corner, the flat-shading value before rounding — and a mask of
the pixels LEFT OUT of a comparison because float64 cannot tell what the exact answer is there:

    the ray is within `rel` (relative) of an edge plane of a drawable face, at that edge (the other two edge tests do not
        rule the face out),
    the two nearest hits are within `rel` (relative) in depth,
    the two largest corner weights of the winning face are within `rel` (relative),
    a shaded channel's value before rounding is within `round_eps` of x.5.

Also here: the fixture scene of the render tests (cube + floor + a slanted quad through the cube, three views).
"""
import numpy as np

REL = 1e-6
ROUND_EPS = 1e-9
DEFAULT_COLOR = 153.0


def look_at(eye, target):
    """camera -> world 4x4 of a camera at `eye` looking at `target`: x right, y down, z forward, world z up"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def render_view(verts, faces, K, pose, height, width, labels=(), backgrounds=(), colors=None, ambient=0.3,
                background_rgb=(255, 255, 255), pixel_center=0.5, znear=0.05, zfar=100.0, cull_back=True, rel=REL,
                round_eps=ROUND_EPS):
    """-> dict: depth f64[H,W] (0 = no hit), face, corner int64[H,W] (-1), labels [int64[H,W]], shade f64[H,W,3] (the value
    before rounding; the background where nothing is hit), rgb uint8[H,W,3], left_out bool[H,W]"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    w2c = np.linalg.inv(np.asarray(pose, np.float64))
    vc = v @ w2c[:3, :3].T + w2c[:3, 3]
    kinv = np.linalg.inv(np.asarray(K, np.float64))
    uu, vv = np.meshgrid(np.arange(width) + float(pixel_center), np.arange(height) + float(pixel_center))
    d = np.stack([uu, vv, np.ones_like(uu)], -1) @ kinv.T
    dn = np.sqrt((d * d).sum(-1))
    shape = (height, width)
    best, second = np.full(shape, np.inf), np.full(shape, np.inf)
    face = np.full(shape, -1, np.int64)
    left = np.zeros(shape, bool)
    for fi, f in enumerate(faces):
        if (f < 0).any() or (f >= len(v)).any():
            continue
        a, b, c = vc[f[0]], vc[f[1]], vc[f[2]]
        z3 = np.array([a[2], b[2], c[2]])
        if z3.max() < znear or z3.min() > zfar:
            continue
        n = np.cross(b - a, c - a)
        nd = n @ a
        if nd == 0 or (cull_back and not nd < 0):
            continue
        edges = [np.cross(a, b), np.cross(b, c), np.cross(c, a)]
        s = np.stack([d @ e for e in edges])
        tol = np.stack([rel * np.linalg.norm(e) * dn for e in edges])
        near = np.abs(s) <= tol
        possible = (s >= -tol).all(0) | (s <= tol).all(0)
        left |= near.any(0) & possible
        cov = (s >= 0).all(0) | (s <= 0).all(0)
        with np.errstate(all="ignore"):
            z = nd / (d @ n) * d[..., 2]
        hit = cov & (z >= znear) & (z <= zfar)
        z = np.where(hit, z, np.inf)
        closer = z < best
        second = np.where(closer, best, np.minimum(second, z))
        face = np.where(closer, fi, face)
        best = np.where(closer, z, best)
    got = face >= 0
    with np.errstate(all="ignore"):
        left |= got & np.isfinite(second) & (second - best <= rel * best)
    corner = np.full(shape, -1, np.int64)
    shade = np.empty(shape + (3,), np.float64)
    shade[...] = np.asarray(background_rgb, np.float64)
    col = None if colors is None else np.asarray(colors, np.float64).reshape(-1, 3)
    for fi in np.unique(face[got]):
        m = face == fi
        f = faces[fi]
        a, b, c = vc[f[0]], vc[f[1]], vc[f[2]]
        dm = d[m]
        w = np.abs(np.stack([dm @ np.cross(b, c), dm @ np.cross(c, a), dm @ np.cross(a, b)], 1))
        slot = np.argmax(w, 1)                         # (first of equals: the earlier slot)
        ws = np.sort(w, 1)
        tie = ws[:, 2] - ws[:, 1] <= rel * ws[:, 2]
        corner[m] = f[slot]
        n = np.cross(b - a, c - a)
        cosine = np.abs(dm @ n) / (np.linalg.norm(n) * dn[m])
        intensity = ambient + (1.0 - ambient) * cosine
        base = np.full((len(dm), 3), DEFAULT_COLOR) if col is None else col[f[slot]]
        val = base * intensity[:, None]
        shade[m] = val
        frac = val + 0.5 - np.floor(val + 0.5)
        edge = (np.minimum(frac, 1.0 - frac) <= round_eps).any(1)
        left[m] |= tie | edge
    rgb = np.where(got[..., None], np.minimum(255.0, np.floor(shade + 0.5)), shade).astype(np.uint8)
    backgrounds = list(backgrounds) + [0] * (len(labels) - len(backgrounds))
    images = []
    for lab, bg in zip(labels, backgrounds):
        lab = np.asarray(lab, np.int64).reshape(-1)
        images.append(np.where(got, lab[np.maximum(corner, 0)] if len(lab) else bg, bg))
    return {"depth": np.where(got, best, 0.0), "face": face, "corner": corner, "labels": images, "shade": shade, "rgb": rgb,
            "left_out": left}


# ------------------------------------------------------------------------------------------------------------- the fixture

H, W = 48, 64
K_SMALL = np.array([[60.0, 0, 31.7], [0, 60.0, 23.3], [0, 0, 1]])
CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                   [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
FLOOR_V = np.array([[-3, -3, -0.8], [3, -3, -0.8], [3, 3, -0.8], [-3, 3, -0.8]], np.float32)
SLANT_V = np.array([[-1.2, -0.9, -0.7], [1.1, -1.0, 0.2], [1.0, 1.2, 0.9], [-1.1, 1.0, -0.1]], np.float32)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)          # counter-clockwise seen from +z: the normal points up


def fixture():
    """-> verts f32[16,3], faces int32[16,3], poses f64[3,4,4]: the unit cube, a floor quad at z = -0.8 spanning +-3 and a
    slanted quad that cuts through the cube; two views from outside and one from inside the cube"""
    verts = np.concatenate([CUBE_V, FLOOR_V, SLANT_V])
    faces = np.concatenate([CUBE_F, QUAD_F + 8, QUAD_F + 12]).astype(np.int32)
    poses = np.stack([look_at([1.6, -2.1, 1.2], [0.05, 0.0, -0.1]), look_at([-2.5, 0.3, 0.3], [0.0, 0.1, 0.0]),
                      look_at([0.1, -0.05, 0.12], [1.0, 0.3, 0.2])])
    return verts, faces, poses


def fixture_labels(n):
    """two per-vertex id arrays and a colour table for n vertices: distinct at every vertex, negative and large ids included"""
    i = np.arange(n, dtype=np.int64)
    sem = (i * 7 + 3) % 21
    ins = np.where(i % 5 == 0, -(i + 2), i * 100003 + 11)
    rng = np.random.default_rng(11)
    return sem.astype(np.int32), ins.astype(np.int32), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def patch(n=9, z=2.0, half=0.5):
    """a tessellated n x n-vertex patch (2 (n-1)^2 faces) facing the camera at the origin, gently curved: each face spans a
    few pixels of the fixture camera"""
    g = np.linspace(-half, half, n)
    x, y = np.meshgrid(g + 0.013, g * 0.8 - 0.021, indexing="ij")
    verts = np.stack([x, y, z + 0.3 * x * x - 0.2 * x * y + 0.1 * y], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(n - 1):
        for j in range(n - 1):
            p = i * n + j
            faces += [[p, p + 1, p + n + 1], [p, p + n + 1, p + n]]
    return verts, np.array(faces, np.int32)


# ------------------------------------------------------------------------------------------------------- the small scene

VOXEL = 0.04
ORIGIN = np.array([-0.5, -0.44, 0.1], np.float32)


def scene24(n=24):
    """an analytic TSDF of two merged balls on an n^3 grid with class-index and instance volumes split by planes (ids 0
    where the TSDF is 1, as a saved scene has them) -> (tsdf f32, semantic int32, instance int32, poses f64[4,4,4])"""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1)
    sdf = np.minimum(np.linalg.norm(g - [9.3, 10.1, 11.2], axis=-1) - 6.1, np.linalg.norm(g - [15.2, 13.4, 12.7], axis=-1) - 4.7)
    tsdf = np.clip(sdf / 3.0, -1.0, 1.0).astype(np.float32)
    x, y, z = g[..., 0], g[..., 1], g[..., 2]
    sem = np.where(x + 0.3 * y < 14.2, 1, np.where(z < 12.5, 5, 13))           # class indices: 1 is stuff (wall)
    ins = np.where(y < 11.5, 4, 9) + np.where(x + 0.3 * y < 14.2, 0, 20)
    seen = tsdf < 1.0
    sem, ins = np.where(seen, sem, 0).astype(np.int32), np.where(seen, ins, 0).astype(np.int32)
    centre = ORIGIN.astype(np.float64) + VOXEL * np.array([12.0, 11.5, 12.0])
    eyes = [[0.7, -0.6, 0.85], [-0.85, 0.13, 0.6], [0.2, 0.8, -0.33], [0.13, -0.9, 0.26]]
    poses = np.stack([look_at(centre + np.array(e), centre) for e in eyes])
    return tsdf, sem, ins, poses


def disagreeing_ground_truth(verts, faces, sem_ids, ins_ids):
    """a ground-truth mesh for the scene's mesh `verts`, `faces` with ScanNet ids `sem_ids`, instance ids `ins_ids` at its
    vertices that disagrees with it in every way the pixel domain counts: another class boundary, a void band (13 is no
    benchmark class), shifted instance ids, a hole in the surface (prediction, no ground truth) and a floor quad the
    prediction does not have (ground truth, no prediction) -> (verts, faces, semantic ids, instance ids)"""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    x = (verts[:, 0] - ORIGIN[0]) / VOXEL
    sem = np.where(x < 11.0, 1, np.where(x < 12.5, 13, sem_ids)).astype(np.int64)
    ins = np.where(verts[:, 2] > 0.6, np.asarray(ins_ids) + 1, ins_ids).astype(np.int64)
    centroid_y = verts[faces].mean(1)[:, 1]
    kept = faces[centroid_y > np.quantile(centroid_y, 0.12)]
    floor = np.array([[-0.62, -0.58, 0.2], [0.58, -0.58, 0.2], [0.58, 0.62, 0.2], [-0.62, 0.62, 0.2]], np.float32)
    n = len(verts)
    return (np.concatenate([verts, floor]), np.concatenate([kept, QUAD_F + n]).astype(np.int32),
            np.concatenate([sem, [2, 2, 2, 2]]), np.concatenate([ins, [0, 0, 0, 0]]))

"""float64 witness of the scene-mesh extraction (eprecon_amd/csrc/marching_cubes.hip) — test helper, numpy, vectorised.

oracle/marching_cubes.py stays the oracle for vertex positions and the face list (fp32, the kernel's own expressions).
This adds what that oracle cannot give:

  normals   g(p) by the kernel's rule (central differences, one-sided at the border with divisor max(xp - xm, 1)),
            n = g0 + t (g1 - g0), t = (level - v0) / (v1 - v0) from the fp32 voxel values, normalised, all in float64.
            With M = max(|g0|inf, |g1|inf) and L = |n|2 the bound per component is 2^-24 (32 M / L + 8): two gradient
            roundings, three in t and three in the interpolation are <= 9 roundings of size M on the unnormalised
            vector; normalising multiplies them by at most (1 + sqrt 3) / L and adds about 4 of its own.  Where L = 0
            exactly in float64 the expected output is the zero vector, exactly (the kernel's `len > 0` branch).
  winding   u = b - a, w = c - a from the fp32 vertices in float64, g the cell gradient from its eight corner values;
            d = (u x w) . g, s = sum_i P_i G_i with P_i the sum of the two absolute products of cross-product component i
            and G_i = 0.25 sum_k |val_k|.  A face is DECIDED when |d| > 2^-20 s (about 16 fp32 roundings relative to
            the magnitudes that enter); its triple must be the witness's.  The winding of an undecided face — one whose
            normal is perpendicular to the cell gradient within 2^-20 s — is unspecified: either order of its last two
            indices is accepted.
  cells     the cell of every face comes from re-walking the cells in raster order with the case table, as the oracle
            does — never from geometry (floor(min of the vertices) is wrong for faces on a cell's upper face).

VOLUMES is the one table of seeded test volumes: tests/test_mesh_ref.py checks the witness's two conditions on every
entry on the CPU, tests/test_mesh_extraction_gpu.py runs the same entries through the kernels.
"""
from collections import namedtuple

import numpy as np

import evaluation_ref
from oracle import marching_cubes as OM

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
DECIDED = 2.0 ** -20
BOUND_CAP, BOUND_SHARE = 1e-3, 0.01          # at most 1 % of a volume's vertices may have a normal bound above 1e-3
UNDECIDED_SHARE = 0.005                      # at most 0.5 % of a general-position volume's faces may be undecided

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = OM.build_table()[0]
    return _TABLE


# ---------------------------------------------------------------------------------------------------------------------
# the volumes
# ---------------------------------------------------------------------------------------------------------------------
def sign_volume(shape, seed):
    """uniform +-1: every crossing at t = 0.5, all arithmetic exact"""
    return np.where(np.random.default_rng(seed).random(shape) < 0.5, -1.0, 1.0).astype(F32)


def gauss_volume(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def clipped_volume(shape, seed):
    """+-1 plateaus (the TSDF default) beside the crossings, a few zero gradients"""
    return np.clip(1.5 * np.random.default_rng(seed).standard_normal(shape), -1, 1).astype(F32)


def on_level_volume(shape, seed):
    """gauss quantised to multiples of 1/8: many values equal the level exactly (t = 0, coincident vertices)"""
    return (np.rint(gauss_volume(shape, seed) * 8) / 8).astype(F32)


def blob_volume(shape, seed):
    """closed blobs (tests/test_marching_cubes.py: blob_volume), cut to `shape`"""
    n = 16
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).astype(F32)
    vol = np.full((n, n, n), 1e9, F32)
    for _ in range(4):
        c, r = rng.uniform(5, n - 6, 3), rng.uniform(2.0, 3.4)
        vol = np.minimum(vol, np.linalg.norm(g - c, axis=-1) - r)
    return np.clip(vol / 3.0, -1, 1).astype(F32)[: shape[0], : shape[1], : shape[2]].copy()


def border_volume(shape, seed):
    """positive everywhere but at some points of the six border planes: every crossing edge touches the border"""
    rng = np.random.default_rng(seed)
    vol = np.abs(rng.standard_normal(shape)).astype(F32) + F32(0.125)
    edge = np.zeros(shape, bool)
    for a in range(3):
        ix = [slice(None)] * 3
        for side in (0, -1):
            ix[a] = side
            edge[tuple(ix)] = True
    flip = edge & (rng.random(shape) < 0.3)
    vol[flip] = -vol[flip]
    return vol


# exact: every operation of the kernel is exact in fp32 (or the division is its only rounding), so the face list is
# compared with the oracle bit for bit and the undecided-share cap does not apply
Volume = namedtuple("Volume", "make shape seed levels exact")

VOLUMES = {
    "sign": Volume(sign_volume, (16, 16, 16), 7, (0.0,), True),
    "gauss": Volume(gauss_volume, (16, 16, 16), 7, (0.0, 0.25, -0.25), False),
    "gauss_9x17x12": Volume(gauss_volume, (9, 17, 12), 7, (0.0,), False),
    "clipped": Volume(clipped_volume, (16, 16, 16), 11, (0.0, -0.25), False),
    "on_level": Volume(on_level_volume, (16, 16, 16), 7, (0.0, 0.25), True),
    "blob_12x14x10": Volume(blob_volume, (12, 14, 10), 3, (0.0,), False),
    "blob": Volume(blob_volume, (16, 16, 16), 3, (0.0,), False),
    "border": Volume(border_volume, (6, 7, 5), 7, (0.0,), False),
    # shapes: the smallest volume; one cell thick in each axis pair; 105 points (no multiple of 256); exactly one
    # 2,048-element scan tile; just above one tile; 8 x 16 x 16 and one more row
    "gauss_2x2x2": Volume(gauss_volume, (2, 2, 2), 7, (0.0,), False),
    "gauss_2x2x9": Volume(gauss_volume, (2, 2, 9), 7, (0.0,), False),
    "gauss_2x9x2": Volume(gauss_volume, (2, 9, 2), 7, (0.0,), False),
    "gauss_9x2x2": Volume(gauss_volume, (9, 2, 2), 7, (0.0,), False),
    "gauss_3x5x7": Volume(gauss_volume, (3, 5, 7), 7, (0.0,), False),
    "gauss_2x32x32": Volume(gauss_volume, (2, 32, 32), 7, (0.0,), False),
    "gauss_2x25x41": Volume(gauss_volume, (2, 25, 41), 7, (0.0,), False),
    "gauss_9x16x16": Volume(gauss_volume, (9, 16, 16), 7, (0.0,), False),
}
SHAPES = [k for k in VOLUMES if k.startswith("gauss_") and k != "gauss_9x17x12"]
CASES = [(name, level) for name, v in VOLUMES.items() for level in v.levels]

_volumes, _oracle = {}, {}


def volume(name):
    """the named volume (built once; read-only)"""
    if name not in _volumes:
        v = VOLUMES[name]
        _volumes[name] = v.make(v.shape, v.seed)
        _volumes[name].setflags(write=False)
    return _volumes[name]


def label_volumes(shape):
    """two int32 label volumes; the ranges are wide, so that neighbouring voxels rarely share a label"""
    rng = np.random.default_rng(shape[0] + 31 * shape[1] + 977 * shape[2])
    return rng.integers(0, 21, shape).astype(np.int32), rng.integers(0, 1 << 20, shape).astype(np.int32)


def oracle(vol, level):
    """oracle.marching_cubes.marching_cubes(vol, level), computed once per (volume, level)"""
    key = (vol.shape, vol.tobytes(), float(level))
    if key not in _oracle:
        _oracle[key] = OM.marching_cubes(vol, level, table())
        for a in _oracle[key]:
            a.setflags(write=False)
    return _oracle[key]


# ---------------------------------------------------------------------------------------------------------------------
# the raster walks
# ---------------------------------------------------------------------------------------------------------------------
def cell_cases(vol, level):
    """-> int[dx-1, dy-1, dz-1] sign case of every cell (bit k: corner k = (k & 1, (k >> 1) & 1, k >> 2) below the level)"""
    vol = np.asarray(vol, F32)
    dx, dy, dz = vol.shape
    inside = vol < F32(level)
    cs = np.zeros((dx - 1, dy - 1, dz - 1), np.int64)
    for k in range(8):
        a, b, c = k & 1, (k >> 1) & 1, k >> 2
        cs |= inside[a:a + dx - 1, b:b + dy - 1, c:c + dz - 1].astype(np.int64) << k
    return cs


def face_cells(vol, level):
    """-> int[M, 3] cell (x, y, z) of every face, in the face list's order: the cells in raster order, each as often as
    its table row has triangles"""
    cs = cell_cases(vol, level)
    nt = (table()[:, 0:15:3] >= 0).sum(1)
    flat = np.repeat(np.arange(cs.size), nt[cs].reshape(-1))
    return np.stack(np.unravel_index(flat, cs.shape), 1).reshape(-1, 3)


def vertex_edges(vol, level):
    """-> int[N, 4] (x, y, z, axis) of the grid edge every vertex lies on, in the vertex list's order (point raster,
    axis x < y < z)"""
    vol = np.asarray(vol, F32)
    inside = vol < F32(level)
    cut = np.zeros(vol.shape + (3,), bool)
    cut[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cut[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cut[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return np.argwhere(cut)


def gradient64(vol):
    """-> f64[dx, dy, dz, 3] the kernel's gradient(): central differences, one-sided at the border"""
    v = np.asarray(vol, F32).astype(F64)
    g = np.zeros(v.shape + (3,))
    for a in range(3):
        i = np.arange(v.shape[a])
        lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, v.shape[a] - 1)
        div = np.maximum(hi - lo, 1).astype(F64)
        bc = [None] * 3
        bc[a] = slice(None)
        g[..., a] = (np.take(v, hi, axis=a) - np.take(v, lo, axis=a)) / div[tuple(bc)]
    return g


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
Normals = namedtuple("Normals", "n bound L")
Winding = namedtuple("Winding", "faces decided d s")


def normals(vol, level):
    """-> Normals(n f64[N,3] expected, bound f64[N] per component (inf where 0 < L underflows it), L f64[N])"""
    vol = np.asarray(vol, F32)
    e = vertex_edges(vol, level)
    p0, axis = e[:, :3], e[:, 3]
    p1 = p0.copy()
    p1[np.arange(len(e)), axis] += 1
    v = vol.astype(F64)
    v0, v1 = v[tuple(p0.T)], v[tuple(p1.T)]
    t = (F64(F32(level)) - v0) / (v1 - v0)
    g = gradient64(vol)
    g0, g1 = g[tuple(p0.T)], g[tuple(p1.T)]
    n = g0 + t[:, None] * (g1 - g0)
    L = np.sqrt((n * n).sum(1))
    M = np.maximum(np.abs(g0).max(1, initial=0.0), np.abs(g1).max(1, initial=0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where(L[:, None] > 0, n / L[:, None], 0.0)
        bound = np.where(L > 0, EPS * (32.0 * M / L + 8.0), 0.0)
    return Normals(unit, bound, L)


def winding(vol, level, verts, faces):
    """verts f32[N,3], faces int[M,3] (either order of the last two) -> Winding(faces wound along the cell gradient,
    decided bool[M], d, s)"""
    vol = np.asarray(vol, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cell = face_cells(vol, level)
    assert len(cell) == len(faces), (len(cell), len(faces))
    v = vol.astype(F64)
    val = [v[cell[:, 0] + (k & 1), cell[:, 1] + ((k >> 1) & 1), cell[:, 2] + (k >> 2)] for k in range(8)]
    g = 0.25 * np.stack([(val[1] + val[3] + val[5] + val[7]) - (val[0] + val[2] + val[4] + val[6]),
                         (val[2] + val[3] + val[6] + val[7]) - (val[0] + val[1] + val[4] + val[5]),
                         (val[4] + val[5] + val[6] + val[7]) - (val[0] + val[1] + val[2] + val[3])], 1)
    G = 0.25 * sum(np.abs(x) for x in val) if len(faces) else np.zeros(0)
    p = np.asarray(verts, F32).astype(F64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    u, w = b - a, c - a
    d = (np.cross(u, w) * g).sum(1)
    P = (np.abs(u[:, [1, 2, 0]] * w[:, [2, 0, 1]]) + np.abs(u[:, [2, 0, 1]] * w[:, [1, 2, 0]])).sum(1)
    s = P * G
    wound = np.where((d < 0)[:, None], faces[:, [0, 2, 1]], faces)
    return Winding(wound.astype(np.int32), np.abs(d) > DECIDED * s, d, s)


def vertex_labels(verts, labels):
    """utils.py:236-239: labels of the nearest voxel, np.rint (half to even), clipped into the volume"""
    r = np.clip(np.rint(np.asarray(verts, F32)).astype(np.int64), 0, np.array(labels.shape) - 1)
    return labels[r[:, 0], r[:, 1], r[:, 2]]


def conditions(vol, level):
    """-> (share of vertices whose normal bound exceeds BOUND_CAP, share of undecided faces, vertices with L = 0)"""
    ov, of = oracle(vol, level)
    nr, wd = normals(vol, level), winding(vol, level, ov, of)
    return (float((nr.bound > BOUND_CAP).mean()) if len(ov) else 0.0, float((~wd.decided).mean()) if len(of) else 0.0,
            int((nr.L == 0).sum()))


def emulated(vol, level, weight=None, labels=()):
    """what the kernels are written to give, from numpy: the oracle's vertices and faces, the normals by the kernel's
    formula with every operation rounded to fp32, the labels by the np.rint rule; the masked form through
    evaluation_ref.masked_mesh.  Stands in for the GPU's output in the CPU tests."""
    vol = np.asarray(vol, F32)
    ov, of = oracle(vol, level)
    e = vertex_edges(vol, level)
    p0, axis = e[:, :3], e[:, 3]
    p1 = p0.copy()
    p1[np.arange(len(e)), axis] += 1
    g = np.zeros(vol.shape + (3,), F32)
    for a in range(3):
        i = np.arange(vol.shape[a])
        lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, vol.shape[a] - 1)
        bc = [None] * 3
        bc[a] = slice(None)
        g[..., a] = (np.take(vol, hi, axis=a) - np.take(vol, lo, axis=a)) / np.maximum(hi - lo, 1).astype(F32)[tuple(bc)]
    v0, v1 = vol[tuple(p0.T)], vol[tuple(p1.T)]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((F32(level) - v0) / (v1 - v0)).astype(F32)
        g0, g1 = g[tuple(p0.T)], g[tuple(p1.T)]
        n = (g0 + t[:, None] * (g1 - g0)).astype(F32)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F32)
        n = np.where(ln[:, None] > 0, n / ln[:, None], n).astype(F32)
    labs = [vertex_labels(ov, l) for l in labels]
    if weight is None:
        return (ov.copy(), of.copy(), n) + tuple(labs)
    keep = evaluation_ref.masked_mesh(vol, weight, ov, of, table())[2]
    return restrict((ov, of, n) + tuple(labs), keep)


def restrict(mesh, keep):
    """(verts, faces, normals, *labels) -> the same with the faces outside `keep` dropped, the vertices that no remaining
    face uses dropped and the faces renumbered; order kept"""
    verts, faces = mesh[0], mesh[1]
    f = faces[keep]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return (verts[used], remap[f].astype(np.int32).reshape(-1, 3)) + tuple(a[used] for a in mesh[2:])


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def compare(got, volume, level, weight=None, labels=()):
    """got = (verts f32[N,3], faces int32[M,3], normals f32[N,3], one int32[N] per volume of `labels`) as numpy arrays, the
    output of save_scene.marching_cubes(volume, level, labels, weight).  Asserts: vertices bit-equal to the oracle; every
    face's first index and the set of its last two equal to the oracle's, every decided face wound as the witness winds it;
    normals within the bound of the witness (exactly zero where L = 0); labels equal to labels[clip(np.rint(v))].  With
    `weight` (level 0 only) the expected mesh is evaluation_ref.masked_mesh's restriction.
    -> {"normal": worst normal error / bound, "undecided": share of undecided faces, "winding_differs": faces the GPU and
    the fp32 oracle wound differently, "verts", "faces"}"""
    vol = np.asarray(volume, F32)
    verts, faces, nrm = (np.asarray(a) for a in got[:3])
    ov, of = oracle(vol, level)
    nr = normals(vol, level)
    wd = winding(vol, level, ov, of)
    want_n, bound, wound, decided = nr.n, nr.bound, wd.faces, wd.decided
    if weight is not None:
        assert float(level) == 0.0, "masked_mesh restates the masked form at level 0"
        mv, mf, keep = evaluation_ref.masked_mesh(vol, np.asarray(weight, F32), ov, of, table())
        used = np.zeros(len(ov), bool)
        used[of[keep].reshape(-1)] = True
        remap = np.cumsum(used) - 1
        ov, of, want_n, bound = mv, mf.reshape(-1, 3), want_n[used], bound[used]
        wound, decided = remap[wound[keep]].astype(np.int32).reshape(-1, 3), decided[keep]
    assert verts.dtype == F32 and faces.dtype == np.int32 and nrm.dtype == F32
    assert verts.shape == ov.shape and faces.shape == of.shape and nrm.shape == ov.shape, \
        (verts.shape, ov.shape, faces.shape, of.shape, nrm.shape)
    assert np.array_equal(verts.view(np.int32), ov.view(np.int32)), "vertices differ from the oracle"
    # faces: the kernel only ever swaps the last two indices
    assert np.array_equal(faces[:, 0], of[:, 0]) and np.array_equal(np.sort(faces[:, 1:], 1), np.sort(of[:, 1:], 1)), \
        "face indices differ from the oracle"
    bad = decided & (faces != wound).any(1)
    assert not bad.any(), f"{int(bad.sum())} decided faces wound against the cell gradient, first {np.flatnonzero(bad)[:5]}"
    differs = (faces != of).any(1)
    assert not (differs & decided).any() and differs.sum() <= (~decided).sum()
    # normals
    err = np.abs(nrm.astype(F64) - want_n).max(1, initial=0.0)
    assert np.isfinite(nrm).all()
    zero = bound == 0
    assert (err[zero] == 0).all(), "a vertex with a zero gradient must have the zero vector as its normal"
    ratio = float((err[~zero] / bound[~zero]).max(initial=0.0))
    assert ratio <= 1.0, f"normals: worst error / bound {ratio:.3g} at vertex {int(np.flatnonzero(~zero)[np.argmax(err[~zero] / bound[~zero])])}"
    # labels
    assert len(got) == 3 + len(labels)
    for out, lab in zip(got[3:], labels):
        out = np.asarray(out)
        assert out.dtype == np.int32 and np.array_equal(out, vertex_labels(ov, np.asarray(lab))), "vertex labels differ"
    return {"normal": ratio, "undecided": float((~decided).mean()) if len(of) else 0.0,
            "winding_differs": int(differs.sum()), "verts": len(ov), "faces": len(of)}

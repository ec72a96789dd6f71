"""Seeded inputs and independent restatements for the fragment ground-truth transform (eprecon_amd/transforms.py,
csrc/gt_crop.hip): the sample layout of tests/golden/transform_space.npz, the crop rule in float64 numpy, the same rule
through torch's CPU grid_sample, and the set of voxels a comparison may leave out.

The rule (datasets/transforms.py:263-359 of the reference): output voxel i of level l samples the scene volume of that level at
    c = (M @ [i 2^l vs + origin_partial, 1] - old_origin) / vs / 2^l,   n = 2 c / (D - 1) - 1,   u = ((n + 1) D - 1) / 2
labels / colour: the cell rint(u), 0 outside the volume; TSDF: that cell's value, the trilinear value (outside corners 0)
where it is inside the band (|v| < 1); wherever some |n| >= 1: TSDF 1, labels 0.

Exclusion: the reference's coordinate product goes through a BLAS call whose summation order is not specified, and a
coordinate that lies on a decision boundary may fall either way.  A voxel may be left out of a comparison only when, in
float64, (a) some u lies within 1e-3 cell of a half-integer (the nearest cell flips) or (b) some n lies within 1e-3 cell of
+-1 (the inside test flips).  EXCLUDED_CAP bounds the share per case and level.
"""
import numpy as np

N_VOX = (32, 24, 16)
VOXEL_SIZE = 0.04
VIEWS, IMG_H, IMG_W, FOCAL = 3, 12, 16, 14.0
SCENE_DIMS = [(45, 51, 27), (23, 26, 14), (12, 13, 7)]      # odd and non-cubic: an axis or level mix-up cannot pass
SCENE_ORIGIN = (-0.3, 0.95, -0.15)
MAX_EPOCH, EPOCH = 4, 1
EDGE = 1e-3
EXCLUDED_CAP = 0.02
TSDF_TOL = 1e-3

# name -> (random_rotation, random_translation, seed, panoptic, scene origin)
CASES = {
    "rot_trans_1": (True, True, 1, True, SCENE_ORIGIN),
    "rot_trans_2": (True, True, 2, True, SCENE_ORIGIN),
    "rot_only": (True, False, 3, True, SCENE_ORIGIN),
    "trans_only": (False, True, 6, True, SCENE_ORIGIN),
    # (with SCENE_ORIGIN no trilinear stencil of the unrotated crop crosses the volume's edge: shifted until some do, at all levels)
    "plain": (False, False, 2, True, (-0.3, 1.25, -0.13)),
    "tsdf_only": (True, True, 7, False, SCENE_ORIGIN),
}
# (seeds: the first ones at which the generator's conditions hold — tests/golden/make_transform_golden.py check_case)


def paddings(rot, trans):
    return (0.3, 0.1) if rot or trans else (0.0, 0.0)


def camera_poses(views=VIEWS):
    """cameras at (0.1 v, -0.2, 0.5) looking along +y, pitched down (forward z -0.2), yawed 10 (v - 1) degrees"""
    poses = []
    for v in range(views):
        yaw = np.deg2rad(10.0 * (v - 1))
        fwd = np.array([np.sin(yaw), np.cos(yaw), -0.2])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        p = np.eye(4)
        p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = right, np.cross(fwd, right), fwd, [0.1 * v, -0.2, 0.5]
        poses.append(p)
    return np.stack(poses).astype(np.float32)


def make_inputs(seed, panoptic=True, scene_origin=SCENE_ORIGIN, scene_dims=SCENE_DIMS, views=VIEWS, h=IMG_H, w=IMG_W):
    """numpy inputs of one sample: depth uniform in 0.3-2.5, scene TSDF clip(N(0,1), -1, 1) (many exact +-1 next to in-band
    values), integer-valued colours 0..255, labels 0..40 / 0..29"""
    rng = np.random.default_rng(seed)
    k = np.array([[FOCAL, 0, (w - 1) / 2], [0, FOCAL, (h - 1) / 2], [0, 0, 1]], np.float32)
    out = {
        "imgs": np.zeros((views, 3, h, w), np.float32),
        "depth": rng.uniform(0.3, 2.5, (views, h, w)).astype(np.float32),
        "intrinsics": np.stack([k] * views), "extrinsics": camera_poses(views),
        "tsdf_list_full": [np.clip(rng.normal(0, 1.0, f), -1, 1).astype(np.float32) for f in scene_dims],
        "vol_origin": np.array(scene_origin, np.float32),
    }
    if panoptic:
        out["rgb_list_full"] = [rng.integers(0, 256, tuple(f) + (3,)).astype(np.float32) for f in scene_dims]
        out["semantic_list_full"] = [rng.integers(0, 41, f).astype(np.float32) for f in scene_dims]
        out["instance_list_full"] = [rng.integers(0, 30, f).astype(np.float32) for f in scene_dims]
    return out


def case_inputs(name):
    rot, trans, seed, panoptic, origin = CASES[name]
    return make_inputs(seed, panoptic, origin)


def second_seed_case():
    """(inputs, T^-1 f32[4,4], vol_origin_partial) of a sample no golden file knows: another seed, a rotation of 0.7 rad with a
    shift, hand-made (no reference tree needed)"""
    inp = make_inputs(11, True, (-0.41, 0.83, -0.21))
    c, s = np.cos(0.7), np.sin(0.7)
    t_mat = np.eye(4)
    t_mat[:2, :2] = [[c, -s], [s, c]]
    t_mat[:3, 3] = [0.37, -0.52, 0.06]
    return inp, np.linalg.inv(t_mat).astype(np.float32), np.array([-0.72, 0.64, -0.32], np.float32)


def sample_dict(inp, torch, scene=None):
    """the dict RandomTransformSpace takes (after ToTensor); scene: a SceneVolumes to hand over instead of the lists"""
    data = {k: torch.from_numpy(inp[k].copy()) for k in ("imgs", "depth", "intrinsics", "extrinsics")}
    data["vol_origin"] = inp["vol_origin"].copy()
    data["epoch"] = [EPOCH]
    if scene is not None:
        data["tsdf_list_full"] = scene
    else:
        for k in ("tsdf_list_full", "rgb_list_full", "semantic_list_full", "instance_list_full"):
            if k in inp:
                data[k] = [torch.from_numpy(v.copy()) for v in inp[k]]
    return data


def coords_f64(n_vox, voxel_size, origin_partial, transform, old_origin, full_dims, level):
    """(n, u) float64 [3, cells of the level] (z fastest)"""
    vs = np.float64(np.float32(voxel_size))
    m = np.asarray(transform, np.float64)
    g = np.stack(np.meshgrid(*[np.arange(0, n, 2 ** level) for n in n_vox], indexing="ij")).reshape(3, -1).astype(np.float64)
    world = g * vs + np.asarray(origin_partial, np.float64).reshape(3, 1)
    world = m[:3, :3] @ world + m[:3, 3:4]
    c = (world - np.asarray(old_origin, np.float64).reshape(3, 1)) / vs / 2 ** level
    dims = np.asarray(full_dims, np.float64).reshape(3, 1)
    n = 2 * c / (dims - 1) - 1
    return n, ((n + 1) * dims - 1) / 2


def crop_f64(n_vox, voxel_size, origin_partial, transform, old_origin, level, tsdf, rgb=None, semantic=None, instance=None):
    """the rule in float64 for one level.  Returns a dict of arrays shaped like the level: tsdf, (rgb, semantic, instance),
    excluded (module docstring), outside (some |n| >= 1), in_band (the trilinear value was taken), crossing (... and its stencil
    reaches over the volume's edge), z_frac (distance of u_z's fraction from one half)"""
    shape = tuple(-(-n // 2 ** level) for n in n_vox)
    dims = np.array(tsdf.shape, np.int64)
    n, u = coords_f64(n_vox, voxel_size, origin_partial, transform, old_origin, dims, level)
    dcol = dims[:, None]
    near_half = (np.abs(u - np.floor(u) - 0.5) < EDGE).any(0)
    near_border = (np.abs(np.abs(n) - 1) < EDGE * 2 / dcol).any(0)
    outside = (np.abs(n) >= 1).any(0)
    idx = np.rint(u).astype(np.int64)

    def fetch(vol, ii):
        ok = ((ii >= 0) & (ii < dcol)).all(0)
        o = np.zeros((ii.shape[1],) + vol.shape[3:])
        o[ok] = vol[ii[0, ok], ii[1, ok], ii[2, ok]]
        return o, ok

    tv = np.asarray(tsdf, np.float64)
    near, inb = fetch(tv, idx)
    fl = np.floor(u).astype(np.int64)
    fr = u - fl
    tri = np.zeros(u.shape[1])
    crossing = np.zeros(u.shape[1], bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wgt = (fr[0] if dx else 1 - fr[0]) * (fr[1] if dy else 1 - fr[1]) * (fr[2] if dz else 1 - fr[2])
                v, ok = fetch(tv, fl + np.array([[dx], [dy], [dz]]))
                tri += wgt * v
                crossing |= ~ok
    band = np.abs(near) < 1
    t = np.where(band, tri, near)
    t[outside] = 1
    out = {"tsdf": t.reshape(shape), "excluded": (near_half | near_border).reshape(shape), "outside": outside.reshape(shape),
           "in_band": (band & inb & ~outside).reshape(shape), "crossing": (crossing & band & inb & ~outside).reshape(shape),
           "z_frac": float(np.abs(u[2] - np.floor(u[2]) - 0.5).min())}
    for name, vol in (("rgb", rgb), ("semantic", semantic), ("instance", instance)):
        if vol is not None:
            v, _ = fetch(np.asarray(vol, np.float64), idx)
            v[outside] = 0
            out[name] = v.reshape(shape + vol.shape[3:])
    return out


def crop_f32(n_vox, voxel_size, origin_partial, transform, old_origin, level, tsdf, label=None):
    """csrc/gt_crop.hip's operation order in float32 numpy (every operation rounded to nearest, the matrix rows as a k-ordered
    fma chain; an fma is taken in float64 and rounded once more, which can differ from a true fma in rare double-rounding
    cases).  Returns (tsdf, label) of the level: what the kernel is expected to store, bit for bit."""
    f = np.float32
    vs, dims = f(voxel_size), tsdf.shape
    shape = tuple(-(-n // 2 ** level) for n in n_vox)
    g = np.stack(np.meshgrid(*[np.arange(0, n, 2 ** level) for n in n_vox], indexing="ij")).reshape(3, -1).astype(f)
    x = g * vs + np.asarray(origin_partial, f).reshape(3, 1)
    m = np.asarray(transform, f).astype(np.float64)
    u, outside = [], np.zeros(g.shape[1], bool)
    for k in range(3):
        acc = f(m[k, 0]) * x[0]
        for j in (1, 2):
            acc = (x[j].astype(np.float64) * m[k, j] + acc).astype(f)
        w = (m[k, 3] + acc.astype(np.float64)).astype(f)
        c = ((w - f(old_origin[k])) / vs) / f(2 ** level)
        d = f(dims[k])
        n = (f(2) * c) / (d - f(1)) - f(1)
        outside |= ~(np.abs(n) < 1)
        u.append((((n + f(1)) * d) - f(1)) / f(2))
    u = np.stack(u)
    dcol = np.array(dims)[:, None]

    def fetch(vol, ii):
        ok = ((ii >= 0) & (ii < dcol)).all(0)
        o = np.zeros(ii.shape[1], f)
        o[ok] = vol[ii[0, ok], ii[1, ok], ii[2, ok]]
        return o

    idx = np.rint(u).astype(np.int64)
    t = fetch(tsdf, idx)
    fl = np.floor(u)
    w1, w0 = u - fl, (fl + f(1)) - u
    acc = np.zeros(g.shape[1], f)
    for corner in range(8):
        bz, by, bx = corner & 1, (corner >> 1) & 1, corner >> 2
        w = ((w1[2] if bz else w0[2]) * (w1[1] if by else w0[1])) * (w1[0] if bx else w0[0])
        acc = acc + fetch(tsdf, fl.astype(np.int64) + np.array([[bx], [by], [bz]])) * w
    t = np.where(np.abs(t) < 1, acc, t)
    t[outside] = 1
    lab = None
    if label is not None:
        lab = fetch(np.asarray(label, f), idx)
        lab[outside] = 0
        lab = lab.reshape(shape)
    return t.reshape(shape), lab


def crop_grid_sample(torch, n_vox, voxel_size, origin_partial, transform, old_origin, level, tsdf, rgb=None, semantic=None,
                     instance=None):
    """the rule through torch.nn.functional.grid_sample on the CPU in float32 (no reference tree needed)"""
    F = torch.nn.functional
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    x, y, z = n_vox
    g = torch.stack(torch.meshgrid(torch.arange(x), torch.arange(y), torch.arange(z), indexing="ij")).reshape(3, -1)
    world = g.float() * voxel_size + f(origin_partial).view(3, 1)
    world = f(transform)[:3, :] @ torch.cat((world, torch.ones_like(world[:1])), dim=0)
    c = (world - f(old_origin).view(3, 1)) / voxel_size
    c = c.view(3, x, y, z)[:, ::2 ** level, ::2 ** level, ::2 ** level] / 2 ** level
    shape = list(c.shape[1:])
    dims = list(tsdf.shape)
    n = 2 * c.reshape(3, -1) / (torch.Tensor(dims) - 1).view(3, 1) - 1
    grid = n[[2, 1, 0]].T.view([1] + shape + [3])
    outside = (grid.abs() >= 1).squeeze(0).any(3)

    def sample(vol, mode):
        return F.grid_sample(f(vol).view([1, 1] + dims), grid, mode=mode, padding_mode="zeros", align_corners=False).view(shape)

    t = sample(tsdf, "nearest")
    band = t.abs() < 1
    t[band] = sample(tsdf, "bilinear")[band]
    t[outside] = 1
    out = {"tsdf": t.numpy()}
    if rgb is not None:
        c3 = torch.stack([sample(np.ascontiguousarray(np.asarray(rgb)[..., k]), "nearest") for k in range(3)], -1)
        c3[outside] = 0
        out["rgb"] = c3.numpy()
    for name, vol in (("semantic", semantic), ("instance", instance)):
        if vol is not None:
            v = sample(vol, "nearest")
            v[outside] = 0
            out[name] = v.numpy()
    return out


def compare(got, want, excluded, where=""):
    """`got` against `want` (dicts of one level: tsdf and, where present, rgb / semantic / instance) outside `excluded`:
    labels and colour exact, TSDF within TSDF_TOL; the excluded share within EXCLUDED_CAP.  Returns (max TSDF error, share)."""
    share = float(excluded.mean())
    print(f"{where}: excluded share {share:.4f}")
    assert share <= EXCLUDED_CAP, (where, share)
    keep = ~excluded
    err = float(np.abs(np.asarray(got["tsdf"], np.float64) - want["tsdf"])[keep].max())
    print(f"{where}: max TSDF error {err:.3e}")
    for name in ("rgb", "semantic", "instance"):
        if name in want:
            bad = int((np.asarray(got[name], np.float64) != want[name])[keep].sum())
            print(f"{where}: {name} mismatches {bad}")
            assert bad == 0, (where, name, bad)
    assert err <= TSDF_TOL, (where, err)
    return err, share

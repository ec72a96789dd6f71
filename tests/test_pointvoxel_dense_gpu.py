"""GPU: the HIP point-voxel path — voxel numbering and strided parents, voxelisation and scatter-mean, trilinear corner tables
(hash probes and the native pass's kernel-map path), devoxelisation, the fused ConvGRU gates, the k=3 / k2s2 / transposed
convolutions and their backward — against the float64 dense formulations of tests/dense_ref.py, not against the oracle.

Integer results (voxel coordinates, parents, point -> voxel ids, corner indices) must match exactly; features within 1e-3
absolute and within 1e-5 of their sum-of-magnitudes scale (sum |a| |w| of the terms) where that is tighter.  The inputs are
the edge cases of test_oracle_dense.py: negative and odd-negative coordinates, interleaved batches, the 1 -> 2 -> 4 -> 8
hierarchy, points on voxel faces and one ulp below them, absent corners, a 1,200-point voxel, empty target voxels."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import dense_ref as DR  # noqa: E402
from test_oracle_dense import (LAYERS, dense_layer, edge_coords, face_points, hierarchy, metric_points,  # noqa: E402
                               sparse_voxel_set, with_far_points)

TOL = 1e-3
RES = 0.37


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def close(got, ref, scale):
    """|got - ref| <= min(1e-3, 1e-5 scale) elementwise; scale = the float64 sum of |terms| of each output"""
    got, ref, scale = (np.asarray(host(a) if torch.is_tensor(a) else a, np.float64) for a in (got, ref, scale))
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    bound = np.minimum(TOL, 1e-5 * scale) + 1e-12
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"err {err[worst]:.3e} > bound {bound[worst]:.3e} at {worst}"


def lib():
    from eprecon_amd import _lib
    return _lib, _lib.load()


def stream():
    from eprecon_amd import _lib
    return _lib.current_stream()


# ---------------------------------------------------------------------------------------------------------------------
# voxel numbering, strided parents, k2s2 maps

def _check_down_up(fine, coarse, down, up, stride):
    """down[k][j] = row of coarse[j] + b_k s in fine, up[k][i] = parent of fine[i] when it is child k (dense-reference lookups)"""
    offs = np.array([((k >> 2) & 1, (k >> 1) & 1, k & 1) for k in range(8)])
    parent = DR.lookup(coarse, DR.quantise_coords(fine, 2 * stride))
    for k in range(8):
        q = coarse.copy()
        q[:, 1:] += offs[k] * stride
        assert np.array_equal(host(down[k]), DR.lookup(fine, q)), f"down map, offset {k}"
        child = ((fine[:, 1:] - DR.quantise_coords(fine, 2 * stride)[:, 1:]) // stride) @ np.array([4, 2, 1])
        assert np.array_equal(host(up[k]), np.where(child == k, parent, -1)), f"transposed map, offset {k}"


def test_numbering_parents_and_strided_maps_on_negative_coordinates():
    """unique_coords at quanta 1 / 2 / 4 / 8, voxel_hierarchy's 1 -> 2 -> 4 sets, VoxelSet.downsample() to 8, and the k2s2 maps
    of every step: odd negatives on every axis (-1, -3 floor to -2, -4 at stride 2), the same xyz in three interleaved batches"""
    from eprecon_amd import sparse as SP
    c = edge_coords(0)
    for q in (1, 2, 4, 8):
        u, inv, _ = SP.unique_coords(dev(c), q)
        ru, rinv = DR.number_first(DR.quantise_coords(c, q))
        assert np.array_equal(host(u), ru) and np.array_equal(host(inv), rinv), f"quantum {q}"
    lv = hierarchy(c)
    base, inv, _ = SP.voxel_hierarchy(dev(c), 3)
    assert np.array_equal(host(base.coords), lv[0][0]) and np.array_equal(host(inv), np.arange(len(c)))
    cur = base
    for lvl in range(1, 4):      # levels 1, 2 from the hierarchy call, level 3 (stride 8) by VoxelSet.downsample()
        coarse, down, up = cur.downsample()
        assert coarse.stride == 2 ** lvl and np.array_equal(host(coarse.coords), lv[lvl][0])
        _check_down_up(lv[lvl - 1][0], lv[lvl][0], down, up, 2 ** (lvl - 1))
        cur = coarse
    fresh = SP.VoxelSet(dev(c), 1)        # the non-hierarchy path: unique_coords(quantum = 2) inside downsample()
    coarse, down, up = fresh.downsample()
    assert np.array_equal(host(coarse.coords), lv[1][0])
    _check_down_up(lv[0][0], lv[1][0], down, up, 1)


# ---------------------------------------------------------------------------------------------------------------------
# voxelisation, scatter-mean, point_to_voxel

def _seg_mean(feat, idx, m, out):
    from eprecon_amd import torchsparse_utils as TU
    lists = TU._segment_lists(idx, m)
    with torch.no_grad():
        return TU._segment_mean(feat, lists, m, out=out)


def _views(n, c, rng):
    """(name, feat view, out view) that force each scatter-mean / devoxelise form: aligned rows with C % 4 == 0 (float4
    kernels), C % 4 != 0, and column slices at an offset that is not a multiple of 4 (scalar kernels)"""
    f = rng.standard_normal((n, c + 8)).astype(np.float32)
    return [("aligned", dev(f[:, :c]), 4 * ((c + 3) // 4), 0),
            ("offset 1", dev(f)[:, 1:1 + c], 4 * ((c + 3) // 4) + 4, 1),
            ("offset 4", dev(f)[:, 4:4 + c], 4 * ((c + 3) // 4) + 8, 4)]


@pytest.mark.parametrize("c", [12, 13])
def test_voxelize_and_scatter_mean_forms(c):
    """floor of the float32 quotient p / res, first-occurrence numbering, and the scatter-mean in every kernel form on a list
    with a 1,200-point voxel; point_to_voxel into sets at strides 1 .. 8 with voxels that hold no point (exactly 0)"""
    from eprecon_amd import torchsparse_utils as TU
    from eprecon_amd.sparse import VoxelSet
    rng = np.random.default_rng(c)
    pts = metric_points(1)
    TU.clear_voxelization_cache()
    e = TU._voxelize_points(dev(pts), RES)
    r_scaled, r_vox = DR.quantise_points(pts, RES)
    assert np.array_equal(host(e.scaled), r_scaled) and np.array_equal(host(e.vox), r_vox)
    ru, rinv = DR.number_first(r_vox)
    assert np.array_equal(host(e.vset.coords), ru) and np.array_equal(host(e.inverse), rinv)
    assert np.bincount(rinv).max() >= 1000
    n = len(pts)
    for name, feat, pitch, off in _views(n, c, rng):
        f64 = host(feat).astype(np.float64)
        for s in (1, 2, 4, 8):
            target = DR.number_first(DR.quantise_coords(r_vox, s))[0]
            extra = target[:40].copy()
            extra[:, 1] += 1000                                  # voxels no point falls into
            target = np.concatenate([extra[:20], target, extra[20:]])
            m = len(target)
            idx = VoxelSet(dev(target.astype(np.int32)), s).grid.query(e.vox, quantum=s)
            ridx = DR.lookup(target, DR.quantise_coords(r_vox, s))
            assert np.array_equal(host(idx), ridx)
            buf = torch.full((m, pitch), float("nan"), device="cuda")
            out = _seg_mean(feat, idx, m, buf[:, off:off + c])
            ref = DR.scatter_mean(f64, ridx, m).numpy()
            close(out, ref, DR.scatter_mean(np.abs(f64), ridx, m).numpy())
            assert not host(out)[:20].any() and not host(out)[-20:].any(), f"{name}: empty voxels must be 0"


def test_voxelize_rotated_frame_points():
    """aligned-camera points (a rotated, translated frame: no coordinate on a lattice) quantised at two resolutions"""
    from eprecon_amd import torchsparse_utils as TU
    c = edge_coords(3)
    a, b = np.deg2rad(31.0), np.deg2rad(-12.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    w2ac = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    w2ac[:, :3, :3] = rz @ rx
    w2ac[:, :3, 3] = [0.3, -0.7, 1.1]
    origin = np.array([[-0.5, 0.2, 0.0], [0.1, -0.3, 0.4], [0.0, 0.0, -0.6]], np.float32)
    r = TU.aligned_camera_coords(dev(c), dev(origin), 0.08, dev(w2ac))
    for res in (0.16, RES):
        TU.clear_voxelization_cache()
        e = TU._voxelize_points(r, res)
        r_scaled, r_vox = DR.quantise_points(host(r), res)
        assert np.array_equal(host(e.scaled), r_scaled) and np.array_equal(host(e.vox), r_vox)
        ru, rinv = DR.number_first(r_vox)
        assert np.array_equal(host(e.vset.coords), ru) and np.array_equal(host(e.inverse), rinv)
        assert (r_vox[:, 1:] < 0).any() and len(ru) < len(c)


# ---------------------------------------------------------------------------------------------------------------------
# trilinear corner tables

def _trilinear_hash(vset_coords, s, pts):
    from eprecon_amd.sparse import VoxelSet
    _lib, L = lib()
    vs = VoxelSet(dev(vset_coords.astype(np.int32)), s)
    p = dev(pts)
    n = len(pts)
    idx8 = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    w8 = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    _lib.check(L.eprecon_trilinear_map_async(_lib.ptr(vs.grid.mem), vs.grid.capacity, _lib.ptr(p), n, s, _lib.ptr(idx8),
                                             _lib.ptr(w8), stream()), "eprecon_trilinear_map_async")
    return idx8, w8


def _check_tables(idx8, w8, ridx, rw):
    assert np.array_equal(host(idx8), ridx)
    np.testing.assert_allclose(host(w8), rw, atol=1e-6, rtol=0)
    none = (ridx < 0).all(1)
    assert not host(w8)[none].any(), "a point without corners must get weights 0, not NaN"


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_corner_tables_hash_path(s):
    """trilinear_map_kernel (voxel_to_point's corner probes) == the closed form, on face / edge / corner points and one ulp
    below them (-0.0 included), with absent corners and points whose eight corners are all absent"""
    rng = np.random.default_rng(s)
    pts = with_far_points(face_points(6), 6)
    vset = sparse_voxel_set(pts, s, rng)
    ridx, rw = DR.corner_tables(vset, s, pts)
    assert (ridx < 0).all(1).sum() >= 40 and ((ridx >= 0).any(1) & (ridx < 0).any(1)).sum() > 50
    _check_tables(*_trilinear_hash(vset, s, pts), ridx, rw)


def test_corner_tables_native_pass():
    """the SPVCNN pass's geometry call (voxel_hierarchy(points=...) -> _hierarchy_with_geometry: trilinear_from_map_kernel on the
    3x3x3 maps) at strides 1 and 4, its voxel sets and strided maps, == the closed form on the dense reference's hierarchy"""
    from eprecon_amd import sparse as SP
    pts = face_points(7, n_random=3000)
    # (no subnormal coordinates here: the stride-4 table of this path takes its base voxel from the integer voxel, which
    # differs from floor(p / 4) only when p / 4 underflows to -0.0 — a known deviation)
    pts = pts[~((pts[:, :3] != 0) & (np.abs(pts[:, :3]) < np.finfo(np.float32).tiny)).any(1)]
    scaled, vox = DR.quantise_points(pts, 1.0)
    lv = hierarchy(DR.number_first(vox)[0], 3)
    s1, inv, t = SP.voxel_hierarchy(dev(vox.astype(np.int32)), 3, points=dev(scaled))
    assert t is not None
    assert np.array_equal(host(s1.coords), lv[0][0]) and np.array_equal(host(inv), DR.lookup(lv[0][0], vox))
    s2, down12, up21 = s1.downsample()
    s4, down24, up42 = s2.downsample()
    assert np.array_equal(host(s2.coords), lv[1][0]) and np.array_equal(host(s4.coords), lv[2][0])
    _check_down_up(lv[0][0], lv[1][0], down12, up21, 1)
    _check_down_up(lv[1][0], lv[2][0], down24, up42, 2)
    assert np.array_equal(host(t["idx4"]), DR.lookup(lv[2][0], DR.quantise_coords(vox, 4)))
    for s, coords, key in ((1, lv[0][0], "1"), (4, lv[2][0], "4")):
        ridx, rw = DR.corner_tables(coords, s, scaled)
        assert ((ridx >= 0).any(1) & (ridx < 0).any(1)).sum() > 50
        _check_tables(t["idx8_" + key], t["weight8_" + key], ridx, rw)


# ---------------------------------------------------------------------------------------------------------------------
# devoxelisation and the ConvGRU gates

def _devox_case(seed, s=2):
    """corner tables of the closed form (int32 / float32, as the kernels take them) over a voxel set with absent corners and
    points without any corner; voxel features in a buffer whose row in front of them is NaN (a read through index -1 shows)"""
    rng = np.random.default_rng(seed)
    pts = with_far_points(face_points(seed), seed)
    vset = sparse_voxel_set(pts, s, rng)
    ridx, rw = DR.corner_tables(vset, s, pts)
    return rng, ridx, rw, dev(ridx.astype(np.int32)), dev(rw.astype(np.float32)), len(vset)


def _guarded(m, c, off, pitch, rng):
    buf = torch.full((m + 1, pitch), float("nan"), device="cuda")
    v = torch.from_numpy(rng.standard_normal((m, c)).astype(np.float32)).cuda()
    buf[1:, off:off + c] = v
    return buf[1:, off:off + c]


@pytest.mark.parametrize("c,off,pitch", [(12, 0, 12), (16, 4, 24), (13, 0, 16), (12, 1, 16), (3, 0, 3)])
def test_devoxelize_forms(c, off, pitch):
    """devoxelize4 (C % 4 == 0, aligned pitch) and the scalar kernel (C % 4 != 0, column offset 1), plain and accumulate=1:
    == sum_k w_k feat[idx_k] in float64; exactly 0 for a point without corners"""
    _lib, L = lib()
    rng, ridx, rw, idx8, w8, m = _devox_case(11 + c + off)
    n = ridx.shape[0]
    vf = _guarded(m, c, off, pitch, rng)
    f64 = host(vf).astype(np.float64)
    ref = DR.devoxelize(f64, ridx, rw).numpy()
    scale = DR.devoxelize(np.abs(f64), ridx, np.abs(rw)).numpy()
    none = (ridx < 0).all(1)
    for acc in (0, 1):
        prev = rng.standard_normal((n, pitch)).astype(np.float32)
        obuf = dev(prev)
        out = obuf[:, off:off + c]
        _lib.check(L.eprecon_devoxelize_async(_lib.ptr(vf), vf.stride(0), _lib.ptr(idx8), _lib.ptr(w8), n, c, _lib.ptr(out),
                                              out.stride(0), acc, stream()), "eprecon_devoxelize_async")
        base = prev[:, off:off + c].astype(np.float64) if acc else 0.0
        close(out, ref + base, scale + np.abs(base))
        if not acc:
            assert not host(out)[none].any(), "a point without corners must devoxelise to exactly 0"
        rest = np.ones(pitch, bool)
        rest[off:off + c] = False
        assert np.array_equal(host(obuf)[:, rest], prev[:, rest]), "columns outside the view were written"


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("c,tail,off", [(12, 8, 0), (12, 5, 0), (13, 4, 0), (12, 12, 1)])
def test_devoxelize_gate_forms(mode, c, tail, off):
    """the fused ConvGRU tail (devoxelise + skip, then sigmoid / sigmoid * h / (1 - z) h + z tanh) with its row copy: the
    float4 kernel (C and tail multiples of 4, aligned) and the scalar one (unaligned tail, C % 4 != 0, column offset 1)"""
    _lib, L = lib()
    rng, ridx, rw, idx8, w8, m = _devox_case(31 + c + tail, s=1)
    n = ridx.shape[0]
    pitch = 2 * c + tail + 4
    vf = _guarded(m, c, off, pitch, rng)
    rows = lambda k: dev(rng.standard_normal((n, pitch)).astype(np.float32))[:, off:off + k]
    skip, h = rows(c), rows(c)
    zg = torch.sigmoid(rows(c))
    src = rows(tail)
    out_buf = torch.full((n, pitch), 7.0, device="cuda")
    out, dst = out_buf[:, off:off + c], out_buf[:, off + c:off + c + tail]
    _lib.check(L.eprecon_devoxelize_gate_tail_async(
        _lib.ptr(vf), vf.stride(0), _lib.ptr(idx8), _lib.ptr(w8), n, c, _lib.ptr(skip), skip.stride(0), mode, _lib.ptr(h),
        h.stride(0), _lib.ptr(zg), zg.stride(0), _lib.ptr(out), out.stride(0), _lib.ptr(src), src.stride(0), _lib.ptr(dst),
        dst.stride(0), tail, stream()), "eprecon_devoxelize_gate_tail_async")
    v = DR.devoxelize(host(vf), ridx, rw) + DR._t64(host(skip))
    ref = DR.gate(v, mode, host(h), host(zg)).numpy()
    close(out, ref, np.abs(ref) + 1.0)
    assert np.array_equal(host(dst), host(src)), "tail copy"
    assert (host(out_buf)[:, off + c + tail:] == 7.0).all() and (host(out_buf)[:, :off] == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# convolutions

_LEVELS = {}


def levels():
    """the dense reference's 1 -> 2 -> 4 -> 8 hierarchy of edge_coords(0) and the HIP voxel sets / maps built on it"""
    if not _LEVELS:
        from eprecon_amd import sparse as SP
        lv = hierarchy(edge_coords(0), 4)
        sets, maps = [SP.VoxelSet(dev(lv[0][0].astype(np.int32)), 1)], []
        for lvl in range(1, 4):
            coarse, down, up = sets[-1].downsample()
            assert np.array_equal(host(coarse.coords), lv[lvl][0])
            sets.append(coarse)
            maps.append((down, up))
        _LEVELS.update(frame=DR.Frame([lv[0][0]], 8), lv=lv, sets=sets, maps=maps)
    return _LEVELS


def _hip_map(kind, stride):
    L = levels()
    lvl = int(np.log2(stride))
    if kind == "k3":
        return L["sets"][lvl].kernel_map(3)
    return L["maps"][lvl][0 if kind == "down" else 1]


def _layer_inputs(kind, stride, cin, cout, seed):
    L = levels()
    lvl = int(np.log2(stride))
    fine = L["lv"][lvl][0]
    coarse = L["lv"][lvl + 1][0] if lvl + 1 < 4 else None
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(coarse) if kind == "up" else len(fine), cin)).astype(np.float32)
    w = (rng.standard_normal((27 if kind == "k3" else 8, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    return L["frame"], fine, coarse, x, w


@pytest.mark.parametrize("kind,stride,cin,cout", LAYERS)
def test_convolution_matches_dense(kind, stride, cin, cout):
    """submanifold k=3 at strides 1 / 2 / 4, k2s2 down and transposed on every hierarchy step, SPVCNN / ConvGRU channel
    shapes at cr = 1, 1/2, 1/4 and ragged ones == conv3d / conv_transpose3d on the dense volume"""
    from eprecon_amd import _lib
    from eprecon_amd import sparse as SP
    frame, fine, coarse, x, w = _layer_inputs(kind, stride, cin, cout, seed=cin * 7 + cout + stride)
    y = SP.sparse_conv(dev(x), dev(w), _hip_map(kind, stride))
    name = _lib.last_conv_kernel()
    assert name.startswith("spconv_"), name          # a gather-GEMM family on the kernel map (not a dense-grid kernel)
    ref = dense_layer(frame, kind, fine, coarse, x, w, stride).numpy()
    scale = dense_layer(frame, kind, fine, coarse, np.abs(x), np.abs(w), stride).numpy()
    close(y, ref, scale)


@pytest.mark.parametrize("kind,stride,cin,cout", [("down", 1, 32, 32), ("down", 2, 13, 7), ("up", 1, 96, 96), ("up", 4, 7, 13),
                                                  ("k3", 1, 39, 16), ("k3", 2, 32, 64), ("k3", 4, 64, 128)])
def test_convolution_gradients_match_dense(kind, stride, cin, cout):
    """dx, dW, db of the HIP backward (eprecon_amd/autograd.py: the inverted map, the weight-gradient kernel) == torch.autograd
    through the float64 dense formulation, which never sees the HIP map"""
    from eprecon_amd import autograd as AG
    frame, fine, coarse, x, w = _layer_inputs(kind, stride, cin, cout, seed=cin + cout * 3 + stride)
    rng = np.random.default_rng(cin)
    b = rng.standard_normal(cout).astype(np.float32)
    n_out = len(fine) if kind != "down" else len(coarse)
    dy = rng.standard_normal((n_out, cout)).astype(np.float32)
    xs, ws, bs = (dev(a).requires_grad_() for a in (x, w, b))
    AG.sparse_conv(xs, ws, _hip_map(kind, stride), bs).backward(dev(dy))
    grads = []
    for xa, wa, dya in ((x, w, dy), (np.abs(x), np.abs(w), np.abs(dy))):
        xr, wr = DR._t64(xa).requires_grad_(), DR._t64(wa).requires_grad_()
        dense_layer(frame, kind, fine, coarse, xr, wr, stride).backward(DR._t64(dya))
        grads.append((xr.grad.numpy(), wr.grad.numpy()))
    (rdx, rdw), (sdx, sdw) = grads
    close(xs.grad, rdx, sdx)
    close(ws.grad, rdw, sdw)
    close(bs.grad, dy.astype(np.float64).sum(0), np.abs(dy).astype(np.float64).sum(0))


def test_devoxelize_and_segment_mean_gradients_match_dense():
    """the CSR-ordered devoxelise backward and the segment-mean backward == torch.autograd through the float64 formulations
    (corner tables with absent corners; a 1,200-point voxel, dropped points (-1) and empty voxels)"""
    from eprecon_amd import autograd as AG
    from eprecon_amd import torchsparse_utils as TU
    rng, ridx, rw, idx8, w8, m = _devox_case(41)
    n, c = ridx.shape[0], 20
    vf = rng.standard_normal((m, c)).astype(np.float32)
    dout = rng.standard_normal((n, c)).astype(np.float32)
    a = dev(vf).requires_grad_()
    AG.devoxelize(a, idx8, w8).backward(dev(dout))
    r = DR._t64(vf).requires_grad_()
    DR.devoxelize(r, ridx, rw).backward(DR._t64(dout))
    s = DR._t64(np.abs(vf)).requires_grad_()
    DR.devoxelize(s, ridx, np.abs(rw)).backward(DR._t64(np.abs(dout)))
    close(a.grad, r.grad.numpy(), s.grad.numpy())

    pts = metric_points(2)
    _, vox = DR.quantise_points(pts, RES)
    ru, rinv = DR.number_first(vox)
    inv = rinv.copy()
    inv[::17] = -1                                              # points that fall into no voxel
    m = len(ru) + 25                                            # voxels that hold no point
    feat = rng.standard_normal((len(pts), c)).astype(np.float32)
    dvox = rng.standard_normal((m, c)).astype(np.float32)
    idx = dev(inv.astype(np.int32))
    a = dev(feat).requires_grad_()
    out = AG.segment_mean(a, idx, TU._segment_lists(idx, m), m)
    out.backward(dev(dvox))
    r = DR._t64(feat).requires_grad_()
    ref = DR.scatter_mean(r, inv, m)
    ref.backward(DR._t64(dvox))
    s = DR._t64(np.abs(feat)).requires_grad_()
    DR.scatter_mean(s, inv, m).backward(DR._t64(np.abs(dvox)))
    close(out, ref.detach().numpy(), DR.scatter_mean(np.abs(feat), inv, m).numpy())
    close(a.grad, r.grad.numpy(), s.grad.numpy())
    assert not host(a.grad)[::17].any(), "a dropped point gets no gradient"

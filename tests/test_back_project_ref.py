"""Pins the float64 witness of the back-projection (tests/back_project_ref.py) itself: against the vectors captured from the
reference (tests/golden/back_project.npz), against torch's float64 grid_sample on the witness's own grid, against the fp32 C
oracle within the witness's own bound, its adjoint by <A x, y> = <x, A^T y>, its closed forms, and the share of voxels the
GPU module (tests/test_back_project_f64_gpu.py) has to hand to the oracle in every scene it uses.  CPU only."""
import os

import numpy as np
import pytest

import back_project_ref as R
from oracle import back_project as O
from test_oracle_back_project import CASES, bp_inputs

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "back_project.npz"))


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max(initial=0.0))


@pytest.mark.parametrize("name", CASES[:4])
@pytest.mark.parametrize("mv", [0, 2])
def test_witness_matches_reference_golden(gold, name, mv):
    """counts, kept rows, coords rows, feature rows and depth rows captured from the reference itself"""
    window, coords, origin, feats, kr = bp_inputs(gold[name + "_meta"])
    H, W = feats.shape[3:]
    G = R.geometry(coords, origin, window["voxel_size"], kr, H, W)
    band = R.in_band(G)
    assert band.mean() <= 0.01
    key = f"{name}_mv{mv}"
    cnt_gold = gold[key + "_count"].astype(np.int64)
    assert np.array_equal(G.vis.sum(axis=0)[~band], cnt_gold[~band])
    # the reference's own decisions for the few rows inside the band (its counts are all the golden file keeps of them: rows whose
    # count differs are left out of the feature comparison)
    has_depth = key + "_depth_rows" in gold.files
    w = R.forward(G, feats, R.MODE_MEAN_DEPTH if has_depth else R.MODE_MEAN, mv)
    same = w.cnt == cnt_gold
    valid_gold = np.nonzero(cnt_gold >= mv)[0]
    assert int(gold[key + "_nvalid"]) == valid_gold.size
    rows = gold[key + "_rows"]
    src = valid_gold[rows]                                   # input row of each sampled output row
    assert np.array_equal(coords[src], gold[key + "_coord_rows"])
    ok = same[src]
    assert ok.mean() > 0.98
    C = feats.shape[2]
    assert _ratio(np.abs(w.y[src][ok][:, :C] - gold[key + "_feat_rows"][ok]), w.bound[src][ok][:, :C]) <= 1.0
    assert np.array_equal(G.vis[:, src][:, ok], gold[key + "_mask_rows"][:, ok])
    gg = np.stack([G.gx[:, src], G.gy[:, src]], axis=-1)
    eg = np.stack([G.eu[:, src] * 2 / (W - 1), G.ev[:, src] * 2 / (H - 1)], axis=-1)
    m = G.vis[:, src] & ok[None]
    assert (np.abs(gg - gold[key + "_grid_rows"])[m] <= eg[m]).all()
    if has_depth and same[valid_gold].all():                  # (the depth statistics run over every kept row)
        assert _ratio(np.abs(w.y[src, C] - gold[key + "_depth_rows"]), w.bound[src, C]) <= 1.0


@pytest.mark.parametrize("name", ["mlp_c12", "vec4_v20_b2_c24", "vec1_c7"])
def test_witness_matches_float64_grid_sample(name):
    sc = R.scene(name)
    G = R.geometry_of(sc)
    w = R.forward(G, sc["feats"], R.MODE_VARIANCE, 0)
    F = torch.from_numpy(sc["feats"]).double()
    V, B, C, H, W = F.shape
    with np.errstate(invalid="ignore"):
        grid = torch.from_numpy(np.nan_to_num(np.stack([G.gx, G.gy], axis=-1), nan=9.0, posinf=9.0, neginf=-9.0).clip(-9, 9))
    s = torch.zeros(V, G.vis.shape[1], C, dtype=torch.float64)
    for b in range(B):
        rows = np.nonzero(G.batch == b)[0]
        smp = torch.nn.functional.grid_sample(F[:, b], grid[:, rows][:, None], mode="bilinear", padding_mode="zeros",
                                              align_corners=True)          # [V, C, 1, rows]
        s[:, rows] = smp[:, :, 0].permute(0, 2, 1)
    m = torch.from_numpy(G.vis)[..., None].double()
    den = m.sum(0).clamp(min=1)
    mean = (s * m).sum(0) / den
    var = (((s - mean[None]) ** 2) * m).sum(0) / den
    assert np.abs(mean.numpy() - w.mean).max() < 1e-11
    assert np.abs(var.numpy() - w.y).max() < 1e-11


@pytest.mark.parametrize("name", ["mlp_c24", "vec4_v21_b1_c24", "vec4_v20_b2_c44", "vec1_c13", "batch_b3"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fp32_oracle_is_within_the_witness_bound(name, mode):
    sc = R.scene(name)
    G = R.geometry_of(sc)
    band = R.in_band(G)
    o = O.back_project(sc["coords"], sc["origin"], sc["voxel_size"], sc["feats"], sc["kr"], 0, mode, want_grid=True)
    assert np.array_equal(o["count"][~band], G.vis.sum(axis=0)[~band])
    vis = np.where(band[None], o["mask"], G.vis)
    assert np.array_equal(vis[:, ~band], o["mask"][:, ~band])
    w = R.forward(G, sc["feats"], mode, 0, vis=vis)
    # (a row no view sees: the reference's variance block divides 0 by 0 there, and so does the oracle; the library and the
    # witness divide by max(cnt, 1) in every mode and give 0.  Only min_view = 0 reaches such rows.)
    seen = w.cnt > 0 if mode == 2 else np.ones_like(band)
    assert mode != 2 or (np.isnan(o["feats"][~seen]).all() and not w.y[~seen].any())
    r = _ratio(np.abs(o["feats"] - w.y)[seen], w.bound[seen])
    assert r <= 1.0, r
    if mode == 2:
        assert _ratio(np.abs(o["mean"] - w.mean)[seen], w.mean_bound[seen]) <= 1.0
    # and the bound is no blanket: a quarter of it is not enough for a shift of 2^-10 px
    C = sc["feats"].shape[2]
    assert _ratio(np.abs(o["feats"] - R.forward(G, sc["feats"], mode, 0, vis=vis, du=2.0 ** -10).y)[seen][:, :C],
                  w.bound[seen][:, :C]) > 1.0


@pytest.mark.parametrize("name", ["bwd_c7", "bwd_b2", "bwd_c1"])
@pytest.mark.parametrize("mode", [0, 2])
def test_adjoint_identity(name, mode):
    """<A x, y> = <x, A^T y>; in variance mode A is the Jacobian, which a central difference of the quadratic gives exactly"""
    sc = R.scene(name)
    G = R.geometry_of(sc)
    rng = np.random.default_rng(3)
    f = sc["feats"].astype(np.float64)
    C = f.shape[2]
    h = rng.standard_normal(f.shape)
    dout = rng.standard_normal((G.vis.shape[1], C))
    dmean = rng.standard_normal((G.vis.shape[1], C))
    df, _ = R.adjoint(G, sc["feats"], mode, dout, dmean if mode == 2 else None)
    rhs = float((h.transpose(0, 1, 3, 4, 2) * df).sum())
    if mode == 0:
        lhs = float((R.forward(G, h.astype(np.float32).astype(np.float64), 0, 0).y * dout).sum())
        h32 = h.astype(np.float32).astype(np.float64)
        rhs = float((h32.transpose(0, 1, 3, 4, 2) * df).sum())
    else:
        # forward() takes fp32 maps; the Jacobian is applied in float64 through the witness's sampler
        def fwd(x):
            acc = np.zeros((G.vis.shape[1], C))
            ss = []
            for v, rows, s, sa, dl in R._sample_views(G, x, G.vis):
                acc[rows] += s
                ss.append((rows, s))
            den = np.maximum(G.vis.sum(0), 1)[:, None]
            m = acc / den
            var = np.zeros_like(m)
            for rows, s in ss:
                var[rows] += (s - m[rows]) ** 2
            return var / den, m
        f32 = sc["feats"]
        e = (h * 2.0 ** -12).astype(np.float32)              # fp32 maps on both sides: f32 +- e are exact fp32 sums here or not,
        xp, xm = (f32.astype(np.float64) + e), (f32.astype(np.float64) - e)   # irrelevant: _sample_views converts what it is given
        (vp, mp), (vm, mm) = fwd(xp), fwd(xm)
        lhs = float((((vp - vm) / 2) * dout).sum() + (((mp - mm) / 2) * dmean).sum())
        rhs = float((e.astype(np.float64).transpose(0, 1, 3, 4, 2) * df).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_closed_forms():
    """constant maps have D = 0 and sample to the constant; an affine ramp a x + b y samples to a u + b v inside the image"""
    sc = R.scene("mlp_c4")
    G = R.geometry_of(sc)
    V, B, C, H, W = sc["feats"].shape
    const = np.broadcast_to(np.arange(1, V * C + 1, dtype=np.float32).reshape(V, 1, C, 1, 1), sc["feats"].shape)
    w = R.forward(G, const, 0, 0)
    exp = np.zeros_like(w.y)
    for v in range(V):
        exp += G.vis[v][:, None] * const[v, 0, :, 0, 0][None]
    exp /= np.maximum(w.cnt, 1)[:, None]
    inner = (G.margin > 1e-3).all(axis=0)                      # (on the very border the zero continuation gives D > 0)
    assert np.abs(w.y - exp).max() < 1e-12
    a, b = np.float32(0.25), np.float32(-0.5)
    ramp = (a * np.arange(W, dtype=np.float32)[None] + b * np.arange(H, dtype=np.float32)[:, None])
    w = R.forward(G, np.broadcast_to(ramp, sc["feats"].shape), 0, 0)
    exp = (np.where(G.vis, a * G.u + b * G.v, 0.0).sum(axis=0) / np.maximum(w.cnt, 1))[:, None]
    assert np.abs(w.y - exp).max() < 1e-11
    assert inner.any()


@pytest.mark.parametrize("views", [3, 21])
def test_exact_scene_is_exact_and_covers_its_faces(views):
    sc = R.exact_scene(V=views)
    G = R.geometry_of(sc)
    u, v, pz = R.fp32_chain(sc)
    for a, b in ((u, G.u), (v, G.v), (pz, G.pz)):
        assert np.array_equal(a.astype(np.float64), b, equal_nan=True)
    H, W = G.H, G.W
    on = lambda x, val: (x == val) & G.vis
    assert on(G.u, 0).any() and on(G.u, W - 1).any() and on(G.v, 0).any() and on(G.v, H - 1).any()
    assert ((G.u == -1) & (G.pz > 0)).any() and ((G.u == W) & (G.pz > 0)).any()          # one voxel step outside: invisible
    assert ((G.v == -1) & (G.pz > 0)).any() and ((G.v == H) & (G.pz > 0)).any()
    assert (G.pz == 0).any() and (G.pz < 0).any() and not G.vis[G.pz <= 0].any()
    assert (G.vis & (G.u % 1 == 0.5)).any() and (G.vis & (G.u % 1 == 0)).any()
    strict = R.geometry_of(sc, strict=True)
    assert (strict.vis.sum(0) != G.vis.sum(0)).any()
    # the last pixel gets weight 1: a voxel on u = W - 1 samples the last column exactly
    only0 = G.vis & (np.arange(G.V) == 0)[:, None]
    w = R.forward(G, sc["feats"], 0, 0, vis=only0)
    n = np.nonzero(on(G.u, W - 1)[0] & (G.v[0] % 1 == 0))[0]
    assert n.size
    assert np.array_equal(w.y[n], sc["feats"][0, 0][:, G.v[0, n].astype(int), W - 1].T.astype(np.float64))


@pytest.mark.parametrize("name", list(R.SCENES))
def test_band_share_is_capped(name):
    """at most 1 % of a scene's voxels have a view within 1e-4 of a frustum face, and that band is ten times the coordinate
    chain's error bound (and more)"""
    share, seen, en = R.band_stats(R.scene(name))
    assert share <= 0.01
    assert en < 1e-6 * 10
    if R.SCENES[name].get("n", (99,))[0] > 20:
        assert 0.5 < seen < 0.95

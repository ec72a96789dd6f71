"""GPU: every kernel path of the back-projection (csrc/back_project.hip) against the float64 witness of
tests/back_project_ref.py, at the edges of its tiles, scans, view counts, batches and frustum.

Rule of every comparison (compare()): where every view of a voxel is further than 1e-4 (normalised) from a frustum face, the
count, the mask, the kept set, the output order and the coords equal the witness exactly; the few voxels with a view inside that
band (<= 1 % of a case, asserted) take their decisions bit for bit from the fp32 oracle, and their features are compared with
the witness evaluated under the oracle's mask.  Every value lies within the witness's own derived bound (its docstring); each
case records err_over_bound = the worst |kernel - witness| / bound.

Worst err_over_bound per path and mode, measured on MI355X (gfx950):
    path                                 mean    mean + depth   variance (+ mean)
    bp_gather_mlp_kernel                 0.045   0.045          0.045     (worst: C = 40)
    bp_gather_kernel VEC 4               0.035   0.035          0.035     (worst: V = 20, B = 2, C = 24)
    bp_gather_kernel VEC 1               0.024   0.024          0.032     (worst: C = 7)
  tiles and scans 0.079 (n = 524,287); n = 524,288 with 29 views 0.039; view counts and min_view 0.059; batches 0.035;
  exact-arithmetic scene 0.002; constant / affine maps 0.014; backward (both entry points) 0.009; autograd wrappers < 0.001.
  (The bound's worst-case coordinate term dominates it, so a correct kernel sits at a few per cent; a 2^-10 px shift exceeds it:
  test_comparison_fails_against_a_perturbed_witness.)
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import back_project_ref as R
from oracle import back_project as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MEAN, DEPTH, VAR = R.MODE_MEAN, R.MODE_MEAN_DEPTH, R.MODE_VARIANCE
GUARD = 129

# kernel path -> the scenes (tests/back_project_ref.py: SCENES) that must reach it; confirmed per case by the name the library
# reports (eprecon_profile_gather_kernel) and by expected_kernel(), the dispatch rule restated
PATHS = {
    "bp_gather_mlp_kernel": ["mlp_c24", "mlp_c32", "mlp_c40", "mlp_c80", "mlp_c4", "mlp_c12", "mlp_c44"],          # QT 6/8/10/20, generic
    "bp_gather_kernel VEC 4": ["vec4_v21_b1_c24", "vec4_v21_b1_c32", "vec4_v32_b1_c40", "vec4_v32_b1_c80", "vec4_v32_b1_c12",
                               "vec4_v20_b2_c24", "vec4_v20_b2_c44"],
    "bp_gather_kernel VEC 1": ["vec1_c1", "vec1_c7", "vec1_c13"],
}


def expected_kernel(C, V, B):
    """gather_mlp_supported(): 4-channel lanes and the 256-voxel tile's 12 bytes per (voxel, view) within 64 KiB of LDS"""
    lds = 256 * V * 12 + ((V * B * 12 + 3) & ~3) * 4 + 256 * 3 * 4 + 4 * 4 + 16
    if C % 4 == 0 and lds <= 64 * 1024:
        return "bp_gather_mlp_kernel"
    return "bp_gather_kernel VEC 4" if C % 4 == 0 else "bp_gather_kernel VEC 1"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max(initial=0.0))


class Case:
    """a scene on the host and on the device, its witness geometry, and the visibility every comparison uses: the witness's own
    outside the band, the fp32 oracle's inside"""

    def __init__(self, sc, band=True):
        self.sc, self.G = sc, R.geometry_of(sc)
        G = self.G
        self.V, self.B, self.C, self.H, self.W = sc["feats"].shape
        self.n = sc["coords"].shape[0]
        self.band = R.in_band(G) if band else np.zeros(self.n, bool)
        assert self.band.mean() <= 0.01 if self.n else True
        self.vis = G.vis.copy()
        if self.band.any():
            rows = np.nonzero(G.in_batch)[0]
            o = O.back_project(sc["coords"][rows], sc["origin"], sc["voxel_size"], sc["feats"][:, :, :1], sc["kr"], 0, O.MODE_MEAN,
                               want_grid=True)
            mask = np.zeros_like(self.vis)
            mask[:, rows] = o["mask"]
            self.vis = np.where(self.band[None], mask, G.vis)
        use = self.vis
        if use.any():      # the band is about a hundred times the chain's error bound: ten times is asserted
            assert float((G.eu * 2 / (self.W - 1))[use].max()) < 1e-5 and float((G.ev * 2 / (self.H - 1))[use].max()) < 1e-5
        self.d = {k: _dev(sc[k]) for k in ("coords", "origin", "feats", "kr")}
        self._w = {}

    def witness(self, mode, mv):
        key = (mode, mv)
        if key not in self._w:
            self._w = {key: R.forward(self.G, self.sc["feats"], mode, mv, vis=self.vis)}
        return self._w[key]

    def run(self, mode, mv, feats=None, **kw):
        from eprecon_amd import back_project as BP
        d = self.d
        return BP.run(d["coords"], d["origin"], self.sc["voxel_size"], d["feats"] if feats is None else feats, d["kr"], mv, mode, **kw)


_cases = {}


def case(name):
    if name not in _cases:
        _cases.clear()
        _cases[name] = Case(R.scene(name))
    return _cases[name]


def compare(cs, got, w, mode):
    """-> (decisions equal, worst |kernel - witness| / bound) of one result dict of back_project.run against one witness"""
    order = w.order
    if got is None:
        return order.size == 0 or bool((np.bincount(cs.G.batch[order], minlength=cs.B) < 1).any()), 0.0
    dec = got["n_valid"] == order.size and np.array_equal(got["count"].cpu().numpy(), w.cnt.astype(np.float32))
    dec = dec and np.array_equal(got["coords"].cpu().numpy(), cs.sc["coords"][order])
    dec = dec and list(got["n_valid_per_batch"]) == np.bincount(cs.G.batch[order], minlength=cs.B).tolist()
    if dec and "mask" in got:
        dec = np.array_equal(got["mask"].cpu().numpy(), w.vis[:, order])
    if not dec:
        return False, np.inf
    r = _ratio(np.abs(got["feats"].cpu().numpy().astype(np.float64) - w.y[order]), w.bound[order])
    if "mean" in got:
        r = max(r, _ratio(np.abs(got["mean"].cpu().numpy().astype(np.float64) - w.mean[order]), w.mean_bound[order]))
    if "grid" in got:     # the image coordinates of the visible pairs: within the chain's bound (part of the decision, not of r)
        G, m = cs.G, w.vis[:, order]
        g = got["grid"].cpu().numpy().astype(np.float64)
        with np.errstate(invalid="ignore"):                                    # (rows behind a camera: inf - inf, masked out)
            rg = max(_ratio(np.abs(g[..., 0] - G.gx[:, order])[m], (G.eu[:, order] * 2 / (cs.W - 1))[m]),
                     _ratio(np.abs(g[..., 1] - G.gy[:, order])[m], (G.ev[:, order] * 2 / (cs.H - 1))[m]))
        if rg > 1.0:
            return False, np.inf
    return True, r


def reported_kernel(fn):
    """run fn() with the library's one-shot gather bracket armed -> (result, name of the gather kernel it launched)"""
    from eprecon_amd import _lib
    lib = _lib.load()
    lib.eprecon_profile_enable(2)
    try:
        out = fn()
    finally:
        name = lib.eprecon_profile_gather_kernel().decode()
        lib.eprecon_profile_enable(0)
    return out, name


# ---------------------------------------------------------------------------------------------------------------------
# the path table: every path x every mode, grid on / off, mean on / off, NCHW / channels-last, through the project's wrappers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [MEAN, DEPTH, VAR])
@pytest.mark.parametrize("name", [n for names in PATHS.values() for n in names])
def test_every_path_and_mode(name, mode, record_property):
    from eprecon_amd import back_project as BP
    cs = case(name)
    path = expected_kernel(cs.C, cs.V, cs.B)
    assert name in PATHS[path]
    w = cs.witness(mode, 2)
    assert w.order.size > 100 and (w.cnt == 2).any() and (w.cnt == 1).any()     # a count of exactly min_view and min_view - 1
    d, vs = cs.d, cs.sc["voxel_size"]
    base, kern = reported_kernel(lambda: cs.run(mode, 2, want_grid=True, want_mean=mode == VAR))
    assert kern == path.split(" ")[0]
    ok, worst = compare(cs, base, w, mode)
    assert ok
    f_cl = BP.to_channels_last(d["feats"])
    assert (cs.C == 1 or f_cl.stride()[2] == 1) and torch.equal(f_cl.contiguous(), d["feats"])
    for feats in (d["feats"], f_cl):
        for grid in (False, True):
            got = cs.run(mode, 2, feats=feats, want_grid=grid, want_mean=(mode == VAR and grid))
            ok, r = compare(cs, got, w, mode)
            assert ok
            worst = max(worst, r)
            assert torch.equal(got["feats"], base["feats"]) and ("mean" in got) == (mode == VAR and grid)
    # the wrappers of the reference's three call sites
    if mode == MEAN:
        out = BP.Back_Project(cs.C, return_projection=True).cuda()(d["coords"], d["origin"], vs, d["feats"], d["kr"], 2)
        assert torch.equal(out[0], base["feats"]) and torch.equal(out[1], base["coords"]) and torch.equal(out[4], base["count"])
        assert torch.equal(out[2], base["grid"]) and torch.equal(out[3], base["mask"])
        pend = BP.run_async(d["coords"], d["origin"], vs, d["feats"], d["kr"], 2, MEAN)
        assert torch.equal(pend.result()["feats"], base["feats"])
    elif mode == DEPTH:
        out = BP.back_project(d["coords"].float(), d["origin"], vs, d["feats"], d["kr"], 2)
        assert torch.equal(out[0], base["feats"]) and out[1].dtype == torch.float32 and torch.equal(out[1], base["coords"].float())
    else:
        out = BP.view_variance(d["coords"], d["origin"], vs, d["feats"], d["kr"], 2, min_valid=1)
        assert torch.equal(out["var"], base["feats"]) and torch.equal(out["mean"], base["mean"])
        w1 = cs.witness(VAR, 1)                                    # the variance of a voxel one view sees is exactly 0
        got1 = cs.run(VAR, 1)
        ok, r = compare(cs, got1, w1, VAR)
        one = w1.cnt[w1.order] == 1
        assert ok and one.any() and not got1["feats"][_dev(one)].any()
        worst = max(worst, r)
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# tiles and scans; the raw entry with sentinels and guard rows
# ---------------------------------------------------------------------------------------------------------------------
def raw_call(cs, mode, mv, want_grid=True):
    """eprecon_back_project_async on buffers filled with sentinels, 129 guard rows behind every output"""
    from eprecon_amd import _lib
    lib = _lib.load()
    n, V, B, C, H, W = cs.n, cs.V, cs.B, cs.C, cs.H, cs.W
    cout = C + 1 if mode == DEPTH else C
    nan = float("nan")
    t = {"feats": torch.full((n + GUARD, cout), nan, device="cuda"),
         "mean": torch.full((n + GUARD, C), nan, device="cuda") if mode == VAR else None,
         "coords": torch.full((n + GUARD, 4), -7, dtype=torch.int32, device="cuda"),
         "count": torch.full((n + GUARD,), nan, device="cuda"),
         "grid": torch.full((V * n * 2 + GUARD,), nan, device="cuda") if want_grid else None,
         "mask": torch.full((V * n + GUARD,), 77, dtype=torch.uint8, device="cuda") if want_grid else None,
         "nv": torch.full((1 + B + GUARD,), -99, dtype=torch.int32, device="cuda")}
    ws = torch.empty((lib.eprecon_back_project_workspace_bytes(n, B, V, C, H, W, 0),), dtype=torch.uint8, device="cuda")
    d = cs.d
    rc = lib.eprecon_back_project_async(
        _lib.ptr(d["coords"]), n, _lib.ptr(d["origin"]), B, float(cs.sc["voxel_size"]), _lib.ptr(d["feats"]), 0, _lib.ptr(d["kr"]),
        V, C, H, W, mv, mode, _lib.ptr(t["feats"]), _lib.ptr(t["mean"]), _lib.ptr(t["coords"]), _lib.ptr(t["count"]),
        _lib.ptr(t["grid"]), _lib.ptr(t["mask"]), _lib.ptr(t["nv"]), _lib.ptr(ws), ws.numel(), _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    nv = t["nv"].cpu().numpy()
    assert (nv[1 + B:] == -99).all()
    k = int(nv[0])
    assert torch.isnan(t["feats"][n:]).all() and (t["coords"][n:] == -7).all() and torch.isnan(t["count"][n:]).all()
    assert not torch.isnan(t["count"][:n]).any()                               # count is written for every input row
    assert torch.isnan(t["feats"][k:n]).all() and (t["coords"][k:n] == -7).all()   # and nothing behind the compacted rows
    res = {"feats": t["feats"][:k], "coords": t["coords"][:k], "count": t["count"][:n], "n_valid": k,
           "n_valid_per_batch": nv[1:1 + B].tolist()}
    if mode == VAR:
        assert torch.isnan(t["mean"][k:]).all()
        res["mean"] = t["mean"][:k]
    if want_grid:                                                              # packed with stride n_valid, not n
        assert torch.isnan(t["grid"][V * k * 2:]).all() and (t["mask"][V * k:] == 77).all()
        res["grid"], res["mask"] = t["grid"][:V * k * 2].view(V, k, 2), t["mask"][:V * k].view(V, k).bool()
        assert not torch.isnan(res["grid"]).any()
    return res


TILE_N = [1, 15, 16, 17, 255, 256, 257, 16385, 49151, 49152, 524287, 524288]


@pytest.mark.parametrize("n", TILE_N)
def test_tile_and_scan_edges(n, record_property, monkeypatch):
    """one tile and its neighbours, the second pass of the scan at tile 16 (16,385 rows = 1,025 tiles), the switches to the
    64- and the 256-voxel tile; sparse lists throughout; the tile order switch on tile counts that are no multiple of 8"""
    from eprecon_amd import back_project as BP
    cs = case(f"tile_n{n}")
    assert cs.n == n
    w = cs.witness(MEAN, 1)
    d = cs.d
    got = BP.run_async(d["coords"], d["origin"], cs.sc["voxel_size"], d["feats"], d["kr"], 1, MEAN, want_grid=n < 100000).result()
    ok, worst = compare(cs, got, w, MEAN)
    assert ok
    tile = 256 if n >= 524288 else (64 if n >= 49152 else 16)
    if -(-n // tile) % 8 != 0:                                                 # 1, 2, 17 and 1,025 tiles
        monkeypatch.setenv("EPRECON_BP_XCD_SLABS", "0")
        other = cs.run(MEAN, 1)
        monkeypatch.delenv("EPRECON_BP_XCD_SLABS")
        assert torch.equal(other["feats"], got["feats"]) and torch.equal(other["coords"], got["coords"])
    if n <= 16385:
        for mode in (MEAN, DEPTH, VAR):
            raw = raw_call(cs, mode, 1)
            ok, r = compare(cs, raw, cs.witness(mode, 1), mode)
            assert ok
            worst = max(worst, r)
    record_property("err_over_bound", worst)
    assert worst <= 1.0


def test_lds_request_of_the_256_voxel_tile_stays_within_the_device_limit(record_property):
    """524,288 rows with 29 views: bp_gather_kernel<256> would ask for 65,936 bytes of dynamic LDS, more than a workgroup may
    have without opting in; the library takes the 64-voxel tile instead.  Decisions of every row against the fp32 oracle, the
    features of every 16th row against the witness (the witness of all 15 M (voxel, view) pairs would take a minute)."""
    sc = R.scene("lds_v29")
    V, B, C, H, W = sc["feats"].shape
    assert expected_kernel(C, V, B) == "bp_gather_kernel VEC 4" and 256 * V * 8 + V * 48 + 256 * 20 + 32 > 64 * 1024
    from eprecon_amd import back_project as BP
    d = {k: _dev(sc[k]) for k in ("coords", "origin", "feats", "kr")}
    got, kern = reported_kernel(lambda: BP.run(d["coords"], d["origin"], sc["voxel_size"], d["feats"], d["kr"], 1, MEAN))
    assert kern == "bp_gather_kernel"
    o = O.back_project(sc["coords"], sc["origin"], sc["voxel_size"], sc["feats"], sc["kr"], 1, O.MODE_MEAN)
    assert got["n_valid"] == o["feats"].shape[0] and np.array_equal(got["count"].cpu().numpy(), o["count"])
    assert np.array_equal(got["coords"].cpu().numpy(), o["coords"])
    rows = np.arange(0, sc["coords"].shape[0], 16)
    G = R.geometry_of(sc, rows)
    band = R.in_band(G)
    assert band.mean() <= 0.01
    w = R.forward(G, sc["feats"], MEAN, 1)
    assert np.array_equal(w.cnt[~band], o["count"][rows][~band])
    out_row = np.cumsum(o["count"] >= 1) - 1                                   # input row -> output row
    pick = w.valid & ~band
    f = got["feats"].cpu().numpy().astype(np.float64)[out_row[rows[pick]]]
    worst = _ratio(np.abs(f - w.y[pick]), w.bound[pick])
    record_property("err_over_bound", worst)
    assert pick.sum() > 20000 and worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# views and validity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", ["0", "1", "max", "V", "V+1"])
@pytest.mark.parametrize("views", [1, 2, 9, 20, 21, 31, 32])
def test_view_counts_and_min_view(views, mv, record_property):
    cs = case(f"views_v{views}")
    cmax = int(cs.vis.sum(axis=0).max())
    m = {"0": 0, "1": 1, "max": cmax, "V": views, "V+1": views + 1}[mv]
    mode = DEPTH if mv in ("0", "max") else MEAN
    w = cs.witness(mode, m)
    got = cs.run(mode, m, want_grid=True)
    if m > cmax:
        assert got is None and w.order.size == 0                               # nothing valid: the reference's `return None`
        return
    assert (w.cnt == m).any() and (m == 0 or (w.cnt == m - 1).any())
    ok, worst = compare(cs, got, w, mode)
    assert ok
    if m == 0:                                                                 # the no-read path of run(): every row comes back
        assert got["n_valid"] == cs.n
        unseen = _dev(w.cnt == 0)
        assert unseen.any() and not got["feats"][unseen].any()                 # (the depth channel included: exactly 0)
    if mv == "1":
        k = got["n_valid"]
        met = cs.run(MEAN, 1, min_valid_per_batch=k)
        assert met is not None and met["n_valid"] == k and torch.equal(met["feats"], got["feats"])
        assert cs.run(MEAN, 1, min_valid_per_batch=k + 1) is None
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------
def _with_foreign_rows(sc):
    """rows with batch index -1 and B in front, inside and behind the list"""
    c = sc["coords"]
    B = sc["origin"].shape[0]
    bad = c[[0, 5, 9, 40]].copy()
    bad[:, 0] = [-1, B, -1, B]
    parts = [bad[:1], c[:37], bad[1:3], c[37:], bad[3:]]
    out = dict(sc)
    out["coords"] = np.ascontiguousarray(np.concatenate(parts))
    return out


@pytest.mark.parametrize("mode", [MEAN, DEPTH, VAR])
@pytest.mark.parametrize("name", ["batch_b2", "batch_b3", "vec4_v20_b2_c24"])
@pytest.mark.parametrize("foreign", [False, True])
def test_batches(name, mode, foreign, record_property):
    """a boundary inside a wave and inside a 16-row tile (70 | 200 rows), an element of 3 rows, the depth statistics per
    element; rows whose batch index is out of range are dropped: count 0, per-batch counts unaffected"""
    sc = R.scene(name)
    cs = Case(_with_foreign_rows(sc) if foreign else sc)
    w = cs.witness(mode, 2)
    got = raw_call(cs, mode, 2)
    ok, worst = compare(cs, got, w, mode)
    assert ok
    if foreign:
        out = ~cs.G.in_batch
        assert out.sum() == 4 and not got["count"].cpu().numpy()[out].any()
        plain = Case(sc).run(mode, 2)
        assert plain["n_valid_per_batch"] == got["n_valid_per_batch"] and torch.equal(plain["feats"], got["feats"])
    else:
        hi = cs.run(mode, 2, want_mean=mode == VAR)
        ok, r = compare(cs, hi, w, mode)
        assert ok and torch.equal(hi["feats"], got["feats"])
    record_property("err_over_bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("mode", [MEAN, DEPTH])
def test_batch_element_without_a_valid_row_and_with_a_single_one(mode, record_property):
    sc = R.scene("batch_b3")
    far = dict(sc)
    far["origin"] = sc["origin"].copy()
    far["origin"][1, 1] -= 50.0                                                # element 1 sees nothing
    cs = Case(far)
    w = cs.witness(mode, 1)
    assert np.bincount(cs.G.batch[w.order], minlength=3)[1] == 0
    assert cs.run(mode, 1) is None                                             # the reference returns None
    got = cs.run(mode, 1, min_valid_per_batch=0)
    ok, worst = compare(cs, got, w, mode)
    assert ok and got["n_valid_per_batch"][1] == 0
    # element 1 with one valid row: two of its three rows moved out of every frustum
    one = dict(sc)
    one["coords"] = sc["coords"].copy()
    rows = np.nonzero(one["coords"][:, 0] == 1)[0]
    G = R.geometry_of(sc)
    keep = rows[np.argmax(G.vis[:, rows].sum(axis=0))]
    for r in rows:
        if r != keep:
            one["coords"][r, 1:] = 2000
    cs = Case(one)
    w = cs.witness(mode, 2)
    assert np.bincount(cs.G.batch[w.order], minlength=3).tolist()[1] == 1
    got = cs.run(mode, 2)
    ok, r = compare(cs, got, w, mode)
    assert ok and got["n_valid_per_batch"][1] == 1
    if mode == DEPTH:                                                          # d == mu: the normalised depth of that row is exactly 0
        row = int(np.nonzero(cs.G.batch[w.order] == 1)[0][0])
        assert got["feats"][row, -1].item() == 0.0
    worst = max(worst, r)
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# exact arithmetic: no band, every decision equals the witness; frustum faces, pz == 0, pz < 0; nothing read beyond the maps
# ---------------------------------------------------------------------------------------------------------------------
EXACT = {"bp_gather_mlp_kernel": dict(C=8, V=3), "bp_gather_kernel VEC 4": dict(C=8, V=21), "bp_gather_kernel VEC 1": dict(C=7, V=3)}


def _guarded_channels_last(feats):
    """the maps channels-last inside a NaN-filled buffer: a tap read beyond either end would put NaN into the output even
    with weight 0"""
    V, B, C, H, W = feats.shape
    n = V * B * H * W * C
    buf = torch.full((n + 2 * 4096,), float("nan"), device="cuda")
    buf[4096:4096 + n] = _dev(feats.transpose(0, 1, 3, 4, 2)).reshape(-1)
    return buf[4096:4096 + n].view(V, B, H, W, C).permute(0, 1, 4, 2, 3)


@pytest.mark.parametrize("mode", [MEAN, DEPTH, VAR])
@pytest.mark.parametrize("path", list(EXACT))
def test_exact_arithmetic_scene(path, mode, record_property):
    sc = R.exact_scene(**EXACT[path])
    cs = Case(sc, band=False)
    assert expected_kernel(cs.C, cs.V, cs.B) == path
    u, v, pz = R.fp32_chain(sc)
    for a, b in ((u, cs.G.u), (v, cs.G.v), (pz, cs.G.pz)):
        assert np.array_equal(a.astype(np.float64), b, equal_nan=True)         # fp32 evaluates the chain exactly
    worst = 0.0
    for mv in (0, 1, 2):
        w = cs.witness(mode, mv)
        (got, kern) = reported_kernel(lambda: cs.run(mode, mv, feats=_guarded_channels_last(sc["feats"]), want_grid=True,
                                                     want_mean=mode == VAR))
        assert kern == path.split(" ")[0]
        ok, r = compare(cs, got, w, mode)
        assert ok and not torch.isnan(got["feats"]).any()
        worst = max(worst, r)
        # the same comparison against `<` at the frustum faces must fail
        ok_strict, _ = compare(cs, got, R.forward(R.geometry_of(sc, strict=True), sc["feats"], mode, mv), mode)
        assert not ok_strict
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# maps that remove the coordinate term
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [MEAN, VAR])
@pytest.mark.parametrize("name", ["mlp_c12", "vec4_v21_b1_c24", "vec1_c7"])
def test_constant_and_affine_maps(name, mode, record_property):
    sc = dict(R.scene(name))
    V, B, C, H, W = sc["feats"].shape
    rng = np.random.default_rng(2)
    const = rng.standard_normal((V, B, C, 1, 1)).astype(np.float32)
    sc["feats"] = np.ascontiguousarray(np.broadcast_to(const, (V, B, C, H, W)))
    cs = Case(sc)
    w = cs.witness(mode, 1)
    inner = (cs.G.margin > 1e-2).all(axis=0)[w.order]                          # (on the border the zero continuation has D > 0)
    got = cs.run(mode, 1, want_mean=mode == VAR)
    ok, worst = compare(cs, got, w, mode)
    assert ok
    f = got["feats"].cpu().numpy().astype(np.float64)
    # D = 0: the 2^-16 S term alone (the witness's bound with the coordinate errors set to zero)
    G0 = SimpleNamespace(**vars(cs.G))
    G0.eu, G0.ev = np.zeros_like(cs.G.eu), np.zeros_like(cs.G.ev)
    w0 = R.forward(G0, sc["feats"], mode, 1, vis=cs.vis)
    assert inner.sum() > 100
    worst = max(worst, _ratio(np.abs(f - w0.y[w.order])[inner], w0.bound[w.order][inner]))
    # affine ramps a x + b y: s_v = a u + b v in closed form
    a, b = rng.standard_normal((2, V, B, C, 1, 1)).astype(np.float32)
    ramp = a * np.arange(W, dtype=np.float32) + b * np.arange(H, dtype=np.float32)[:, None]
    sc["feats"] = np.ascontiguousarray(ramp.astype(np.float32))
    cs2 = Case(sc)
    got = cs2.run(MEAN, 1)
    G = cs2.G
    a64, b64 = a.astype(np.float64)[:, :, :, 0, 0], b.astype(np.float64)[:, :, :, 0, 0]    # [V, B, C]
    # (the fp32 ramp itself is rounded: the closed form is taken on the maps as stored, through the witness, and checked here)
    w2 = cs2.witness(MEAN, 1)
    order = w2.order
    bb = G.batch[order]
    s, e, t = np.zeros((order.size, C)), np.zeros((order.size, C)), np.zeros((order.size, C))
    for v in range(V):
        m = cs2.vis[v, order][:, None]
        uu, vv = G.u[v, order][:, None], G.v[v, order][:, None]
        s += m * (a64[v, bb] * uu + b64[v, bb] * vv)
        t += m * (np.abs(a64[v, bb]) * np.abs(uu) + np.abs(b64[v, bb]) * np.abs(vv))
        e += m * (np.abs(a64[v, bb]) * G.eu[v, order][:, None] + np.abs(b64[v, bb]) * G.ev[v, order][:, None])
    den = np.maximum(w2.cnt[order], 1)[:, None]
    # (the stored fp32 ramp carries three roundings of |a| x + |b| y per pixel: 4 U of that scale is added for them)
    bound = R.EPS * t / den + e / den + R.U * 4 * t / den
    ok, r = compare(cs2, got, w2, MEAN)
    assert ok
    r2 = _ratio(np.abs(got["feats"].cpu().numpy().astype(np.float64) - s / den), bound)
    worst = max(worst, r, r2)
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: the same comparison must fail against a witness that is wrong in one of four ways
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mlp_c24", "vec4_v21_b1_c24", "vec1_c7"])
def test_comparison_fails_against_a_perturbed_witness(name):
    cs = case(name)
    for mode in (MEAN, VAR):
        got = cs.run(mode, 0, want_mean=mode == VAR)
        ok, r = compare(cs, got, cs.witness(mode, 0), mode)
        assert ok and r <= 1.0
        # u shifted by 2^-10 px
        ok, r = compare(cs, got, R.forward(cs.G, cs.sc["feats"], mode, 0, vis=cs.vis, du=2.0 ** -10), mode)
        assert ok and r > 1.0
        # the denominator V instead of the visible count
        ok, r = compare(cs, got, R.forward(cs.G, cs.sc["feats"], mode, 0, vis=cs.vis, den_views=True), mode)
        assert ok and r > 1.0
        # one visible view dropped (from the features alone: the count is left as it is, so that the values are what fails)
        vis = cs.vis.copy()
        first = np.argmax(vis, axis=0)
        vis[first, np.arange(cs.n)] = False
        wd = R.forward(cs.G, cs.sc["feats"], mode, 0, vis=vis)
        wd.cnt = cs.vis.sum(axis=0)
        ok, r = compare(cs, got, wd, mode)
        assert ok and r > 1.0
    # (`<` instead of `<=` at the frustum: test_exact_arithmetic_scene, where voxels lie exactly on the faces)


# ---------------------------------------------------------------------------------------------------------------------
# backward: both entry points against the witness's adjoint, built from the witness's own visibility and weights
# ---------------------------------------------------------------------------------------------------------------------
def backward(sc, coords, mode, dout, dmean, det, ld=None):
    """-> df float32 [V, B, H, W, C] of eprecon_back_project_backward(_det)_async; dout is handed over as the first C columns
    of a NaN-filled [n, ld] buffer"""
    from eprecon_amd import _lib
    lib = _lib.load()
    V, B, C, H, W = sc["feats"].shape
    n = coords.shape[0]
    ld = C if ld is None else ld
    buf = torch.full((max(n, 1), ld), float("nan"), device="cuda")
    if n:
        buf[:n, :C] = _dev(dout.astype(np.float32))
    dm = None if dmean is None else _dev(dmean.astype(np.float32))
    cv = _dev(coords.astype(np.int32)) if n else None
    nhwc = _dev(sc["feats"].transpose(0, 1, 3, 4, 2))
    origin, kr = _dev(sc["origin"]), _dev(sc["kr"])
    df = torch.full((V, B, H, W, C), float("nan"), device="cuda")
    args = (_lib.ptr(cv), n, _lib.ptr(origin), B, float(sc["voxel_size"]), _lib.ptr(nhwc), _lib.ptr(kr), V, C, H, W, mode,
            _lib.ptr(buf) if n else None, ld, _lib.ptr(dm), _lib.ptr(df))
    if det:
        ws = torch.empty((lib.eprecon_back_project_backward_workspace_bytes(B, V, C, H, W),), dtype=torch.uint8, device="cuda")
        rc = lib.eprecon_back_project_backward_det_async(*args, _lib.ptr(ws), ws.numel(), _lib.current_stream())
    else:
        rc = lib.eprecon_back_project_backward_async(*args, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return df


def _bwd_rows(sc, mv=1):
    """the kept rows of a forward run that no band touches (the backward takes any list of voxels)"""
    G = R.geometry_of(sc)
    rows = np.nonzero(G.in_batch & (G.vis.sum(axis=0) >= mv) & ~R.in_band(G))[0]
    return rows, R.geometry_of(sc, rows)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("mode,with_dmean", [(MEAN, False), (DEPTH, False), (VAR, True), (VAR, False)])
@pytest.mark.parametrize("name", ["bwd_c1", "bwd_c7", "bwd_c24", "bwd_b2"])
def test_backward_matches_the_adjoint(name, mode, with_dmean, det, record_property):
    """C = 1 / 7 / 24, V = 1 / 9 / 32, B = 1 / 2; ld_dout wider than C; dmean present and null"""
    sc = R.scene(name)
    rows, G = _bwd_rows(sc)
    C = sc["feats"].shape[2]
    rng = np.random.default_rng(8)
    dout = rng.standard_normal((rows.size, C)).astype(np.float32)
    dmean = rng.standard_normal((rows.size, C)).astype(np.float32) if with_dmean else None
    ref, bound = R.adjoint(G, sc["feats"], mode, dout, dmean, det=det)
    df = backward(sc, sc["coords"][rows], mode, dout, dmean, det, ld=C + (1 if mode == DEPTH else 3))
    worst = _ratio(np.abs(df.cpu().numpy().astype(np.float64) - ref), bound)
    if det:
        again = backward(sc, sc["coords"][rows], mode, dout, dmean, True, ld=C + 5)
        assert torch.equal(again, df)                                          # the same bits on a second run
    if mode == VAR and not with_dmean and G.V == 1:
        assert not df.any()                                                    # one view: the variance has no gradient at all
    assert np.abs(ref).max() > 0 or G.V == 1
    record_property("err_over_bound", worst)
    assert worst <= 1.0


def test_backward_of_nothing_is_zero():
    sc = R.scene("bwd_c7")
    for det in (True, False):
        df = backward(sc, np.zeros((0, 4), np.int32), MEAN, np.zeros((0, 7), np.float32), None, det)
        assert not df.any() and not torch.isnan(df).any()


@pytest.mark.parametrize("det", [True, False])
def test_backward_marks_what_it_cannot_hold(det, record_property):
    """exact-arithmetic scene (weights are exact, so 'touched' is the same set on both sides): one Inf and one NaN in dout
    mark exactly the map elements their taps touch; so does, in the deterministic form, a finite contribution beyond the range
    of the fixed-point word (+-8.0e6, include/eprecon_hip.h); everything else stays within the bound"""
    sc = R.exact_scene(C=8, V=3)
    rows, G = _bwd_rows(sc)
    C = 8
    rng = np.random.default_rng(9)
    dout = rng.standard_normal((rows.size, C)).astype(np.float32)
    cnt = G.vis.sum(axis=0)
    idx = np.nonzero(cnt >= 2)[0]
    assert idx.size >= 10
    a, b, c = int(idx[idx.size // 5]), int(idx[idx.size // 2]), int(idx[-(idx.size // 5)])
    bad = np.zeros_like(dout)
    bad[a, 1], bad[b, 5], bad[c, 2] = 1, 1, 1
    touched = R.adjoint(G, sc["feats"], MEAN, bad)[0] > 0
    clean = dout.copy()
    clean[bad > 0] = 0
    ref, bound = R.adjoint(G, sc["feats"], MEAN, clean, det=det)
    dirty = dout.copy()
    dirty[a, 1], dirty[b, 5], dirty[c, 2] = np.inf, np.nan, (1e9 if det else 0.0)
    df = backward(sc, sc["coords"][rows], MEAN, dirty, None, det).cpu().numpy().astype(np.float64)
    if not det:
        touched = R.adjoint(G, sc["feats"], MEAN, bad * (dirty != 0))[0] > 0
    assert touched.sum() >= 6
    assert (np.isnan(df[touched]).all() if det else (~np.isfinite(df[touched])).all()) and np.isfinite(df[~touched]).all()
    worst = _ratio(np.abs(df - ref)[~touched], bound[~touched])
    if det:   # a large contribution inside the range is added, not marked
        ok = clean.copy()
        ok[c, 2] = 4.0e6
        ref2, bound2 = R.adjoint(G, sc["feats"], MEAN, ok, det=True)
        df2 = backward(sc, sc["coords"][rows], MEAN, ok, None, True).cpu().numpy().astype(np.float64)
        assert np.isfinite(df2).all()
        worst = max(worst, _ratio(np.abs(df2 - ref2), bound2))
    record_property("err_over_bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("mode", [MEAN, VAR])
def test_autograd_wrappers_carry_the_adjoint(mode, record_property):
    """autograd.back_project, Back_Project.forward and view_variance under autograd, on the exact-arithmetic scene (no band,
    so the kept rows of the forward are the witness's)"""
    from eprecon_amd import autograd as AG
    from eprecon_amd import back_project as BP
    sc = R.exact_scene(C=8, V=3)
    cs = Case(sc, band=False)
    w = cs.witness(mode, 1)
    Gv = R.geometry_of(sc, w.order)
    rng = np.random.default_rng(4)
    dout = rng.standard_normal((w.order.size, 8)).astype(np.float32)
    dmean = rng.standard_normal((w.order.size, 8)).astype(np.float32)
    ref, bound = R.adjoint(Gv, sc["feats"], mode, dout, dmean if mode == VAR else None, det=True)
    d = cs.d
    worst = 0.0
    for api in ("autograd", "module"):
        feats = d["feats"].clone().requires_grad_(True)
        if api == "autograd":
            res = AG.back_project(d["coords"], d["origin"], 0.125, feats, d["kr"], 1, mode, want_mean=mode == VAR)
            out, mean = res["feats"], res.get("mean")
        elif mode == MEAN:
            out, mean = BP.Back_Project(8)(d["coords"], d["origin"], 0.125, feats, d["kr"], 1)[0], None
        else:
            res = BP.view_variance(d["coords"], d["origin"], 0.125, feats, d["kr"], 1, min_valid=1)
            out, mean = res["var"], res["mean"]
        assert out.shape[0] == w.order.size
        loss = (out * _dev(dout)).sum() + ((mean * _dev(dmean)).sum() if mean is not None else 0.0)
        loss.backward()
        g = feats.grad.permute(0, 1, 3, 4, 2).cpu().numpy().astype(np.float64)
        worst = max(worst, _ratio(np.abs(g - ref), bound))
    record_property("err_over_bound", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# views_to_rows on its own: an exact permutation
# ---------------------------------------------------------------------------------------------------------------------
def _views_to_rows(shapes, n_views, levels=None, spoil=None):
    from eprecon_amd import _lib
    lib = _lib.load()
    d = _lib.ViewsDesc()
    d.levels, d.n_views = len(shapes) if levels is None else levels, n_views
    g = torch.Generator(device="cpu").manual_seed(5)
    src, bufs = [], []
    for l, (c, hw) in enumerate(shapes):
        maps = [torch.randn((c, hw), generator=g).cuda() for _ in range(max(n_views, 1))]
        buf = torch.full((GUARD + max(n_views, 1) * hw * c + GUARD,), -5.0, device="cuda")
        d.channels[l], d.hw[l], d.dst[l] = c, hw, buf.data_ptr() + GUARD * 4
        for v, m in enumerate(maps[:16]):
            d.src[l][v] = m.data_ptr()
        src.append(maps)
        bufs.append(buf)
    if spoil:
        spoil(d)
    rc = lib.eprecon_views_to_rows_async(ctypes.byref(d), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, src, bufs


@pytest.mark.parametrize("n_views", [1, 16])
@pytest.mark.parametrize("shapes", [[(1, 63)], [(24, 64)], [(80, 65)], [(24, 65), (1, 64)], [(80, 63), (24, 64), (1, 65)],
                                    [(1, 64), (80, 65), (24, 63)]])
def test_views_to_rows_is_an_exact_permutation(shapes, n_views):
    rc, src, bufs = _views_to_rows(shapes, n_views)
    assert rc == 0
    for (c, hw), maps, buf in zip(shapes, src, bufs):
        assert (buf[:GUARD] == -5.0).all() and (buf[-GUARD:] == -5.0).all()    # guard words around each destination
        rows = buf[GUARD:-GUARD].view(n_views, hw, c)
        assert torch.equal(rows, torch.stack(maps).permute(0, 2, 1).contiguous())


def test_views_to_rows_refuses_bad_arguments():
    from eprecon_amd import _lib
    ok = [(24, 64), (8, 63)]

    def field(name, l, value):
        def f(d):
            getattr(d, name)[l] = value
        return f
    assert _views_to_rows(ok, 2)[0] == 0
    assert _views_to_rows(ok, 2, levels=0)[0] == -1 and _views_to_rows(ok, 2, levels=4)[0] == -1
    assert _views_to_rows(ok, 0)[0] == -1 and _views_to_rows(ok, 17)[0] == -1
    for spoil in (field("channels", 1, 0), field("hw", 0, 0), field("dst", 1, None), lambda d: d.src[1].__setitem__(1, None)):
        rc, _, bufs = _views_to_rows(ok, 2, spoil=spoil)
        assert rc == -1 and all((b == -5.0).all() for b in bufs)               # refused before any launch
    rc, _, bufs = _views_to_rows([(253, 64)], 1)                               # 253 x 65 floats of LDS: more than 64 KiB
    assert rc == -3 and (bufs[0] == -5.0).all()
    assert _lib.load().eprecon_views_to_rows_async(None, _lib.current_stream()) == -1

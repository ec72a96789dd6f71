"""GPU: Occupancy_Initialization.forward as composed — 2D fusion stack, view-variance volume, submanifold stack — on every path
it has, and its backward under autograd, against the float64 restatement of tests/occupancy_init_ref.py; not against a second
float32 run of the same code, where a mistake shared by two paths cancels.

One set of inputs and one witness per case (occupancy_init_cases.py).  The witness evaluates with the KERNEL's visibility
(back_project.run(..., want_grid=True)["mask"]), which may differ from the witness's own only at (view, row) pairs inside
back_project_ref.BAND of a frustum face (asserted); the returned coordinates and view counts equal that visibility's.  Every
element of `out`, `fused`, `var` and of every gradient is compared: error = max |got - float64| / scale, bound = FACTOR x TWIN
(test_occupancy_init_witness_host.py pins the constants, their ceilings and that eight composition mistakes exceed 10 x the
bound).  Each measured error is printed with its bound and handed to record_property.

Observed on an MI355X, worst err / bound over the quantities of a test (bound = 4 x TWIN; no (view, row) decision inside the band
differed from the witness's own on any case):
  case A forward     default (first call and second replay) 0.34, direct launches 0.34, EPRECON_INIT_GLUE=0 0.34,
                     MIOpen 2D stack 0.39, kernel-map layers 0.34, `between` 0.34   (out 0.27, fused 0.17, var 0.34)
  case B forward     0.51 (out 0.26, fused 0.16, var 0.51)
  case R forward     out 0.62, fused 0.22, var 1.51 -> 0.76 of its widened bound
  case A gradients   180 quantities: 0.55 and below, and grad:norm4.weight at 1.50 -> 0.75 of its widened bound
  selection          A 410, B 755, R 4,039 cells: equal to the witness's selection (R: 2 free voxels, both selections equal)
The two quantities over 1 are bounded by 8 x TWIN, with figures and reasons in occupancy_init_cases.WIDENED: the twin's variance
volume is float64 by construction, so TWIN["var"] lacks the variance kernel's own float32 arithmetic (0.048 of the bound its own
witness derives for it); the twin's one-element sum for norm4's weight gradient cancelled to a tenth of what its terms' errors
allow.  No defect was found in eprecon_amd/."""
import contextlib
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import back_project_ref as BR  # noqa: E402
import occupancy_init_cases as C  # noqa: E402
import occupancy_init_ref as R  # noqa: E402
from oracle import grid_ops as OG  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def tapped(net, kernels=None):
    """while a forward of `net` runs: keep a copy of the fused maps handed to the variance volume and of the variance rows
    handed to the submanifold stack; kernels (a dict): the convolution kernel of every launch, under "2d" / "3d" """
    from eprecon_amd import _lib
    from eprecon_amd import back_project as BP
    tap = {"fused": None, "var": []}
    saved = {fn: getattr(BP, fn) for fn in ("run_async", "view_variance")}
    lib = _lib.load()
    launches = {fn: getattr(lib, fn) for fn in ("eprecon_conv_desc_async", "eprecon_sparse_conv_fused_async")}
    phase = ["2d"]

    def variance(orig):
        def call(coords, origin, voxel_size, fused, *args, **kw):
            tap["fused"] = fused.detach().clone()
            return orig(coords, origin, voxel_size, fused, *args, **kw)
        return call

    def launch(orig):
        def call(*args):
            rc = orig(*args)
            kernels.setdefault(phase[0], set()).add(_lib.last_conv_kernel())
            return rc
        return call

    stack = net.sparse_stack

    def sparse_stack(var, vset):
        tap["var"].append(var.detach().clone())
        phase[0] = "3d"
        try:
            return stack(var, vset)
        finally:
            phase[0] = "2d"

    try:
        for fn, orig in saved.items():
            setattr(BP, fn, variance(orig))
        if kernels is not None:
            for fn, orig in launches.items():
                setattr(lib, fn, launch(orig))
        net.sparse_stack = sparse_stack
        yield tap
    finally:
        for fn, orig in {**saved}.items():
            setattr(BP, fn, orig)
        for fn, orig in launches.items():
            setattr(lib, fn, orig)
        del net.__dict__["sparse_stack"]


class Bench:
    """a case on the device, the kernel's visibility for it, and the witness under that visibility"""

    def __init__(self, name):
        from eprecon_amd import back_project as BP
        self.case = case = C.Case(name)
        self.coords = dev(case.coords)
        if case.batch == 1:         # the dense raster of generate_grid, tagged as such: the gather writes the rank volume
            self.coords = BP.mark_dense(self.coords, case.shape, C.INTERVAL)
        self.origin, self.kr = dev(case.origin), dev(case.kr)
        self.maps = [dev(f) for f in case.feats]            # level 0 (1/4), 1 (1/8), 2 (1/16): [V, B, C, h, w]
        n = case.coords.shape[0]
        # visibility does not depend on the maps: one channel of zeros, every row kept (min_view 0)
        zeros = torch.zeros((C.N_VIEWS, case.batch, 1, case.h8, case.w8), device="cuda")
        res = BP.run(dev(case.coords), self.origin, C.VOXEL_SIZE, zeros, self.kr, 0, BP.MODE_MEAN, min_valid_per_batch=0,
                     want_grid=True)
        assert res["n_valid"] == n and np.array_equal(res["coords"].cpu().numpy(), case.coords)
        mask = res["mask"].cpu().numpy()
        self.vis, self.flips = [], 0
        for b, rows in enumerate(case.rows):
            G = case.G[b]
            vis = mask[:, rows]
            differs = vis != G.vis
            assert not (differs & (G.margin > BR.BAND)).any(), "the kernel decides a view outside the band otherwise"
            self.flips += int(differs.sum())
            self.vis.append(vis)
        self.q64, self.info = case.quantities(C.F64, vis=self.vis)
        self.valid_coords = case.valid_coords(self.info)
        self.count = np.zeros(n, np.float32)
        for rows, cnt in zip(case.rows, self.info["cnt"]):
            self.count[rows] = cnt
        self.net = copy.deepcopy(case.net).cuda().train()
        assert all(m.eps == R.BN_EPS for m in self.net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
        assert all(m.eps == R.LN_EPS for m in self.net.modules() if isinstance(m, torch.nn.LayerNorm))
        self._default = None

    def features(self, maps=None):
        """the reference's list over views of [1/4, 1/8, 1/16] maps, each [B, C, h, w]"""
        maps = self.maps if maps is None else maps
        return [[maps[l][v] for l in range(3)] for v in range(C.N_VIEWS)]

    def forward(self, net, between=None, maps=None, kernels=None):
        """-> (quantities {out, fused, var}, coords, count) of one forward, or None"""
        with tapped(net, kernels) as tap:
            out = net(self.coords, self.origin, C.VOXEL_SIZE, self.features(maps), self.kr, self.case.shape, 1, C.MIN_VIEW,
                      between=between)
        if out is None:
            return None
        occ, coords, count = out
        assert np.array_equal(coords.cpu().numpy(), self.valid_coords), "the kept rows are not the visibility's"
        assert np.array_equal(count.cpu().numpy(), self.count), "the view counts are not the visibility's"
        return {"out": occ, "fused": tap["fused"], "var": torch.cat(tap["var"])}, coords, count

    def default(self):
        """the default path, run twice (graphed: capture + first replay, then the second replay); cached for the case"""
        if self._default is None:
            kernels = {}
            with torch.no_grad():
                first = self.forward(self.net, kernels=kernels)
                first = ({k: v.clone() for k, v in first[0].items()},) + first[1:]
                second = self.forward(self.net)
            self._default = dict(first=first, second=second, kernels=kernels, dense_map=self.net.dense_map)
        return self._default


_benches = {}


def bench(name):
    if name not in _benches:
        _benches[name] = Bench(name)
    return _benches[name]


def check(record_property, tag, got, b):
    """every quantity of `got` within its bound (FACTOR x TWIN: cases.bound) of the float64 witness; prints and records each"""
    name = b.case.name
    err = C.errors(got, b.q64)
    bad, worst = [], 0.0
    for q, e in err.items():
        bound = C.bound(name, q)
        worst = max(worst, e / bound)
        print(f"{tag} {q}: err {e:.3e} bound {bound:.3e} ratio {e / bound:.2f}")
        record_property(f"{tag} {q}", f"err {e:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((round(e / bound, 2), q))
    print(f"{tag}: worst err / bound {worst:.2f}")
    record_property(f"{tag} worst err / bound", f"{worst:.2f}")
    assert not bad, f"{tag}: {len(bad)} of {len(err)} quantities over their bound, worst {sorted(bad)[-5:]}"


# ---------------------------------------------------------------------------------------------------------------------
# forward

@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_default_path(name, record_property):
    """the default path of every case: the HIP 2D stack through its graph (first and second replay), the count half beside it and
    the rank volume from the gather (one batch element), the dense-grid 3x3x3 layers, norm4 from the logit layer's summaries"""
    b = bench(name)
    print(f"case {name}: {b.flips} (view, row) decisions inside the band differ from the witness's own")
    assert b.net.use_hip_graph and b.net.use_hip_conv
    d = b.default()
    assert (d["dense_map"] is not None) == (b.case.batch == 1)
    assert d["kernels"]["2d"] and any(k.startswith("conv3d") for k in d["kernels"]["3d"]), d["kernels"]
    check(record_property, f"case {name} default, first call", d["first"][0], b)
    check(record_property, f"case {name} default, second replay", d["second"][0], b)


def _path(name, b, monkeypatch):
    """-> (net, forward keyword arguments, what must hold afterwards) of one path on case A"""
    from eprecon_amd import sparse as SP
    net, kw, after = b.net, {}, lambda: True
    if name == "direct":
        monkeypatch.setattr(net, "use_hip_graph", False)
    elif name == "no_glue":
        monkeypatch.setenv("EPRECON_INIT_GLUE", "0")
    elif name == "miopen":          # (its own copy: the MIOpen path turns the module's weights channels-last)
        net = copy.deepcopy(b.case.net).cuda().train()
        net.use_hip_conv = False
    elif name == "kernel_map":
        monkeypatch.setattr(SP, "DENSE_MIN_FILL", 1.5)
        after = lambda: net.dense_map is None
    elif name == "between":
        called = []
        kw["between"] = lambda: called.append(1)
        after = lambda: called == [1]
    return net, kw, after


@pytest.mark.parametrize("path", ["direct", "no_glue", "miopen", "kernel_map", "between"])
def test_forward_paths_on_case_a(path, monkeypatch, record_property):
    """direct launches in place of the graph; EPRECON_INIT_GLUE=0; the MIOpen 2D stack; the kernel-map 3x3x3 layers; a `between`
    callback (the variance volume queued, its count read later)"""
    b = bench("A")
    net, kw, after = _path(path, b, monkeypatch)
    kernels = {}
    with torch.no_grad():
        got = b.forward(net, kernels=kernels, **kw)
    assert got is not None and after()
    if path == "kernel_map":
        assert not any(k.startswith("conv3d") for k in kernels["3d"]), kernels["3d"]       # (the dense-grid family)
    if path == "miopen":
        assert "2d" not in kernels, kernels
    check(record_property, f"case A {path}", got[0], b)


def test_a_batch_element_below_the_guard_returns_none(monkeypatch):
    from eprecon_amd import occupancy_initialization as OI
    b = bench("B")
    counts = [int(v.sum()) for v in b.info["valid"]]
    assert min(counts) >= OI.INIT_MIN_VALID and counts[0] != counts[1]
    monkeypatch.setattr(OI, "INIT_MIN_VALID", min(counts) + 1)      # above the smaller element's count, not the larger one's
    with torch.no_grad():
        assert b.forward(b.net) is None
    monkeypatch.setattr(OI, "INIT_MIN_VALID", min(counts))
    with torch.no_grad():
        assert b.forward(b.net) is not None


def test_case_r_reaches_the_kernels_of_the_production_size():
    """case R's layers go to the kernels written down for it, and those cover what 640 x 480 / 96^3 reaches"""
    d = bench("R").default()
    for part in ("2d", "3d"):
        assert sorted(d["kernels"][part]) == sorted(C.KERNELS_R[part]), d["kernels"][part]
        assert set(C.KERNELS_R[part]) >= set(C.KERNELS_PRODUCTION[part]) and C.KERNELS_PRODUCTION[part]


# ---------------------------------------------------------------------------------------------------------------------
# gradients

def _backward(b, net):
    maps = [m.clone().requires_grad_() for m in b.maps]
    net.zero_grad(set_to_none=True)
    got, _, _ = b.forward(net, maps=maps)
    occ = got["out"]
    assert occ.requires_grad and got["fused"] is not None
    dout = dev(b.case.dout_rows[b.info["valid"][0]].astype(np.float32)).reshape(-1, 1)
    (occ * dout).sum().backward()
    got.update({"grad:" + n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    got.update({"grad:" + n: maps[l].grad[:, 0].clone() for l, n in enumerate(("feat4", "feat8", "feat16"))})
    return got


def test_gradients_on_case_a(record_property):
    """the recording path (PyTorch 2D modules, autograd.back_project in variance mode, the recording sparse operators):
    d sum(logit * dout) / d (every parameter, the 27 input maps) against the three-segment float64 chain; every parameter of
    the branch gets a gradient and nothing else does; a second backward gives the same bits"""
    b = bench("A")
    net = copy.deepcopy(b.case.net).cuda().train()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        got = _backward(b, net)
        again = _backward(b, net)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert set(got) == set(b.q64), set(got) ^ set(b.q64)
    assert {n for n in got if n.startswith("grad:") and "feat" not in n} == {"grad:" + n for n, _ in net.named_parameters()}
    check(record_property, "case A gradients", got, b)
    different = [n for n in got if not torch.equal(got[n], again[n])]
    assert not different, different[:10]


# ---------------------------------------------------------------------------------------------------------------------
# selection

def _rows(a):
    return set(map(tuple, np.asarray(a).tolist()))


@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_selection_lies_between_the_witness_selections(name, record_property):
    """OR-pool, erosion and dilation are monotone, so the stage-0 selection is monotone in the marks: the selection of the
    witness logits with the free voxels (within the bound of `out` of logit(0.3)) forced off is a subset of the GPU's, which
    is a subset of the one with them forced on — set equality when no voxel is free.  List form and rank-volume form."""
    from eprecon_amd import grid_ops as GO
    b = bench(name)
    case, d = b.case, b.default()
    dim = case.shape[0] // 2
    free = C.free_voxels(name, b.q64)
    logit = b.q64["out"].reshape(-1).numpy()
    lower = _rows(OG.init_select(np.where(free, -30.0, logit).astype(np.float32), b.valid_coords, case.batch, dim=dim))
    upper = _rows(OG.init_select(np.where(free, 30.0, logit).astype(np.float32), b.valid_coords, case.batch, dim=dim))
    assert lower <= upper and len(lower) > 0 and len(upper) < case.batch * dim ** 3, "the selection keeps nothing, or everything"
    record_property(f"case {name} free voxels", int(free.sum()))
    got, coords, _ = d["second"]
    forms = [None] + ([d["dense_map"]] if d["dense_map"] is not None else [])
    for dense in forms:
        sel, per_batch = GO.init_select(got["out"], coords, case.batch, dim=dim, cell=4, threshold=C.THRESHOLD, dense=dense)
        sel = sel.cpu().numpy()
        assert sum(per_batch) == sel.shape[0] == len(_rows(sel))
        assert lower <= _rows(sel) <= upper, (len(lower), sel.shape[0], len(upper))
        # and it is the oracle's selection of the GPU's own logits
        assert np.array_equal(sel, OG.init_select(got["out"].cpu().numpy(), b.valid_coords, case.batch, dim=dim))
    print(f"case {name}: {int(free.sum())} free voxels, selection {len(lower)} <= {sel.shape[0]} <= {len(upper)} cells")

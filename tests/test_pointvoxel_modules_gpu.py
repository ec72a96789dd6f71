"""GPU: SPVCNN, ConvGRU and one GRUFusion level as they run under autograd (the recording path training uses) and on their
inference paths, against float64 autograd of the plain restatement in tests/pointvoxel_modules_ref.py — not against a second
float32 run of the same module code, where a composition mistake cancels.

Every element of every output, input gradient and parameter gradient is compared; error = max |got - float64| / scale (block
scales: pointvoxel_modules_cases.py), bound = FACTOR x TWIN (cases.bound), TWIN being the float32-CPU twin's own distance from float64
(test_pointvoxel_modules_host.py pins the constants, their ceilings and that six composition mistakes exceed 10 x the bound).
Each measured error is printed with its bound and handed to record_property.

Observed on an MI355X, worst err / bound over the quantities of a test (bound = 4 x TWIN):
  SPVCNN forward     A: recording 0.11, issued 0.13, native 0.13      B: recording 0.08, issued 0.07, native 0.07
  SPVCNN gradients   A: 0.31 (85 tensors)                             B: 0.25 (85 tensors)
  ConvGRU forward    0.17 - 0.19 on every case, literal mode and path (fused, recording)
  ConvGRU gradients  A literal 0.23, A own 0.23, B literal 0.41, B own 0.27
  fusion level       scale 1: fragment 1 0.30, fragment 2 0.28 + one bias gradient at 1.29
                     scale 2: fragment 1 0.60, fragment 2 0.23 + one bias gradient at 1.02
The two bias gradients over 1 are torch's own dy.sum(0) one float32 ulp from a twin that landed within a tenth of an ulp; they
are bounded by 8 x TWIN, stated with the figures in pointvoxel_modules_cases.WIDENED.  No defect was found in eprecon_amd/."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pointvoxel_modules_cases as C  # noqa: E402
import pointvoxel_modules_ref as R  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(record_property, tag, got, q64, kind, key, prefix=""):
    """every quantity of `got` within its bound (FACTOR x TWIN: cases.bound) of the float64 witness; prints and records each"""
    err = C.errors({prefix + k: v for k, v in got.items()}, q64)
    bad, worst = [], 0.0
    for name, e in err.items():
        bound = C.bound(kind, key, name)
        worst = max(worst, e / bound)
        print(f"{tag} {name}: err {e:.3e} bound {bound:.3e} ratio {e / bound:.2f}")
        record_property(f"{tag} {name}", f"err {e:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((round(e / bound, 2), name))
    print(f"{tag}: worst err / bound {worst:.2f}")
    record_property(f"{tag} worst err / bound", f"{worst:.2f}")
    assert not bad, f"{tag}: {len(bad)} of {len(err)} quantities over their bound, worst {sorted(bad)[-5:]}"


def param_grads(net, prefixes=("",)):
    return {"grad:" + n: p.grad for n, p in net.named_parameters() if n.startswith(prefixes)}


# ---------------------------------------------------------------------------------------------------------------------
# SPVCNN

@pytest.fixture(scope="module", params=sorted(C.SPVCNN_CASES))
def spvcnn_case(request):
    case = C.SpvcnnCase(request.param, *C.SPVCNN_CASES[request.param])
    with C.one_thread():
        case.q64 = case.quantities(C.F64)
    case.gpu = copy.deepcopy(case.net).cuda()
    assert all(m.eps == R.BN_EPS for m in case.gpu.modules() if isinstance(m, torch.nn.BatchNorm1d))
    return case


def _points(case, feat=None):
    from eprecon_amd import torchsparse_utils as TU
    from eprecon_amd.tensor import PointTensor
    TU.clear_voxelization_cache()
    return PointTensor(dev(case.feat) if feat is None else feat, dev(case.pts))


def test_spvcnn_forward_on_three_paths(spvcnn_case, monkeypatch, record_property):
    """recording, the Python-issued inference pass and the one-call native pass, each against the float64 forward"""
    from eprecon_amd import modules as M
    case, net = spvcnn_case, spvcnn_case.gpu
    rec = net(_points(case))
    assert rec.requires_grad
    with torch.no_grad():
        monkeypatch.setattr(M, "_NATIVE_SPVCNN", False)
        issued = net(_points(case))
        monkeypatch.setattr(M, "_NATIVE_SPVCNN", True)
        taken = []
        native_pass = net._forward_native
        monkeypatch.setattr(net, "_forward_native", lambda z: taken.append(native_pass(z)) or taken[-1])
        native = net(_points(case))
    assert net.native_ready() and len(taken) == 1 and taken[0] is native, "the one-call native pass was not taken"
    for tag, out in (("recording", rec), ("issued", issued), ("native", native)):
        check(record_property, f"spvcnn {case.name} {tag}", {"out": out}, case.q64, "spvcnn", case.name)


def test_spvcnn_gradients(spvcnn_case, record_property):
    """d (tanh(out) * probe).sum() / d (input features, every parameter) against float64 autograd, every element"""
    case, net = spvcnn_case, spvcnn_case.gpu
    x = dev(case.feat).requires_grad_()
    net.zero_grad(set_to_none=True)
    out = net(_points(case, x))
    (torch.tanh(out) * dev(case.probe)).sum().backward()
    got = {"out": out, "grad:input": x.grad, **param_grads(net)}
    assert set(got) == set(case.q64)
    check(record_property, f"spvcnn {case.name} gradients", got, case.q64, "spvcnn", case.name)


# ---------------------------------------------------------------------------------------------------------------------
# ConvGRU

@pytest.fixture(scope="module", params=[(n, lit) for n in sorted(C.GRU_CASES) for lit in (True, False)],
                ids=lambda p: f"{p[0]}-{'literal' if p[1] else 'own'}")
def gru_case(request):
    name, literal = request.param
    case = C.GruCase(name, *C.GRU_CASES[name], literal)
    with C.one_thread():
        case.q64 = case.quantities(C.F64)
    case.gpu = copy.deepcopy(case.net).cuda()
    return case


def _gru_inputs(case, monkeypatch):
    from eprecon_amd import torchsparse_utils as TU
    monkeypatch.setattr(TU, "LITERAL_CONVR", case.literal)
    TU.clear_voxelization_cache()
    return dev(case.h), dev(case.x), dev(case.pts)


def test_convgru_forward_fused_and_recording(gru_case, monkeypatch, record_property):
    from eprecon_amd.tensor import PointTensor
    case, net = gru_case, gru_case.gpu
    h, x, pts = _gru_inputs(case, monkeypatch)
    with torch.no_grad():
        fused = net(PointTensor(h.clone(), pts), PointTensor(x.clone(), pts))
    h, x, pts = _gru_inputs(case, monkeypatch)
    rec = net(PointTensor(h.clone(), pts), PointTensor(x.clone(), pts))
    assert rec.requires_grad and not fused.requires_grad
    for tag, out in (("fused", fused), ("recording", rec)):
        check(record_property, f"convgru {case.name} literal={case.literal} {tag}", {"out": out}, case.q64, "convgru",
              (case.name, case.literal))


def test_convgru_gradients(gru_case, monkeypatch, record_property):
    """d out.square().mean() / d (h, x, every parameter of convz, convr, convq); the module gets clones of h and x, whose .F
    it overwrites"""
    from eprecon_amd.tensor import PointTensor
    case, net = gru_case, gru_case.gpu
    h, x, pts = _gru_inputs(case, monkeypatch)
    h.requires_grad_()
    x.requires_grad_()
    net.zero_grad(set_to_none=True)
    out = net(PointTensor(h.clone(), pts), PointTensor(x.clone(), pts))
    out.square().mean().backward()
    got = {"out": out, "grad:h": h.grad, "grad:x": x.grad, **param_grads(net)}
    assert set(got) == set(case.q64)
    check(record_property, f"convgru {case.name} literal={case.literal} gradients", got, case.q64, "convgru",
          (case.name, case.literal))


# ---------------------------------------------------------------------------------------------------------------------
# one GRUFusion level: fragment 0 seeds the map under no_grad, fragments 1 and 2 run under autograd

@pytest.fixture(scope="module", params=[1, 2])
def fusion_walk(request):
    """the float64 walk and the module's walk, both run once; the module's results are checked by the tests below"""
    from eprecon_amd import torchsparse_utils as TU
    scale = request.param
    case = C.FusionCase(scale, literal=TU.LITERAL_CONVR)
    with C.one_thread():
        ref = case.walk(C.F64)
    fus = copy.deepcopy(case.net).cuda()
    steps = []
    for k, fr in enumerate(case.frags):
        TU.clear_voxelization_cache()
        inputs = {"fragment": ["f"], "scene": ["scene0"], "vol_origin": dev(case.origin[None]),
                  "vol_origin_partial": dev(fr["origin_partial"][None]), "world_to_aligned_camera": dev(C.W2AC[None])}
        vin = dev(fr["values"])
        if k == 0:
            with torch.no_grad():
                fus(dev(fr["coords"]), vin, inputs, scale)
            steps.append(None)
            continue
        vin.requires_grad_()
        fus.zero_grad(set_to_none=True)
        coords, values, _, _ = fus(dev(fr["coords"]), vin, inputs, scale)
        map_c, map_f = fus.global_volume[scale].export()
        values.square().mean().backward()
        steps.append(dict(vin=vin, coords=coords, values=values, map_c=map_c, map_f=map_f, grad_in=vin.grad.clone(),
                          q={"out": values.detach(), "grad:values_in": vin.grad.clone(),
                             **{k_: v.clone() for k_, v in param_grads(fus, case.prefixes).items()}}))
    q64 = {f"f{k}:{name}": t for k, s in enumerate(ref) if k for name, t in s["q"].items()}
    return case, ref, steps, q64


@pytest.mark.parametrize("k", [1, 2])
def test_fusion_level_fragment(fusion_walk, k, record_property):
    """values and the gradients of values_in and of the level's two ConvGRUs against fuse_level in float64; rows of values_in
    outside the union get exactly zero; the map holds values.detach() for the appended rows bit for bit"""
    case, ref, steps, q64 = fusion_walk
    got, want = steps[k], ref[k]
    n = len(want["updated"])
    assert np.array_equal(got["coords"].cpu().numpy()[:, 1:], want["updated"] * case.interval)
    assert min(want["kinds"]) > 0 if k == 1 else True
    assert set(f"f{k}:{name}" for name in got["q"]) == set(name for name in q64 if name.startswith(f"f{k}:"))
    check(record_property, f"fusion scale {case.scale} fragment {k}", got["q"], q64, "fusion", case.scale, prefix=f"f{k}:")
    unused = torch.from_numpy(want["unused"]).cuda()
    assert int(unused.sum()) > 0 and not got["grad_in"][unused].any(), "a row outside the union has a gradient"
    assert np.array_equal(got["map_c"].cpu().numpy(), want["map_C"])
    assert torch.equal(got["map_f"][-n:], got["values"].detach()), "the map does not hold the fused rows"


def test_fusion_map_rows_are_state(fusion_walk):
    """fragment 2's backward leaves fragment 1's leaf gradient bit-identical: no graph reaches back through the map"""
    _, _, steps, _ = fusion_walk
    assert torch.equal(steps[1]["vin"].grad, steps[1]["grad_in"])
    assert steps[1]["values"].grad_fn is not None and not steps[2]["map_f"].requires_grad

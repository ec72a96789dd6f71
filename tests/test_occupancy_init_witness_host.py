"""CPU: the float64 restatement of the occupancy-initialisation branch (tests/occupancy_init_ref.py) that
test_occupancy_init_witness_gpu.py holds Occupancy_Initialization.forward against — is it the right function, how far is its own
float32 twin from it, and does a bound of FACTOR x that distance tell a wrong composition from a right one?

  * independence: at float32 the sparse half agrees with oracle/occupancy_init.py (numpy) and oracle/torch_cpu.py, the 2D stack
    with the package's own modules run on the CPU, each within the GPU bound of that quantity (two float32 evaluations of one
    function in two summation orders);
  * every TWIN constant of occupancy_init_cases.py is recomputed: recomputed <= constant <= 2 x recomputed, and every
    FACTOR x TWIN lies under its ceiling (1e-3 of the logit range forward, 2e-3 for gradients);
  * the cases hold what they are for: rows with a view inside the band <= 1 % of the cells, "free" voxels (witness logit
    within the bound of `out` of logit(0.3)) <= 0.5 % of the valid ones, >= 1000 valid voxels per batch element (INIT_MIN_VALID
    unpatched), fill >= DENSE_MIN_FILL;
  * eight composition mistakes, one at a time in the float64 restatement, each move the NAMED quantity by >= 10 x its bound;
  * the three segments of branch_gradients are one adjoint: <J x, y> = <x, J^T y> in float64."""
import numpy as np
import pytest
import torch

import occupancy_init_cases as C
import occupancy_init_ref as R


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in C.SPECS:
        case = C.Case(name)
        case.q64, case.info = case.quantities(C.F64)
        with C.one_thread():
            case.twin = C.errors(case.quantities(C.F32)[0], case.q64)
        out[name] = case
    return out


# ---------------------------------------------------------------------------------------------------------------------
# independence

def test_sparse_half_matches_both_oracles_at_float32(cases):
    from oracle import occupancy_init as OI
    from oracle import torch_cpu as TC
    for name, case in cases.items():
        start = 0
        for b in range(case.batch):
            valid = case.info["valid"][b]
            n = int(valid.sum())
            coords = case.coords[case.rows[b]][valid]
            var = case.q64["var"][start:start + n].to(C.F32)
            with C.one_thread(), torch.no_grad():
                got = R.sparse_stack(case.sd, var, coords, C.F32, C.INTERVAL).numpy().astype(np.float64)
                sd = {k: v for k, v in case.sd.items() if v.is_floating_point()}
                ref_t = TC.sparse_stack(sd, var, TC.kernel_map_pairs(coords, C.INTERVAL)).numpy()
            scale = float(np.abs(got).max())
            d = {"torch_cpu": float(np.abs(got - ref_t).max()) / scale}
            if name == "A":         # (the numpy oracle walks a Python-level hash: the smallest case only)
                ref_n = OI.sparse_stack({k: v.numpy() for k, v in sd.items()}, var.numpy(), coords.astype(np.int32), C.INTERVAL)
                d["numpy"] = float(np.abs(got - ref_n).max()) / scale
            print(f"case {name} b {b}: sparse half, distance from the oracles {d}, bound {C.bound(name, 'out'):.2e}")
            assert max(d.values()) <= C.bound(name, "out")
            start += n


def test_fusion_stack_matches_the_modules_on_the_cpu_at_float32(cases):
    for name in ("A", "B"):
        case = cases[name]
        for b in range(case.batch):
            f4, f8, f16 = (torch.from_numpy(case.feats[l][:, b]) for l in range(3))
            with C.one_thread(), torch.no_grad():
                got = R.fusion2d(case.sd, f16, f8, f4, C.F32)
                ref = case.net.feat_fusion_pre(f16, f8, f4)
            d = float((got - ref).abs().max()) / float(ref.abs().max())
            print(f"case {name} b {b}: fusion stack, distance from the modules {d:.2e}, bound {C.bound(name, 'fused'):.2e}")
            assert tuple(got.shape) == (C.N_VIEWS, C.CH_DOWN, case.h8, case.w8) and d <= C.bound(name, "fused")
    assert all(m.eps == R.BN_EPS for m in cases["A"].net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    assert all(m.eps == R.LN_EPS for m in cases["A"].net.modules() if isinstance(m, torch.nn.LayerNorm))


# ---------------------------------------------------------------------------------------------------------------------
# twin constants and ceilings

def test_twin_constants_are_the_measured_distances(cases):
    assert set(C.TWIN) == set(cases)
    bad = []
    for name, case in cases.items():
        assert set(C.TWIN[name]) == set(case.twin) == set(case.q64), name
        for q, measured in case.twin.items():
            if not measured <= C.TWIN[name][q] <= 2 * measured:
                bad.append((name, q, measured, C.TWIN[name][q]))
    assert not bad, bad[:10]


def test_quantities_of_case_a_cover_every_parameter(cases):
    case = cases["A"]
    names = {"grad:" + n for n, _ in case.net.named_parameters()}
    assert names | {"out", "fused", "var", "grad:feat16", "grad:feat8", "grad:feat4"} == set(case.q64) and len(names) == 174
    blocks = {C.group_of(n) for n in names}
    assert blocks == {"self_fusion_1x", "self_fusion_2x", "self_fusion_4x", "fusion_down", "post_fusion_1", "post_fusion_2",
                      "post_fusion_3", "post_fusion_4", "similary_1", "norm0", "stage1", "stage2", "stage3", "stage4"}


def test_gpu_bounds_stay_under_the_suites_ceilings(cases):
    worst = {C.FORWARD_CEILING: 0.0, C.GRADIENT_CEILING: 0.0}
    for name in cases:
        for q in C.TWIN[name]:
            assert 0 < C.bound(name, q) <= C.ceiling(q), (name, q)
            worst[C.ceiling(q)] = max(worst[C.ceiling(q)], C.bound(name, q))
    for (name, q), factor in C.WIDENED.items():      # a widened bound is a power of two over FACTOR of a real quantity
        assert factor in (8, 16, 32) and q in C.TWIN[name]
    print(f"largest bounds: forward {worst[C.FORWARD_CEILING]:.3e}, gradient {worst[C.GRADIENT_CEILING]:.3e}")
    assert C.ceiling("out") == C.ceiling("fused") == C.ceiling("var") == 1e-3 and C.ceiling("grad:feat8") == 2e-3
    assert C.FACTOR == 4


# ---------------------------------------------------------------------------------------------------------------------
# the cases hold what they are for

def test_case_conditions(cases):
    from eprecon_amd import config, dense2d, sparse
    for name, case in cases.items():
        free = C.free_voxels(name, case.q64)
        n_valid = sum(int(v.sum()) for v in case.info["valid"])
        assert free.shape[0] == n_valid and free.mean() <= 0.005, (name, int(free.sum()))
        for b in range(case.batch):
            valid, band = case.info["valid"][b], case.in_band()[b]
            print(f"case {name} b {b}: {int(valid.sum())} of {valid.size} valid, {int(band.sum())} rows in the band, "
                  f"{int(free.sum())} free voxels in the case")
            assert band.mean() <= 0.01
            assert valid.sum() >= config.INIT_MIN_VALID == 1000
            assert valid.mean() >= sparse.DENSE_MIN_FILL
            assert band.sum() > 0 and not valid.all(), "the case has no undecided view, or no hole in the grid"
    assert sparse.DENSE_MIN_FILL == 0.4
    # case R: the three pixel lists lie on the three sides of the row thresholds of the 2D stack's kernel selection
    r = cases["R"]
    lists = sorted(C.N_VIEWS * (r.height // s) * (r.width // s) for s in (4, 8, 16))
    assert lists == [6912, 27648, 110592]
    thresholds = (dense2d.DIRECT_2D_MIN_ROWS, dense2d.K1_DIRECT_2D_MIN_ROWS, dense2d.SHORT_2D_MAX_ROWS)
    assert lists[0] < min(thresholds) <= lists[1] < max(thresholds) <= lists[2]
    a = cases["A"]
    assert (a.h8 % 2, a.w8 % 2) == (0, 0) and (a.h8 // 2) % 2 == 1 and (a.w8 // 2) % 2 == 1, "odd 1/16 maps"


# ---------------------------------------------------------------------------------------------------------------------
# the bound discriminates

# perturbation -> (the quantity it is shown on, the quantities it must leave exactly alone)
MISTAKES = {"norm0_unbiased": ("grad:norm0.weight", ("fused", "var")), "den_views": ("var", ("fused",)), "level_order": ("fused", ()),
            "align_corners": ("fused", ()), "elan2d_swap": ("fused", ()), "elan3d_swap": ("out", ("fused", "var")),
            "ln_of_relu": ("out", ("fused", "var")), "residual2d_form": ("fused", ())}


@pytest.mark.parametrize("perturb", sorted(MISTAKES))
def test_mistakes_exceed_the_bound(cases, perturb):
    assert set(MISTAKES) == set(R.PERTURBATIONS)
    case = cases["A"]
    name, untouched = MISTAKES[perturb]
    moved = C.errors(case.quantities(C.F64, perturb=perturb, grads=name.startswith("grad:"))[0], case.q64)
    print(f"{perturb}: " + ", ".join(f"{k} moved {moved[k] / C.bound('A', k):.1f} x bound" for k in ("out", "fused", "var", name)))
    assert moved[name] >= 10 * C.bound("A", name)
    assert all(moved[k] == 0 for k in untouched)


# ---------------------------------------------------------------------------------------------------------------------
# the three segments are one adjoint

def test_chain_adjoint_identity(cases):
    """x: a direction in the 27 input maps; J x through the 2D stack and the sparse stack by forward-mode differentiation, through
    the variance by the central difference of back_project_ref.forward (exact for a quadratic form); J^T y: branch_gradients"""
    case = cases["A"]
    G, coords, valid = case.G[0], case.coords, case.info["valid"][0]
    rng = np.random.default_rng(21)
    f4, f8, f16 = (R.tens(case.feats[l][:, 0], C.F64) for l in range(3))
    x16, x8, x4 = (R.tens(rng.standard_normal(tuple(t.shape)), C.F64) for t in (f16, f8, f4))
    sd = {k: R.tens(v, C.F64) for k, v in case.sd.items() if v.is_floating_point()}
    fused, t1 = torch.func.jvp(lambda a, b, c: R.fusion2d(sd, a, b, c, C.F64), (f16, f8, f4), (x16, x8, x4))
    up = R.variance(G, fused + t1, C.MIN_VIEW).y[valid]
    dn = R.variance(G, fused - t1, C.MIN_VIEW).y[valid]
    t2 = R.tens((up - dn) / 2, C.F64)
    vox = R.Voxels(coords[valid], C.INTERVAL)
    out, t3 = torch.func.jvp(lambda v: R.sparse_stack(sd, v, coords[valid], C.F64, C.INTERVAL, vox=vox), (case.q64["var"],), (t2,))
    assert torch.equal(out, case.q64["out"])
    dout = R.tens(case.dout_rows[valid].reshape(-1, 1), C.F64)
    lhs = float((t3 * dout).sum())
    terms = [x * case.q64["grad:" + n] for n, x in (("feat16", x16), ("feat8", x8), ("feat4", x4))]
    rhs = float(sum(t.sum() for t in terms))
    size = float(sum(t.abs().sum() for t in terms))
    print(f"<J x, y> = {lhs:.15e}, <x, J^T y> = {rhs:.15e}, difference {abs(lhs - rhs):.2e}, sum of |terms| {size:.3e}")
    assert abs(lhs) > 1e-3 * size / np.sqrt(sum(t.numel() for t in terms)), "the two sides are both nothing"
    assert abs(lhs - rhs) <= 1e-11 * size

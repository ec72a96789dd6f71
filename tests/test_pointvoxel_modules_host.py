"""CPU: the float64 restatement of SPVCNN, ConvGRU and one GRUFusion level (tests/pointvoxel_modules_ref.py) that
test_pointvoxel_modules_gpu.py holds the HIP modules against — is it the right function, how far is its own float32 twin from
it, and does a bound of FACTOR x that distance tell a wrong composition from a right one?

  * forward == the numpy oracle (oracle/spvcnn.py: spvcnn_forward, convgru) on every case, within FACTOR x TWIN["out"]: the
    oracle is one more float32 evaluation in one more summation order, which is what the twin distance measures;
  * every TWIN_* constant of pointvoxel_modules_cases.py is recomputed: recomputed <= constant <= 2 x recomputed;
  * every GPU bound FACTOR x TWIN stays under the ceilings the suite already uses for the same paths (1e-3 forward, 2e-3
    gradients);
  * six composition mistakes, one at a time in the float64 restatement, each move a compared quantity by >= 10 x its bound;
  * the cases hold what they are for (the conditions of the cloud and of the fusion walk)."""
import numpy as np
import pytest

import pointvoxel_modules_cases as C
from oracle import spvcnn as ON


def _measured(case):
    with C.one_thread():
        case.q64 = case.quantities(C.F64)
        case.twin = C.errors(case.quantities(C.F32), case.q64)
    return case


@pytest.fixture(scope="module")
def spvcnn_cases():
    return {n: _measured(C.SpvcnnCase(n, *a)) for n, a in C.SPVCNN_CASES.items()}


@pytest.fixture(scope="module")
def gru_cases():
    return {(n, lit): _measured(C.GruCase(n, *a, lit)) for n, a in C.GRU_CASES.items() for lit in (True, False)}


@pytest.fixture(scope="module")
def fusion_cases():
    out = {}
    for scale in (1, 2):
        case = C.FusionCase(scale)
        with C.one_thread():
            case.steps = case.walk(C.F64)
        out[scale] = _measured(case)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases hold what they are for

def test_cloud_conditions():
    pts = C.cloud()
    g = C.R.SpvcnnGeometry(pts, 1, C.RES)
    assert len(pts) <= 1500 and pts.dtype == np.float32
    assert (g.vox[:, 1:].max(0) - g.vox[:, 1:].min(0) + 1 <= 16).all() and g.frame.side <= 16
    assert (g.vox[:, 1:].min(0) < 0).all() and (g.vox[:, 1:].max(0) > 0).all() and len(np.unique(g.vox[:, 0])) == 3
    assert min(len(g.c1), len(g.c2), len(g.c4)) >= 2 and len(g.c1) > len(g.c2) > len(g.c4)
    xyz = g.scaled[:, :3]
    on_face = (xyz == np.floor(xyz)) & (xyz != 0)
    below = np.nextafter(xyz, np.float32(np.inf), dtype=np.float32) == np.ceil(xyz)
    assert on_face.sum() >= 20 and (below & ~on_face).sum() >= 20, "points on voxel faces and one ulp below them"
    for idx in (g.idx1, g.idx4):
        assert (idx < 0).any() and (idx >= 0).any(1).all(), "absent corners, but never all eight"
    assert np.bincount(g.inv1).max() >= 50, "one crowded voxel"


def test_convgru_geometry_conditions(gru_cases):
    for (name, literal), case in gru_cases.items():
        first, second = case.geometry.first, case.geometry.second
        assert len(first[1]) >= 2 and len(second[1]) >= 2 and len(first[1]) != len(second[1])
        assert (first[3] < 0).any() and (second[3] < 0).any()
        if literal:      # the stale tables: the first set's indices and weights, whatever the second set holds there
            assert second[4] is first[4] and not np.array_equal(first[1], second[1])


def test_fusion_walk_conditions(fusion_cases):
    for scale, case in fusion_cases.items():
        s0, s1, s2 = case.steps
        assert s0["kinds"][0] == 0 and s0["kinds"][2] == 0 and s0["kinds"][1] > 0
        assert min(s1["kinds"]) > 0, "fragment 1's union holds rows only in the map, only in the fragment, and in both"
        assert min(s2["kinds"]) > 0 and s1["unused"].sum() > 0 and s2["unused"].sum() > 0
        assert len(C.R.GruGeometry(s1["pts"], 1, case.vres, True).second[1]) >= 2


def test_packed_frame_keeps_every_neighbour():
    """PackedFrame lays the clusters of a spread-out voxel set side by side: every voxel keeps exactly its 27 neighbours"""
    from oracle import sparse as OS
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([rng.integers(0, 2, (300, 1)), rng.integers(-40, 40, (300, 3)) * rng.choice([1, 1, 9], (300, 1))],
                                    1), axis=0)
    rows = np.concatenate([rows, [[0, 200, 200, 200], [0, 201, 201, 199], [1, 200, 200, 200]]])
    rows = rows[np.unique(rows, axis=0, return_index=True)[1]]
    frame = C.R.PackedFrame(rows)
    x = rng.standard_normal((len(rows), 3))
    w = rng.standard_normal((27, 3, 2))
    got = C.R.DR.subm_conv3(frame, rows, x, w).numpy()
    nbr = OS.kernel_map(rows, rows, 3, 1)
    assert (nbr >= 0).sum() > len(rows), "no voxel has a neighbour: the case checks nothing"
    ref = np.zeros((len(rows), 2))
    for k in range(27):
        m = nbr[k] >= 0
        ref[m] += x[nbr[k][m]] @ w[k]
    np.testing.assert_allclose(got, ref, atol=1e-12)
    assert np.prod(frame.shape) < 40 * len(rows)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement is the oracle's function

def _oracle_distance(out64, ref):
    return float(np.abs(out64.numpy() - ref).max()) / float(out64.abs().max())


def test_spvcnn_forward_matches_oracle(spvcnn_cases):
    for name, case in spvcnn_cases.items():
        ref = ON.spvcnn_forward({k: v.numpy() for k, v in case.sd.items()}, case.feat, case.pts, 1, case.vres)
        d = _oracle_distance(case.q64["out"], ref)
        print(f"spvcnn {name}: oracle distance {d:.3e}, bound {C.bound('spvcnn', name, 'out'):.3e}")
        assert d <= C.bound("spvcnn", name, "out")


def test_convgru_forward_matches_oracle(gru_cases):
    for (name, literal), case in gru_cases.items():
        sd = {"g." + k: v.numpy() for k, v in case.sd.items()}
        ref = ON.convgru(sd, "g", case.h, case.x, case.pts, 1, case.vres, literal=literal)
        d = _oracle_distance(case.q64["out"], ref)
        print(f"convgru {name} literal={literal}: oracle distance {d:.3e}")
        assert d <= C.bound("convgru", (name, literal), "out")


def test_fusion_level_forward_matches_oracle(fusion_cases):
    for scale, case in fusion_cases.items():
        sd = {k: v.numpy() for k, v in case.sd.items()}
        cv = C.CH_VOXEL[scale]
        for k, s in enumerate(case.steps):
            fv = ON.convgru(sd, f"fusion_nets_voxel.{scale}", s["h"][:, :cv], s["x"][:, :cv], s["pts"], 1, case.vres, literal=True)
            fi = ON.convgru(sd, f"fusion_nets_img.{scale}", s["h"][:, cv:], s["x"][:, cv:], s["pts"], 1, case.vres, literal=True)
            d = _oracle_distance(s["out"].detach(), np.concatenate([fv, fi], 1))
            print(f"fusion scale {scale} fragment {k}: oracle distance {d:.3e}")
            assert d <= C.bound("fusion", scale, f"f{max(k, 1)}:out")


# ---------------------------------------------------------------------------------------------------------------------
# twin constants and ceilings

def _all_cases(spvcnn_cases, gru_cases, fusion_cases):
    """(kind, key, TWIN table, measured case) of every case"""
    for kind, table, cases in (("spvcnn", C.TWIN_SPVCNN, spvcnn_cases), ("convgru", C.TWIN_CONVGRU, gru_cases),
                               ("fusion", C.TWIN_FUSION, fusion_cases)):
        assert set(table) == set(cases)
        for key, case in cases.items():
            yield kind, key, table[key], case


def test_twin_constants_are_the_measured_distances(spvcnn_cases, gru_cases, fusion_cases):
    bad = []
    for kind, key, table, case in _all_cases(spvcnn_cases, gru_cases, fusion_cases):
        assert set(table) == set(case.twin) == set(case.q64), key
        for name, measured in case.twin.items():
            if not measured <= table[name] <= 2 * measured:
                bad.append((key, name, measured, table[name]))
    assert not bad, bad[:10]


def test_gpu_bounds_stay_under_the_suites_ceilings(spvcnn_cases, gru_cases, fusion_cases):
    worst = {C.FORWARD_CEILING: 0.0, C.GRADIENT_CEILING: 0.0}
    for kind, key, table, _ in _all_cases(spvcnn_cases, gru_cases, fusion_cases):
        for name in table:
            assert 0 < C.bound(kind, key, name) <= C.ceiling(name), (key, name)
            worst[C.ceiling(name)] = max(worst[C.ceiling(name)], C.bound(kind, key, name))
    for (kind, key, name), factor in C.WIDENED.items():      # a widened bound is a power of two over FACTOR of a real quantity
        assert factor in (8, 16, 32) and name in C.twin_table(kind, key)
    print(f"largest bounds: forward {worst[C.FORWARD_CEILING]:.3e}, gradient {worst[C.GRADIENT_CEILING]:.3e}")
    assert C.ceiling("out") == 1e-3 == C.ceiling("f1:out") and C.ceiling("grad:h") == 2e-3 == C.ceiling("f2:grad:values_in")


# ---------------------------------------------------------------------------------------------------------------------
# the bound discriminates

def _moved(case, kind, key, perturb):
    """largest (movement of a quantity under the perturbation) / (its GPU bound)"""
    moved = C.errors(case.quantities(C.F64, perturb), case.q64)
    return max(moved[name] / C.bound(kind, key, name) for name in moved)


@pytest.mark.parametrize("perturb", ["unbiased_var", "drop_up1_skip", "swap_concat"])
def test_spvcnn_mistakes_exceed_the_bound(spvcnn_cases, perturb):
    assert _moved(spvcnn_cases["A"], "spvcnn", "A", perturb) >= 10


@pytest.mark.parametrize("perturb", ["swap_z", "no_r"])
def test_convgru_mistakes_exceed_the_bound(gru_cases, perturb):
    assert _moved(gru_cases[("B", True)], "convgru", ("B", True), perturb) >= 10


def test_a_gradient_through_the_map_exceeds_the_bound(fusion_cases):
    case = fusion_cases[1]
    moved = C.errors(case.quantities(C.F64, "map_grad"), case.q64)
    assert all(v == 0 for name, v in moved.items() if name.startswith("f1:") or name == "f2:out"), "only fragment 2's gradients move"
    assert max(moved[name] / C.bound("fusion", 1, name) for name in moved) >= 10

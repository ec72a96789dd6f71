"""Pins the float64 witness of the TSDF integration (tests/tsdf_ref.py) itself: against the fp32 oracle (oracle/tsdf_fusion.py,
itself pinned to the reference's TSDFVolumeTorch) under the assertion the GPU module (tests/test_tsdf_edges_gpu.py) applies to the
kernel, in both variants, on the sweep cases of that module; the share of voxels it leaves undecided; what the cases cover; and its
closed forms where every fp32 step is exact.  CPU only."""
import numpy as np
import pytest

import tsdf_ref as R
from oracle import tsdf_fusion as OT

F32 = np.float32
UNDECIDED_CAP = 0.10


def oracle_fuse(case, variant, obs=1.0):
    mats = R.mats_of(case, variant)
    tsdf, weight = np.ones(case["dims"], F32), np.zeros(case["dims"], F32)
    for v in range(len(case["depths"])):
        OT.integrate(tsdf, weight, case["origin"], case["voxel_size"], case["depths"][v], case["intrs"][v], mats[v], case["trunc"],
                     obs, variant)
    return tsdf, weight, (tsdf < F32(0.999)) & (tsdf > F32(-0.999)) & (weight > 1)


def witness(case, variant, obs=1.0):
    return R.fuse(case["dims"], case["origin"], case["voxel_size"], case["depths"], case["intrs"], R.mats_of(case, variant),
                  case["trunc"], obs, variant)


@pytest.mark.parametrize("variant", ["torch", "cuda"])
@pytest.mark.parametrize("name", list(R.SWEEP))
def test_witness_agrees_with_the_fp32_oracle(name, variant, record_property):
    case = R.sweep_case(name)
    wit = witness(case, variant)
    undecided = 1.0 - float(wit.decided.mean())
    print(f"{name} {variant}: undecided share {undecided:.4f}")
    record_property("undecided_share", undecided)
    assert undecided <= UNDECIDED_CAP           # a condition on the derivation of the bands, not a measurement
    tsdf, weight, occ = oracle_fuse(case, variant)
    ratio = R.check(wit, tsdf, weight, occ)
    print(f"{name} {variant}: max |tsdf - tsdf64| / E = {ratio:.3f}")
    record_property("observed_over_bound", ratio)
    # fuse_views is the same loop with the data pipeline's occupancy rule
    ft, fw, focc = OT.fuse_views(case["dims"], case["origin"], case["voxel_size"], case["depths"], case["intrs"],
                                 R.mats_of(case, variant), margin=R.MARGIN, variant=variant)
    assert np.array_equal(ft, tsdf) and np.array_equal(fw, weight) and np.array_equal(focc, occ)


@pytest.mark.parametrize("obs", [0.5, 2.0])
def test_witness_agrees_with_the_oracle_at_other_observation_weights(obs):
    case = R.sweep_case("23x17x29")
    for variant in ("torch", "cuda"):
        wit = witness(case, variant, obs)
        R.check(wit, *oracle_fuse(case, variant, obs))
        assert set(np.unique(wit.weight / obs)) <= set(range(len(case["depths"]) + 1))


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_sweep_cases_cover_what_they_are_for(name):
    case = R.sweep_case(name)
    wit = witness(case, "torch")
    observed = float((wit.weight > 0).mean())
    assert 0.30 <= observed <= 0.90, observed
    occ64, sure = R.occupancy(wit)
    assert (occ64 & sure & wit.decided).sum() > 100
    k = case["intrs"][0]
    assert k[0, 0] != k[1, 1] and case["depths"].shape[1] != case["depths"].shape[2]
    # every branch of the update is taken: dist clipped to 1, dist inside (-1, 1), a view skipped by the truncation or the depth
    assert (wit.tsdf[wit.weight > 0] == 1.0).any() and (np.abs(wit.tsdf) < 0.5).any() and (wit.tsdf < 0).any()
    assert len(np.unique(wit.weight)) > 3
    # with obs = 0.5 two views do not make a cell occupied; with 2 one view does
    half, twice = witness(case, "torch", 0.5), witness(case, "torch", 2.0)
    assert R.occupancy(half)[0].sum() < occ64.sum() < R.occupancy(twice)[0].sum()
    assert not R.occupancy(half)[0][half.weight == 1.0].any() and (half.weight == 1.0).any()


def test_witness_is_exact_where_fp32_is():
    """identity pose, power-of-two sizes: u = ix exactly, depth by column -> dist = (d - 1) / 1; the bands stay open off the ties"""
    W, H = 6, 2
    depth = (1.0 + (1.0 + np.arange(W)[None, :] + W * np.arange(H)[:, None]) / 64.0).astype(F32)[None]
    intr = np.array([[[4, 0, 0], [0, 4, 0], [0, 0, 1]]], F32)
    eye = np.eye(4, dtype=F32)[None]
    for variant in ("torch", "cuda"):
        wit = R.fuse((W + 1, H, 1), (0, 0, 1), 0.25, depth, intr, eye, 1.0, 1.0, variant)
        assert wit.decided.all()
        want = np.ones((W + 1, H, 1))
        want[:W, :, 0] = (depth[0].T.astype(np.float64) - 1.0)
        assert np.array_equal(wit.tsdf, want) and np.array_equal(wit.weight[:, :, 0], (want[:, :, 0] < 1).astype(float))
        assert wit.E.max() <= 16 * R.U
        # on a tie (u = ix - 1/2) nothing is decided, in front of the camera; behind it everything is
        intr_tie = intr.copy()
        intr_tie[0, 0, 2] = -0.5
        assert not R.fuse((W + 1, H, 1), (0, 0, 1), 0.25, depth, intr_tie, eye, 1.0, 1.0, variant).decided.any()
        assert R.fuse((W + 1, H, 1), (0, 0, -1), 0.25, depth, intr_tie, eye, 1.0, 1.0, variant).decided.all()


def test_oracle_follows_fminf_under_a_nan_depth():
    """the reference's CUDA kernel takes fminf(1, diff / trunc): a NaN pixel, which only the "cuda" form lets through, gives 1"""
    depth = np.array([[np.nan, 2.0]], F32)
    intr = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    for variant, want_t, want_w in (("cuda", [1.0, 0.25], [1.0, 1.0]), ("torch", [1.0, 0.25], [0.0, 1.0])):
        tsdf, weight = np.full((2, 1, 1), 0.5, F32), np.zeros((2, 1, 1), F32)
        OT.integrate(tsdf, weight, (0, 0, 1), 1.0, depth, intr, np.eye(4, dtype=F32), 4.0, 1.0, variant)
        want_t = [0.5 if (variant == "torch" and i == 0) else t for i, t in enumerate(want_t)]
        assert tsdf.reshape(-1).tolist() == want_t and weight.reshape(-1).tolist() == want_w


@pytest.mark.parametrize("variant", ["torch", "cuda"])
def test_hand_results_of_the_constructed_cases_are_the_oracles(variant):
    """the results written out by hand in tests/test_tsdf_edges_gpu.py (pixel ties, camera plane, truncation, depth values),
    bit for bit; and the two variants differ exactly where the cases say they do"""
    from test_tsdf_edges_gpu import CONSTRUCTED, oracle_of_constructed, same_bits
    for name, case in CONSTRUCTED.items():
        tsdf, weight = oracle_of_constructed(case, variant)
        want_t, want_w = case["want"][variant]
        assert same_bits(tsdf, want_t) and same_bits(weight, want_w), name
    for name in ("tie_u", "tie_v", "depth_values"):
        assert not same_bits(CONSTRUCTED[name]["want"]["torch"][0], CONSTRUCTED[name]["want"]["cuda"][0])

"""Writes tests/golden/transform_space.npz from the reference's own RandomTransformSpace (datasets/transforms.py:122-429),
run on the CPU under ref_shim on the seeded samples of tests/transform_ref.py.  Build container only.

    python tests/golden/make_transform_golden.py

Per case (transform_ref.CASES) the file holds the small host quantities — random_r, random_t, T, T^-1 as the reference
handed it to transform(), the transformed extrinsics and their torch.inverse, vol_origin_partial — and the five target
lists (colour and labels as uint8: the inputs are integer valued).  Inputs are not stored: they come from the seed.
The generator refuses to write a file whose cases do not exercise the rule (assertions in check_case).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

torch = ref_shim.install()
import transform_ref as R  # noqa: E402
from datasets import transforms as T  # noqa: E402


def run_case(name):
    rot, trans, seed, panoptic, scene_origin = R.CASES[name]
    torch.manual_seed(seed)
    pad_xy, pad_z = R.paddings(rot, trans)
    rts = T.RandomTransformSpace(list(R.N_VOX), R.VOXEL_SIZE, rot, trans, pad_xy, pad_z, max_epoch=R.MAX_EPOCH)
    inp = R.case_inputs(name)
    seen = {}
    inner = rts.transform

    def capture(data, transform=None, old_origin=None):
        seen["Tinv"] = transform.clone()
        return inner(data, transform, old_origin=old_origin)

    rts.transform = capture
    out = rts(R.sample_dict(inp, torch))
    # T itself: the same call on identity poses, stopped in front of the volume work (T @ I is exact)
    probe = R.sample_dict(inp, torch)
    probe["extrinsics"] = torch.eye(4).repeat(R.VIEWS, 1, 1)
    rts.transform = lambda data, transform=None, old_origin=None: data
    t_mat = rts(probe)["extrinsics"][0].clone()
    assert torch.equal(t_mat.inverse(), seen["Tinv"])
    rec = {"random_r": rts.random_r.numpy(), "random_t": rts.random_t.numpy(), "T": t_mat.numpy(), "Tinv": seen["Tinv"].numpy(),
           "extrinsics": out["extrinsics"].numpy(), "world2cam": torch.stack([torch.inverse(e) for e in out["extrinsics"]]).numpy(),
           "vol_origin_partial": out["vol_origin_partial"].numpy()}
    for l in range(3):
        rec[f"tsdf_{l}"] = out["tsdf_list"][l].numpy()
        rec[f"occ_{l}"] = out["occ_list"][l].numpy()
        if panoptic:
            for key in ("rgb", "semantic", "instance"):
                v = out[f"{key}_list"][l].numpy()
                assert np.array_equal(v, v.astype(np.uint8))
                rec[f"{key}_{l}"] = v.astype(np.uint8)
    check_case(name, inp, rec, out)
    return rec


def check_case(name, inp, rec, out):
    # the fragment origin is not decided by a rounding tie: center / 8 (round in x, y; floor in z)
    bnds = torch.zeros((3, 2))
    bnds[:, 0], bnds[:, 1] = np.inf, -np.inf
    for i in range(R.VIEWS):
        pts = T.get_view_frustum(3.0, (R.IMG_H, R.IMG_W), torch.from_numpy(inp["intrinsics"][i]), out["extrinsics"][i])
        bnds[:, 0] = torch.min(bnds[:, 0], pts.min(dim=1)[0])
        bnds[:, 1] = torch.max(bnds[:, 1], pts.max(dim=1)[0])
    center = np.array([(bnds[0, 1] + bnds[0, 0]) / 2, (bnds[1, 1] + bnds[1, 0]) / 2, -0.2], np.float64) / R.VOXEL_SIZE / 8
    frac = center - np.floor(center)
    tie = min(abs(frac[0] - 0.5), abs(frac[1] - 0.5), frac[2], 1 - frac[2])
    assert tie >= 0.05, (name, center)
    crossing = 0
    for l in range(3):
        ref = R.crop_f64(R.N_VOX, R.VOXEL_SIZE, rec["vol_origin_partial"], rec["Tinv"], inp["vol_origin"], l,
                         inp["tsdf_list_full"][l], *(inp[k][l] if k in inp else None
                                                     for k in ("rgb_list_full", "semantic_list_full", "instance_list_full")))
        inside, band = 1 - ref["outside"].mean(), ref["in_band"].mean()
        crossing += int(ref["crossing"].sum())
        print(f"{name} level {l}: inside {inside:.3f} in-band {band:.3f} crossing {int(ref['crossing'].sum())} "
              f"excluded {ref['excluded'].mean():.4f} z-frac {ref['z_frac']:.3f} occ {rec[f'occ_{l}'].mean():.3f}")
        if l < 2:
            assert 0.25 <= inside <= 0.9 and band >= 0.1, (name, l, inside, band)
        assert ref["z_frac"] > 0.01, (name, l, ref["z_frac"])
        got = {"tsdf": rec[f"tsdf_{l}"], **{k: rec[f"{k}_{l}"] for k in ("rgb", "semantic", "instance") if f"{k}_{l}" in rec}}
        R.compare(got, ref, ref["excluded"], f"{name} level {l} (reference against float64)")
    assert crossing > 0, name


def main():
    out = {}
    for name in R.CASES:
        for k, v in run_case(name).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "transform_space.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()

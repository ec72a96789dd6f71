"""CPU-only: the float64 oracle of the panoptic export (tests/label_transfer_ref.py) against the reference's own run recorded
in tests/golden/semantic_instance.npz, and the host half of eprecon_amd/generate_semantic_instance.py (the file writer, the
refusal of CPU tensors)."""
import os

import numpy as np
import pytest
import torch

import label_transfer_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "semantic_instance.npz")))


@pytest.fixture(scope="module")
def brute(golden):
    g = golden
    return R.brute_force(g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"])


def test_fixture_shape(golden):
    g = golden
    assert g["semantic"].shape == (13, 10, 7) and g["vertices"].shape == (3000, 3) and g["vertices"].dtype == np.float32
    assert g["origin"].dtype == np.float32 and g["voxel_size"].dtype == np.float64
    assert sorted(np.unique(g["instance"]).tolist()) == [0, 7, 14, 21, 28]


def test_mapping_is_the_reference_table():
    from eprecon_amd import generate_semantic_instance as GSI
    assert list(GSI.SCANNET20_MAPPING) == R.SCANNET20.tolist() and len(GSI.SCANNET20_MAPPING) == 21


def test_brute_force_equals_reference_for_every_vertex(golden, brute):
    """cap on vertices left out: 0 (the generator asserted that no vertex is within a relative 1e-9 of a tie)"""
    assert not (brute["second"] <= brute["d2"] * (1.0 + 1e-9)).any()
    assert (brute["semantic"] == golden["ref_semantic"]).all()
    ids = np.unique(brute["instance"])
    assert golden["ref_masks"].shape == (len(ids), 3000)
    for row, k in zip(golden["ref_masks"], ids):
        assert (row == (brute["instance"] == k)).all()


def test_vote_oracle_equals_reference_lines(golden, brute):
    ids, classes, counts = R.vote(brute["semantic"], brute["instance"])
    assert classes.tolist() == golden["ref_instance_class"].tolist()
    assert counts.tolist() == golden["ref_masks"].sum(1).tolist()


def test_vote_oracle_tie_goes_to_first_seen_class():
    """a "smallest class id" rule would give 3 for instance 40"""
    ids, classes, counts = R.vote(R.TIE_SEM, R.TIE_INS)
    assert ids.tolist() == [0, 40] and classes.tolist() == [4, 9] and counts.tolist() == [3, 4]


def test_write_submission_bytes(golden, brute, tmp_path):
    from eprecon_amd import generate_semantic_instance as GSI
    ids, classes, _ = R.vote(brute["semantic"], brute["instance"])
    files = GSI.write_submission(str(tmp_path), "s0", brute["semantic"], brute["instance"], ids, classes)
    read = lambda *p: (tmp_path.joinpath(*p)).read_bytes()
    assert read("semantic", "s0.txt") == golden["semantic_txt"].tobytes()
    assert read("instance", "s0.txt") == golden["instance_txt"].tobytes()
    for i, row in enumerate(golden["mask_txt"]):
        assert read("instance", "predicted_masks", f"s0_{i:03d}.txt") == row.tobytes()
    assert len(files) == 2 + len(golden["mask_txt"]) and all(os.path.exists(f) for f in files)
    assert sorted(os.listdir(tmp_path / "instance" / "predicted_masks")) == [f"s0_{i:03d}.txt" for i in range(len(ids))]


def test_write_submission_accepts_tensors_and_negative_ids(tmp_path):
    from eprecon_amd import generate_semantic_instance as GSI
    sem, ins = torch.tensor([12, 0, 39], dtype=torch.int32), torch.tensor([-3, 200, -3], dtype=torch.int32)
    GSI.write_submission(str(tmp_path), "x", sem, ins, torch.tensor([-3, 200]), torch.tensor([12, 0]))
    assert (tmp_path / "semantic" / "x.txt").read_bytes() == b"12\n0\n39\n"
    assert (tmp_path / "instance" / "predicted_masks" / "x_000.txt").read_bytes() == b"1\n0\n1\n"
    assert (tmp_path / "instance" / "predicted_masks" / "x_001.txt").read_bytes() == b"0\n1\n0\n"
    assert (tmp_path / "instance" / "x.txt").read_text() == ("predicted_masks/x_000.txt 12 1.0000\n"
                                                             "predicted_masks/x_001.txt 0 1.0000\n")


def test_module_refuses_cpu_tensors():
    from eprecon_amd import _lib
    from eprecon_amd import generate_semantic_instance as GSI
    vol = torch.zeros((4, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.EpreconError):
        GSI.transfer_labels(vol, vol, (0.0, 0.0, 0.0), 0.04, torch.zeros((5, 3)))
    with pytest.raises(_lib.EpreconError):
        GSI.instance_table(torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32))


def test_search_walked_on_the_host(tmp_path):
    """the search helpers of csrc/label_transfer.hip are host + device C++: tests/label_transfer_host_walk.cpp walks them in
    the thread form and the (emulated) wave form against a brute force, exact ties included, and checks every shell
    enumeration — the kernels' control flow, bounds and tie rule without a GPU"""
    import subprocess
    from eprecon_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "walk")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17",
                           "-ffp-contract=off", "-I", build.CSRC, "-x", "hip",
                           os.path.join(root, "tests", "label_transfer_host_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout[-2000:]

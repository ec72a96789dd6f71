"""GPU: the panoptic export (eprecon_amd/generate_semantic_instance.py, csrc/label_transfer.hip) against the float64 oracle of
tests/label_transfer_ref.py and the reference's own run recorded in tests/golden/semantic_instance.npz: every vertex, every
kernel path, exact ties, the smallest shapes, the empty scene, a class id out of range, the vote, and the files end to end."""
import os

import numpy as np
import pytest
import torch

import label_transfer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("index", "dist", "semantic", "instance")


@pytest.fixture(scope="module")
def GSI():
    from eprecon_amd import generate_semantic_instance
    return generate_semantic_instance


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "semantic_instance.npz")))


@pytest.fixture(scope="module")
def brute(golden):
    g = golden
    return R.brute_force(g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"])


def transfer(GSI, sem, ins, origin, voxel_size, verts, **kw):
    out = GSI.transfer_labels(torch.as_tensor(sem).to(DEV), torch.as_tensor(ins).to(DEV), origin, voxel_size,
                              torch.as_tensor(verts).to(DEV), **kw)
    return {k: out[k].cpu().numpy() for k in KEYS}


def assert_matches(out, bf):
    """index and labels exactly; dist within 1 ulp of fp32 of the brute-force root"""
    assert (out["index"] == bf["index"]).all()
    assert (out["semantic"] == bf["semantic"]).all() and (out["instance"] == bf["instance"]).all()
    finite = np.isfinite(bf["dist"])
    assert (np.isinf(out["dist"]) == ~finite).all() and (out["dist"][~finite] > 0).all()
    assert (np.abs(out["dist"][finite].astype(np.float64) - bf["dist"][finite]) <= np.spacing(bf["dist"][finite])).all()


def bits(out):
    return {k: out[k].view(np.int32).tolist() for k in KEYS}


def test_golden_every_vertex(GSI, golden, brute):
    g = golden
    out = transfer(GSI, g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"])
    assert out["index"].dtype == np.int32 and out["dist"].dtype == np.float32
    assert_matches(out, brute)
    assert (out["semantic"] == g["ref_semantic"]).all()                      # the reference's own run, every vertex
    for row, k in zip(g["ref_masks"], np.unique(out["instance"])):
        assert (row == (out["instance"] == k)).all()


@pytest.mark.parametrize("near_shells", [2, 0])
def test_paths_are_bit_identical(GSI, golden, monkeypatch, near_shells):
    g = golden
    runs = []
    for path in ("0", "1", "2", "0"):             # ... and the default path twice: run to run
        monkeypatch.setenv("EPRECON_LT_PATH", path)
        runs.append(bits(transfer(GSI, g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"],
                                  near_shells=near_shells)))
    assert runs[0] == runs[1] == runs[2] == runs[3]


def test_bad_path_switch(GSI, golden, monkeypatch):
    monkeypatch.setenv("EPRECON_LT_PATH", "3")
    with pytest.raises(ValueError):
        transfer(GSI, golden["semantic"], golden["instance"], golden["origin"], golden["voxel_size"], golden["vertices"][:4])


def test_volume_dtypes_and_origin_tensor(GSI, golden, brute):
    """float volumes truncate like the reference's .astype(int); origin may be a tensor"""
    g = golden
    out = transfer(GSI, g["semantic"].astype(np.float32) + 0.75, g["instance"].astype(np.int64), torch.tensor(g["origin"]),
                   float(g["voxel_size"]), g["vertices"][:200])
    assert (out["index"] == brute["index"][:200]).all() and (out["semantic"] == brute["semantic"][:200]).all()


# ---------------------------------------------------------------------------------------------------------------- exact ties

TIE_DIMS, TIE_ORIGIN, TIE_VS = (9, 6, 5), np.array([-1.25, 0.5, 2.0], np.float32), 0.0625


def tie_scene(density=1.0):
    """density 1: 2-, 4- and 8-way ties around the vertex's own cell; sparse: equally near sites in DIFFERENT bricks, where the one
    of the smaller index may be met later (a brick whose box bound equals the best distance must still be opened)"""
    sem = (np.random.default_rng(5).random(TIE_DIMS) < density).astype(np.int32)
    ins = np.arange(np.prod(TIE_DIMS), dtype=np.int32).reshape(TIE_DIMS) % 97
    half = [np.arange(-1, 2 * d + 1) * 0.03125 for d in TIE_DIMS]          # half steps: sites, face / edge midpoints, corners
    verts = np.stack(np.meshgrid(*half, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) + TIE_ORIGIN
    return sem, ins, verts


@pytest.mark.parametrize("density,ties", [(1.0, 1000), (0.12, 100)])
@pytest.mark.parametrize("path", ["0", "1", "2"])
def test_exact_ties_on_a_dyadic_lattice(GSI, monkeypatch, path, density, ties):
    monkeypatch.setenv("EPRECON_LT_PATH", path)
    sem, ins, verts = tie_scene(density)
    bf = R.brute_force(sem, ins, TIE_ORIGIN, TIE_VS, verts)
    assert (bf["second"] == bf["d2"]).sum() > ties                           # the lattice really ties
    assert_matches(transfer(GSI, sem, ins, TIE_ORIGIN, TIE_VS, verts), bf)


def test_tie_winner_is_the_smallest_linear_index(GSI):
    sem, ins, _ = tie_scene()
    h = 0.0625
    cases = [((1.5, 2, 1), 2), ((1.5, 2.5, 1), 4), ((1.5, 2.5, 1.5), 8),     # face midpoint, edge midpoint, cell corner
             ((3.5, 2, 1), 2), ((3.5, 3.5, 3.5), 8),                          # on a brick boundary (cells 3 | 4)
             ((0, 3.5, 0), 2), ((8, 4.5, 3.5), 4), ((7.5, 5, 4), 2)]          # on the volume's boundary
    verts = np.array([np.array(c) * h for c, _ in cases], np.float32) + TIE_ORIGIN
    out = transfer(GSI, sem, ins, TIE_ORIGIN, TIE_VS, verts)
    for k, (_, ways) in enumerate(cases):
        m = R.minima(sem, TIE_ORIGIN, TIE_VS, verts[k])
        assert len(m) == ways and out["index"][k] == m.min(), (cases[k], m, out["index"][k])


def test_tie_across_bricks_goes_to_the_brick_met_later(GSI):
    """two sites only, cells (3, 2, 1) and (6, 2, 1); the vertex at x = 4.5 cells lives in the second one's brick, whose site is
    found first, and the first brick's box bound EQUALS that distance: the smaller index, in the brick met later, must win"""
    sem = np.zeros(TIE_DIMS, np.int32)
    sem[3, 2, 1] = sem[6, 2, 1] = 1
    vert = (np.array([[4.5, 2, 1]]) * 0.0625).astype(np.float32) + TIE_ORIGIN
    m = R.minima(sem, TIE_ORIGIN, TIE_VS, vert[0])
    assert m.tolist() == [np.ravel_multi_index((3, 2, 1), TIE_DIMS), np.ravel_multi_index((6, 2, 1), TIE_DIMS)]
    for near_shells in (2, 0):
        out = transfer(GSI, sem, sem * 7, TIE_ORIGIN, TIE_VS, vert, near_shells=near_shells)
        assert out["index"].tolist() == [m.min()] and out["instance"].tolist() == [7]


# -------------------------------------------------------------------------------------------------------------- small shapes

@pytest.mark.parametrize("dims,site", [((1, 1, 1), (0, 0, 0)), ((3, 2, 1), (2, 1, 0)), ((4, 4, 4), (3, 3, 3)),
                                       ((5, 4, 4), (4, 2, 1))])          # the last: the site in the partial brick
@pytest.mark.parametrize("n", [0, 1, 65])
def test_small_shapes_one_site(GSI, golden, dims, site, n):
    sem, ins = np.zeros(dims, np.int32), np.zeros(dims, np.int32)
    sem[site], ins[site] = 20, 28
    rng = np.random.default_rng(n)
    verts = (golden["origin"] + rng.uniform(-0.5, 0.5, (n, 3))).astype(np.float32)
    if n:
        verts[-1] = (100.0, -3.0, 7.0)                                     # a vertex 100 m away
    out = transfer(GSI, sem, ins, golden["origin"], golden["voxel_size"], verts)
    assert all(out[k].shape == (n,) for k in KEYS)
    assert_matches(out, R.brute_force(sem, ins, golden["origin"], golden["voxel_size"], verts))
    assert (out["index"] == np.ravel_multi_index(site, dims)).all() and (out["semantic"] == 39).all()


# ------------------------------------------------------------------------------------------------- no site, class out of range

def write_scene(tmp_path, sem, ins, origin, voxel_size, verts, sparse=False, scene="s0"):
    from eprecon_amd.save_scene import export_ply
    pred, ply = tmp_path / "pred", tmp_path / "ply"
    pred.mkdir(exist_ok=True), ply.mkdir(exist_ok=True)
    if sparse:
        rows = np.argwhere((sem != 0) | (ins != 0))
        at = tuple(rows.T)
        np.savez_compressed(pred / f"{scene}.npz", origin=origin, voxel_size=float(voxel_size), dims=np.array(sem.shape),
                            sparse_coords=rows.astype(np.int32), sparse_tsdf=np.zeros(len(rows), np.float32),
                            sparse_semantic=sem[at], sparse_instance=ins[at])
    else:
        np.savez_compressed(pred / f"{scene}.npz", origin=origin, voxel_size=float(voxel_size), tsdf=np.ones(sem.shape, np.float32),
                            semantic=sem, instance=ins)
    export_ply({"vertices": verts, "vertex_normals": np.zeros_like(verts), "faces": np.array([[0, 1, 2]], np.int32)},
               str(ply / f"{scene}_vh_clean_2.ply"))
    return str(pred), str(ply), tmp_path / "out"


def test_no_site(GSI, golden, tmp_path, capsys):
    g = golden
    sem = np.zeros((5, 4, 4), np.int32)
    out = transfer(GSI, sem, sem + 3, g["origin"], g["voxel_size"], g["vertices"][:65])
    assert (out["index"] == -1).all() and np.isposinf(out["dist"]).all()
    assert (out["semantic"] == 0).all() and (out["instance"] == 0).all()
    pred, ply, out_dir = write_scene(tmp_path, sem, sem + 3, g["origin"], g["voxel_size"], g["vertices"][:65])
    assert GSI.generate_semantic_instance("s0", pred, ply, str(out_dir)) is None
    assert "warning" in capsys.readouterr().out and not out_dir.exists()


@pytest.mark.parametrize("bad", [21, -1])
def test_class_out_of_range(GSI, golden, tmp_path, bad):
    g = golden
    sem = g["semantic"].copy()
    sem[6, 3, 3] = bad
    with pytest.raises(ValueError):
        transfer(GSI, sem, g["instance"], g["origin"], g["voxel_size"], g["vertices"][:65])
    pred, ply, out_dir = write_scene(tmp_path, sem, g["instance"], g["origin"], g["voxel_size"], g["vertices"][:65])
    with pytest.raises(ValueError):
        GSI.generate_semantic_instance("s0", pred, ply, str(out_dir))
    assert not out_dir.exists()


# ------------------------------------------------------------------------------------------------------------------ the vote

def test_vote_equals_counter(GSI, golden, brute):
    for sem, ins in ((brute["semantic"], brute["instance"]), (R.TIE_SEM, R.TIE_INS)):
        want = R.vote(sem, ins)
        runs = [GSI.instance_table(torch.as_tensor(sem).to(DEV), torch.as_tensor(ins).to(DEV)) for _ in range(2)]
        for got in runs:
            assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in got)
            assert [t.cpu().tolist() for t in got] == [w.tolist() for w in want]
    assert R.vote(R.TIE_SEM, R.TIE_INS)[1].tolist() == [4, 9]
    assert golden["ref_instance_class"].tolist() == R.vote(brute["semantic"], brute["instance"])[1].tolist()
    empty = GSI.instance_table(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert [t.numel() for t in empty] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- end to end

def assert_files_equal_golden(out_dir, g):
    assert (out_dir / "semantic" / "s0.txt").read_bytes() == g["semantic_txt"].tobytes()
    assert (out_dir / "instance" / "s0.txt").read_bytes() == g["instance_txt"].tobytes()
    names = sorted(os.listdir(out_dir / "instance" / "predicted_masks"))
    assert names == [f"s0_{i:03d}.txt" for i in range(len(g["mask_txt"]))]
    for name, row in zip(names, g["mask_txt"]):
        assert (out_dir / "instance" / "predicted_masks" / name).read_bytes() == row.tobytes()


@pytest.mark.parametrize("sparse", [False, True])
def test_end_to_end_files(GSI, golden, tmp_path, sparse):
    g = golden
    pred, ply, out_dir = write_scene(tmp_path, g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"], sparse)
    res = GSI.generate_semantic_instance("s0", pred, ply, str(out_dir))
    assert res["n_vertices"] == 3000 and res["n_instances"] == len(g["mask_txt"]) and len(res["files"]) == 2 + res["n_instances"]
    assert_files_equal_golden(out_dir, g)


def test_command_line(GSI, golden, tmp_path, capsys):
    g = golden
    pred, ply, out_dir = write_scene(tmp_path, g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"])
    (tmp_path / "scenes.txt").write_text("s0\n")
    assert GSI.main(["--pred", pred, "--ply", ply, "--scenes", str(tmp_path / "scenes.txt"), "--out", str(out_dir)]) == 0
    assert capsys.readouterr().out.split() == ["s0"]
    assert_files_equal_golden(out_dir, g)

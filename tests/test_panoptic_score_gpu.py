"""GPU: panoptic scoring (eprecon_amd/panoptic_score.py, csrc/panoptic_score.hip) against the set-and-loop restatement of
tests/panoptic_score_ref.py: the pair-count kernel at the wave and workgroup edges, the voxel kernel against an
enumeration of the lattice (shifted grids, identical grids, a shift of exactly half a cell, disjoint boxes, the surface
rule, both file forms), the vertex domain on the committed scene against the brute-force label transfer, and the command
line in both domains.  Integer tables compare exactly, figures to 1e-12 (exact rationals)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import label_transfer_ref as LT
import panoptic_score_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def PS():
    from eprecon_amd import panoptic_score
    return panoptic_score


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------------------- pair_counts

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_pair_counts_random_ranks(PS, n):
    rng = np.random.default_rng(n)
    n_pred, n_gt = 5, 3
    p, g = rng.integers(-1, n_pred, n), rng.integers(-1, n_gt + 1, n)       # -1, every segment, the void column
    if n >= 63:
        assert {-1, n_pred - 1} <= set(p.tolist()) and {-1, n_gt} <= set(g.tolist())
    want, skipped = R.table_of_ranks(p, g, n_pred, n_gt)
    got = PS.pair_counts(dev(p), dev(g), n_pred, n_gt)
    assert got.dtype == torch.int64 and got.device.type == "cuda" and tuple(got.shape) == (n_pred + 1, n_gt + 2)
    assert skipped == 0 and (got.cpu().numpy() == want).all() and int(got.sum()) == n


def test_pair_counts_a_wave_of_64_pairs_and_a_wave_of_one(PS):
    k = np.arange(64)
    for p, g in ((k % 8, k // 8), (np.full(64, 3), np.full(64, 8)), (np.full(64, -1), np.full(64, -1))):
        want, _ = R.table_of_ranks(p, g, 8, 8)
        assert (PS.pair_counts(dev(p), dev(g), 8, 8).cpu().numpy() == want).all()
    assert (R.table_of_ranks(k % 8, k // 8, 8, 8)[0][:8, :8] == 1).all()


@pytest.mark.parametrize("n_pred,n_gt", [(63, 126), (63, 127), (100, 100)])
@pytest.mark.parametrize("lds", ["1", "0"])
def test_pair_counts_around_the_lds_table_limit(PS, monkeypatch, n_pred, n_gt, lds):
    """(n_pred + 1) * (n_gt + 2) = 8,192 is the largest table summed in LDS first; 8,256 and 10,302 go straight to memory;
    EPRECON_PC_LDS=0 sends the small one there too"""
    monkeypatch.setenv("EPRECON_PC_LDS", lds)
    rng = np.random.default_rng(n_gt)
    p, g = rng.integers(-1, n_pred, 1000), rng.integers(-1, n_gt + 1, 1000)
    p[:3], g[:3] = [n_pred - 1, -1, n_pred - 1], [n_gt, -1, -1]           # the table's last row, last columns, last entry
    want, _ = R.table_of_ranks(p, g, n_pred, n_gt)
    assert (PS.pair_counts(dev(p), dev(g), n_pred, n_gt).cpu().numpy() == want).all()


def test_pair_counts_300000_sites_of_two_segments(PS):
    n = 300000
    k = np.arange(n)
    for first in (k < 123457, (k // 1000) % 2 == 0, k % 2 == 0):      # one boundary, long runs, alternating lanes
        p, g = np.where(first, 0, 1), np.where(first, 1, 0)
        got = PS.pair_counts(dev(p), dev(g), 2, 2).cpu().numpy()
        want = np.zeros((3, 4), np.int64)
        want[0, 1], want[1, 0] = int(first.sum()), int(n - first.sum())
        assert (got == want).all() and got.sum() == n


def test_pair_counts_rank_out_of_range(PS):
    rng = np.random.default_rng(7)
    n_pred, n_gt = 4, 4
    p, g = rng.integers(-1, n_pred, 500), rng.integers(-1, n_gt + 1, 500)
    p[[3, 64, 499]] = n_pred                                                # a rank EQUAL to n_pred
    g[[100]] = n_gt + 1
    p[[200]] = -2
    want, skipped = R.table_of_ranks(p, g, n_pred, n_gt)
    assert skipped == 5
    with pytest.raises(ValueError) as err:
        PS.pair_counts(dev(p), dev(g), n_pred, n_gt)
    got = err.value.counts.cpu().numpy()
    assert (got == want).all() and got.sum() == 495


def test_pair_counts_table_too_large(PS):
    from eprecon_amd import _lib
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.EpreconError):
        PS.pair_counts(z, z, 4096, 4096)
    # the C entry itself: -3 before any launch (the buffers are never touched)
    small = torch.zeros(8, dtype=torch.int64, device=DEV)
    rc = _lib.load().eprecon_pair_count_async(_lib.ptr(z), _lib.ptr(z), 8, 4096, 4096, _lib.ptr(small), _lib.ptr(z), _lib.current_stream())
    assert rc == -3
    assert int(small.sum()) == 0
    assert tuple(PS.pair_counts(z, z, 2047, 2046).shape) == (2048, 2048)     # exactly 2^22 entries is supported


def test_segment_table(PS):
    """stuff merges instances; an instance of two classes is two segments; void and absent codes"""
    sem = np.array([1, 1, 5, 5, 6, 0, 40, 2, 5], np.int64)
    ins = np.array([3, 4, 9, 9, 9, 1, 1, 7, 2], np.int64)
    rank, classes, keys = PS.segment_table(dev(sem), dev(ins))
    assert PS.key_pairs(keys).tolist() == [[1, 0], [2, 0], [5, 2], [5, 9], [6, 9]] and classes.tolist() == [1, 2, 5, 5, 6]
    assert rank.dtype == torch.int32 and rank.tolist() == [0, 0, 3, 3, 4, 5, 5, 1, 2]           # 5 = void (class 0 and class 40)
    rank, classes, keys = PS.segment_table(dev(sem.clip(0, 20)), dev(ins), mapping=R.MAPPING)
    assert rank.tolist() == [0, 0, 3, 3, 4, -1, 5, 1, 2] and classes.tolist() == [1, 2, 5, 5, 6, 39]
    with pytest.raises(ValueError):
        PS.segment_table(dev([1, 21]), dev([0, 0]), mapping=R.MAPPING)


# ------------------------------------------------------------------------------------------------------------ voxel domain

VS = 0.04


def volumes(seed, dims_p, dims_g, distinct=False):
    """-> prediction (class indices, mostly 0; instances), ground truth (tsdf with |values| on both sides of 1 and exactly
    1, ids with 0 and the void id 40, instances), labels in runs along z like surfaces; distinct: an instance id per cell
    (hundreds of segments on both sides: a table too large for the LDS path)"""
    rng = np.random.default_rng(seed)
    blocks = lambda dims, values: np.repeat(rng.choice(values, (dims[0], dims[1], (dims[2] + 2) // 3)), 3, axis=2)[:, :, :dims[2]]
    p_sem = blocks(dims_p, [0, 0, 1, 2, 5, 5, 7]).astype(np.int32)
    p_ins = blocks(dims_p, [1, 2]).astype(np.int32)
    g_sem = blocks(dims_g, [0, 1, 2, 5, 5, 7, 40]).astype(np.int64)
    g_ins = blocks(dims_g, [1, 2, 3]).astype(np.int64)
    if distinct:
        p_ins, g_ins = np.arange(p_ins.size, dtype=np.int32).reshape(dims_p), np.arange(g_ins.size, dtype=np.int64).reshape(dims_g)
    tsdf = rng.uniform(-1.2, 1.2, dims_g).astype(np.float32)
    tsdf.reshape(-1)[::7] = 1.0
    tsdf.reshape(-1)[3::11] = -1.0
    return p_sem, p_ins, tsdf, g_sem, g_ins


def write_pred(root, scene, sem, ins, origin, voxel_size, sparse=False):
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, scene + ".npz")
    if sparse:
        rows = np.argwhere((sem != 0) | (ins != 0))
        at = tuple(rows.T)
        np.savez_compressed(path, origin=np.asarray(origin, np.float32), voxel_size=float(voxel_size), dims=np.array(sem.shape),
                            sparse_coords=rows.astype(np.int32), sparse_tsdf=np.zeros(len(rows), np.float32),
                            sparse_semantic=sem[at], sparse_instance=ins[at])
    else:
        np.savez_compressed(path, origin=np.asarray(origin, np.float32), voxel_size=float(voxel_size),
                            tsdf=np.ones(sem.shape, np.float32), semantic=sem, instance=ins)
    return path


def write_gt(root, scene, tsdf, sem, ins, origin, voxel_size):
    d = os.path.join(root, scene)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "tsdf_info.pkl"), "wb") as fh:
        pickle.dump({"vol_origin": np.asarray(origin, np.float32), "voxel_size": float(voxel_size)}, fh)
    np.savez_compressed(os.path.join(d, "full_tsdf_layer0"), tsdf)
    np.savez_compressed(os.path.join(d, "full_semantic_layer_interpolate0"), sem)
    np.savez_compressed(os.path.join(d, "full_instance_layer_interpolate0"), ins)
    return d


# name: prediction dims and origin, ground-truth dims and origin, voxel size, guard of the reference
GRIDS = {
    # fractional shifts 0.325, 0.475, 0.825 of a cell: far from a rounding decision (the reference asserts 1e-6)
    "shifted": ((9, 7, 5), (0.08, -0.04, 0.0), (8, 8, 6), (-0.013, 0.021, 0.007), VS, 1e-6),
    "identical": ((8, 8, 6), (-0.013, 0.021, 0.007), (8, 8, 6), (-0.013, 0.021, 0.007), VS, 1e-6),
    # exactly half a cell on every axis (dyadic numbers: every operation is exact): floor(x + 0.5) keeps the bijection
    "half": ((9, 7, 5), (0.25, -0.5, 1.0), (8, 8, 6), (0.25 + 0.015625, -0.5 - 3 * 0.015625, 1.0 + 5 * 0.015625), 0.03125, None),
    # the prediction's box two metres off: no site has both
    "outside": ((5, 4, 3), (2.0, 0.0, 0.0), (4, 5, 6), (-0.013, 0.021, 0.007), VS, 1e-6),
    # the shifted grids with an instance per cell: more than 8,192 table entries, the kernel's straight-to-memory path
    "many": ((9, 7, 5), (0.08, -0.04, 0.0), (8, 8, 6), (-0.013, 0.021, 0.007), VS, 1e-6),
}


@pytest.fixture(scope="module")
def voxel_cases():
    out = {}
    for seed, (name, (dims_p, o_p, dims_g, o_g, vs, guard)) in enumerate(GRIDS.items()):
        vols = volumes(seed, dims_p, dims_g, distinct=name == "many")
        pred, gt = R.voxel_labels(vols[0], vols[1], o_p, vs, vols[2], vols[3], vols[4], o_g, vs, guard=guard)
        out[name] = (vols, R.score(pred, gt), pred, gt)
    return out


@pytest.mark.parametrize("name", list(GRIDS))
def test_score_voxels_against_lattice_enumeration(PS, voxel_cases, tmp_path, name):
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS[name]
    (p_sem, p_ins, tsdf, g_sem, g_ins), want, pred, gt = voxel_cases[name]
    npz = write_pred(str(tmp_path / "pred"), "s0", p_sem, p_ins, o_p, vs)
    gt_dir = write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs)
    tables = PS.score_voxels(npz, gt_dir)
    R.assert_tables_equal(tables, want)
    G = len(want["gt_keys"])
    # ground-truth cells with |tsdf| >= 1 are absent; every present cell is the cell of exactly one site
    assert int(tables.counts[:, :G + 1].sum()) == int((np.abs(tsdf) < 1).sum()) < tsdf.size
    assert int(tables.counts[:-1].sum()) == int((np.asarray(R.MAPPING)[p_sem] != 0).sum())
    if name == "outside":
        assert int(tables.counts[:-1, :G + 1].sum()) == 0 and tables.tp.sum() == 0
    else:
        assert int(tables.counts[:-1, :G].sum()) > 0
    if name == "identical":
        assert tables.counts.sum() == np.prod(dims_p)
    if name == "many":
        assert tables.counts.size > 8192
    R.assert_summaries_equal(PS.PanopticScore().add(tables).summary(), R.summary([want]))


def test_score_voxels_sparse_and_dense_forms_agree(PS, voxel_cases, tmp_path):
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS["shifted"]
    (p_sem, p_ins, tsdf, g_sem, g_ins), want, _, _ = voxel_cases["shifted"]
    p_ins = np.where(p_sem != 0, p_ins, 0)           # (the sparse form stores the rows with a label)
    gt_dir = write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs)
    dense = PS.score_voxels(write_pred(str(tmp_path / "dense"), "s0", p_sem, p_ins, o_p, vs), gt_dir)
    sparse = PS.score_voxels(write_pred(str(tmp_path / "sparse"), "s0", p_sem, p_ins, o_p, vs, sparse=True), gt_dir)
    assert (dense.counts == sparse.counts).all() and (dense.pred_keys == sparse.pred_keys).all()
    R.assert_tables_equal(sparse, want)


def test_score_voxels_paths_agree(PS, voxel_cases, tmp_path, monkeypatch):
    """the small table summed in LDS first and sent straight to memory: the same integers"""
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS["shifted"]
    (p_sem, p_ins, tsdf, g_sem, g_ins), want, _, _ = voxel_cases["shifted"]
    npz = write_pred(str(tmp_path / "pred"), "s0", p_sem, p_ins, o_p, vs)
    gt_dir = write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs)
    monkeypatch.setenv("EPRECON_PC_LDS", "0")
    from eprecon_amd import _lib
    reads = _lib.HOST_READS
    R.assert_tables_equal(PS.score_voxels(npz, gt_dir), want)
    assert _lib.HOST_READS - reads == 1


def test_score_voxels_surface_threshold(PS, voxel_cases, tmp_path):
    """a smaller gt_surface leaves fewer ground-truth cells present, exactly those of the reference"""
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS["shifted"]
    p_sem, p_ins, tsdf, g_sem, g_ins = voxel_cases["shifted"][0]
    pred, gt = R.voxel_labels(p_sem, p_ins, o_p, vs, tsdf, g_sem, g_ins, o_g, vs, gt_surface=0.5)
    npz = write_pred(str(tmp_path / "pred"), "s0", p_sem, p_ins, o_p, vs)
    tables = PS.score_voxels(npz, write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs), gt_surface=0.5)
    R.assert_tables_equal(tables, R.score(pred, gt))
    assert int(tables.counts[:, :-1].sum()) == int((np.abs(tsdf) < 0.5).sum())


def test_score_voxels_unequal_voxel_sizes(PS, voxel_cases, tmp_path):
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS["shifted"]
    p_sem, p_ins, tsdf, g_sem, g_ins = voxel_cases["shifted"][0]
    npz = write_pred(str(tmp_path / "pred"), "s0", p_sem, p_ins, o_p, vs)
    with pytest.raises(ValueError):
        PS.score_voxels(npz, write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs * (1 + 1e-6)))


def test_no_labelled_voxel_scores_all_fn(PS, voxel_cases, tmp_path, capsys):
    dims_p, o_p, dims_g, o_g, vs, _ = GRIDS["shifted"]
    p_sem, p_ins, tsdf, g_sem, g_ins = voxel_cases["shifted"][0]
    npz = write_pred(str(tmp_path / "pred"), "s0", np.zeros_like(p_sem), p_ins, o_p, vs)
    tables = PS.score_voxels(npz, write_gt(str(tmp_path / "gt"), "s0", tsdf, g_sem, g_ins, o_g, vs))
    assert "warning: No labelled voxel" in capsys.readouterr().out
    pred, gt = R.voxel_labels(np.zeros_like(p_sem), p_ins, o_p, vs, tsdf, g_sem, g_ins, o_g, vs)
    want = R.score(pred, gt)
    R.assert_tables_equal(tables, want)
    assert tables.tp.sum() == 0 and tables.fp.sum() == 0 and tables.fn.sum() == len(want["gt_keys"]) > 0


# ----------------------------------------------------------------------------------------------------------- vertex domain

@pytest.fixture(scope="module")
def vertex_case(golden_dir):
    """the committed scene, its brute-force label transfer, and seeded ground-truth vertex labels: the transferred labels with
    other instance ids, a fifth of the vertices relabelled (the unlabelled id 0 and the void id 40 among them)"""
    g = dict(np.load(os.path.join(golden_dir, "semantic_instance.npz")))
    bf = LT.brute_force(g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"])
    rng = np.random.default_rng(11)
    n = len(g["vertices"])
    noise = rng.random(n) < 0.2
    gt_sem = np.where(noise, rng.choice([0, 1, 3, 5, 40], n), bf["semantic"]).astype(np.int64)
    gt_ins = np.where(noise, rng.choice([50, 51], n), bf["instance"] + 100).astype(np.int64)
    want = R.score(R.pred_labels(bf["semantic"], bf["instance"], mapping=None), R.gt_labels(gt_sem, gt_ins))
    return g, gt_sem, gt_ins, want


def write_info(root, scene, verts, sem, ins):
    os.makedirs(root, exist_ok=True)
    for name, a in (("vert", verts), ("sem_label", sem), ("ins_label", ins)):
        np.save(os.path.join(root, f"{scene}_{name}.npy"), a)
    return root


def test_score_vertices_on_the_committed_scene(PS, vertex_case, tmp_path):
    g, gt_sem, gt_ins, want = vertex_case
    npz = write_pred(str(tmp_path / "pred"), "s0", g["semantic"], g["instance"], g["origin"], g["voxel_size"])
    info = write_info(str(tmp_path / "info"), "s0", g["vertices"], gt_sem, gt_ins)
    tables = PS.score_vertices(npz, info, "s0")
    R.assert_tables_equal(tables, want)
    assert tables.counts.sum() == 3000 and tables.counts[:, -1].sum() == 0          # no vertex is "absent"
    assert tables.tp.sum() >= 3 and tables.counts[:, -2].sum() > 0                    # it scores, and some ground truth is void
    R.assert_summaries_equal(PS.PanopticScore().add(tables).summary(), R.summary([want]))


def test_score_sites_equals_score_vertices_labels(PS, vertex_case):
    """score_sites on class indices (through the mapping) and on ids (mapping=None) agree with the reference"""
    g, gt_sem, gt_ins, want = vertex_case
    bf = LT.brute_force(g["semantic"], g["instance"], g["origin"], g["voxel_size"], g["vertices"][:500])
    index = {v: k for k, v in enumerate(R.MAPPING)}
    cls = np.array([index[int(s)] for s in bf["semantic"]])
    want = R.score(R.pred_labels(cls, bf["instance"]), R.gt_labels(gt_sem[:500], gt_ins[:500]))
    from eprecon_amd import _lib
    reads = _lib.HOST_READS
    a = PS.score_sites(dev(cls), dev(bf["instance"]), dev(gt_sem[:500], torch.int64), dev(gt_ins[:500], torch.int64))
    assert _lib.HOST_READS - reads == 1                                      # flags, keys and table in one transfer
    b = PS.score_sites(dev(bf["semantic"]), dev(bf["instance"]), dev(gt_sem[:500]), dev(gt_ins[:500]), mapping=None)
    R.assert_tables_equal(a, want)
    R.assert_tables_equal(b, want)
    with pytest.raises(ValueError):
        PS.score_sites(dev(cls + 21), dev(bf["instance"]), dev(gt_sem[:500]), dev(gt_ins[:500]))


def test_score_vertices_no_labelled_voxel(PS, vertex_case, tmp_path, capsys):
    g, gt_sem, gt_ins, _ = vertex_case
    npz = write_pred(str(tmp_path / "pred"), "s0", np.zeros_like(g["semantic"]), g["instance"], g["origin"], g["voxel_size"])
    tables = PS.score_vertices(npz, write_info(str(tmp_path / "info"), "s0", g["vertices"], gt_sem, gt_ins), "s0")
    assert "warning: No labelled voxel" in capsys.readouterr().out
    want = R.score([None] * 3000, R.gt_labels(gt_sem, gt_ins))
    R.assert_tables_equal(tables, want)
    assert tables.tp.sum() == 0 and tables.fp.sum() == 0 and tables.fn.sum() == len(want["gt_keys"])


# ------------------------------------------------------------------------------------------------------------ command line

@pytest.mark.parametrize("threshold", [0.5, 0.25])
def test_command_line_both_domains(PS, voxel_cases, vertex_case, tmp_path, capsys, threshold):
    pred_dir, gt_root, info = str(tmp_path / "pred"), str(tmp_path / "gt"), str(tmp_path / "info")
    g, gt_sem, gt_ins, _ = vertex_case
    wants_voxel, wants_vertex = [], []
    for scene, name in (("scene_a", "shifted"), ("scene_b", "half")):
        dims_p, o_p, dims_g, o_g, vs, _ = GRIDS[name]
        (p_sem, p_ins, tsdf, g_sem, g_ins), _, pred, gt = voxel_cases[name]
        write_pred(pred_dir, scene, p_sem, p_ins, o_p, vs)
        write_gt(gt_root, scene, tsdf, g_sem, g_ins, o_g, vs)
        wants_voxel.append(R.score(pred, gt, threshold))
        # the vertex domain of the same two predictions: 200 of the committed scene's vertices moved onto the volume
        verts = (np.asarray(o_p, np.float32) + (g["vertices"][:200] - g["origin"])).astype(np.float32)
        write_info(info, scene, verts, gt_sem[:200], gt_ins[:200])
        bf = LT.brute_force(p_sem, p_ins, np.asarray(o_p, np.float32), vs, verts)
        wants_vertex.append(R.score(R.pred_labels(bf["semantic"], bf["instance"], mapping=None), R.gt_labels(gt_sem[:200], gt_ins[:200]),
                                    threshold))
    (tmp_path / "scenes.txt").write_text("scene_a\nscene_b\n")
    common = ["--pred", pred_dir, "--scenes", str(tmp_path / "scenes.txt"), "--threshold", str(threshold)]
    for extra, wants, out in ((["--gt", gt_root], wants_voxel, "voxel.json"), (["--info", info], wants_vertex, "vertex.json")):
        assert PS.main(common + extra + ["--out", str(tmp_path / out)]) == 0
        text = capsys.readouterr().out
        assert text.splitlines()[0].split()[:4] == ["class", "PQ", "SQ", "RQ"] and "mIoU" in text
        with open(tmp_path / out) as fh:
            got = json.load(fh)
        assert got["scenes"] == 2
        R.assert_summaries_equal(got, R.summary(wants, threshold))

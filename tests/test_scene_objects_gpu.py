"""GPU: the object inventory (eprecon_amd/scene_objects.py, csrc/segment_stats.hip) against the host restatement of
tests/scene_objects_ref.py.  Every statistic of the kernels is an integer sum, an integer min / max or a min / max of doubles,
and `finish` and the restatement apply the same stated arithmetic, so every comparison is exact:
np.array_equal on the int64 table, equality of the bits on the extents, == on the records.

Seeded cases: M coordinates in the 12^3 box [-6, 6)^3, duplicates allowed, in the order they were drawn; ranks drawn from
{-1, 0 .. n-1, n}, so that both silent skips occur; a direction per segment from a seeded angle, the first two (1, 0) and
(0, 1) exactly."""
import functools
import json
import math
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scene_objects_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)
TOP = 2 ** 19 - 2
VS = 0.04
ORIGIN = (-1.5, 0.25, 0.125)


@pytest.fixture(scope="module")
def SO():
    from eprecon_amd import scene_objects
    return scene_objects


@pytest.fixture(scope="module")
def L():
    from eprecon_amd import _lib
    return int(_lib.load().eprecon_segment_stats_lds_segments())


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.array(a)).to(dtype).to(DEV)      # (a copy: the cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def seeded_dirs(rng, n):
    angle = rng.uniform(-np.pi, np.pi, n)
    dirs = np.stack([np.cos(angle), np.sin(angle)], 1).reshape(n, 2)
    dirs[:2] = [[1.0, 0.0], [0.0, 1.0]][:min(n, 2)]
    return dirs


@functools.lru_cache(maxsize=None)
def seeded_case(m, n):
    """-> (coords int64[m,3], rank int64[m], dirs f64[n,2], the restatement's table int64[n,16] and extents f64[n,4])"""
    rng = np.random.default_rng(1000 * n + m)
    coords = rng.integers(-6, 6, (m, 3))
    rank = rng.integers(-1, n + 1, m)
    rank[:1] = n - 1                       # the table's last row
    if m >= 3:
        rank[1:3] = [-1, n]                # both silent skips
    dirs = seeded_dirs(rng, n)
    table, status = R.moments(coords, rank, n)
    ext, status_e = R.extents(coords, rank, n, dirs)
    assert status == 0 and status_e == 0
    for a in (coords, rank, dirs, ext):
        a.setflags(write=False)
    return coords, rank, dirs, R.table_array(table), ext


def run_moments(SO, coords, rank, n):
    table = SO.segment_moments(dev(np.asarray(coords).reshape(-1, 3)), dev(rank), n)
    assert table.dtype == torch.int64 and table.device.type == "cuda" and tuple(table.shape) == (n, 16)
    return table.cpu().numpy()


def run_extents(SO, coords, rank, n, dirs):
    ext = SO.segment_extents(dev(np.asarray(coords).reshape(-1, 3)), dev(rank), n, dev(np.asarray(dirs).reshape(-1, 2), torch.float64))
    assert ext.dtype == torch.float64 and ext.device.type == "cuda" and tuple(ext.shape) == (n, 4)
    return ext.cpu().numpy()


def check_case(SO, m, n):
    coords, rank, dirs, table, ext = seeded_case(m, n)
    got_t, got_e = run_moments(SO, coords, rank, n), run_extents(SO, coords, rank, n, dirs)
    assert np.array_equal(got_t, table)
    assert np.array_equal(bits(got_e), bits(ext))
    return got_t, got_e


# -------------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("m", SIZES)
def test_row_counts(SO, m):
    """wave, workgroup and grid-stride edges"""
    check_case(SO, m, 5)


@pytest.mark.parametrize("which", ["1", "2", "L-1", "L", "L+1"])
def test_segment_counts_around_the_lds_limit(SO, L, monkeypatch, which):
    """up to L segments the table is combined in LDS first, above it and with EPRECON_SS_LDS=0 every update goes to memory:
    the same tables either way"""
    n = {"1": 1, "2": 2, "L-1": L - 1, "L": L, "L+1": L + 1}[which]
    monkeypatch.setenv("EPRECON_SS_LDS", "1")
    lds = check_case(SO, 1023, n)
    monkeypatch.setenv("EPRECON_SS_LDS", "0")
    mem = check_case(SO, 1023, n)
    assert np.array_equal(lds[0], mem[0]) and np.array_equal(bits(lds[1]), bits(mem[1]))


@pytest.mark.parametrize("lds", ["1", "0"])
def test_every_row_its_own_segment(SO, monkeypatch, lds):
    monkeypatch.setenv("EPRECON_SS_LDS", lds)
    rng = np.random.default_rng(7)
    m = 1025
    coords, rank, dirs = rng.integers(-6, 6, (m, 3)), rng.permutation(m), seeded_dirs(rng, m)
    table = run_moments(SO, coords, rank, m)
    assert np.array_equal(table, R.table_array(R.moments(coords, rank, m)[0]))
    assert (table[:, 0] == 1).all() and np.array_equal(table[rank, 10:13], coords) and np.array_equal(table[rank, 13:16], coords)
    ext = run_extents(SO, coords, rank, m, dirs)
    assert np.array_equal(bits(ext), bits(R.extents(coords, rank, m, dirs)[0]))
    assert np.array_equal(bits(ext[:, 0]), bits(ext[:, 1])) and np.array_equal(bits(ext[:, 2]), bits(ext[:, 3]))


@pytest.mark.parametrize("lds", ["1", "0"])
def test_all_rows_in_one_segment(SO, monkeypatch, lds):
    """the contended case: 1,025 rows update one table row"""
    monkeypatch.setenv("EPRECON_SS_LDS", lds)
    rng = np.random.default_rng(8)
    m = 1025
    coords, rank, dirs = rng.integers(-6, 6, (m, 3)), np.zeros(m, np.int64), np.array([[0.6, 0.8]])
    table = run_moments(SO, coords, rank, 1)
    assert np.array_equal(table, R.table_array(R.moments(coords, rank, 1)[0])) and table[0, 0] == m
    assert np.array_equal(bits(run_extents(SO, coords, rank, 1, dirs)), bits(R.extents(coords, rank, 1, dirs)[0]))


# --------------------------------------------------------------------------------------------------------------- limits

def corner_rows():
    """the eight sign patterns of +-(2^19 - 2) on the three axes, and rows with one axis at the limit"""
    rows = [[sx * TOP, sy * TOP, sz * TOP] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    rows += [[TOP, 0, -3], [0, -TOP, 5], [7, 1, TOP], [-TOP, TOP, 0]]
    return np.array(rows, np.int64)


@pytest.mark.parametrize("lds", ["1", "0"])
def test_coordinates_at_the_limit(SO, monkeypatch, lds):
    """sign handling of min / max and of the squares at +-(2^19 - 2)"""
    monkeypatch.setenv("EPRECON_SS_LDS", lds)
    coords = corner_rows()
    rank = np.arange(len(coords)) % 2
    dirs = np.array([[np.cos(0.3), np.sin(0.3)], [0.0, 1.0]])
    table = run_moments(SO, coords, rank, 2)
    assert np.array_equal(table, R.table_array(R.moments(coords, rank, 2)[0]))
    assert table[:, 4].max() >= 4 * TOP * TOP and table[:, 5].min() < 0
    assert np.array_equal(bits(run_extents(SO, coords, rank, 2, dirs)), bits(R.extents(coords, rank, 2, dirs)[0]))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_a_coordinate_beyond_the_limit(SO, axis, sign):
    """2^19 - 1 on one axis of one row: ValueError, status bit 2, and the table of the other rows as the kernel left it"""
    coords = corner_rows()
    coords[5, axis] = sign * (TOP + 1)
    rank = np.arange(len(coords)) % 2
    want, status = R.moments(coords, rank, 2)
    assert status == 2
    with pytest.raises(ValueError, match="coordinate") as e:
        SO.segment_moments(dev(coords), dev(rank), 2)
    assert e.value.status == 2 and np.array_equal(e.value.table.cpu().numpy(), R.table_array(want))
    dirs = np.array([[0.8, -0.6], [1.0, 0.0]])
    with pytest.raises(ValueError, match="coordinate") as e:
        SO.segment_extents(dev(coords), dev(rank), 2, dev(dirs, torch.float64))
    assert e.value.status == 2 and np.array_equal(bits(e.value.table.cpu().numpy()), bits(R.extents(coords, rank, 2, dirs)[0]))


@pytest.mark.parametrize("bad,word", [((4,), 1), ((-2,), 1), ((4, -2), 1)])
def test_a_rank_out_of_range(SO, bad, word):
    """n + 1 and -2 set status bit 1; -1 and n beside them are skipped silently"""
    coords, rank, dirs, _, _ = seeded_case(257, 3)
    rank = rank.copy()
    rank[10:10 + len(bad)] = bad
    want, status = R.moments(coords, rank, 3)
    assert status == word
    with pytest.raises(ValueError, match="rank") as e:
        SO.segment_moments(dev(coords), dev(rank), 3)
    assert e.value.status == word and np.array_equal(e.value.table.cpu().numpy(), R.table_array(want))
    with pytest.raises(ValueError, match="rank") as e:
        SO.segment_extents(dev(coords), dev(rank), 3, dev(dirs, torch.float64))
    assert e.value.status == word and np.array_equal(bits(e.value.table.cpu().numpy()), bits(R.extents(coords, rank, 3, dirs)[0]))


def test_both_status_bits(SO):
    coords, rank, _, _, _ = seeded_case(65, 3)
    coords, rank = coords.copy(), rank.copy()
    rank[:4] = [0, 1, 7, 2]
    coords[1, 2] = -(TOP + 1)
    coords[2, 0] = TOP + 1                  # (behind a rank out of range: the rank is looked at first)
    want, status = R.moments(coords, rank, 3)
    assert status == 3
    with pytest.raises(ValueError) as e:
        SO.segment_moments(dev(coords), dev(rank), 3)
    assert e.value.status == 3 and np.array_equal(e.value.table.cpu().numpy(), R.table_array(want))


def test_no_rows_and_no_segments(SO):
    identity = R.table_array([R.identity_row()] * 3)
    inf = np.tile([np.inf, -np.inf, np.inf, -np.inf], (3, 1))
    none = np.zeros((0, 3), np.int64)
    assert np.array_equal(run_moments(SO, none, np.zeros(0, np.int64), 3), identity)
    assert np.array_equal(bits(run_extents(SO, none, np.zeros(0, np.int64), 3, np.ones((3, 2)))), bits(inf))
    coords, rank, _, _, _ = seeded_case(65, 3)
    assert run_moments(SO, coords, np.zeros(65, np.int64), 0).shape == (0, 16)
    assert run_extents(SO, coords, np.zeros(65, np.int64), 0, np.zeros((0, 2))).shape == (0, 4)
    assert run_moments(SO, none, np.zeros(0, np.int64), 0).shape == (0, 16)


@pytest.mark.parametrize("lds", ["1", "0"])
def test_an_empty_segment_keeps_the_initial_values(SO, monkeypatch, lds):
    monkeypatch.setenv("EPRECON_SS_LDS", lds)
    coords, rank, dirs, _, _ = seeded_case(255, 5)
    rank = np.where(rank == 2, -1, rank)
    table, ext = run_moments(SO, coords, rank, 5), run_extents(SO, coords, rank, 5, dirs)
    assert table[2].tolist() == R.identity_row() and table[2, 10] == 2 ** 31 - 1 and table[2, 13] == -2 ** 31
    assert np.array_equal(bits(ext[2]), bits([np.inf, -np.inf, np.inf, -np.inf]))
    assert np.array_equal(table, R.table_array(R.moments(coords, rank, 5)[0]))
    assert np.array_equal(bits(ext), bits(R.extents(coords, rank, 5, dirs)[0]))


def test_two_segments_share_their_footprint(SO):
    """the same (x, y) in two segments with different directions: the extents differ, the moments do not"""
    coords, _, _, _, _ = seeded_case(257, 1)
    both = np.concatenate([coords, coords])
    rank = np.repeat([0, 1], len(coords))
    dirs = np.array([[np.cos(0.7), np.sin(0.7)], [np.cos(-1.1), np.sin(-1.1)]])
    table, ext = run_moments(SO, both, rank, 2), run_extents(SO, both, rank, 2, dirs)
    assert np.array_equal(table[0], table[1])
    assert np.array_equal(bits(ext), bits(R.extents(both, rank, 2, dirs)[0])) and not np.array_equal(ext[0], ext[1])


def test_a_zero_extent_is_plus_zero(SO):
    """x c = -0 for x = 0 and c < 0: the stored zero is +0 whichever row came first"""
    coords = np.array([[0, 0, 1], [0, 0, 2]])
    ext = run_extents(SO, coords, [0, 0], 1, [[-1.0, -0.0]])
    assert np.array_equal(bits(ext), np.zeros((1, 4), np.int64))


def test_one_host_read(SO):
    from eprecon_amd import _lib
    coords, rank, dirs, _, _ = seeded_case(64, 5)
    c, r, d = dev(coords), dev(rank), dev(dirs, torch.float64)
    reads = _lib.HOST_READS
    SO.segment_moments(c, r, 5)
    SO.segment_extents(c, r, 5, d)
    assert _lib.HOST_READS == reads + 2


# ----------------------------------------------------------------------------------------------------------------- rule

def run_scene(SO, coords, tsdf, sem, ins, origin=ORIGIN, vs=VS, **rule):
    return SO.scene_objects(dev(np.asarray(coords).reshape(-1, 3)), dev(tsdf, torch.float32), dev(sem, torch.int64),
                            dev(ins, torch.int64), np.float32(origin), vs, **rule)


def hand_scene():
    """a stuff class split across two instance ids (one object), an instance carrying two classes (two objects), a void
    class (none), and rows at tsdf = +-1 (left out)"""
    rows = []      # (cell, tsdf, class index, instance)
    rows += [((x, 0, 0), 0.1, 2, 4) for x in range(6)] + [((x, 1, 0), -0.2, 2, 9) for x in range(6)]       # floor, ids 4 and 9
    rows += [((k, k + 3, 2), 0.0, 5, 7) for k in range(5)] + [((k, k + 3, 3), 0.5, 6, 7) for k in range(4)]   # instance 7, classes 5 and 6
    rows += [((9, 9, z), 0.3, 0, 2) for z in range(3)]                                                      # class 0: nothing here
    rows += [((1, 7, 1), 1.0, 5, 7), ((2, 7, 1), -1.0, 5, 7), ((3, 7, 1), 0.999, 8, 1)]                     # tsdf +-1 left out
    rows += [((-4, -2, z), -0.5, 20, 3) for z in range(2)]                                                  # ScanNet id 39
    cells, tsdf, sem, ins = (np.array([r[k] for r in rows]) for k in range(4))
    order = np.random.default_rng(3).permutation(len(rows))
    return cells[order], tsdf[order].astype(np.float32), sem[order], ins[order]


@pytest.mark.parametrize("oriented", [True, False])
def test_hand_built_scene(SO, oriented):
    cells, tsdf, sem, ins = hand_scene()
    got = run_scene(SO, cells, tsdf, sem, ins, oriented=oriented)
    assert got == R.scene(cells, tsdf, sem, ins, ORIGIN, VS, oriented=oriented)
    assert [(r["class_id"], r["instance"], r["voxels"]) for r in got] == [(2, 0, 12), (5, 7, 5), (6, 7, 4), (8, 1, 1), (39, 3, 2)]
    assert ("heading" in got[0]) == oriented
    small = run_scene(SO, cells, tsdf, sem, ins, oriented=oriented, min_voxels=4, surface=0.45)
    assert small == R.scene(cells, tsdf, sem, ins, ORIGIN, VS, oriented=oriented, min_voxels=4, surface=0.45)
    assert [(r["id"], r["voxels"]) for r in small] == [(0, 12), (1, 5)]


def test_ids_without_a_mapping_and_a_class_outside_it(SO):
    cells, tsdf, sem, ins = hand_scene()
    ids = np.array(R.MAPPING)[sem]
    assert run_scene(SO, cells, tsdf, ids, ins, mapping=None) == R.scene(cells, tsdf, sem, ins, ORIGIN, VS)
    sem = sem.copy()
    sem[0] = 21
    with pytest.raises(ValueError, match="outside"):
        run_scene(SO, cells, tsdf, sem, ins)


@pytest.mark.parametrize("m", [65, 1025])
def test_boxes_hold_their_cells(SO, m):
    """Every participating cell centre lies inside both boxes of its segment, and each of the six faces of both boxes is
    half a voxel from some cell centre.  Exact where the numbers are lattice units (the table's min / max, the extents
    along the box's own axes); the records, with origin 0 and voxel size 1, are compared to those within 1e-12: they come
    from fewer than ten float64 operations on numbers below 16 (relative rounding 1.1e-16 each)."""
    coords, rank, _, _, _ = seeded_case(m, 5)
    part = (rank >= 0) & (rank < 5)
    # five classes with one instance each: the segments are the ranks
    objs = run_scene(SO, coords[part], np.zeros(part.sum()), 3 + rank[part], np.ones(part.sum()), (0, 0, 0), 1.0)
    assert [r["id"] for r in objs] == sorted(set(rank[part].tolist()))
    table = run_moments(SO, coords, rank, 5)
    dirs = SO.directions(table)
    ext = run_extents(SO, coords, rank, 5, dirs)
    for rec in objs:
        cells = coords[rank == rec["id"]].astype(np.float64)
        assert rec["voxels"] == len(cells)
        lo, hi = table[rec["id"], 10:13], table[rec["id"], 13:16]
        assert np.array_equal(lo, cells.min(0)) and np.array_equal(hi, cells.max(0))
        assert rec["aabb_min"] == (lo - 0.5).tolist() and rec["aabb_max"] == (hi + 0.5).tolist()      # (origin 0, size 1: exact)
        c, s = dirs[rec["id"]]
        assert (c, s) == (math.cos(rec["heading"]), math.sin(rec["heading"]))
        u, v = cells[:, 0] * c + cells[:, 1] * s, cells[:, 1] * c - cells[:, 0] * s
        assert np.array_equal(bits(ext[rec["id"]]), bits([u.min() + 0.0, u.max() + 0.0, v.min() + 0.0, v.max() + 0.0]))
        # the record's box in its own axes: centre +- size / 2 is half a voxel outside the extreme cell centres
        centre, size = np.array(rec["obb_centre"]), np.array(rec["obb_size"])
        own = np.array([centre[0] * c + centre[1] * s, centre[1] * c - centre[0] * s, centre[2]])
        want_lo = np.array([u.min(), v.min(), cells[:, 2].min()]) - 0.5
        want_hi = np.array([u.max(), v.max(), cells[:, 2].max()]) + 0.5
        assert np.abs(own - size / 2 - want_lo).max() < 1e-12 and np.abs(own + size / 2 - want_hi).max() < 1e-12
        assert -np.pi / 2 < rec["heading"] <= np.pi / 2
        assert all(a <= x <= b for a, x, b in zip(rec["aabb_min"], rec["centroid"], rec["aabb_max"]))


# ---------------------------------------------------------------------------------------------------------------- files

def volume_scene(seed=5, dims=(10, 9, 8)):
    rng = np.random.default_rng(seed)
    tsdf = np.ones(dims, np.float32)
    sem, ins = np.zeros(dims, np.int32), np.zeros(dims, np.int32)
    near = rng.random(dims) < 0.4
    tsdf[near] = rng.uniform(-1, 1, near.sum()).astype(np.float32)
    tsdf[2, 3, 4], tsdf[5, 5, 5] = -1.0, 0.0
    labelled = near & (rng.random(dims) < 0.8)
    sem[labelled] = rng.integers(0, 8, labelled.sum())
    ins[labelled] = rng.integers(1, 4, labelled.sum())
    sem[0, 0, 0], ins[0, 0, 0] = 3, 2        # a labelled cell at tsdf 1: a row of the file, not of the inventory
    return tsdf, sem, ins


def reference_of_volumes(tsdf, sem, ins, mapping=R.MAPPING, **rule):
    cells = np.argwhere((tsdf != 1) | (sem != 0) | (ins != 0))
    at = tuple(cells.T)
    return R.scene(cells, tsdf[at], sem[at], ins[at], ORIGIN, VS, mapping=mapping, **rule)


def write_both_forms(SIO, root, tsdf, sem, ins):
    os.makedirs(root, exist_ok=True)
    head = dict(origin=np.asarray(ORIGIN, np.float32), voxel_size=VS)
    dense, sparse = os.path.join(root, "dense", "s0.npz"), os.path.join(root, "sparse", "s0.npz")
    os.makedirs(os.path.dirname(dense)), os.makedirs(os.path.dirname(sparse))
    SIO.write_scene(dense, tsdf, sem, ins, **head)
    rows = np.argwhere((tsdf != 1) | (sem != 0) | (ins != 0))
    rows = rows[np.random.default_rng(0).permutation(len(rows))]
    at = tuple(rows.T)
    SIO.write_scene(sparse, tsdf[at], sem[at], ins[at], coords=rows.astype(np.int32), dims=np.array(tsdf.shape), **head)
    return dense, sparse


def test_dense_and_sparse_files_give_the_same_objects(SO, tmp_path):
    from eprecon_amd import scene_io as SIO
    tsdf, sem, ins = volume_scene()
    dense, sparse = write_both_forms(SIO, str(tmp_path), tsdf, sem, ins)
    want = reference_of_volumes(tsdf, sem, ins, min_voxels=2)
    assert len(want) >= 5
    out = str(tmp_path / "out" / "s0_objects.json")
    a = SO.describe_scene(dense, out_json=out, boxes_ply=str(tmp_path / "out" / "boxes_s0.ply"), min_voxels=2)
    b = SO.describe_scene(sparse, min_voxels=2)
    assert a == want and b == want
    with open(out) as fh:
        doc = json.load(fh)
    assert doc["objects"] == want and doc["scene"] == "s0" and doc["rule"]["min_voxels"] == 2
    verts, faces = SIO.read_ply(str(tmp_path / "out" / "boxes_s0.ply"))
    assert verts.shape == (8 * len(want), 3) and faces.shape == (0, 3)


def test_command_line_with_ground_truth(SO, tmp_path, capsys):
    from eprecon_amd import scene_io as SIO
    tsdf, sem, ins = volume_scene()
    dense, _ = write_both_forms(SIO, str(tmp_path), tsdf, sem, ins)
    g_tsdf, g_sem, g_ins = volume_scene(seed=6, dims=(7, 8, 9))
    g_sem = np.array([0, 1, 2, 13, 5, 40, 24, 39])[g_sem].astype(np.int32)      # ScanNet ids, two of them (13, 40) void
    gt = tmp_path / "gt" / "s0"
    os.makedirs(gt)
    with open(gt / "tsdf_info.pkl", "wb") as fh:
        pickle.dump({"vol_origin": np.asarray(ORIGIN, np.float32), "voxel_size": VS}, fh)
    np.savez_compressed(str(gt / "full_tsdf_layer0"), g_tsdf)
    np.savez_compressed(str(gt / "full_semantic_layer_interpolate0"), g_sem)
    np.savez_compressed(str(gt / "full_instance_layer_interpolate0"), g_ins)
    (tmp_path / "scenes.txt").write_text("s0\n")
    (tmp_path / "names.txt").write_text("1 wall\n2 floor\n")
    out = tmp_path / "objects"
    assert SO.main(["--pred", os.path.dirname(dense), "--scenes", str(tmp_path / "scenes.txt"), "--out", str(out), "--gt",
                    str(tmp_path / "gt"), "--boxes", "--names", str(tmp_path / "names.txt"), "--no-oriented"]) == 0
    assert sorted(os.listdir(out)) == ["boxes_s0.ply", "boxes_s0_gt.ply", "s0_objects.json", "s0_objects_gt.json"]
    names = {1: "wall", 2: "floor"}
    named = lambda objs: [dict(r, class_name=names.get(r["class_id"], "")) for r in objs]
    with open(out / "s0_objects.json") as fh:
        assert json.load(fh)["objects"] == named(reference_of_volumes(tsdf, sem, ins, oriented=False))
    with open(out / "s0_objects_gt.json") as fh:
        doc = json.load(fh)
    want = named(reference_of_volumes(g_tsdf, g_sem, g_ins, mapping=None, oriented=False))
    assert doc["objects"] == want and len(want) >= 5 and doc["rule"]["mapping"] is None
    assert not {13, 40} & {r["class_id"] for r in want}
    assert "s0: " in capsys.readouterr().out


def test_reconstruct_writes_the_file_beside_the_scene(SO, tmp_path):
    from eprecon_amd import reconstruct
    from eprecon_amd import scene_io as SIO
    tsdf, sem, ins = volume_scene()
    save = tmp_path / "log_fusion_eval_47"
    os.makedirs(save)
    SIO.write_scene(str(save / "scene0000_00.npz"), tsdf, sem, ins, origin=np.asarray(ORIGIN, np.float32), voxel_size=VS)
    saver = SimpleNamespace(log_dir=str(tmp_path / "log"))
    reconstruct.describe_saved_scenes({"scene_name": ["scene0000_00", "scene0000_01"]}, saver, 47)
    assert sorted(os.listdir(save)) == ["scene0000_00.npz", "scene0000_00_objects.json"]
    with open(save / "scene0000_00_objects.json") as fh:
        assert json.load(fh)["objects"] == reference_of_volumes(tsdf, sem, ins)


def test_reconstruct_objects_then_the_command_line(SO, tmp_path, capsys):
    """reconstruct --objects writes <scene>_objects.json beside the scene it saved; the command line on that scene gives the
    same records and the box file; both are the restatement's records of the file's rows"""
    pytest.importorskip("PIL")
    from test_reconstruct_gpu import HEIGHT, SCENE, WIDTH, write_scene
    from eprecon_amd import reconstruct
    from eprecon_amd import scene_io as SIO
    root, out = str(tmp_path / "data"), str(tmp_path / "run")
    write_scene(root)
    assert reconstruct.main(["--data_path", root, "--out", out, "--size", str(WIDTH), str(HEIGHT), "--objects"]) == 0
    saved = os.path.join(out, "scene_scannet_fusion_eval_0")
    assert SCENE + "_objects.json" in os.listdir(saved) and f"{SCENE}_objects.json" in capsys.readouterr().out
    with open(os.path.join(saved, SCENE + "_objects.json")) as fh:
        beside = json.load(fh)
    (tmp_path / "scenes.txt").write_text(SCENE + "\n")
    assert SO.main(["--pred", saved, "--scenes", str(tmp_path / "scenes.txt"), "--out", str(tmp_path / "objects"), "--boxes"]) == 0
    assert sorted(os.listdir(tmp_path / "objects")) == sorted([f"{SCENE}_objects.json", f"boxes_{SCENE}.ply"])
    with open(tmp_path / "objects" / f"{SCENE}_objects.json") as fh:
        doc = json.load(fh)
    assert doc == beside and doc["scene"] == SCENE
    scene = SIO.read_scene(os.path.join(saved, SCENE + ".npz"))
    rows, tsdf, sem, ins, _ = SIO.raster_rows(scene)
    assert doc["objects"] == R.scene(rows, tsdf, sem, ins, scene.origin, scene.voxel_size)
    verts, _ = SIO.read_ply(str(tmp_path / "objects" / f"boxes_{SCENE}.ply"))
    assert len(verts) == 8 * len(doc["objects"])


def test_an_empty_scene(SO, tmp_path, capsys):
    from eprecon_amd import scene_io as SIO
    dims = (4, 4, 4)
    path = str(tmp_path / "empty.npz")
    SIO.write_scene(path, np.ones(dims, np.float32), np.zeros(dims, np.int32), np.zeros(dims, np.int32),
                    origin=np.asarray(ORIGIN, np.float32), voxel_size=VS)
    assert SO.describe_scene(path, out_json=str(tmp_path / "empty_objects.json")) == []
    assert "No valid data for scene empty" in capsys.readouterr().out
    with open(tmp_path / "empty_objects.json") as fh:
        assert json.load(fh)["objects"] == []

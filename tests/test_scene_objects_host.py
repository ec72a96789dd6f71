"""CPU: the host half of the object inventory (eprecon_amd/scene_objects.py: finish, the files, the arguments) against the
restatement of tests/scene_objects_ref.py, and that restatement against scenes built by hand.  What `finish` and the
restatement share is the stated arithmetic, so their records are compared with ==; the hand-made scenes are
compared with the numbers a reader can work out, to 1e-12 where cos(pi/2) = 6e-17 enters."""
import json
import math

import numpy as np
import pytest
import torch

import scene_objects_ref as R

VS = 0.04
ORIGIN = (-1.5, 0.25, 0.125)


@pytest.fixture(scope="module")
def SO():
    from eprecon_amd import scene_objects
    return scene_objects


def hand_scene(cells, cls=3, ins=7):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    m = len(cells)
    return R.scene(cells, np.zeros(m, np.float32), np.full(m, cls), np.full(m, ins), ORIGIN, VS)


def close(a, b):
    return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the restatement by hand

def test_one_voxel_has_the_size_of_a_voxel():
    (rec,) = hand_scene([[5, -2, 3]])
    centre = [ORIGIN[0] + 5 * VS, ORIGIN[1] - 2 * VS, ORIGIN[2] + 3 * VS]
    assert rec["voxels"] == 1 and (rec["class_id"], rec["instance"]) == (3, 7) and rec["heading"] == 0.0
    assert close(rec["centroid"], centre) and close(rec["obb_centre"], centre)
    assert close(rec["obb_size"], [VS] * 3)
    assert close(np.subtract(rec["aabb_max"], rec["aabb_min"]), [VS] * 3)
    assert close(np.add(rec["aabb_max"], rec["aabb_min"]) / 2, centre)


def test_bar_along_y_heads_along_y():
    (rec,) = hand_scene([[2, y, 1] for y in range(5)])
    assert rec["heading"] == math.pi / 2
    assert close(rec["obb_size"], [5 * VS, VS, VS])
    assert close(rec["obb_centre"], [ORIGIN[0] + 2 * VS, ORIGIN[1] + 2 * VS, ORIGIN[2] + VS])
    assert close(np.subtract(rec["aabb_max"], rec["aabb_min"]), [VS, 5 * VS, VS])


def test_diagonal_bar_heads_along_the_diagonal():
    (rec,) = hand_scene([[k, k, 0] for k in range(6)])
    assert rec["heading"] == math.pi / 4
    assert close(rec["obb_size"], [(5 * math.sqrt(2) + 1) * VS, VS, VS])
    assert close(rec["obb_centre"], [ORIGIN[0] + 2.5 * VS, ORIGIN[1] + 2.5 * VS, ORIGIN[2]])


def test_anti_diagonal_bar_has_a_negative_heading():
    (rec,) = hand_scene([[k, -k, 0] for k in range(6)])
    assert rec["heading"] == -math.pi / 4


def test_square_footprint_has_no_heading():
    (rec,) = hand_scene([[x, y, z] for x in range(3) for y in range(3) for z in range(2)])
    assert rec["heading"] == 0.0 and rec["voxels"] == 18
    assert close(rec["obb_size"], [3 * VS, 3 * VS, 2 * VS])
    assert close(rec["obb_centre"], np.add(rec["aabb_min"], rec["aabb_max"]) / 2)


def test_segments_follow_the_stuff_rule():
    cells = [[0, 0, 0], [1, 0, 0], [5, 5, 0], [6, 5, 0], [9, 9, 9], [3, 3, 3], [4, 4, 4]]
    sem = [1, 1, 4, 5, 0, 4, 13]            # class indices: 13 -> ScanNet id 14
    ins = [3, 8, 2, 2, 6, 2, 1]
    tsdf = [0, 0.5, 0, 0, 0, 1.0, -0.25]
    objs = R.scene(cells, tsdf, sem, ins, ORIGIN, VS)
    assert [(r["class_id"], r["instance"], r["voxels"]) for r in objs] == [(1, 0, 2), (4, 2, 1), (5, 2, 1), (14, 1, 1)]
    assert [r["id"] for r in objs] == [0, 1, 2, 3]
    assert [r["id"] for r in R.scene(cells, tsdf, sem, ins, ORIGIN, VS, min_voxels=2)] == [0]


# -------------------------------------------------------------------------------------------------------------- finish

def seeded_tables(seed, n, big=False):
    """n moment rows of Python ints with a count >= 1, the sums within what that many rows in range can give (at the top of
    the range with `big`: sums of squares near 2^62), and extents with min <= max"""
    rng = np.random.default_rng(seed)
    table = []
    for _ in range(n):
        count = int(rng.integers(2 ** 24 - 1000, 2 ** 24)) if big else int(rng.integers(1, 5000))
        span = R.LIMIT if big else 300
        lo = [int(v) for v in rng.integers(-span, span // 2, 3)]
        hi = [int(l + v) for l, v in zip(lo, rng.integers(0, span // 2, 3))]
        if big:
            sums = [int(count * h - rng.integers(0, 1000)) for h in hi]
            sq = [int(count * R.LIMIT ** 2 - rng.integers(0, 10 ** 6)) for _ in range(6)]
        else:
            sums = [int(rng.integers(count * l, count * h + 1)) for l, h in zip(lo, hi)]
            sq = [int(rng.integers(-count * span ** 2, count * span ** 2)) for _ in range(6)]
            sq[0], sq[3], sq[5] = abs(sq[0]), abs(sq[3]), abs(sq[5])
        table.append([count] + sums + sq + lo + hi)
    ext = np.sort(rng.uniform(-span, span, (n, 2, 2)), axis=2).reshape(n, 4)
    keys = sorted({(int(c), 0 if c in R.STUFF else int(i)) for c, i in zip(rng.choice(R.VALID, 4 * n), rng.integers(-5, 90, 4 * n))})[:n]
    assert len(keys) == n
    return table, ext, keys


def pack_keys(keys):
    return np.array([(c << 32) + (i + (1 << 31)) for c, i in keys], np.int64)


@pytest.mark.parametrize("seed,big", [(0, False), (1, False), (2, True)])
@pytest.mark.parametrize("oriented", [True, False])
def test_finish_equals_the_restatement(SO, seed, big, oriented):
    table, ext, keys = seeded_tables(seed, 12, big)
    if big:
        assert max(max(t) for t in table) > 2 ** 61 and max(max(t) for t in table) < 2 ** 62
    arr = R.table_array(table)
    got = SO.finish(arr, ext if oriented else None, pack_keys(keys), np.float32(ORIGIN), VS, min_voxels=1)
    want = R.records(table, ext if oriented else None, keys, ORIGIN, VS, 1)
    assert got == want and len(got) == 12
    assert np.array_equal(SO.directions(arr), R.directions(table))


def test_finish_drops_small_and_empty_segments_and_keeps_the_rank(SO):
    table, ext, keys = seeded_tables(3, 6)
    table[2] = R.identity_row()
    table[4][0] = 3
    arr = R.table_array(table)
    got = SO.finish(arr, ext, pack_keys(keys), ORIGIN, VS, min_voxels=4)
    want = R.records(table, ext, keys, ORIGIN, VS, 4)
    assert got == want
    ids = [r["id"] for r in got]
    assert 2 not in ids and 4 not in ids and ids == sorted(ids)
    assert 2 not in [r["id"] for r in SO.finish(arr, ext, pack_keys(keys), ORIGIN, VS, min_voxels=0)]


def test_record_key_order_and_json_round_trip(SO, tmp_path):
    table, ext, keys = seeded_tables(4, 5)
    objs = SO.finish(R.table_array(table), ext, pack_keys(keys), ORIGIN, VS)
    assert all(tuple(r) == SO.RECORD_KEYS for r in objs)
    plain = SO.finish(R.table_array(table), None, pack_keys(keys), ORIGIN, VS)
    assert all(tuple(r) == SO.RECORD_KEYS[:7] for r in plain)
    rule = dict(mapping=SO.SCANNET20_MAPPING, surface=1.0, min_voxels=1, oriented=True)
    path = tmp_path / "out" / "s0_objects.json"
    named = SO.write_objects("s0", objs, ORIGIN, VS, rule, str(path), None, {keys[0][0]: "a name"})
    assert all(tuple(r) == SO.RECORD_KEYS + ("class_name",) for r in named)
    assert named[0]["class_name"] == "a name"
    with open(path) as fh:
        doc = json.load(fh)
    assert list(doc) == ["scene", "voxel_size", "origin", "rule", "objects"]
    assert doc["objects"] == named and doc["scene"] == "s0" and doc["voxel_size"] == VS
    assert doc["origin"] == [float(np.float32(v)) for v in ORIGIN]
    assert doc["rule"] == {"surface": 1.0, "min_voxels": 1, "oriented": True, "mapping": list(SO.SCANNET20_MAPPING)}
    assert [tuple(r) for r in doc["objects"]] == [tuple(r) for r in named]


def test_an_empty_scene_writes_an_empty_list_with_the_warning(SO, tmp_path, capsys):
    rule = dict(mapping=None, surface=1.0, min_voxels=1, oriented=False)
    assert SO.write_objects("s1", [], ORIGIN, VS, rule, str(tmp_path / "s1_objects.json"), str(tmp_path / "boxes_s1.ply"), None) == []
    assert "No valid data for scene s1" in capsys.readouterr().out
    with open(tmp_path / "s1_objects.json") as fh:
        doc = json.load(fh)
    assert doc["objects"] == [] and doc["rule"]["mapping"] is None
    from eprecon_amd.scene_io import read_ply
    verts, faces = read_ply(str(tmp_path / "boxes_s1.ply"))
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------- files

def test_names_file(SO, tmp_path):
    path = tmp_path / "names.txt"
    path.write_text("1 wall\n\n  5   office chair  \n39\totherfurniture\n7\n")
    assert SO.read_names(str(path)) == {1: "wall", 5: "office chair", 39: "otherfurniture", 7: ""}
    path.write_text("1 wall\nchair 5\n")
    with pytest.raises(ValueError, match="names.txt:2"):
        SO.read_names(str(path))


def test_arguments(SO):
    args = SO.parse_args(["--pred", "p", "--scenes", "s.txt", "--out", "o"])
    assert (args.pred, args.scenes, args.out, args.gt, args.names) == ("p", "s.txt", "o", None, None)
    assert (args.min_voxels, args.surface, args.oriented, args.boxes) == (1, 1.0, True, False)
    args = SO.parse_args(["--pred", "p", "--scenes", "s.txt", "--out", "o", "--gt", "g", "--min_voxels", "50", "--surface", "0.5",
                          "--no-oriented", "--boxes", "--names", "n.txt"])
    assert (args.gt, args.min_voxels, args.surface, args.oriented, args.boxes, args.names) == ("g", 50, 0.5, False, True, "n.txt")
    with pytest.raises(SystemExit):
        SO.parse_args(["--pred", "p", "--scenes", "s.txt"])


def test_reconstruct_takes_objects():
    from eprecon_amd import reconstruct
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o", "--objects"]).objects is True
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o"]).objects is False


def read_edges(path, n_vertices):
    """the `edge` element behind the vertices of a file write_boxes wrote"""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    n_edges = int([l for l in lines if l.startswith("element edge")][0].split()[2])
    assert "property int vertex1" in lines and "property int vertex2" in lines
    vertex_bytes = 3 * 4 + 3
    assert len(body) == n_vertices * vertex_bytes + n_edges * 8
    return np.frombuffer(body, "<i4", 2 * n_edges, n_vertices * vertex_bytes).reshape(-1, 2)


@pytest.mark.parametrize("oriented", [True, False])
def test_boxes_file_reads_back(SO, tmp_path, oriented):
    from eprecon_amd.scene_io import read_ply
    cells = [[k, 2 * k, 0] for k in range(4)] + [[10, 10, z] for z in range(3)]
    objs = R.scene(cells, np.zeros(7), [3] * 4 + [1] * 3, [5] * 4 + [9] * 3, ORIGIN, VS, oriented=oriented)
    assert len(objs) == 2
    path = str(tmp_path / "boxes_s0.ply")
    SO.write_boxes(objs, path)
    verts, faces = read_ply(path)
    assert verts.shape == (16, 3) and faces.shape == (0, 3)
    edges = read_edges(path, 16)
    assert edges.shape == (24, 2)
    for k, rec in enumerate(objs):
        corners = SO.box_corners(rec)
        assert np.array_equal(verts[8 * k:8 * k + 8], corners.astype(np.float32))
        e = edges[12 * k:12 * k + 12] - 8 * k
        assert e.min() == 0 and e.max() == 7 and (np.bincount(e.reshape(-1)) == 3).all()
        # an edge of a box joins corners that differ along one of its axes only: its length is one of the three sizes
        size = rec["obb_size"] if oriented else np.subtract(rec["aabb_max"], rec["aabb_min"])
        length = np.linalg.norm(corners[e[:, 0]] - corners[e[:, 1]], axis=1)
        assert np.allclose(np.sort(length), np.sort(np.repeat(size, 4)), rtol=0, atol=1e-12)
        assert np.allclose(corners.mean(0), rec["obb_centre"] if oriented else np.add(rec["aabb_min"], rec["aabb_max"]) / 2, atol=1e-12)


def test_export_ply_still_writes_meshes(tmp_path):
    from eprecon_amd.scene_io import export_ply, read_ply
    mesh = {"vertices": np.eye(3, dtype=np.float32), "vertex_normals": np.ones((3, 3), np.float32), "faces": np.array([[0, 1, 2]])}
    export_ply(mesh, str(tmp_path / "m.ply"))
    verts, faces = read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(verts, mesh["vertices"]) and np.array_equal(faces, mesh["faces"])


# --------------------------------------------------------------------------------------------------------------- errors

def test_errors(SO, tmp_path):
    from eprecon_amd import _lib
    table, ext, keys = seeded_tables(5, 3)
    arr = R.table_array(table)
    with pytest.raises(ValueError, match="keys"):
        SO.finish(arr, None, pack_keys(keys)[:2], ORIGIN, VS)
    with pytest.raises(ValueError, match="extents"):
        SO.finish(arr, ext[:2], pack_keys(keys), ORIGIN, VS)
    coords, rank = torch.zeros((4, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.EpreconError):
        SO.segment_moments(coords, rank, 1)
    with pytest.raises(_lib.EpreconError):
        SO.segment_extents(coords, rank, 1, torch.zeros((1, 2), dtype=torch.float64))
    with pytest.raises(_lib.EpreconError):
        SO.scene_objects(coords, torch.zeros(4), rank, rank, ORIGIN, VS)
    with pytest.raises(TypeError, match="unknown"):
        SO.describe_scene(str(tmp_path / "none.npz"), threshold=3)
    with pytest.raises(ValueError, match="outside the mapping"):
        R.labels([21], [0], [0.0])

"""GPU: connected components of voxel rows (eprecon_amd/clean_scene.py, csrc/components.hip) and the clean-up rule built on
them against the host restatement of tests/clean_scene_ref.py and against scenes built by hand.  Every comparison is exact.

Random boxes: seeded occupancy at the densities 0.32 / 0.14 / 0.10 for connectivity 6 / 18 / 26 (at the site-percolation
thresholds 0.312 / 0.137 / 0.098 of the cubic lattice, so components run from single rows to hundreds; at 0.30 the largest
6-connected component of 1,025 rows had 64 rows, at 0.32 it has 170).  A 12^3 box holds about 550 / 240 / 170 rows at those
densities; where a case wants more rows than that, the box is the smallest cube from 12 upward in which the same seeded
occupancy has them (15^3 / 20^3 / 22^3 for 1,025 rows).  The first M rows in raster order (a slab of the box at full
density) are then put into a seeded random order."""
import functools
import os
import pickle
from collections import Counter

import numpy as np
import pytest
import torch

import clean_scene_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DENSITY = {6: 0.32, 18: 0.14, 26: 0.10}
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)
ALL_ON = dict(min_voxels=3, min_segment_voxels=2, split_instances=True)


@pytest.fixture(scope="module")
def CS():
    from eprecon_amd import clean_scene
    return clean_scene


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def run_components(CS, coords, keys=None, connectivity=26):
    label = CS.components(dev(np.asarray(coords).reshape(-1, 3)), None if keys is None else dev(keys), connectivity)
    assert label.dtype == torch.int32 and label.device.type == "cuda"
    return label.cpu().numpy()


def assert_label_properties(label, keys=None):
    i = np.arange(len(label))
    live = label >= 0
    assert (label[live] <= i[live]).all() and (label[label[live]] == label[live]).all()
    if keys is not None:
        assert ((np.asarray(keys) < 0) == ~live).all()
    else:
        assert live.all()


# ------------------------------------------------------------------------------------------------------------ components

@functools.lru_cache(maxsize=None)
def box_case(connectivity, m):
    """-> (coords int32[m,3], keys int32[m] of three values and -1, label without keys, label with keys)"""
    for side in range(12, 40):
        rng = np.random.default_rng(1000 * connectivity + m)
        rows = np.argwhere(rng.random((side, side, side)) < DENSITY[connectivity])
        if len(rows) >= m:
            break
    coords = rows[:m][rng.permutation(m)].astype(np.int32)
    keys = rng.integers(-1, 3, m).astype(np.int32)
    return coords, keys, R.components_ref(coords, None, connectivity), R.components_ref(coords, keys, connectivity)


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_random_box_against_restatement(CS, connectivity, m):
    coords, keys, want_plain, want_keyed = box_case(connectivity, m)
    got = run_components(CS, coords, None, connectivity)
    assert_label_properties(got)
    assert np.array_equal(got, want_plain)
    got = run_components(CS, coords, keys, connectivity)
    assert_label_properties(got, keys)
    assert np.array_equal(got, want_keyed)


def test_random_boxes_have_components_of_many_sizes():
    """what the densities are for: at 1,025 rows the components run from single rows to a hundred and more"""
    for connectivity in (6, 18, 26):
        sizes = np.bincount(box_case(connectivity, 1025)[2])
        assert (sizes == 1).any() and sizes.max() >= 100, (connectivity, sizes.max())


def snake():
    path = []
    for z in range(16):
        for yi, y in enumerate(range(16) if z % 2 == 0 else range(15, -1, -1)):
            forward = (16 * z + yi) % 2 == 0
            path += [(x, y, z) for x in (range(16) if forward else range(15, -1, -1))]
    path = np.array(path, np.int32)
    assert len(path) == 4096 and (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
    return path


@pytest.mark.parametrize("order", ["path", "reversed", "permuted"])
def test_snake_is_one_component(CS, order):
    """one 6-connected path of 4,096 rows through a 16^3 box: incomplete propagation, or a chain lost between workgroups,
    leaves a label above 0"""
    path = snake()
    rows = {"path": path, "reversed": path[::-1], "permuted": path[np.random.default_rng(7).permutation(4096)]}[order]
    for connectivity in (6, 18, 26):
        assert not run_components(CS, rows, None, connectivity).any()


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_block_keyed_by_parity(CS, connectivity):
    """a full 8^3 block keyed by the parity of x + y + z: rows of one key never share a face, always an edge"""
    coords = np.argwhere(np.ones((8, 8, 8), bool)).astype(np.int32)
    keys = coords.sum(1) & 1
    got = run_components(CS, coords, keys, connectivity)
    if connectivity == 6:
        assert np.array_equal(got, np.arange(512))
    else:
        assert np.array_equal(got, keys)          # rows 0 = (0,0,0) and 1 = (0,0,1) are the two components' smallest
    assert np.array_equal(got, R.components_ref(coords, keys, connectivity))


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_component_straddling_the_origin(CS, connectivity):
    block = np.argwhere(np.ones((5, 5, 5), bool)).astype(np.int32) - 2
    axes = block[(block != 0).sum(1) <= 1]                       # the three axes from -2 to 2: 13 rows through the origin
    diagonal = np.array([(t, t, t) for t in range(-2, 3)], np.int32)
    rng = np.random.default_rng(5)
    for coords in (block[rng.permutation(125)], axes[rng.permutation(13)], diagonal):
        got = run_components(CS, coords, None, connectivity)
        assert np.array_equal(got, R.components_ref(coords, None, connectivity))
    assert not run_components(CS, axes, None, connectivity).any()
    assert np.array_equal(run_components(CS, diagonal, None, connectivity), [0] * 5 if connectivity == 26 else np.arange(5))


def test_argument_handling(CS):
    from eprecon_amd._lib import EpreconError
    empty = CS.components(torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert empty.shape == (0,) and empty.dtype == torch.int32 and empty.device.type == "cuda"
    with pytest.raises(ValueError):
        CS.components(dev([(0, 0, 0), (1, 0, 0), (0, 0, 0)]))
    with pytest.raises(EpreconError):
        CS.components(torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        CS.components(dev([(0, 0, 0)]), connectivity=8)
    with pytest.raises(EpreconError):
        CS.components(dev([(0, 0, 0), (1 << 19, 0, 0)]))


def test_two_runs_are_bit_equal(CS):
    coords, keys, _, _ = box_case(26, 1025)
    first = CS.components(dev(coords), dev(keys), 26)
    assert torch.equal(first, CS.components(dev(coords), dev(keys), 26))
    path = dev(snake())
    assert torch.equal(CS.components(path, None, 6), CS.components(path, None, 6))


def test_exported_workspace_query(CS):
    from eprecon_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 64, 65, 1025):
        assert lib.eprecon_components_workspace_bytes(n) >= 4 * n
    status = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    assert lib.eprecon_components_async(None, 0, None, 26, None, _lib.ptr(status), None, 0, _lib.current_stream()) == 0
    assert int(status.item()) == 0                                   # n == 0 clears the status word and nothing else
    nbr = torch.full((27, 4), -1, dtype=torch.int32, device=DEV)
    label = torch.empty(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(8, dtype=torch.uint8, device=DEV)
    call = lambda c, size: lib.eprecon_components_async(_lib.ptr(nbr), 4, None, c, _lib.ptr(label), _lib.ptr(status), _lib.ptr(ws),
                                                        size, _lib.current_stream())
    assert call(26, 8) == -2 and call(7, 8) == -1                    # workspace too small, bad connectivity: nothing launched


# ------------------------------------------------------------------------------------------------------------------ rule

def run_clean(CS, coords, tsdf, semantic, instance, **rule):
    c, t, s, i, report = CS.clean_rows(dev(coords), dev(tsdf, torch.float32), dev(semantic, torch.int64), dev(instance, torch.int64),
                                       **rule)
    assert c.dtype == torch.int32 and t.dtype == torch.float32 and s.dtype == torch.int64 and i.dtype == torch.int64
    return c.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), report


def assert_same_as_ref(got, coords, tsdf, semantic, instance, **rule):
    want = R.clean_rows_ref(coords, np.asarray(tsdf, np.float32), semantic, instance, **rule)
    for g, w in zip(got[:4], want[:4]):
        assert g.shape == w.shape and np.array_equal(g, w)
    assert got[4] == want[4]


def block(lo, size):
    return [tuple(int(v) for v in np.add(lo, d)) for d in np.ndindex(*size)]


PLATE = [(x, y, z) for x in range(20) for y in range(20) for z in range(3)]
BLOB1 = [(2, 2, 6)]
BLOB7 = [(8, 8, 7)] + [tuple(int(v) for v in np.add((8, 8, 7), d)) for d in
                        ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
BLOB8 = block((14, 2, 6), (2, 2, 2))
BLOB27 = block((14, 12, 6), (3, 3, 3))
DIMS = (24, 24, 12)


def plate_scene(extra=()):
    coords = np.array(PLATE + BLOB1 + BLOB7 + BLOB8 + BLOB27 + list(extra), np.int32)
    rng = np.random.default_rng(11)
    tsdf = np.concatenate([np.array([(-0.5, 0.0, 0.5)[z] for _, _, z in PLATE], np.float32),
                           rng.uniform(-0.9, 0.9, len(coords) - len(PLATE)).astype(np.float32)])
    order = rng.permutation(len(coords))
    zeros = np.zeros(len(coords), np.int64)
    return coords[order], tsdf[order], zeros, zeros


def as_set(coords):
    return {tuple(r) for r in np.asarray(coords).tolist()}


def test_plate_and_blobs(CS):
    scene = plate_scene()
    assert len(BLOB7) == 7 and len(BLOB8) == 8 and len(BLOB27) == 27 and len(as_set(scene[0])) == 1200 + 43
    got = run_clean(CS, *scene, min_voxels=8)
    assert as_set(got[0]) == as_set(PLATE + BLOB8 + BLOB27)
    assert got[4] == dict(zip(R.REPORT_KEYS, (1243, 8, 5, 2, 0, 0, 0)))
    assert_same_as_ref(got, *scene, min_voxels=8)
    kept = np.array([tuple(r) in as_set(got[0]) for r in scene[0].tolist()])
    assert np.array_equal(got[0], scene[0][kept]) and np.array_equal(got[1], scene[1][kept])     # the rows keep their order
    got = run_clean(CS, *scene, keep_largest=1)
    assert as_set(got[0]) == as_set(PLATE) and got[4]["components_removed"] == 4
    assert_same_as_ref(got, *scene, keep_largest=1)
    got = run_clean(CS, *scene, keep_largest=2, min_voxels=100)             # keep_largest replaces min_voxels
    assert as_set(got[0]) == as_set(PLATE + BLOB27)


def test_blob_touching_the_plate_at_a_corner(CS):
    corner = (20, 20, 3)                                                   # shares only a corner with the plate's (19, 19, 2)
    scene = plate_scene([corner])
    for connectivity, stays in ((26, True), (18, False), (6, False)):
        got = run_clean(CS, *scene, min_voxels=8, connectivity=connectivity)
        assert (corner in as_set(got[0])) == stays
        assert_same_as_ref(got, *scene, min_voxels=8, connectivity=connectivity)


def triangles(volume):
    from eprecon_amd.save_scene import marching_cubes
    verts, faces, _ = marching_cubes(dev(volume, torch.float32), 0.0)
    corners = verts[faces.long()].cpu().numpy().astype(np.float32)         # [T,3,3]
    bits = np.ascontiguousarray(corners.reshape(len(corners), 9)).view(np.uint32).tobytes()
    return Counter(bits[36 * t:36 * t + 36] for t in range(len(corners)))


def test_meshes_of_kept_and_removed_rows_add_up(CS):
    """connectivity 26: separated components share no marching-cubes cell, so the triangles of the original volume are the
    disjoint union of those of the cleaned volume and of the volume holding the removed rows alone (positions bit for
    bit; normals reach a cell further and are not compared)"""
    coords, tsdf, sem, ins = plate_scene()
    got = run_clean(CS, coords, tsdf, sem, ins, min_voxels=8, connectivity=26)

    def volume(c, t):
        vol = np.ones(DIMS, np.float32)
        vol[c[:, 0], c[:, 1], c[:, 2]] = t
        return vol

    gone = np.array([tuple(r) not in as_set(got[0]) for r in coords.tolist()])
    assert gone.sum() == 8
    original, cleaned, removed = triangles(volume(coords, tsdf)), triangles(volume(got[0], got[1])), triangles(volume(coords[gone], tsdf[gone]))
    assert sum(removed.values()) > 0 and sum(cleaned.values()) > sum(removed.values())
    assert original == cleaned + removed


def pieces_scene(first, second):
    """instance 5 of class 3 in two separated blocks of first / second rows (the second block comes first in the rows) and
    a speck of 2 rows, plus one block of another instance"""
    a, b = block((0, 0, 0), (5, 3, 2))[:first], block((10, 0, 0), (5, 3, 2))[:second]
    speck, other = [(0, 10, 0), (0, 11, 0)], block((10, 10, 0), (2, 2, 2))
    coords = np.array(b + a + speck + other, np.int32)
    tsdf = np.random.default_rng(2).uniform(-0.9, 0.9, len(coords)).astype(np.float32)
    sem = np.array([3] * (len(coords) - 8) + [4] * 8, np.int64)
    ins = np.array([5] * (len(coords) - 8) + [6] * 8, np.int64)
    return coords, tsdf, sem, ins, len(b), len(a)


def test_instance_in_pieces(CS):
    coords, tsdf, sem, ins, nb, na = pieces_scene(30, 10)
    speck = slice(nb + na, nb + na + 2)
    got = run_clean(CS, coords, tsdf, sem, ins, min_segment_voxels=3)
    assert np.array_equal(got[0], coords) and np.array_equal(got[1], tsdf)                    # nothing leaves, no TSDF changes
    assert not got[2][speck].any() and not got[3][speck].any()
    assert np.array_equal(np.delete(got[2], speck), np.delete(sem, speck)) and np.array_equal(np.delete(got[3], speck), np.delete(ins, speck))
    assert got[4] == dict(zip(R.REPORT_KEYS, (50, 0, 4, 0, 1, 2, 0)))
    got = run_clean(CS, coords, tsdf, sem, ins, min_segment_voxels=3, split_instances=True)
    assert (got[3][:nb] == 7).all() and (got[3][nb:nb + na] == 5).all() and (got[3][-8:] == 6).all()    # max + 1 = 7
    assert got[4]["instances_split"] == 1 and np.array_equal(got[2], np.where(np.arange(50) // 2 == 20, 0, sem))
    assert_same_as_ref(got, coords, tsdf, sem, ins, min_segment_voxels=3, split_instances=True)
    got = run_clean(CS, coords, tsdf, sem, ins, split_instances=True)                        # the speck is a piece too
    assert (got[3][:nb] == 7).all() and (got[3][nb:nb + na] == 5).all() and (got[3][speck] == 8).all()


def test_equal_pieces_the_smaller_row_keeps_the_id(CS):
    coords, tsdf, sem, ins, nb, na = pieces_scene(10, 10)
    got = run_clean(CS, coords, tsdf, sem, ins, min_segment_voxels=3, split_instances=True)
    assert (got[3][:nb] == 5).all() and (got[3][nb:nb + na] == 7).all()
    assert_same_as_ref(got, coords, tsdf, sem, ins, min_segment_voxels=3, split_instances=True)


def random_scene(seed):
    rng = np.random.default_rng(seed)
    coords = np.argwhere(rng.random((10, 10, 10)) < 0.2).astype(np.int32)
    coords = coords[rng.permutation(len(coords))]
    n = len(coords)
    tsdf = rng.uniform(-1.0, 1.3, n).astype(np.float32)                    # about a fifth of the rows are no geometry
    tsdf[::9] = 1.0
    return coords, tsdf, rng.integers(0, 3, n), rng.integers(0, 3, n)


@pytest.mark.parametrize("seed", range(5))
def test_random_scenes_with_all_options(CS, seed):
    scene = random_scene(seed)
    rule = dict(ALL_ON, connectivity=(6, 18, 26)[seed % 3])
    got = run_clean(CS, *scene, **rule)
    assert_same_as_ref(got, *scene, **rule)
    assert got[4]["rows_removed"] > 0 and got[4]["rows_cleared"] > 0 and got[4]["instances_split"] > 0
    rule = dict(rule, keep_largest=2)
    assert_same_as_ref(run_clean(CS, *scene, **rule), *scene, **rule)
    # idempotence: a cleaned scene comes back as it is
    again = run_clean(CS, *got[:4], **dict(ALL_ON, connectivity=rule["connectivity"]))
    for a, b in zip(again[:4], got[:4]):
        assert np.array_equal(a, b)
    assert again[4] == dict(dict.fromkeys(R.REPORT_KEYS, 0), rows_in=len(got[0]), components=again[4]["components"])


# ----------------------------------------------------------------------------------------------------- files and drivers

def labelled_scene():
    """the plate (floor, stuff class 2) and blobs (class 3 instance 1, 2, 2, 4: the 1-row and the 7-row blob share an id)
    as dense volumes float32 / int64 / int64, as SaveScene writes them"""
    tsdf, sem, ins = np.ones(DIMS, np.float32), np.zeros(DIMS, np.int64), np.zeros(DIMS, np.int64)
    rng = np.random.default_rng(4)
    for cells, s, i in ((PLATE, 2, 0), (BLOB8, 3, 1), (BLOB1, 3, 2), (BLOB7, 3, 2), (BLOB27, 3, 4)):
        c = np.array(cells)
        tsdf[c[:, 0], c[:, 1], c[:, 2]] = rng.uniform(-0.9, 0.9, len(c)).astype(np.float32)
        sem[c[:, 0], c[:, 1], c[:, 2]], ins[c[:, 0], c[:, 1], c[:, 2]] = s, i
    sem[22, 22, 10] = 5                                                    # a labelled cell without geometry: kept as it is
    return tsdf, sem, ins


def write_both_forms(root):
    tsdf, sem, ins = labelled_scene()
    os.makedirs(root, exist_ok=True)
    origin, vs = np.array([-1.0, 0.5, 0.25], np.float32), 0.04
    dense, sparse = os.path.join(root, "dense.npz"), os.path.join(root, "sparse.npz")
    np.savez_compressed(dense, origin=origin, voxel_size=vs, tsdf=tsdf, semantic=sem, instance=ins)
    rows = np.argwhere((tsdf != 1) | (sem != 0) | (ins != 0))
    rows = rows[np.random.default_rng(8).permutation(len(rows))]
    at = tuple(rows.T)
    np.savez_compressed(sparse, origin=origin, voxel_size=vs, dims=np.array(DIMS), sparse_coords=rows.astype(np.int32),
                        sparse_tsdf=tsdf[at], sparse_semantic=sem[at].astype(np.int32), sparse_instance=ins[at].astype(np.int32))
    return dense, sparse


FILE_RULE = dict(min_voxels=2, min_segment_voxels=2, split_instances=True)


def test_dense_and_sparse_files_clean_to_the_same_scene(CS, tmp_path):
    from eprecon_amd.save_scene import load_scene_npz
    dense, sparse = write_both_forms(str(tmp_path))
    out_d, out_s = str(tmp_path / "out" / "dense.npz"), str(tmp_path / "out" / "sparse.npz")
    rep_d, rep_s = CS.clean_scene(dense, out_d, **FILE_RULE), CS.clean_scene(sparse, out_s, **FILE_RULE)
    assert {k: v for k, v in rep_d.items() if k != "path"} == {k: v for k, v in rep_s.items() if k != "path"}
    assert rep_d["rows_removed"] == 1 and rep_d["instances_split"] == 0 and rep_d["path"] == out_d and os.path.exists(out_d)
    with np.load(dense) as before, np.load(out_d) as after:               # the same keys and dtypes
        assert sorted(before.files) == sorted(after.files)
        assert all(before[k].dtype == after[k].dtype and before[k].shape == after[k].shape for k in before.files)
        assert np.array_equal(before["origin"], after["origin"]) and float(before["voxel_size"]) == float(after["voxel_size"])
    with np.load(sparse) as before, np.load(out_s) as after:
        assert sorted(before.files) == sorted(after.files) and len(after["sparse_tsdf"]) == len(before["sparse_tsdf"]) - 1
        assert all(before[k].dtype == after[k].dtype for k in before.files)
        pos = {tuple(r): n for n, r in enumerate(before["sparse_coords"].tolist())}
        order = [pos[tuple(r)] for r in after["sparse_coords"].tolist()]
        assert order == sorted(order)                                     # the kept rows in the file's order
    a, b = load_scene_npz(out_d), load_scene_npz(out_s)
    for k in ("tsdf", "semantic", "instance"):
        assert np.array_equal(a[k], b[k]), k
    tsdf, sem, ins = labelled_scene()
    assert a["tsdf"][2, 2, 6] == 1 and a["semantic"][2, 2, 6] == 0 and a["instance"][2, 2, 6] == 0     # the 1-row blob is gone
    tsdf[2, 2, 6], sem[2, 2, 6], ins[2, 2, 6] = 1, 0, 0
    sem[22, 22, 10] = 0                                                   # a 1-row segment: cleared
    assert np.array_equal(a["tsdf"], tsdf) and np.array_equal(a["semantic"], sem) and np.array_equal(a["instance"], ins)


def test_cleaned_files_are_read_by_the_mesh_and_the_scorer(CS, tmp_path):
    from eprecon_amd import panoptic_score as PS
    from eprecon_amd import render
    from eprecon_amd.save_scene import load_scene_npz
    dense, sparse = write_both_forms(str(tmp_path))
    outs = [CS.clean_scene(src, str(tmp_path / "out" / os.path.basename(src)), **FILE_RULE)["path"] for src in (dense, sparse)]
    meshes = [render.scene_mesh(p) for p in outs]
    assert meshes[0][0].shape[0] > 1000 and meshes[0][1].shape[0] > 1000
    assert all(torch.equal(x, y) for x, y in zip(*meshes))
    # the voxel-domain scorer, against the cleaned scene itself as ground truth: every segment found again
    scene = load_scene_npz(outs[0])
    gt = str(tmp_path / "gt" / "s0")
    os.makedirs(gt)
    with open(os.path.join(gt, "tsdf_info.pkl"), "wb") as fh:
        pickle.dump({"vol_origin": scene["origin"], "voxel_size": float(scene["voxel_size"])}, fh)
    for name, vol in (("full_tsdf_layer0", scene["tsdf"]), ("full_semantic_layer_interpolate0", scene["semantic"]),
                      ("full_instance_layer_interpolate0", scene["instance"])):
        np.savez_compressed(os.path.join(gt, name), vol)
    tables = [PS.score_voxels(p, gt) for p in outs]
    assert (tables[0].counts == tables[1].counts).all()
    assert tables[0].tp.sum() == 4 and tables[0].fp.sum() == 0 and tables[0].fn.sum() == 0


def test_the_three_layouts_are_one_scene_on_the_device(CS, tmp_path):
    """tests/scene_io_cases.py's 12 x 10 x 8 scene: every layout gives the same device volumes and the same mesh; the legacy
    rows are read by the mesh and refused by clean_scene"""
    import scene_io_cases as SC
    from eprecon_amd import render, scene_io
    paths = SC.write_layouts(str(tmp_path))
    truth = SC.volumes()
    vols = {k: scene_io.scene_volumes(p, DEV) for k, p in paths.items()}
    meshes = {k: render.scene_mesh(p) for k, p in paths.items()}
    for layout in paths:
        *got, origin, voxel_size = vols[layout]
        assert np.array_equal(origin, SC.ORIGIN) and voxel_size == SC.VOXEL
        for vol, want in zip(got, truth):
            assert vol.device.type == "cuda" and vol.dtype == torch.from_numpy(want).dtype, layout
            assert np.array_equal(vol.cpu().numpy(), want), layout
        assert all(torch.equal(x, y) for x, y in zip(meshes[layout], meshes["dense"])), layout
    verts, faces, vsem, vins = meshes["dense"]
    assert verts.shape[0] > 50 and faces.shape[0] > 50 and vsem.shape == vins.shape == (verts.shape[0],)
    with pytest.raises(ValueError, match="neither the dense nor the sparse form"):
        CS.clean_scene(paths["legacy"], str(tmp_path / "out" / "legacy.npz"))
    assert not os.path.exists(tmp_path / "out" / "legacy.npz")
    outs = [CS.clean_scene(paths[k], str(tmp_path / "out" / (k + ".npz")), min_voxels=2)["path"] for k in ("dense", "sparse")]
    a, b = (scene_io.scene_volumes(p, DEV)[:3] for p in outs)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], vols["dense"][0])


def test_command_line(CS, tmp_path, capsys):
    dense, _ = write_both_forms(str(tmp_path / "pred"))
    os.rename(dense, str(tmp_path / "pred" / "scene0001_00.npz"))
    scenes = tmp_path / "scenes.txt"
    scenes.write_text("scene0001_00\n")
    out = tmp_path / "clean"
    assert CS.main(["--pred", str(tmp_path / "pred"), "--scenes", str(scenes), "--out", str(out), "--min_voxels", "8",
                    "--min_segment_voxels", "2", "--split_instances", "--connectivity", "18", "--mesh"]) == 0
    assert sorted(os.listdir(out)) == ["mesh_instance_scene0001_00.ply", "mesh_semantic_scene0001_00.ply", "scene0001_00.npz",
                                       "scene0001_00.ply"]
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith("scene0001_00: 1244 rows, 8 removed with 2 of 5 components; 1 rows cleared in 1 segment")
    from eprecon_amd.evaluation import read_ply
    verts, faces = read_ply(str(out / "scene0001_00.ply"))
    assert len(verts) > 1000 and len(faces) > 1000
    CS.main(["--pred", str(tmp_path / "pred"), "--scenes", str(scenes), "--out", str(tmp_path / "plain")])
    assert os.listdir(tmp_path / "plain") == ["scene0001_00.npz"]
    with np.load(str(tmp_path / "pred" / "scene0001_00.npz")) as a, np.load(str(tmp_path / "plain" / "scene0001_00.npz")) as b:
        assert all(np.array_equal(a[k], b[k]) for k in a.files)           # no option: nothing changes


def test_reconstruct_clean_writes_beside_the_saved_scene(tmp_path, capsys):
    """--clean writes clean/<scene>.npz and the three meshes; the scene file itself is byte for byte what a run without
    the flag writes"""
    pytest.importorskip("PIL")
    from test_reconstruct_gpu import HEIGHT, SCENE, WIDTH, write_scene
    from eprecon_amd import reconstruct
    from eprecon_amd.save_scene import load_scene_npz
    root = str(tmp_path / "data")
    write_scene(root)
    files = {}
    for name, extra in (("plain", []), ("clean", ["--clean", "20", "--clean_segments", "5"])):
        out = str(tmp_path / name)
        assert reconstruct.main(["--data_path", root, "--out", out, "--size", str(WIDTH), str(HEIGHT)] + extra) == 0
        files[name] = os.path.join(out, "scene_scannet_fusion_eval_0")
        with open(os.path.join(files[name], SCENE + ".npz"), "rb") as fh:
            files[name + "_bytes"] = fh.read()
    assert files["plain_bytes"] == files["clean_bytes"]
    assert not os.path.exists(os.path.join(files["plain"], "clean"))
    assert sorted(os.listdir(os.path.join(files["clean"], "clean"))) == sorted(
        [SCENE + ".npz", SCENE + ".ply", "mesh_semantic_" + SCENE + ".ply", "mesh_instance_" + SCENE + ".ply"])
    log = capsys.readouterr().out
    assert log.count(" instances split -> ") == 1 and f"clean/{SCENE}.npz" in log.replace(os.sep, "/")
    before = load_scene_npz(os.path.join(files["clean"], SCENE + ".npz"))
    after = load_scene_npz(os.path.join(files["clean"], "clean", SCENE + ".npz"))
    coords = np.argwhere(before["tsdf"] < 1)
    label = R.components_ref(coords, None, 26)
    small = np.bincount(label, minlength=len(label))[label] < 20
    want = before["tsdf"].copy()
    want[tuple(coords[small].T)] = 1
    assert np.array_equal(after["tsdf"], want)


# --------------------------------------------------------------------------------------------------------------- scoring

def test_clean_up_closes_the_panoptic_gap(CS):
    """the prediction is the ground truth plus four spurious 2-voxel chairs inside the floor and one table id shared by two
    separated tables: before, the specks are false positives and the shared id matches at most one table; after, every
    thing is matched with IoU 1.  (The floor keeps the holes the specks leave, so its own IoU stays below 1: the figures
    asserted are those of the things.)"""
    from eprecon_amd import panoptic_score as PS
    floor = [(x, y, 0) for x in range(16) for y in range(16)]
    tables = block((1, 1, 2), (3, 3, 2)), block((9, 9, 2), (2, 2, 2))            # 18 and 8 rows, class 7
    chair = block((1, 9, 2), (2, 2, 3))                                          # 12 rows, class 5
    coords = np.array(floor + tables[0] + tables[1] + chair, np.int32)
    n = len(coords)
    gt_sem = np.array([2] * 256 + [7] * 26 + [5] * 12, np.int64)
    gt_ins = np.array([0] * 256 + [1] * 18 + [2] * 8 + [3] * 12, np.int64)
    sem, ins = gt_sem.copy(), gt_ins.copy()
    ins[256 + 18:256 + 26] = 1                                                   # the second table carries the first's id
    for k, (x, y) in enumerate(((3, 12), (12, 3), (6, 6), (13, 13))):            # specks: (x, y, 0) and (x + 1, y, 0)
        for row in (16 * x + y, 16 * (x + 1) + y):
            sem[row], ins[row] = 5, 10 + k
    tsdf = np.random.default_rng(6).uniform(-0.9, 0.9, n).astype(np.float32)
    score = lambda s, i: PS.PanopticScore().add(PS.score_sites(dev(s, torch.int64), dev(i, torch.int64), dev(gt_sem, torch.int64),
                                                               dev(gt_ins, torch.int64))).summary()
    before = score(sem, ins)
    assert before["things"]["rq"] < 1 and before["classes"]["5"]["fp"] == 4 and before["classes"]["7"]["fn"] == 1
    c, t, s, i, report = run_clean(CS, coords, tsdf, sem, ins, min_segment_voxels=3, split_instances=True)
    assert np.array_equal(c, coords) and report["rows_cleared"] == 8 and report["instances_split"] == 1
    after = score(s, i)
    assert (after["things"]["pq"], after["things"]["sq"], after["things"]["rq"]) == (1.0, 1.0, 1.0)
    assert after["all"]["rq"] == 1.0 and after["stuff"]["rq"] == 1.0
    assert sum(r["fp"] + r["fn"] for r in after["classes"].values()) == 0

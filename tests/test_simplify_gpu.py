"""GPU: mesh simplification (eprecon_amd/simplify.py, csrc/mesh_simplify.hip) against the restatement of
tests/simplify_ref.py.

Exact (np.array_equal): the cluster ids, the surviving faces and their order, which clusters are written, the labels, the
colours, the integers of the report.  The cell of a vertex is one fp64 expression rounded as numpy rounds it, the colour an
integer expression, everything else follows from the ids.

Positions, as float64, within 1e-6 cell.  Derivation: a cluster's A, b and mean are sums of n terms; each term is a handful
of fp64 operations on the same inputs in both implementations (relative error at most 4 * 2^-53 a term), and the two sums
differ in the association of the products inside a term, not in their order, so every entry differs by at most
4 n 2^-53 times the sum of the magnitudes, which the trace bounds.  The system (A + lambda I) x = b + lambda m has the
condition number (trace + lambda) / lambda <= 1 + 3 / regularize, and all of x*, m lie within a few cells of the centre, so
the two minimisers differ by at most (1 + 3 / regularize) 4 n 2^-53 cell up to a small factor: 1.3e-8 cell for n = 10^4
corner entries and regularize = 1e-3.  The clip is 1-Lipschitz along the segment away from the fragile set (the restatement's
`fragile` mark: asserted empty on every fixture here, so no cluster is left out).  1e-6 cell is about 100 times that bound.

Normals: the face normal is computed from the float32 vertices as they are, by the same fp64 expression in the same order,
and the sum runs in the same order, so the sums agree to the bit: exact zero where the restatement's is zero, else within 4
float32 ulps of 1 (the normalisation and the cast)."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import simplify_cases as C
import simplify_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
FANS = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
ORIGIN = (0.3, 0.7, 0.1)          # no multiple of any cell size used below
INTS = ("vertices_in", "faces_in", "clusters", "vertices_out", "faces_out", "faces_degenerate", "faces_duplicate")


@pytest.fixture(scope="module")
def S():
    from eprecon_amd import simplify
    return simplify


def run(S, verts, faces, cell, semantic=None, instance=None, colors=None, origin=None, regularize=1e-3):
    dev = lambda a, dtype: None if a is None else torch.as_tensor(np.array(a)).to(dtype).to(DEV)
    out = S.simplify_device(dev(np.asarray(verts, np.float32).reshape(-1, 3), torch.float32), dev(np.asarray(faces).reshape(-1, 3), torch.int32),
                            cell, dev(semantic, torch.int32), dev(instance, torch.int32), dev(colors, torch.uint8), origin, regularize)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def compare(got, want, cell):
    assert not want["fragile"].any()
    assert np.array_equal(got["cluster"], want["cluster"])
    assert np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["faces"], want["faces"])
    assert got["faces"].shape == want["faces"].shape and got["faces"].dtype == np.int32
    assert np.array_equal(got["written"], want["written"])
    for k in ("cluster_semantic", "cluster_instance", "rgb"):
        assert (got[k] is None) == (want[k] is None)
        if want[k] is not None:
            assert np.array_equal(got[k], want[k]), k
    assert [got["report"][k] for k in INTS] == [want["report"][k] for k in INTS]
    k = want["positions"].shape[0]
    assert got["positions"].dtype == np.float64 and got["positions"].shape == (k, 3)
    err = float(np.abs(got["positions"] - want["positions"]).max()) if k else 0.0
    print(f"positions: {k} clusters, largest difference {err / cell:.3g} cell")
    assert err <= 1e-6 * cell
    assert abs(got["report"]["max_shift"] - want["report"]["max_shift"]) <= 2e-6 * cell
    zero = (want["normals"] == 0).all(1)
    assert (got["normals"][zero] == 0).all()
    assert np.abs(got["normals"].astype(np.float64) - want["normals"].astype(np.float64)).max(initial=0.0) <= 4 * 2.0 ** -23
    assert np.array_equal(got["vertices"], got["positions"][got["written"]].astype(np.float32))
    properties(got, want, cell)


def properties(got, want, cell):
    """every position in the closed box of its cell (the box's faces are computed in fp64: a rounding of the coordinate's
    magnitude is allowed); the largest shift at most sqrt(3) cell; three distinct indices a face; no unordered triple twice"""
    lo = want["cells"] * cell + np.asarray(want.get("origin", (0, 0, 0)), np.float64)
    slack = 4 * np.spacing(np.abs(lo).max(initial=0.0) + cell)
    assert (got["positions"] >= lo - slack).all() and (got["positions"] <= lo + cell + slack).all()
    assert got["report"]["max_shift"] <= math.sqrt(3) * cell * (1 + 1e-12)
    f = np.sort(got["faces"], 1)
    assert ((f[:, 0] < f[:, 1]) & (f[:, 1] < f[:, 2])).all()
    assert len(np.unique(f, axis=0)) == len(f)
    assert f.min(initial=0) >= 0 and f.max(initial=-1) < got["report"]["vertices_out"]
    assert len(np.unique(got["faces"])) == got["report"]["vertices_out"]      # every written vertex is used


def reference(verts, faces, cell, **kw):
    want = R.simplify(verts, faces, cell, **kw)
    want["origin"] = kw.get("origin") if kw.get("origin") is not None else (0, 0, 0)
    return want


# ---------------------------------------------------------------------------------------------------------------- fans

@functools.lru_cache(maxsize=None)
def fan_case(triangles, collapse):
    verts, faces = C.fan(triangles, collapse)
    return verts, faces, reference(verts, faces, 1.0)


@pytest.mark.parametrize("triangles", FANS)
def test_fan_with_the_hub_alone_in_its_cell(S, triangles):
    verts, faces, want = fan_case(triangles, False)
    got = run(S, verts, faces, 1.0)
    compare(got, want, 1.0)
    assert (got["cluster"] == got["cluster"][0]).sum() == 1


@pytest.mark.parametrize("triangles", FANS)
def test_fan_with_the_rim_in_one_cell_collapses(S, triangles):
    verts, faces, want = fan_case(triangles, True)
    got = run(S, verts, faces, 1.0)
    compare(got, want, 1.0)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["report"]["faces_degenerate"] == triangles


def test_meshes_of_zero_one_and_two_faces(S):
    verts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]], np.float32)
    for faces in ([], [[0, 1, 2]], [[0, 1, 2], [0, 3, 1]]):
        faces = np.array(faces, np.int32).reshape(-1, 3)
        compare(run(S, verts, faces, 1.0), reference(verts, faces, 1.0), 1.0)
    none = run(S, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert none["report"]["clusters"] == 0 and none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3)
    assert none["report"]["max_shift"] == 0.0


def test_zero_area_faces_among_good_ones(S):
    """faces with a repeated corner and a face of three collinear points (dyadic: |n| = 0 exactly) in three cells of their own:
    they count as faces, add nothing to any quadric, and the clusters that have no other face keep their mean and a zero normal"""
    verts, faces = C.fan(12)
    n = len(verts)
    verts = np.concatenate([verts, np.array([[2.5, 2.5, 2.5], [3.5, 3.5, 3.5], [4.5, 4.5, 4.5]], np.float32)])
    extra = np.array([[0, 0, 5], [0, 3, 3], [4, 4, 4], [n, n + 1, n + 2]], np.int32)
    faces = np.concatenate([faces[:5], extra, faces[5:]]).astype(np.int32)
    want = reference(verts, faces, 1.0)
    got = run(S, verts, faces, 1.0)
    compare(got, want, 1.0)
    lone = got["cluster"][n:]
    assert (got["normals"][lone] == 0).all() and got["written"][lone].all()
    assert np.array_equal(got["positions"][lone], verts[n:].astype(np.float64))
    assert got["report"]["faces_degenerate"] == want["report"]["faces_degenerate"] >= 3


def test_all_negative_coordinates_floor(S):
    verts, faces = C.fan(40)
    verts = (verts - np.float32(7.25)).astype(np.float32)
    want = reference(verts, faces, 1.0)
    assert want["cells"].max() < 0
    compare(run(S, verts, faces, 1.0), want, 1.0)


def test_two_labels_in_one_cell_give_two_clusters(S):
    verts = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]], np.float32)
    faces, sem, ins = [[0, 2, 3], [1, 2, 3]], [3, 1, 0, 0], [0, 0, -2, 5]
    want = reference(verts, faces, 1.0, semantic=sem, instance=ins)
    got = run(S, verts, faces, 1.0, semantic=sem, instance=ins)
    compare(got, want, 1.0)
    assert got["report"]["clusters"] == 4 and got["cluster"].tolist() == [1, 0, 3, 2]
    assert got["cluster_semantic"].tolist() == [1, 3, 0, 0] and got["cluster_instance"].tolist() == [0, 0, 5, -2]
    one = run(S, verts, faces, 1.0)
    assert one["report"]["clusters"] == 3 and one["report"]["faces_duplicate"] == 1


def test_the_dyadic_lattice(S):
    verts, faces = C.dyadic_lattice()
    want = reference(verts, faces, 0.25)
    got = run(S, verts, faces, 0.25)
    compare(got, want, 0.25)
    on_face = np.flatnonzero(verts[:, 0] == 0.25)
    assert (want["cells"][got["cluster"][on_face], 0] == 1).all()
    shifted = reference(verts, faces, 0.25, origin=(0.0625, -0.125, 0.03125))
    compare(run(S, verts, faces, 0.25, origin=(0.0625, -0.125, 0.03125)), shifted, 0.25)


def test_the_ridge_and_a_flat_patch(S):
    verts, faces = C.dihedral()
    origin = (-0.5, -0.5, -0.5)
    want = reference(verts, faces, 1.0, origin=origin)
    got = run(S, verts, faces, 1.0, origin=origin)
    compare(got, want, 1.0)
    k = int(np.flatnonzero((want["cells"] == 0).all(1))[0])
    assert np.abs(got["positions"][k] - [0, 0, 0.3]).max() < 2e-3
    s = 0.0625 + 0.3125 * np.arange(10)
    verts, faces = C.grid(s, s, lambda x, y: 0.25 + 0.25 * x - 0.125 * y)
    want = reference(verts, faces, 1.0)
    got = run(S, verts, faces, 1.0)
    compare(got, want, 1.0)
    assert np.abs(got["positions"] - want["means"]).max() < 1e-12


# ---------------------------------------------------------------------------------------------------- marching cubes

def _axes(n):
    return np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")


def _rotation():
    a, b = 0.5, 0.3
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return rz @ rx


@functools.lru_cache(maxsize=None)
def mc_mesh(which):
    """marching cubes of a 24^3 volume -> (verts in voxel units, faces, semantic, instance, colours), host arrays, read-only"""
    from eprecon_amd.save_scene import marching_cubes
    x, y, z = _axes(24)
    p = np.stack([x - 11.3, y - 11.7, z - 12.1], -1)
    if which == "sphere":
        vol = np.linalg.norm(p, axis=-1) - 6.3
    elif which == "box":
        vol = (np.abs(p @ _rotation()) - np.array([5.2, 4.1, 3.3])).max(-1)
    else:
        vol = p @ PLANE_N
    verts, faces, _ = marching_cubes(torch.from_numpy(vol.astype(np.float32)).to(DEV), 0.0)
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    sem, ins = C.block_labels(verts, seed=len(which), block=4.0)
    out = (verts, faces, sem, ins, C.seeded_colors(len(verts), seed=3))
    for a in out:
        a.setflags(write=False)
    return out


PLANE_N = np.array([0.48, -0.6, 0.64])      # a unit vector: 0.2304 + 0.36 + 0.4096 = 1


@functools.lru_cache(maxsize=None)
def mc_reference(which, cell, labelled):
    verts, faces, sem, ins, colors = mc_mesh(which)
    kw = dict(semantic=sem, instance=ins, colors=colors) if labelled else {}
    return reference(verts, faces, cell, origin=ORIGIN, **kw)


@pytest.mark.parametrize("labelled", [False, True])
@pytest.mark.parametrize("cell", [1.5, 2.0, 3.7])
@pytest.mark.parametrize("which", ["sphere", "box"])
def test_marching_cubes_meshes(S, which, cell, labelled):
    verts, faces, sem, ins, colors = mc_mesh(which)
    assert len(verts) > 500 and len(faces) > 1000
    want = mc_reference(which, cell, labelled)
    kw = dict(semantic=sem, instance=ins, colors=colors) if labelled else {}
    got = run(S, verts, faces, cell, origin=ORIGIN, **kw)
    compare(got, want, cell)
    assert 0 < got["report"]["vertices_out"] < len(verts) and 0 < got["report"]["faces_out"] < len(faces)
    if labelled:
        plain = mc_reference(which, cell, False)
        assert got["report"]["clusters"] > plain["report"]["clusters"]      # the labels split cells


def test_a_tilted_plane_stays_a_plane(S):
    """Marching cubes of the linear volume n . (p - c), |n| = 1.  With ulp = 2^-19 (float32 between 16 and 32): the volume's
    samples are rounded to float32 (at most ulp / 2 each, which moves a crossing by as much in distance from the plane), and
    the one coordinate of a vertex that is no integer is rounded once (ulp / 2 times a component of n): the input lies within
    2 ulp of the plane.  Every face plane passes within that distance of three points of the true plane, the mean of a
    cluster lies within it too, and the regularised minimiser lies between the face planes and the mean; a sliver tilts its
    plane more, but weighs in by its area.  The output is rounded to float32 once more.  Allowed: 16 ulp = 3.1e-5 voxels."""
    verts, faces, *_ = mc_mesh("plane")
    assert len(verts) > 500
    ulp = 2.0 ** -19
    dist = lambda v: np.abs((np.asarray(v, np.float64) - [11.3, 11.7, 12.1]) @ PLANE_N)
    assert dist(verts).max() <= 2 * ulp
    for cell in (2.0, 3.7):
        got = run(S, verts, faces, cell, origin=ORIGIN)
        print(f"cell {cell}: input off the plane by {dist(verts).max() / ulp:.2f} ulp, output by {dist(got['vertices']).max() / ulp:.2f} ulp")
        assert got["report"]["vertices_out"] > 20
        assert dist(got["vertices"]).max() <= 16 * ulp
    want = mc_reference("plane", 2.0, False)
    compare(run(S, verts, faces, 2.0, origin=ORIGIN), want, 2.0)


def test_two_runs_give_the_same_bits(S):
    verts, faces, sem, ins, colors = mc_mesh("box")
    a = run(S, verts, faces, 2.0, semantic=sem, instance=ins, colors=colors, origin=ORIGIN)
    b = run(S, verts, faces, 2.0, semantic=sem, instance=ins, colors=colors, origin=ORIGIN)
    for k in ("positions", "normals", "vertices", "faces", "rgb", "cluster", "kept"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["report"] == b["report"]


# -------------------------------------------------------------------------------------------------------------- errors

@pytest.mark.parametrize("bad", [4, -1])
def test_a_face_index_out_of_range(S, bad):
    verts, faces = C.fan(3)
    faces = faces.copy()
    faces[1, 2] = bad if bad < 0 else len(verts)
    with pytest.raises(ValueError, match="face index"):
        run(S, verts, faces, 1.0)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_vertex_that_is_not_finite(S, value):
    verts, faces = C.fan(3)
    verts = verts.copy()
    verts[2, 1] = value
    with pytest.raises(ValueError, match="not finite"):
        run(S, verts, faces, 1.0)


def test_a_cell_the_key_cannot_hold(S):
    verts, faces = C.fan(3)
    with pytest.raises(ValueError, match="key"):
        run(S, verts, faces, 1e-6)          # 2.5 / 1e-6 > 2^20
    assert run(S, verts, faces, 2.5 / 2 ** 20 * 1.01)["report"]["clusters"] == 5


def test_cpu_tensors_are_refused(S):
    from eprecon_amd._lib import EpreconError
    verts, faces = C.fan(3)
    with pytest.raises(EpreconError):
        S.simplify_device(torch.from_numpy(verts), torch.from_numpy(faces), 1.0)
    with pytest.raises(EpreconError):
        S.simplify_device(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces), 1.0)


def test_arguments(S):
    verts, faces = C.fan(3)
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=1.0, regularize=0.0), dict(cell=float("nan"))):
        with pytest.raises(ValueError):
            run(S, verts, faces, **kw)


# ------------------------------------------------------------------------------------------------------------- drivers

VS, SCENE_ORIGIN = 0.04, (-1.5, 0.25, 0.125)


def small_scene():
    x, y, z = _axes(14)
    tsdf = np.clip((np.sqrt((x - 6.4) ** 2 + (y - 6.7) ** 2 + (z - 7.1) ** 2) - 4.2) / 3.0, -1, 1).astype(np.float32)
    sem = (1 + (x > 6) + 2 * (y > 7)).astype(np.int32)
    ins = (1 + (z > 6)).astype(np.int32)
    sem[tsdf == 1], ins[tsdf == 1] = 0, 0
    return tsdf, sem, ins


def write_both_forms(SIO, root):
    tsdf, sem, ins = small_scene()
    head = dict(origin=np.asarray(SCENE_ORIGIN, np.float32), voxel_size=VS)
    dense, sparse = os.path.join(root, "dense", "s0.npz"), os.path.join(root, "sparse", "s0.npz")
    os.makedirs(os.path.dirname(dense)), os.makedirs(os.path.dirname(sparse))
    SIO.write_scene(dense, tsdf, sem, ins, **head)
    rows = np.argwhere((tsdf != 1) | (sem != 0) | (ins != 0))
    rows = rows[np.random.default_rng(0).permutation(len(rows))]
    at = tuple(rows.T)
    SIO.write_scene(sparse, tsdf[at], sem[at], ins[at], coords=rows.astype(np.int32), dims=np.array(tsdf.shape), **head)
    return dense, sparse


LOD_FILES = ["mesh_instance_s0_lod.ply", "mesh_semantic_s0_lod.ply", "s0_lod.ply"]


def test_dense_and_sparse_files_give_identical_meshes(S, tmp_path):
    from eprecon_amd import scene_io as SIO
    from eprecon_amd.save_scene import tsdf_panoptic2mesh
    dense, sparse = write_both_forms(SIO, str(tmp_path))
    ra = S.simplify_scene(dense, str(tmp_path / "a"), 2 * VS)
    rb = S.simplify_scene(sparse, str(tmp_path / "b"), 2 * VS)
    assert ra == rb and len(ra) == 3
    assert sorted(os.listdir(tmp_path / "a")) == LOD_FILES == sorted(os.listdir(tmp_path / "b"))
    for name in LOD_FILES:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # the files hold what the restatement makes of the scene's meshes
    tsdf, sem, ins = (torch.from_numpy(a).to(DEV) for a in small_scene())
    meshes = tsdf_panoptic2mesh(VS, torch.tensor(SCENE_ORIGIN, dtype=torch.float32, device=DEV), tsdf, sem, ins)
    for mesh, name, label in zip(meshes, ("s0_lod.ply", "mesh_semantic_s0_lod.ply", "mesh_instance_s0_lod.ply"),
                                 (None, "vertex_semantic", "vertex_instance")):
        kw = {} if label is None else {label[7:]: mesh[label], "colors": mesh["vertex_colors"]}
        want = R.simplify(mesh["vertices"], mesh["faces"], 2 * VS, **kw)
        verts, faces = SIO.read_ply(str(tmp_path / "a" / name))
        assert np.array_equal(faces, want["faces"]) and len(faces) > 20
        assert np.abs(verts - want["vertices"]).max() <= 1e-6 * 2 * VS + np.spacing(np.float32(2.0))
    assert ra[1]["clusters"] > ra[0]["clusters"] and ra[0]["faces_out"] < ra[0]["faces_in"]


def test_command_line_on_ply_files_and_scenes(S, tmp_path, capsys):
    from eprecon_amd import scene_io as SIO
    dense, _ = write_both_forms(SIO, str(tmp_path))
    verts, faces, *_ = mc_mesh("sphere")
    normals = np.zeros_like(verts)
    SIO.export_ply({"vertices": verts, "faces": faces, "vertex_normals": normals}, str(tmp_path / "ball.ply"))
    (tmp_path / "scenes.txt").write_text("s0\n")
    out = tmp_path / "lod"
    assert S.main(["--out", str(out), "--cell", "2.0", "--ply", str(tmp_path / "ball.ply")]) == 0
    assert os.listdir(out) == ["ball_lod.ply"]
    got_v, got_f = SIO.read_ply(str(out / "ball_lod.ply"))
    want = R.simplify(verts, faces, 2.0)
    assert np.array_equal(got_f, want["faces"]) and np.abs(got_v - want["vertices"]).max() <= 4e-6
    assert "ball: " in capsys.readouterr().out
    assert S.main(["--pred", os.path.dirname(dense), "--scenes", str(tmp_path / "scenes.txt"), "--out", str(out), "--cell", str(2 * VS),
                   "--regularize", "1e-2"]) == 0
    assert sorted(os.listdir(out)) == sorted(LOD_FILES + ["ball_lod.ply"])
    assert "s0: " in capsys.readouterr().out
    with pytest.raises(SystemExit):
        S.main(["--out", str(out), "--cell", "1.0"])


def test_reconstruct_writes_the_meshes_beside_the_scene(S, tmp_path, capsys):
    from eprecon_amd import reconstruct
    from eprecon_amd import scene_io as SIO
    tsdf, sem, ins = small_scene()
    save = tmp_path / "log_fusion_eval_47"
    os.makedirs(save)
    SIO.write_scene(str(save / "scene0000_00.npz"), tsdf, sem, ins, origin=np.asarray(SCENE_ORIGIN, np.float32), voxel_size=VS)
    saver = SimpleNamespace(log_dir=str(tmp_path / "log"))
    reconstruct.simplify_saved_scenes({"scene_name": ["scene0000_00", "scene0000_01"]}, saver, 47, 2 * VS)
    assert sorted(os.listdir(save)) == ["mesh_instance_scene0000_00_lod.ply", "mesh_semantic_scene0000_00_lod.ply", "scene0000_00.npz",
                                        "scene0000_00_lod.ply"]
    S.simplify_scene(str(save / "scene0000_00.npz"), str(tmp_path / "direct"), 2 * VS)
    assert (save / "scene0000_00_lod.ply").read_bytes() == (tmp_path / "direct" / "scene0000_00_lod.ply").read_bytes()
    assert "scene0000_00: " in capsys.readouterr().out
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o"]).simplify is None
    assert reconstruct.parse_args(["--data_path", "d", "--out", "o", "--simplify", "0.08"]).simplify == 0.08

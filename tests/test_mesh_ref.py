"""The float64 mesh witness (tests/mesh_ref.py) checked on the CPU: it agrees with the fp32 oracle where it may, its two
conditions hold on every volume the GPU tests use (tests/test_mesh_extraction_gpu.py reads the same VOLUMES table), the
+-1 volume reaches every sign case that emits triangles, and compare() rejects each way a mesh can be subtly wrong."""
import numpy as np
import pytest

import mesh_ref as M


@pytest.mark.parametrize("name", ["blob", "blob_12x14x10", "gauss"])
def test_witness_agrees_with_the_oracle(name):
    vol = M.volume(name)
    ov, of = M.oracle(vol, 0.0)
    wd = M.winding(vol, 0.0, ov, of)
    assert len(of) > 300 and wd.decided.mean() > 0.995
    assert np.array_equal(wd.faces[wd.decided], of[wd.decided])        # every decided face is wound as the oracle wound it
    # the witness's answer does not depend on the order it is handed
    flipped = M.winding(vol, 0.0, ov, of[:, [0, 2, 1]])
    assert np.array_equal(flipped.faces[wd.decided], of[wd.decided]) and np.array_equal(flipped.decided, wd.decided)
    # the raster walk puts every face into the cell its three vertices lie in (closed cell: upper faces included)
    cell = M.face_cells(vol, 0.0)[:, None, :]
    tri = ov[of]
    assert ((tri >= cell) & (tri <= cell + 1)).all()
    # the walk of the cut edges gives the oracle's vertices: integer coordinates off the edge's axis, a crossing on it
    e = M.vertex_edges(vol, 0.0)
    assert len(e) == len(ov)
    off = np.arange(3)[None, :] != e[:, 3:]
    assert np.array_equal(ov[off], e[:, :3][off].astype(np.float32)) and (np.floor(ov) == e[:, :3]).all()
    # the kernel's formula, every operation rounded to fp32, is well inside the bound
    labels = M.label_volumes(vol.shape)
    r = M.compare(M.emulated(vol, 0.0, labels=labels), vol, 0.0, labels=labels)
    assert r["normal"] < 0.5 and r["winding_differs"] == 0


@pytest.mark.parametrize("name,level", M.CASES)
def test_conditions_hold_on_every_volume_of_the_gpu_tests(name, level, record_property):
    vol = M.volume(name)
    assert vol.shape == M.VOLUMES[name].shape and max(vol.shape) <= 41 and vol.size <= 4096
    loose, undecided, zero = M.conditions(vol, level)
    record_property("bound_above_1e-3", loose)
    record_property("undecided", undecided)
    record_property("zero_gradient_vertices", zero)
    assert len(M.oracle(vol, level)[1]) > 0
    assert loose <= M.BOUND_SHARE
    if not M.VOLUMES[name].exact:
        assert undecided <= M.UNDECIDED_SHARE
    labels = M.label_volumes(vol.shape)
    M.compare(M.emulated(vol, level, labels=labels), vol, level, labels=labels)


def test_sign_volume_reaches_every_case_with_every_vertex_on_a_tie():
    nonempty = set(range(1, 255))
    for name in ("sign", "gauss"):
        assert set(np.unique(M.cell_cases(M.volume(name), 0.0))) - {0, 255} == nonempty, name     # all 254
    # (not every shape does: 9 x 17 x 12 misses one or two of the rarest)
    assert len(set(np.unique(M.cell_cases(M.volume("gauss_9x17x12"), 0.0))) - {0, 255}) >= 250
    vol = M.volume("sign")
    assert set(np.unique(vol)) == {-1.0, 1.0}
    ov, _ = M.oracle(vol, 0.0)
    frac = ov - np.floor(ov)
    assert len(ov) > 5000 and ((frac == 0.5).sum(1) == 1).all() and ((frac == 0).sum(1) == 2).all()
    # a tie rounds to the even neighbour, so the label rule reads the voxel below as often as the one above
    up = np.rint(ov).astype(int)[frac == 0.5] > np.floor(ov).astype(int)[frac == 0.5]
    assert 0.3 < up.mean() < 0.7
    nr = M.normals(vol, 0.0)
    assert 0 < (nr.L == 0).sum() < 0.05 * len(ov) and (nr.n[nr.L == 0] == 0).all()
    # the quantised volume has values on the level: coincident vertices, zero-area faces
    for level in M.VOLUMES["on_level"].levels:
        qv, qf = M.oracle(M.volume("on_level"), level)
        assert (M.volume("on_level") == np.float32(level)).sum() > 50
        tri = qv[qf]
        assert ((tri[:, 0] == tri[:, 1]).all(1) | (tri[:, 0] == tri[:, 2]).all(1) | (tri[:, 1] == tri[:, 2]).all(1)).sum() > 50


def _weight():
    rng = np.random.default_rng(4)
    w = (rng.random((16, 16, 16)) > 0.03).astype(np.float32) * rng.uniform(0.5, 3, (16, 16, 16)).astype(np.float32)
    w[:, :, 11:] = 0
    return w


MUTATIONS = ["winding", "face_index", "vertex_ulp", "normal_swapped", "normal_rotated", "label", "masked_face_back"]


@pytest.mark.parametrize("what", MUTATIONS)
def test_comparison_fails_against_a_perturbed_mesh(what):
    vol, level = M.volume("gauss"), 0.0
    labels = M.label_volumes(vol.shape)
    weight = _weight() if what == "masked_face_back" else None
    good = M.emulated(vol, level, weight, labels)
    M.compare(good, vol, level, weight, labels)
    verts, faces, nrm, la, lb = (a.copy() for a in good)
    nr = M.normals(vol, level)
    if what == "winding":
        f = int(np.flatnonzero(M.winding(vol, level, verts, faces).decided)[len(faces) // 2])
        faces[f, 1], faces[f, 2] = faces[f, 2], faces[f, 1]
    elif what == "face_index":
        faces[len(faces) // 3, 1] += 1
    elif what == "vertex_ulp":
        v, k = np.argwhere(verts != np.floor(verts))[len(verts) // 2]
        verts[v, k] = np.nextafter(verts[v, k], np.float32(np.inf))
    elif what == "normal_swapped":
        v = int(np.argmax(np.abs(nrm[:, 0] - nrm[:, 1]) - 1e3 * nr.bound))
        nrm[v, 0], nrm[v, 1] = nrm[v, 1], nrm[v, 0]
    elif what == "normal_rotated":
        v = int(np.argmin(nr.bound))
        assert nr.bound[v] < 1e-5
        n = nrm[v].astype(np.float64)
        axis = np.cross(n, np.eye(3)[np.argmin(np.abs(n))])
        axis /= np.linalg.norm(axis)
        nrm[v] = (n * np.cos(1e-4) + np.cross(axis, n) * np.sin(1e-4)).astype(np.float32)      # (axis is perpendicular to n)
        assert abs(np.linalg.norm(nrm[v]) - 1) < 1e-6
    elif what == "label":
        lb[len(lb) // 2] += 1
    elif what == "masked_face_back":
        full = M.emulated(vol, level, None, labels)
        keep = M.evaluation_ref.masked_mesh(vol, weight, full[0], full[1], M.table())[2]
        assert 0 < keep.sum() < len(keep)
        keep[np.flatnonzero(~keep)[0]] = True
        verts, faces, nrm, la, lb = M.restrict(full, keep)
        assert len(faces) == len(good[1]) + 1
    with pytest.raises(AssertionError):
        M.compare((verts, faces, nrm, la, lb), vol, level, weight, labels)


def test_undecided_faces_may_be_wound_either_way_but_keep_their_indices():
    """the exact volumes have faces perpendicular to the cell gradient: compare() accepts both windings there, nothing else"""
    vol = M.volume("sign")
    good = M.emulated(vol, 0.0)
    wd = M.winding(vol, 0.0, good[0], good[1])
    f = int(np.flatnonzero(~wd.decided & (wd.d == 0))[0])
    faces = good[1].copy()
    faces[f, 1], faces[f, 2] = faces[f, 2], faces[f, 1]
    assert M.compare((good[0], faces, good[2]), vol, 0.0)["winding_differs"] == 1
    faces[f] = faces[f, [1, 2, 0]]                                   # a rotation moves the first vertex: not the kernel's
    with pytest.raises(AssertionError):
        M.compare((good[0], faces, good[2]), vol, 0.0)

"""Mesh extraction (eprecon_amd/csrc/marching_cubes.hip through save_scene.marching_cubes) against the fp32 oracle and the
float64 witness of tests/mesh_ref.py: every sign case, the normals' direction, the winding, values on the level, other
levels, +-1 plateaus, half-to-even label ties, zero gradients, the smallest volume, point counts around the scan tile,
empty output, the masked form on noise and at the volume border.  The volumes are those of mesh_ref.VOLUMES, whose
conditions tests/test_mesh_ref.py checks on the CPU."""
from collections import Counter

import numpy as np
import pytest

import mesh_ref as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared volumes are read-only)


def run(vol, level, weight=None, labels=()):
    from eprecon_amd import save_scene as SS
    out = SS.marching_cubes(dev(vol), level, labels=tuple(dev(l) for l in labels),
                            weight=None if weight is None else dev(weight))
    return tuple(t.cpu().numpy() for t in out)


def check(got, vol, level, record_property, weight=None, labels=(), exact=False, tag=""):
    r = M.compare(got, vol, level, weight, labels)
    for k in ("normal", "undecided", "winding_differs", "verts", "faces"):
        record_property(f"{tag}{k}", r[k])
    print(f"{tag} level {level}: {r}")
    verts, faces = got[0], got[1]
    if len(faces):                                                   # the output is one consistent indexed mesh
        assert faces.min() >= 0 and faces.max() < len(verts)
    assert len(np.unique(faces)) == len(verts)                       # every vertex is used by a face
    if exact:
        expect = M.oracle(vol, level)[1]
        if weight is not None:
            expect = M.evaluation_ref.masked_mesh(vol, weight, *M.oracle(vol, level), M.table())[1].reshape(-1, 3)
        assert np.array_equal(faces, expect) and r["winding_differs"] == 0
    return r


@pytest.mark.parametrize("name,level", [c for c in M.CASES if c[0] not in M.SHAPES])
def test_every_volume_against_oracle_and_witness(name, level, record_property):
    vol = M.volume(name)
    labels = M.label_volumes(vol.shape)
    got = run(vol, level, labels=labels)
    check(got, vol, level, record_property, labels=labels, exact=M.VOLUMES[name].exact, tag=name)
    # without label volumes: the same mesh, no label outputs
    bare = run(vol, level)
    assert len(bare) == 3 and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(bare, got))


@pytest.mark.parametrize("name", M.SHAPES)
def test_shapes(name, record_property):
    vol = M.volume(name)
    labels = M.label_volumes(vol.shape)
    check(run(vol, 0.0, labels=labels), vol, 0.0, record_property, labels=labels, tag=name)


def test_blob_surfaces_are_closed_and_wound_outwards():
    verts, faces, _ = run(M.volume("blob"), 0.0)                     # (the 12 x 14 x 10 cut opens the blobs at its border)
    directed = Counter((int(p), int(q)) for a, b, c in faces for p, q in ((a, b), (b, c), (c, a)))
    assert len(directed) > 500 and set(directed.values()) == {1}                 # no edge twice in one direction ...
    assert all((q, p) in directed for p, q in directed)                          # ... and each one in both: two faces
    a, b, c = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    assert np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0 > 0


@pytest.mark.parametrize("side", ["above", "below"])
def test_empty_output(side, monkeypatch):
    from eprecon_amd import _lib
    lib = _lib.load()

    def no_launch(*a):
        raise AssertionError("the emit phase was launched for an empty mesh")
    monkeypatch.setattr(lib, "eprecon_marching_cubes_emit_async", no_launch, raising=False)
    monkeypatch.setattr(lib, "eprecon_marching_cubes_emit_masked_async", no_launch, raising=False)
    vol = np.abs(M.volume("gauss")) + np.float32(0.5)
    vol = vol if side == "above" else -vol
    labels = M.label_volumes(vol.shape)
    for weight in (None, np.ones(vol.shape, np.float32)):
        for level in (0.0, 0.25, -0.25):
            verts, faces, normals, la, lb = run(vol, level, weight=weight, labels=labels)
            assert verts.shape == (0, 3) and verts.dtype == np.float32 and normals.shape == (0, 3) and normals.dtype == np.float32
            assert faces.shape == (0, 3) and faces.dtype == np.int32
            assert la.shape == lb.shape == (0,) and la.dtype == lb.dtype == np.int32
    assert M.oracle(vol, 0.0)[0].shape == (0, 3)
    # a volume whose values all EQUAL the level is entirely "not below" it
    verts, faces, normals = run(np.full((5, 4, 3), 0.25, np.float32), 0.25)
    assert verts.shape == faces.shape == normals.shape == (0, 3)


MASKS = ["random", "x0", "x1", "y0", "y1", "z0", "z1", "slab", "special"]


def mask(kind, shape):
    rng = np.random.default_rng(len(kind) + 17 * ord(kind[0]) + ord(kind[-1]))
    w = rng.uniform(0.5, 3, shape).astype(np.float32)
    if kind == "random":
        w[rng.random(shape) < 0.03] = 0
    elif kind == "slab":
        w[:, 6:9, :] = 0
    elif kind == "special":                     # both zeros mask; the smallest normal float does not
        w = rng.choice(np.array([0.0, -0.0, 2.0 ** -126, 1.0, 3.0], np.float32), shape, p=[0.02, 0.02, 0.32, 0.32, 0.32])
        assert np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all() and (w == np.float32(2.0 ** -126)).any()
    else:
        ix = [slice(None)] * 3
        ix["xyz".index(kind[0])] = 0 if kind[1] == "0" else -1
        w[tuple(ix)] = 0
    return w


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", ["gauss", "sign"])
def test_masked_form(name, kind, record_property):
    vol = M.volume(name)
    weight = mask(kind, vol.shape)
    labels = M.label_volumes(vol.shape)
    got = run(vol, 0.0, weight=weight, labels=labels)
    r = check(got, vol, 0.0, record_property, weight=weight, labels=labels, exact=M.VOLUMES[name].exact, tag=f"{name}/{kind} ")
    assert 0 < r["faces"] < len(M.oracle(vol, 0.0)[1])
    # no face lies in a cell with a zero-weight corner (cells from the raster walk of the live cells)
    cell = M.face_cells(vol, 0.0)[M.evaluation_ref.masked_mesh(vol, weight, *M.oracle(vol, 0.0), M.table())[2]]
    assert len(cell) == len(got[1])
    for k in range(8):
        assert (weight[cell[:, 0] + (k & 1), cell[:, 1] + ((k >> 1) & 1), cell[:, 2] + (k >> 2)] > 0).all()


@pytest.mark.parametrize("name", ["gauss", "sign"])
def test_masked_form_all_or_nothing(name):
    vol = M.volume(name)
    labels = M.label_volumes(vol.shape)
    plain = run(vol, 0.0, labels=labels)
    for w in (np.full(vol.shape, 0.5, np.float32), np.full(vol.shape, 2.0 ** -126, np.float32)):
        full = run(vol, 0.0, weight=w, labels=labels)
        assert len(full) == len(plain) == 5
        for a, b in zip(plain, full):                                # every weight > 0: the unmasked output, bit for bit
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
    for w in (np.zeros(vol.shape, np.float32), np.full(vol.shape, -0.0, np.float32)):
        verts, faces, normals, la, lb = run(vol, 0.0, weight=w, labels=labels)
        assert verts.shape == faces.shape == normals.shape == (0, 3) and la.shape == lb.shape == (0,)


def test_refusals():
    from eprecon_amd import _lib
    from eprecon_amd import save_scene as SS
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
        with pytest.raises(_lib.EpreconError):
            SS.marching_cubes(dev(M.gauss_volume(shape, 0)), 0.0)
        with pytest.raises(_lib.EpreconError):
            SS.marching_cubes(dev(M.gauss_volume(shape, 0)), 0.0, weight=dev(np.ones(shape, np.float32)))
    with pytest.raises(ValueError):
        SS.marching_cubes(dev(M.volume("gauss")), 0.0, weight=dev(np.ones((16, 16, 15), np.float32)))


def test_two_calls_give_identical_bytes():
    vol = M.volume("gauss")
    labels = M.label_volumes(vol.shape)
    for weight in (None, mask("random", vol.shape)):
        first = run(vol, 0.0, weight=weight, labels=labels)
        second = run(vol, 0.0, weight=weight, labels=labels)
        assert len(first[1]) > 1000
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()

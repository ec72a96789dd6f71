"""Host: the one reader and writer of saved scenes and the ScanNet-directory reader (eprecon_amd/scene_io.py) on the small
scene of tests/scene_io_cases.py in all three layouts.  Every comparison is exact."""
import os

import numpy as np
import pytest

import scene_io_cases as SC

from eprecon_amd import scene_io as SIO
from eprecon_amd.save_scene import load_scene_npz


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return SC.write_layouts(tmp_path_factory.mktemp("scene_io"))


def test_the_reader_names_each_layout(paths):
    for layout, path in paths.items():
        s = SIO.read_scene(path)
        assert s.layout == layout and s.dims == SC.DIMS
        assert s.origin.dtype == np.float32 and np.array_equal(s.origin, SC.ORIGIN)
        assert isinstance(s.voxel_size, float) and s.voxel_size == SC.VOXEL
        assert sorted(s.arrays) == sorted(SIO.VOLUME_KEYS) and s.rest == {}
        assert (s.coords is None) == (layout == "dense")
    assert SIO.read_scene(paths["sparse"]).arrays["semantic"].dtype == np.int32
    assert SIO.read_scene(paths["legacy"]).arrays["semantic"].dtype == np.int64


def test_all_layouts_give_the_same_dense_volumes(paths):
    truth = dict(zip(SIO.VOLUME_KEYS, SC.volumes()))
    assert truth["tsdf"][0, 0, 0] != 1 and truth["tsdf"][11, 9, 7] != 1 and (truth["semantic"] > 0).sum() == SC.N_ROWS
    for layout, path in paths.items():
        *vols, origin, voxel_size = SIO.scene_volumes(path)
        loaded = load_scene_npz(path)
        assert np.array_equal(origin, SC.ORIGIN) and voxel_size == SC.VOXEL
        assert np.array_equal(loaded["origin"], SC.ORIGIN) and float(loaded["voxel_size"]) == SC.VOXEL
        for key, vol in zip(SIO.VOLUME_KEYS, vols):
            assert vol.device.type == "cpu" and tuple(vol.shape) == SC.DIMS, (layout, key)
            assert vol.numpy().dtype == truth[key].dtype and np.array_equal(vol.numpy(), truth[key]), (layout, key)
            assert loaded[key].shape == SC.DIMS and np.array_equal(loaded[key], truth[key]), (layout, key)
    assert load_scene_npz(paths["dense"])["semantic"].dtype == np.int64           # a dense file: the arrays as stored
    assert load_scene_npz(paths["legacy"])["semantic"].dtype == np.int32          # rows: rebuilt as int32


class CountingArchive:
    """an NpzFile that writes down every entry that is decompressed, and its closing"""

    def __init__(self, z, log):
        self.z, self.log, self.files, self.zip = z, log, z.files, z.zip

    def __getitem__(self, key):
        self.log.append(key)
        return self.z[key]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log.append("<closed>")
        return self.z.__exit__(*exc)


def test_ids_only_never_reads_the_tsdf(paths, tmp_path, monkeypatch):
    log, real = [], np.load
    monkeypatch.setattr(np, "load", lambda path, *a, **kw: (log.append("<open>"), CountingArchive(real(path, *a, **kw), log))[1])
    truth = SC.volumes()
    for layout, path in paths.items():
        for want in (SIO.LABEL_KEYS, SIO.VOLUME_KEYS):
            del log[:]
            vols = SIO.scene_volumes(path, None, want)[:-2]
            assert all(np.array_equal(v.numpy(), truth[SIO.VOLUME_KEYS.index(k)]) for k, v in zip(want, vols))
            assert log.count("<open>") == 1 and log[-1] == "<closed>", (layout, log)
            assert len(set(log)) == len(log), (layout, log)                       # no entry decompressed twice
            assert any(k.endswith("tsdf") for k in log) == ("tsdf" in want), (layout, log)
    monkeypatch.undo()
    # ... and a sparse file without a TSDF entry serves the label tools
    with np.load(paths["sparse"]) as z:
        np.savez_compressed(tmp_path / "ids.npz", **{k: z[k] for k in z.files if k != "sparse_tsdf"})
    sem, ins, _, _ = SIO.scene_volumes(str(tmp_path / "ids.npz"), None, SIO.LABEL_KEYS)
    assert np.array_equal(sem.numpy(), truth[1]) and np.array_equal(ins.numpy(), truth[2])
    with pytest.raises(KeyError):
        SIO.scene_volumes(str(tmp_path / "ids.npz"))


def test_a_file_of_no_layout(tmp_path):
    path = str(tmp_path / "other.npz")
    np.savez_compressed(path, origin=SC.ORIGIN, voxel_size=SC.VOXEL, tsdf=np.ones(SC.DIMS, np.float32), weight=np.arange(4))
    with pytest.raises(ValueError, match="other.npz"):
        SIO.read_scene(path)
    plain = load_scene_npz(path)
    assert isinstance(plain, dict) and sorted(plain) == ["origin", "tsdf", "voxel_size", "weight"]
    assert np.array_equal(plain["weight"], np.arange(4)) and plain["tsdf"].shape == SC.DIMS
    # rows under the dense names without `dims`, and volumes that are not 3-D, are no layout either
    c, tsdf, sem, ins = SC.rows()
    for name, keys in (("rows", dict(coords=c, tsdf=tsdf, semantic=sem, instance=ins)),
                       ("flat", dict(tsdf=tsdf, semantic=sem, instance=ins))):
        np.savez_compressed(tmp_path / (name + ".npz"), origin=SC.ORIGIN, voxel_size=SC.VOXEL, **keys)
        with pytest.raises(ValueError, match=name + ".npz"):
            SIO.read_scene(str(tmp_path / (name + ".npz")))
        assert sorted(load_scene_npz(str(tmp_path / (name + ".npz")))) == sorted(["origin", "voxel_size"] + list(keys))


def test_the_writer_round_trips_both_layouts(tmp_path):
    """with the dtypes SaveScene writes: float32 origin and TSDF, int32 ids and coordinates, voxel_size a Python float"""
    c, tsdf, sem, ins = SC.rows()
    vt, vs, vi = SC.volumes()
    dense, sparse = str(tmp_path / "dense.npz"), str(tmp_path / "sparse.npz")
    SIO.write_scene(dense, vt, vs, vi, origin=SC.ORIGIN, voxel_size=SC.VOXEL)
    SIO.write_scene(sparse, tsdf, sem.astype(np.int32), ins.astype(np.int32), c, dims=np.array(SC.DIMS), origin=SC.ORIGIN,
                    voxel_size=SC.VOXEL, note=np.array([7]))
    assert sorted(os.listdir(tmp_path)) == ["dense.npz", "sparse.npz"]             # no second .npz on the names
    with np.load(dense) as z:
        assert sorted(z.files) == ["instance", "origin", "semantic", "tsdf", "voxel_size"]
        assert [z[k].dtype for k in sorted(z.files)] == [np.int32, np.float32, np.int32, np.float32, np.float64]
    with np.load(sparse) as z:
        assert sorted(z.files) == ["dims", "note", "origin", "sparse_coords", "sparse_instance", "sparse_semantic", "sparse_tsdf",
                                   "voxel_size"]
        assert z["sparse_coords"].dtype == np.int32 and z["sparse_tsdf"].dtype == np.float32 and z["voxel_size"].shape == ()
        assert z["sparse_semantic"].dtype == np.int32 and z["sparse_instance"].dtype == np.int32
    d, s = SIO.read_scene(dense, rest=True), SIO.read_scene(sparse, rest=True)
    assert (d.layout, s.layout) == ("dense", "sparse") and d.dims == s.dims == SC.DIMS
    assert sorted(d.rest) == ["origin", "voxel_size"] and sorted(s.rest) == ["dims", "note", "origin", "voxel_size"]
    for key, vol, values in zip(SIO.VOLUME_KEYS, (vt, vs, vi), (tsdf, sem, ins)):
        assert np.array_equal(d.arrays[key], vol) and d.arrays[key].dtype == vol.dtype
        assert np.array_equal(s.arrays[key], values) and np.array_equal(s.coords, c)
    for path in (dense, sparse):
        for got, vol in zip(SIO.scene_volumes(path)[:3], (vt, vs, vi)):
            assert np.array_equal(got.numpy(), vol)
    # the rows of either file in raster order, with the position each has in its file
    cells, rt, rs, ri, order = SIO.raster_rows(s)
    raster = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))
    assert np.array_equal(order, raster) and np.array_equal(cells, c[raster]) and np.array_equal(rt, tsdf[raster])
    dense_rows = SIO.raster_rows(d)
    assert dense_rows[4] is None and all(np.array_equal(x, y) for x, y in zip(dense_rows[:4], (cells, rt, rs, ri)))


def test_scene_list(tmp_path):
    (tmp_path / "scenes.txt").write_text("scene0000_00\n\n  scene0001_00  \nscene0002_00")
    assert SIO.read_scene_list(str(tmp_path / "scenes.txt")) == ["scene0000_00", "scene0001_00", "scene0002_00"]


def test_the_directory_reader_splits_at_any_whitespace(tmp_path):
    rng = np.random.default_rng(3)
    k4 = np.eye(4)
    k4[:3, :3] = [[577.870605, 0.0, 319.5], [0.0, 577.870605, 239.5], [0.0, 0.0, 1.0]]
    pose4 = np.eye(4)
    pose4[:3] = rng.uniform(-3, 3, (3, 4))
    lost = np.full((4, 4), -np.inf)
    text = lambda m, sep, tail: "".join(sep.join(repr(float(v)) for v in row) + tail + "\n" for row in m)
    got = []
    for name, sep, tail in (("spaces", " ", ""), ("tabs", "\t", ""), ("trailing", " ", " ")):
        root = tmp_path / name
        for sub in ("intrinsic", "pose", "depth"):
            os.makedirs(root / sub)
        for sensor in ("depth", "color"):
            (root / "intrinsic" / f"intrinsic_{sensor}.txt").write_text(text(k4 * (1 if sensor == "depth" else 2), sep, tail))
        (root / "pose" / "pose_0.txt").write_text(text(pose4, sep, tail))
        (root / "pose" / "pose_1.txt").write_text(text(lost, sep, tail))
        (root / "pose" / "notes.txt").write_text("")
        (root / "depth" / "depth_0.png").write_bytes(b"")
        got.append((SIO.intrinsic(str(root), "depth"), SIO.intrinsic(str(root), "color"), SIO.pose(str(root), 0), SIO.pose(str(root), 1)))
        assert SIO.pose_frame_ids(str(root)) == [0, 1] and SIO.pose_frame_ids(str(root), 2) == [0]
        assert SIO.count_depth_frames(str(root)) == 1
    for kd, kc, p0, p1 in got:
        assert kd.dtype == kc.dtype == p0.dtype == np.float64 and kd.shape == (3, 3) and p0.shape == p1.shape == (4, 4)
        assert np.array_equal(kd, k4[:3, :3]) and np.array_equal(kc, 2 * k4[:3, :3]) and np.array_equal(p0, pose4)
        assert np.isinf(p1).all()
    # the single-space files read the same with the delimiter the earlier readers passed
    assert np.array_equal(np.loadtxt(tmp_path / "spaces" / "pose" / "pose_0.txt", delimiter=" "), got[0][2])


def test_depth_metres(tmp_path):
    image_mod = pytest.importorskip("PIL.Image")
    mm = np.array([[0, 500, 2999], [3000, 3001, 65535]], np.uint16)
    image_mod.fromarray(mm).save(tmp_path / "depth_0.png")
    d = SIO.depth_metres(str(tmp_path / "depth_0.png"), 3.0)
    assert d.dtype == np.float32 and np.array_equal(d, np.array([[0, 0.5, 2.999], [3.0, 0, 0]], np.float32))
    assert np.array_equal(SIO.depth_metres(str(tmp_path / "depth_0.png"), 10.0)[1], np.array([3.0, 3.001, 0], np.float32))

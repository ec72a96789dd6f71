"""GPU: the call descriptor of the back-projection (eprecon_bp_call, include/eprecon_hip.h) against the positional entry, its
halves against the whole call, and `rank` as a field of one call.  Every comparison is between launches of the same kernels on
the same inputs, so it is byte for byte; what the kernels compute is checked in test_back_project_gpu.py and
test_back_project_f64_gpu.py, the rank volume, the halves on a side stream and the levels in test_init_glue_gpu.py,
test_back_project_launches_gpu.py and test_bp_levels_gpu.py.

Shapes: V = 3 views of 12 x 16 maps; C = 8 (the gather with taps in LDS) and C = 6 (the scalar gather); one and two batch
elements; 17 and 257 voxels (two and seventeen 16-voxel tiles, the last one partial, and two count workgroups)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

V, H, W = 3, 12, 16
VOXEL_SIZE, MIN_VIEW = 0.1, 2
ERR_ARG, ERR_WORKSPACE = -1, -2
NCHW, NHWC = 0, 1
COUNT, GATHER = 1, 2


def scene(n, B, C, seed=0):
    """a sparse list, grouped by batch element, in front of three pinhole cameras half a metre apart: most voxels are seen
    by two views or more, the rim by fewer; every eighth voxel lies out of every frustum (far to the side, or behind the
    cameras) and the last entry has a batch index out of range: about two voxels in three are valid at MIN_VIEW, every batch
    element has some, and the last tile of both list lengths has none.  -> numpy arrays"""
    rng = np.random.default_rng(seed)
    coords = np.zeros((n, 4), np.int32)
    coords[:, 0] = np.arange(n) * B // n
    coords[:, 1:] = rng.integers(0, 20, (n, 3))
    coords[3::8, 1] = 500
    coords[7::16, 3] = -50
    coords[n - 1, 0] = B
    origin = np.tile(np.array([-1.0, -0.6, 1.0], np.float32), (B, 1))
    kr = np.zeros((V, B, 4, 4), np.float32)
    for v in range(V):      # K [I | t]: f = 10 px, principal point the image centre, t = ((v - 1) / 2, 0, 0)
        kr[v, :] = np.array([[10, 0, 7.5, 10 * 0.5 * (v - 1)], [0, 10, 5.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    feats = rng.standard_normal((V, B, C, H, W)).astype(np.float32)
    return coords, origin, kr, feats


class Buffers:
    """the device inputs of one scene and, per call, sentinel-filled outputs"""

    def __init__(self, n, B, C, layout=NCHW):
        from eprecon_amd import _lib
        self.lib, self.n, self.B, self.C, self.layout = _lib.load(), n, B, C, layout
        coords, origin, kr, feats = scene(max(n, 1), B, C)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.coords, self.origin, self.kr = dev(coords[:n]), dev(origin), dev(kr)
        self.feats = dev(feats if layout == NCHW else feats.transpose(0, 1, 3, 4, 2))
        self.ws_bytes = self.lib.eprecon_back_project_workspace_bytes(n, B, V, C, H, W, layout)

    def outputs(self, mode):
        n, B, C, nan = max(self.n, 1), self.B, self.C, float("nan")
        return {"feats": torch.full((n, C + 1 if mode == 1 else C), nan, device="cuda"),
                "mean": torch.full((n, C), nan, device="cuda") if mode == 2 else None,
                "coords": torch.full((n, 4), -7, dtype=torch.int32, device="cuda"),
                "count": torch.full((n,), nan, device="cuda"),
                "grid": torch.full((V * n * 2,), nan, device="cuda"),
                "mask": torch.full((V * n,), 77, dtype=torch.uint8, device="cuda"),
                "nv": torch.full((1 + B,), -99, dtype=torch.int32, device="cuda"),
                "ws": torch.zeros((self.ws_bytes,), dtype=torch.uint8, device="cuda")}

    def desc(self, mode, t, phase=0, rank=None):
        from eprecon_amd import _lib
        p, d = _lib.ptr, _lib.BpCall()
        d.coords, d.n, d.origin, d.batch, d.voxel_size = p(self.coords), self.n, p(self.origin), self.B, VOXEL_SIZE
        d.feats, d.feats_layout, d.krcam = p(self.feats), self.layout, p(self.kr)
        d.n_views, d.channels, d.height, d.width, d.min_view, d.mode = V, self.C, H, W, MIN_VIEW, mode
        d.count, d.n_valid_dev, d.workspace, d.workspace_bytes = p(t["count"]), p(t["nv"]), p(t["ws"]), t["ws"].numel()
        d.phase, d.out_feats, d.out_mean, d.out_coords = phase, p(t["feats"]), p(t["mean"]), p(t["coords"])
        d.out_grid, d.out_mask, d.rank = p(t["grid"]), p(t["mask"]), p(rank)
        return d

    def call(self, d):
        from eprecon_amd import _lib
        return self.lib.eprecon_back_project_call_async(ctypes.byref(d), _lib.current_stream())

    def positional(self, mode, t):
        from eprecon_amd import _lib
        p = _lib.ptr
        return self.lib.eprecon_back_project_async(
            p(self.coords), self.n, p(self.origin), self.B, VOXEL_SIZE, p(self.feats), self.layout, p(self.kr), V, self.C, H, W,
            MIN_VIEW, mode, p(t["feats"]), p(t["mean"]), p(t["coords"]), p(t["count"]), p(t["grid"]), p(t["mask"]), p(t["nv"]),
            p(t["ws"]), t["ws"].numel(), _lib.current_stream())


def assert_same_bytes(a, b, keys=("feats", "mean", "coords", "count", "grid", "mask", "nv")):
    torch.cuda.synchronize()
    for k in keys:
        if a[k] is not None:
            assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def untouched(t, keys):
    torch.cuda.synchronize()
    fresh = {"feats": float("nan"), "mean": float("nan"), "coords": -7, "count": float("nan"), "grid": float("nan"), "mask": 77,
             "nv": -99}
    for k in keys:
        x = t[k]
        assert bool(torch.isnan(x).all() if x.is_floating_point() else (x == fresh[k]).all()), k


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("n", [17, 257])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [8, 6])
def test_descriptor_equals_positional(C, B, n, layout):
    bufs = Buffers(n, B, C, layout)
    for mode in (0, 1, 2):
        a, b = bufs.outputs(mode), bufs.outputs(mode)
        assert bufs.positional(mode, a) == 0
        assert bufs.call(bufs.desc(mode, b)) == 0
        assert_same_bytes(a, b)
        nv = b["nv"].tolist()
        assert 0 < nv[0] < n and sum(nv[1:]) == nv[0] and all(x > 0 for x in nv[1:])
        assert torch.isnan(b["feats"][nv[0]:]).all() and not torch.isnan(b["feats"][:nv[0]]).any()


@pytest.mark.parametrize("C,B,n", [(8, 2, 257), (6, 1, 17), (8, 1, 257), (6, 2, 17)])
def test_halves_equal_the_whole_call(C, B, n):
    bufs = Buffers(n, B, C, NHWC)
    for mode in (0, 1, 2):
        whole, halves = bufs.outputs(mode), bufs.outputs(mode)
        assert bufs.call(bufs.desc(mode, whole)) == 0
        d = bufs.desc(mode, halves, phase=COUNT)
        assert bufs.call(d) == 0
        untouched(halves, ("feats", "mean", "coords", "grid", "mask") if mode == 2 else ("feats", "coords", "grid", "mask"))
        d.phase = GATHER
        assert bufs.call(d) == 0
        assert_same_bytes(whole, halves)


def test_phase_errors_launch_nothing():
    nchw, nhwc = Buffers(17, 1, 8, NCHW), Buffers(17, 1, 8, NHWC)
    t = nchw.outputs(0)
    assert nchw.call(nchw.desc(0, t, phase=COUNT)) == ERR_ARG
    assert nchw.call(nchw.desc(0, t, phase=GATHER)) == ERR_ARG
    assert nhwc.call(nhwc.desc(0, t, phase=3)) == ERR_ARG
    assert nhwc.call(nhwc.desc(0, t, phase=-1)) == ERR_ARG
    untouched(t, ("feats", "coords", "count", "grid", "mask", "nv"))


@pytest.mark.parametrize("C", [8, 6])
def test_rank_of_a_failed_call_does_not_reach_the_next(C):
    """the first call names a rank buffer and fails before any launch; the call after it names none and leaves it alone"""
    n = 257
    bufs = Buffers(n, 1, C)
    rank = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    t = bufs.outputs(2)
    d = bufs.desc(2, t, rank=rank)
    d.workspace_bytes -= 1
    assert bufs.call(d) == ERR_WORKSPACE
    untouched(t, ("feats", "mean", "coords", "count", "grid", "mask", "nv"))
    assert bufs.call(bufs.desc(2, t)) == 0
    torch.cuda.synchronize()
    assert 0 < int(t["nv"][0]) < n
    assert bool((rank == -5).all())


def test_rank_needs_one_batch_element():
    bufs = Buffers(17, 2, 8)
    rank = torch.full((18,), -5, dtype=torch.int32, device="cuda")
    t = bufs.outputs(0)
    assert bufs.call(bufs.desc(0, t, rank=rank)) == ERR_ARG
    untouched(t, ("feats", "coords", "count", "grid", "mask", "nv"))
    assert bool((rank == -5).all())
    d = bufs.desc(0, t, phase=COUNT, rank=rank)      # the count half ignores rank
    d.feats_layout = NHWC
    assert bufs.call(d) == 0
    torch.cuda.synchronize()
    assert bool((rank == -5).all())


@pytest.mark.parametrize("layout", [NCHW, NHWC])
def test_empty_list_clears_rank_word_and_counters(layout):
    bufs = Buffers(0, 1, 8, layout)
    rank = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    t = bufs.outputs(0)
    assert bufs.call(bufs.desc(0, t, rank=rank)) == 0
    torch.cuda.synchronize()
    assert rank.tolist() == [0] and t["nv"].tolist() == [0, 0]
    untouched(t, ("feats", "coords", "count", "grid", "mask"))

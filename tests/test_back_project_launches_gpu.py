"""GPU: the launch chain of a back-projection (csrc/back_project.hip) gives the bits of the four-launch chain it replaces.

A call is prepare -> gather on NCHW maps (re-layout and count in one grid) and count -> gather on channels-last maps; the gather
workgroups sum the tile totals in front of their tile themselves (tile_base) instead of a scan launch in between, up to
EPRECON_BP_FOLD tiles.  EPRECON_BP_FOLD=0 is the chain as it was: re-layout, count, scan, gather.  Every comparison here is
byte for byte between the two (compare_chains), a second run of the default must repeat its own bits, and which of the two forms
ran is read back from the workspace (form_that_ran): the tile totals stay raw when the gather folded the scan and are an
exclusive scan when the scan launch ran.  That the values are RIGHT is the business of tests/test_back_project_f64_gpu.py.

Scenes: tests/back_project_ref.py's windows on the 40 x 30 maps of level 1 (or rescaled to smaller maps), C = 4 / 8 (the
4-channel-lane gather) and C = 6 (the scalar gather), V = 2-3, so that the long lists stay at a few MB.
"""
import os

import numpy as np
import pytest

import back_project_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MEAN, DEPTH, VAR = R.MODE_MEAN, R.MODE_MEAN_DEPTH, R.MODE_VARIANCE
DEFAULT_CAP = 6144      # kFoldCapDefault of csrc/back_project.hip
KEYS = ("feats", "coords", "count", "n_valid", "n_valid_per_batch", "grid", "mask", "mean")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_scenes = {}


def scene(**kw):
    """R.scene on the level-1 maps, built once per argument set and never modified (callers copy what they edit)"""
    key = tuple(sorted(kw.items()))
    if key not in _scenes:
        if len(_scenes) > 6:
            _scenes.clear()
        _scenes[key] = R.scene(**{"lvl": 1, "V": 3, **kw})
    return _scenes[key]


def with_maps(sc, h, w, seed=11):
    """the same voxels and cameras seen through h x w maps: pixel coordinates scale with (w - 1, h - 1), so the frustum is kept"""
    V, B, C, H, W = sc["feats"].shape
    s = np.diag([(w - 1) / (W - 1), (h - 1) / (H - 1), 1.0, 1.0]).astype(np.float64)
    kr = (s[None, None] @ sc["kr"].astype(np.float64)).astype(np.float32)
    feats = np.random.default_rng(seed).standard_normal((V, B, C, h, w)).astype(np.float32)
    return dict(sc, kr=kr, feats=feats)


def far_rows(rows):
    """rows no camera sees (in the batch, far outside every frustum): valid only with min_view <= 0"""
    out = rows.copy()
    out[:, 1:] += 1 << 20
    return out


def vox_of(n):
    return 256 if n >= 512 * 1024 else (64 if n >= 48 * 1024 else 16)


def run(sc, mode, mv, nhwc=False, fold=None):
    """one back-projection through run_async (the counts are always read) -> (dict of host arrays, first ntile workspace words)"""
    from eprecon_amd import _lib, back_project as BP
    feats = _dev(sc["feats"])
    if nhwc:
        feats = feats.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    old = os.environ.pop("EPRECON_BP_FOLD", None)
    if fold is not None:
        os.environ["EPRECON_BP_FOLD"] = str(fold)
    try:
        res = BP.run_async(_dev(sc["coords"]), _dev(sc["origin"]), sc["voxel_size"], feats, _dev(sc["kr"]), mv, mode,
                           min_valid_per_batch=0, want_grid=True, want_mean=mode == VAR).result()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("EPRECON_BP_FOLD", None)
        if old is not None:
            os.environ["EPRECON_BP_FOLD"] = old
    assert res is not None
    n = sc["coords"].shape[0]
    ntile = -(-n // vox_of(n))
    words = _lib.workspace(0, feats.device)[: 4 * ntile].view(torch.int32).cpu().numpy().copy()
    out = {k: (res[k].cpu().numpy() if torch.is_tensor(res[k]) else np.asarray(res[k])) for k in KEYS if k in res}
    return out, words


def form_that_ran(sc, out, mv, words):
    """"fold" | "scan" | None (both forms leave the same words: no valid voxel, or one tile) from the workspace's tile words"""
    n, B = sc["coords"].shape[0], sc["origin"].shape[0]
    b = sc["coords"][:, 0]
    valid = (b >= 0) & (b < B) & (out["count"] >= mv)
    vox = vox_of(n)
    totals = np.add.reduceat(valid.astype(np.int32), np.arange(0, n, vox))
    scanned = np.cumsum(totals) - totals
    assert int(totals.sum()) == int(out["n_valid"])
    if np.array_equal(totals, scanned):
        return None
    if np.array_equal(words, totals):
        return "fold"
    assert np.array_equal(words, scanned)
    return "scan"


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert x.tobytes() == y.tobytes(), k


def compare_chains(sc, mode, mv, nhwc=False, fold=None, expect=None):
    """default (or EPRECON_BP_FOLD=fold) against EPRECON_BP_FOLD=0, byte for byte; the default twice; the form that ran
    (expect; None: by the cap in force -- 524,287 voxels are 8,192 tiles of 64, above the default cap)"""
    n = sc["coords"].shape[0]
    if expect is None:
        expect = "fold" if -(-n // vox_of(n)) <= (DEFAULT_CAP if fold is None else fold) else "scan"
    old, w_old = run(sc, mode, mv, nhwc, fold=0)
    new, w_new = run(sc, mode, mv, nhwc, fold=fold)
    again, _ = run(sc, mode, mv, nhwc, fold=fold)
    same_bits(new, old)
    same_bits(again, new)
    assert form_that_ran(sc, old, mv, w_old) in ("scan", None)
    assert form_that_ran(sc, new, mv, w_new) in (expect, None)
    return new


# ---------------------------------------------------------------------------------------------------------------------
# modes x gather kernels x layouts x re-layout forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C", [8, 6])
@pytest.mark.parametrize("mode", [MEAN, DEPTH, VAR], ids=["mean", "depth", "var"])
def test_modes_kernels_layouts(mode, C, nhwc):
    sc = scene(seed=4, nvox=96, C=C, n=(16385,))     # 1,025 tiles of 16, the last of one voxel
    got = compare_chains(sc, mode, 2, nhwc)
    assert 0 < got["n_valid"] < 16385


@pytest.mark.parametrize("hw", [(8, 10), (7, 9), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [8, 6])
def test_prepare_on_small_maps(C, hw):
    """the prepare launch's re-layout half on both sides of its 16-byte rule (hw % 4, C % 4), a ragged and a whole last tile"""
    sc = with_maps(scene(seed=4, nvox=96, C=C, n=(5000,)), *hw)
    got = compare_chains(sc, VAR, 1)
    assert got["n_valid"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# tile sizes, list lengths, empty tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [0, 2])
@pytest.mark.parametrize("n", [1, 100, 49151, 49152])
def test_short_lists(n, mv):
    compare_chains(scene(seed=4, nvox=96, C=8, n=(n,)), VAR if n % 2 else MEAN, mv)


@pytest.mark.parametrize("mv", [0, 2])
@pytest.mark.parametrize("n", [524287, 524288])
def test_tile_64_to_256(n, mv):
    compare_chains(scene(seed=0, nvox=96, interval=1, C=4, n=(n,)), MEAN, mv)


@pytest.mark.parametrize("n", [1000, 50000], ids=["vox16", "vox64"])
def test_last_tile_without_a_valid_voxel(n):
    """the workgroup of the last tile publishes the counters and then has nothing to gather"""
    sc = dict(scene(seed=4, nvox=96, C=8, n=(n,)))
    coords = sc["coords"].copy()
    coords[-(vox_of(n) + 3):] = far_rows(coords[-(vox_of(n) + 3):])
    sc["coords"] = coords
    got = compare_chains(sc, DEPTH, 1)
    assert got["count"][-vox_of(n):].max() == 0 and got["n_valid"] > 0


@pytest.mark.parametrize("mode", [MEAN, DEPTH, VAR], ids=["mean", "depth", "var"])
def test_no_valid_voxel_at_all(mode):
    sc = dict(scene(seed=4, nvox=96, C=8, n=(1000,)))
    sc["coords"] = far_rows(sc["coords"])
    got = compare_chains(sc, mode, 2)
    assert got["n_valid"] == 0 and got["feats"].shape[0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# batches and foreign rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [0, 2])
@pytest.mark.parametrize("n", [(270,), (70, 200), (100, 3, 300)], ids=["b1", "b2", "b3"])
@pytest.mark.parametrize("C", [8, 6])
def test_batches(C, n, mv):
    """batch boundaries inside a wave and inside a 16-row tile (70, 100, 103)"""
    sc = scene(seed=4, B=len(n), C=C, n=n)
    got = compare_chains(sc, DEPTH, mv)
    assert int(got["n_valid_per_batch"].sum()) == int(got["n_valid"])
    if mv == 0:
        assert got["n_valid_per_batch"].tolist() == list(n)


@pytest.mark.parametrize("mv", [0, 2])
def test_foreign_rows(mv):
    """rows of no batch element (index -1 and B) in front of, inside and behind the list: counted 0, never kept"""
    sc = dict(scene(seed=4, B=2, C=8, n=(70, 200)))
    c = sc["coords"]
    f = lambda rows, b: np.concatenate([np.full((rows.shape[0], 1), b, np.int32), rows[:, 1:]], axis=1)
    sc["coords"] = np.ascontiguousarray(np.concatenate(
        [f(c[:5], -1), f(c[5:8], 2), c[:40], f(c[40:43], 2), c[40:70], f(c[:19], -1), c[70:], f(c[:33], 2), f(c[:2], -1)]))
    got = compare_chains(sc, VAR, mv)
    foreign = (sc["coords"][:, 0] < 0) | (sc["coords"][:, 0] >= 2)
    assert not got["count"][foreign].any()
    assert set(np.unique(got["coords"][:, 0]).tolist()) <= {0, 1}
    if mv == 0:
        assert got["n_valid_per_batch"].tolist() == [70, 200]


# ---------------------------------------------------------------------------------------------------------------------
# the cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,expect", [(80, 5, "fold"), (81, 5, "scan"), (49152, 768, "fold"), (49153, 768, "scan")],
                         ids=["vox16_at", "vox16_over", "vox64_at", "vox64_over"])
def test_cap_both_sides(n, cap, expect):
    sc = scene(seed=4, nvox=96, C=8, n=(n,))
    new, words = run(sc, MEAN, 2, fold=cap)
    assert form_that_ran(sc, new, 2, words) == expect
    compare_chains(sc, VAR, 2, fold=cap, expect=expect)
    compare_chains(sc, VAR, 2, nhwc=True, fold=cap, expect=expect)


@pytest.mark.parametrize("over", [0, 1], ids=["at", "over"])
def test_default_cap(over):
    """DEFAULT_CAP tiles of 256 voxels and one voxel more, with no switch set"""
    n = DEFAULT_CAP * 256 + over
    assert n < 3_000_000
    sc = scene(seed=0, nvox=128, interval=1, V=2, C=4, n=(n,))
    compare_chains(sc, MEAN, 1, expect="scan" if over else "fold")


# ---------------------------------------------------------------------------------------------------------------------
# the re-layout alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 10), (7, 9), (16, 16), (10, 13), (30, 40), (1, 68), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [4, 8, 6, 3, 24])
def test_relayout_is_a_copy(C, hw):
    """hw % 4 and C % 4 on both sides of the 16-byte rule; last tiles of 16, 63, 64, 2, 48 and 4 pixels"""
    from eprecon_amd import back_project as BP
    h, w = hw
    x = _dev(np.random.default_rng(C * 100 + h * w).standard_normal((3, 2, C, h, w)).astype(np.float32))
    got = BP.to_channels_last(x)
    assert got.shape == x.shape and got.stride() == (2 * h * w * C, h * w * C, 1, w * C, C)
    want = x.permute(0, 1, 3, 4, 2).contiguous()
    assert got.permute(0, 1, 3, 4, 2).contiguous().cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_relayout_of_an_unaligned_view():
    """maps that start 4 bytes into an allocation take the 4-byte form"""
    from eprecon_amd import _lib
    lib = _lib.load()
    C, hw = 8, 80
    buf = _dev(np.random.default_rng(5).standard_normal(2 * C * hw + 1).astype(np.float32))
    src = buf[1:]
    dst = torch.empty(2 * hw * C, dtype=torch.float32, device="cuda")
    _lib.check(lib.eprecon_nchw_to_nhwc_async(_lib.ptr(src), _lib.ptr(dst), 2, C, hw, _lib.current_stream()), "relayout")
    want = src.view(2, C, hw).permute(0, 2, 1).contiguous().view(-1)
    assert dst.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()

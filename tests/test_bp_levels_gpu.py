"""GPU: the first halves of several back-projections as ONE launch (back_project.prepare_levels_async,
eprecon_back_project_prepare_levels_async) give the bits of every level's own launches.

The grid of that launch is the concatenation of the levels' re-layout and count blocks; a workgroup finds its level and its half
from range compares.  Every case here runs the default against EPRECON_BP_LEVELS=0 — once through the same entry, which then
queues one launch per level, and once through plain run_async calls, every level with its own read — on the same inputs, and
every output is compared byte for byte: rows, coordinates, per-voxel count, n_valid, per-batch counts and None results.  That
the values are RIGHT is the business of tests/test_back_project_f64_gpu.py.

Scene: three views of a 24^3 volume (128 x 96 images: maps 6x8 / 12x16 / 24x32 with C = 80 / 40 / 24, the workload's three
levels), lists five entries short of their grid, so that no list is a multiple of its tile and 6 x 8 = 48 pixels are no
multiple of the re-layout's 64-pixel tile.  Lists of 63,995 and 531,436 entries select the 64- and 256-voxel tiles.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

V = 3
SIDE = 0.96          # edge of the volume in metres (24 voxels of 0.04)
KEYS = ("feats", "coords", "count", "n_valid", "n_valid_per_batch")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_window = {}


def window():
    from eprecon_amd import synthetic as S
    if not _window:
        _window.update(S.make_window(seed=0, width=128, height=96, n_views=V, n_vox=(24, 24, 24)))
    return _window


def level(dim, c, h, w, mv=0, drop=5, nhwc=False, cams="window", listed=True, seed=0):
    """one level as host arrays: the dense dim^3 raster of the volume less its last `drop` entries, V maps of c x h x w.
    cams: "window" (the synthetic arc: some voxels seen, some not), "none" (every voxel behind every camera) or "all" (every
    voxel projects to the centre pixel of every view)"""
    from eprecon_amd import synthetic as S
    win = window()
    lvl = {6: 2, 12: 1}.get(dim, 0)
    kr = win["proj_matrices"][:, lvl][:, None].astype(np.float64)            # [V, 1, 4, 4], for the pyramid's maps of this level
    h0, w0 = 96 // (4 << lvl), 128 // (4 << lvl)
    kr = np.diag([(w - 1) / (w0 - 1), (h - 1) / (h0 - 1), 1.0, 1.0])[None, None] @ kr
    if cams == "none":
        kr[:, :, 2] = -kr[:, :, 2]
    elif cams == "all":
        kr[:] = 0.0
        kr[:, :, 0, 3], kr[:, :, 1, 3], kr[:, :, 2, 3], kr[:, :, 3, 3] = (w - 1) / 2, (h - 1) / 2, 1.0, 1.0
    coords = S.dense_coords((dim,) * 3, 1)
    return dict(coords=coords[:coords.shape[0] - drop] if listed else None, origin=win["vol_origin_partial"][None].copy(),
                voxel_size=SIDE / dim, feats=S.make_features(100 + seed + c, V, (c, h, w)), kr=kr.astype(np.float32), mv=mv, nhwc=nhwc)


def workload_levels(mv=(2, 0, 0)):
    return [level(6, 80, 6, 8, mv[0]), level(12, 40, 12, 16, mv[1]), level(24, 24, 24, 32, mv[2])]


def _args(lv):
    feats = _dev(lv["feats"])
    if lv["nhwc"]:
        feats = feats.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    coords = None if lv["coords"] is None else _dev(lv["coords"])
    return coords, _dev(lv["origin"]), lv["voxel_size"], feats, _dev(lv["kr"]), lv["mv"]


def _host(res):
    if res is None:
        return None
    return {k: (res[k].cpu().numpy() if torch.is_tensor(res[k]) else np.asarray(res[k])) for k in KEYS}


def run_levels(levels, monkeypatch, off=False, plain=False, side=False, bracket=False):
    """-> per level: dict of host arrays | None (no valid voxel) | the channels-last maps of a level without a list.
    off: under EPRECON_BP_LEVELS=0; plain: run_async per level, each with its own read (and to_channels_last for a level
    without a list) instead of prepare_levels_async; side: the prepare launch on a side stream; bracket: the profile bracket
    armed in front of the last level's gather"""
    from eprecon_amd import _lib, back_project as BP
    if off:
        monkeypatch.setenv("EPRECON_BP_LEVELS", "0")
    else:
        monkeypatch.delenv("EPRECON_BP_LEVELS", raising=False)
    assert bool(_lib.load().eprecon_bp_levels()) == (not off)
    args = [_args(lv) for lv in levels]
    if plain:
        out = [BP.to_channels_last(a[3]).cpu().numpy() if a[0] is None else _host(BP.run_async(*a).result()) for a in args]
    else:
        # (the process-wide set-up stream, as Cfg2Step uses it: the suite creates no streams of its own)
        handles = BP.prepare_levels_async(args, stream=_lib.side_stream(args[0][3].device, _lib.SIDE_SETUP) if side else None)
        pends, counted = [], []
        for i, (a, hd) in enumerate(zip(args, handles)):
            if a[0] is None:
                if hd.stream is not None:
                    torch.cuda.current_stream().wait_stream(hd.stream)
                continue
            if bracket and i == len(args) - 1:
                _lib.load().eprecon_profile_enable(2)
            pends.append(BP.run_async(*a[:3], hd.nhwc, *a[4:], hold_read=True, counted=hd))
            counted.append(hd)
        reads0 = _lib.HOST_READS
        res = iter(BP.PendingLevels(pends, counted).results() if pends else [])
        assert _lib.HOST_READS == reads0 + (1 if pends else 0)          # one blocking read for all levels
        out = [hd.nhwc.cpu().numpy() if a[0] is None else _host(next(res)) for a, hd in zip(args, handles)]
    torch.cuda.synchronize()
    monkeypatch.delenv("EPRECON_BP_LEVELS", raising=False)
    return out


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is None:
            continue
        if isinstance(g, np.ndarray):
            assert g.shape == w.shape and g.strides == w.strides and g.tobytes() == w.tobytes()
            continue
        for k in KEYS:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and g[k].tobytes() == w[k].tobytes(), k


def check(levels, monkeypatch, **kw):
    """the default against both forms of EPRECON_BP_LEVELS=0 -> the default's outputs"""
    got = run_levels(levels, monkeypatch, **kw)
    same_bits(got, run_levels(levels, monkeypatch, off=True))
    same_bits(got, run_levels(levels, monkeypatch, off=True, plain=True))
    return got


# ------------------------------------------------------------------------------------------------
# the workload's three levels and their orderings
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [(2, 0, 0), (0, 2, 2)])
def test_three_levels_of_the_workload(mv, monkeypatch):
    levels = workload_levels(mv)
    got = check(levels, monkeypatch)
    for lv, o, m in zip(levels, got, mv):
        n = lv["coords"].shape[0]
        assert n % 16 != 0                                    # five short of the grid: the last tile is partial
        if m == 0:
            assert o["n_valid"] == n
        else:
            assert 0 < o["n_valid"] < n                       # the window's cameras see a part of the volume
    assert (6 * 8) % 64 != 0                                  # the smallest maps end inside a re-layout tile


@pytest.mark.parametrize("order", ["largest_first", "smallest_first", "one", "four_two_equal"])
def test_level_orderings(order, monkeypatch):
    small, mid, large = workload_levels((2, 2, 2))
    levels = {"largest_first": [large, mid, small], "smallest_first": [small, mid, large], "one": [mid],
              "four_two_equal": [mid, large, mid, small]}[order]
    got = check(levels, monkeypatch)
    assert all(o is not None for o in got)
    if order == "four_two_equal":
        same_bits([got[0]], [got[2]])


def test_the_three_tile_sizes(monkeypatch):
    """lists of 13,819 / 63,995 / 531,436 entries: the gather's tiles of 16 / 64 / 256 voxels, whose totals the count blocks
    write; 9 x 11 maps with C = 8 keep the long lists cheap"""
    levels = [level(24, 8, 9, 11, 2), level(81, 8, 9, 11, 2), level(40, 8, 9, 11, 2)]
    sizes = [lv["coords"].shape[0] for lv in levels]
    assert sizes[0] < 48 * 1024 <= sizes[2] < 512 * 1024 <= sizes[1]
    got = check(levels, monkeypatch)
    assert all(0 < o["n_valid"] < n for o, n in zip(got, sizes))


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
def test_a_channels_last_level_has_no_relayout_blocks(monkeypatch):
    small, mid, large = workload_levels((2, 2, 2))
    for levels in ([small, dict(mid, nhwc=True), large], [dict(small, nhwc=True), mid, large],
                   [dict(small, nhwc=True), dict(mid, nhwc=True), dict(large, nhwc=True)]):
        check(levels, monkeypatch)


def test_channels_and_pixels_that_are_no_multiple_of_four(monkeypatch):
    """C % 4 != 0 and H W % 4 != 0: the 4-byte re-layout (VEC4 false) beside 16-byte ones, and the scalar gather"""
    levels = [level(6, 80, 6, 8, 2), level(12, 6, 12, 16, 2), level(12, 8, 7, 9, 2), level(24, 24, 24, 32, 0)]
    check(levels, monkeypatch)


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_level_without_a_list_is_relaid_out_only(where, monkeypatch):
    from eprecon_amd import back_project as BP
    levels = workload_levels((2, 0, 2))
    levels[where] = dict(levels[where], coords=None)
    got = check(levels, monkeypatch)
    maps = got[where]
    want = BP.to_channels_last(_dev(levels[where]["feats"])).cpu().numpy()
    assert maps.shape == levels[where]["feats"].shape and maps.strides == want.strides and maps.tobytes() == want.tobytes()
    assert np.array_equal(maps, levels[where]["feats"])
    assert all(isinstance(o, dict) for i, o in enumerate(got) if i != where)


def test_only_levels_without_a_list(monkeypatch):
    levels = [dict(level(6, 80, 6, 8), coords=None), dict(level(12, 6, 7, 9), coords=None), dict(level(12, 40, 12, 16, nhwc=True), coords=None)]
    got = check(levels, monkeypatch)
    for o, lv in zip(got, levels):
        assert np.array_equal(o, lv["feats"])


# ------------------------------------------------------------------------------------------------
# visibility
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blind", [0, 1, 2])
def test_cameras_that_see_none_of_one_level(blind, monkeypatch):
    dims = [(6, 80, 6, 8), (12, 40, 12, 16), (24, 24, 24, 32)]
    levels = [level(*d, mv=2, cams="none" if i == blind else "window") for i, d in enumerate(dims)]
    got = check(levels, monkeypatch)
    assert [o is None for o in got] == [i == blind for i in range(3)]


@pytest.mark.parametrize("mv", [0, 2])
def test_cameras_that_see_every_voxel(mv, monkeypatch):
    levels = [level(6, 80, 6, 8, mv, cams="all"), level(12, 40, 12, 16, mv, cams="all"), level(24, 24, 24, 32, mv, cams="all")]
    got = check(levels, monkeypatch)
    for lv, o in zip(levels, got):
        assert o["n_valid"] == lv["coords"].shape[0] and np.all(o["count"] == V)
        assert np.array_equal(o["coords"], lv["coords"])


def test_min_view_above_what_any_voxel_reaches(monkeypatch):
    got = check(workload_levels((V + 1, 0, V + 1)), monkeypatch)
    assert [o is None for o in got] == [True, False, True]


# ------------------------------------------------------------------------------------------------
# streams, bracket
# ------------------------------------------------------------------------------------------------
def test_prepare_on_a_side_stream(monkeypatch):
    levels = workload_levels((2, 0, 2))
    levels.insert(1, dict(level(12, 6, 7, 9), coords=None))
    same_bits(check(levels, monkeypatch, side=True), run_levels(levels, monkeypatch))


def test_the_bracket_closes_around_the_last_gather(monkeypatch):
    from eprecon_amd import _lib
    lib = _lib.load()
    levels = workload_levels()
    try:
        got = run_levels(levels, monkeypatch, bracket=True)
        ms = float(lib.eprecon_profile_gather_ms())
        assert 0.0 < ms < 50.0
        assert lib.eprecon_profile_gather_kernel() == b"bp_gather_mlp_kernel"
        # one-shot: the next step's launches — its prepare and its three gathers — leave the recorded pair alone
        same_bits(run_levels(levels, monkeypatch), got)
        assert float(lib.eprecon_profile_gather_ms()) == ms
        # armed in front of the call of the parent's form, the bracket is that level's gather again
        run_levels(levels[2:], monkeypatch, off=True, bracket=True)
        assert float(lib.eprecon_profile_gather_ms()) > 0.0 and lib.eprecon_profile_gather_kernel() == b"bp_gather_mlp_kernel"
    finally:
        lib.eprecon_profile_enable(0)


# ------------------------------------------------------------------------------------------------
# the whole step
# ------------------------------------------------------------------------------------------------
def _same_level(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert a["n_valid"] == b["n_valid"] and list(a["n_valid_per_batch"]) == list(b["n_valid_per_batch"])
    for k in ("feats", "coords", "count"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


@pytest.fixture(scope="module")
def small_step():
    """one Cfg2Step per graph setting for the whole module (the switch is read at every step): one graph capture, and the
    networks are dropped before the module's heap is collected"""
    from eprecon_amd.fragment_step import Cfg2Step
    steps = {}

    def get(graph):
        if graph not in steps:
            steps[graph] = Cfg2Step(seed=0, height=128, width=160, n_vox=(24, 24, 24))
            steps[graph].init_net.use_hip_graph = graph
        return steps[graph]
    yield get
    steps.clear()


@pytest.mark.parametrize("beside", [False, True])       # the prepare launch in front of the gathers / beside the 2D stack
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("defer", [False, True])
def test_a_whole_step_on_a_small_volume(defer, graph, beside, small_step, monkeypatch):
    from eprecon_amd import _lib
    from eprecon_amd import occupancy_initialization as OI
    from eprecon_amd import sparse as SP
    from eprecon_amd.fragment_step import LEVELS
    # (12^3 cells: below the reference's guard of 1000 valid voxels and the dense-grid fill, as in tests/test_init_glue_gpu.py)
    # Images of 160 x 128, not 160 x 120: the 2D fusion stack joins its levels by exact factors of two, so the image sides
    # have to be multiples of 16 (120 / 16 = 7.5 gives maps of 7, 15 and 30 rows, which the joins refuse under either switch).
    monkeypatch.setattr(OI, "INIT_MIN_VALID", 100)
    monkeypatch.setattr(SP, "DENSE_MIN_FILL", 0.1)
    step = small_step(graph)

    def three_steps(off):
        if off:
            monkeypatch.setenv("EPRECON_BP_LEVELS", "0")
        else:
            monkeypatch.delenv("EPRECON_BP_LEVELS", raising=False)
        step.defer_reads, step.levels_beside_2d = defer, beside
        reads0 = _lib.HOST_READS
        outs = [dict(step.run()) for _ in range(3)]
        if defer:
            assert outs[0] == {}
            outs = outs[1:] + [dict(step.flush())]
        torch.cuda.synchronize()
        step.defer_reads, step.levels_beside_2d = False, False
        return outs, _lib.HOST_READS - reads0

    want, reads_off = three_steps(True)
    got, reads_on = three_steps(False)
    assert reads_off - reads_on == 2 * 3            # one read of the three levels' counts instead of three, every step
    for g, w in zip(got, want):
        assert w["init"] is not None and torch.equal(g["stage0_coords"], w["stage0_coords"])
        assert list(g) == list(w)
        for name, _, _, mv in LEVELS:
            _same_level(g[name], w[name])
        assert w["bp96"] is not None and w["bp48"]["n_valid"] == 12 ** 3

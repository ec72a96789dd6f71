"""GPU: the count mailbox (csrc/count_mailbox.hip, _lib.MailboxRead) hands the host the very counts the kernels write to device
memory, from every publisher — the scan launch, the gather's last workgroup, the early scan of a count half, the stage-0
selection — and never changes what a call or a step computes.

Every count that came through a slot is compared with `n_valid_dev.tolist()` (or with the copy path's result), and
`MailboxRead.from_mailbox` says that it did come through the slot and not through the fallback.  "Switch off" inside this
process is the Python side of the switch (_lib._MAILBOX_ON): the library reads EPRECON_COUNT_MAILBOX once, when it is loaded, so
the environment variable itself is checked in a child process.  Scenes: tests/test_bp_levels_gpu.py's three-view 24^3 window.
"""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from test_bp_levels_gpu import _args, _dev, _host, level, same_bits  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = 2                     # back_project.MODE_VARIANCE
TILES_24 = 24 ** 3 // 16    # a 24^3 raster takes the 16-voxel tile


def raster(cams="window", mv=2, drop=0):
    """the variance call's level: the 24^3 raster (less its last `drop` entries), 3 views of 8-channel 15 x 20 maps, channels-last"""
    return level(24, 8, 15, 20, mv, drop=drop, nhwc=True, cams=cams)


def switch(monkeypatch, on):
    from eprecon_amd import _lib
    assert _lib.load().eprecon_count_mailbox() == 1        # (the suite runs with the default)
    monkeypatch.setattr(_lib, "_MAILBOX_ON", bool(on))


def ring_is_idle():
    from eprecon_amd import _lib
    gc.collect()
    torch.cuda.synchronize()
    return _lib.load().eprecon_mailbox_free_slots() == 64


def variance_call(lv, min_valid=1, side=False, read_early=False, whole=False, fold=None, monkeypatch=None):
    """the initialisation branch's call: count half (count_async), then the gather half — or the whole call (whole) -> (result
    | None, counts as result() had them, n_valid_dev.tolist(), the read object)"""
    from eprecon_amd import _lib, back_project as BP
    if fold is not None:
        monkeypatch.setenv("EPRECON_BP_FOLD", str(fold))
    coords, origin, vs, feats, kr, mv = _args(lv)
    early = None
    if whole:
        pend = BP.run_async(coords, origin, vs, feats, kr, mv, VAR, min_valid_per_batch=min_valid)
    else:
        stream = _lib.side_stream(feats.device, _lib.SIDE_SETUP) if side else None
        counted = BP.count_async(coords, origin, vs, feats.shape, kr, mv, VAR, stream=stream)
        if read_early:      # before the gather half is even queued: only the count half's own publish can answer
            assert counted.mailbox is not None and counted.early
            early = counted.mailbox.result()
            assert counted.mailbox.from_mailbox
        pend = BP.run_async(coords, origin, vs, feats, kr, mv, VAR, min_valid_per_batch=min_valid, counted=counted)
    res = pend.result()
    counts = pend._read.result()
    torch.cuda.synchronize()
    dev = pend.n_valid_dev.tolist()
    if early is not None:
        assert early == dev
    if fold is not None:
        monkeypatch.delenv("EPRECON_BP_FOLD")
    return res, counts, dev, pend._read


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("cams,n_valid", [("all", 24 ** 3), ("none", 0), ("window", None)])
def test_variance_counts_come_through_the_mailbox(cams, n_valid, whole):
    from eprecon_amd import _lib
    res, counts, dev, read = variance_call(raster(cams), whole=whole)
    assert isinstance(read, _lib.MailboxRead) and read.from_mailbox
    assert counts == dev and len(counts) == 2 and counts[0] == counts[1]
    if n_valid is not None:
        assert counts[0] == n_valid
    assert (res is None) == (counts[1] < 1)                 # ("none": the reference's `return None`)
    if res is not None:
        assert res["n_valid"] == dev[0] and res["feats"].shape[0] == dev[0]


def test_two_batch_elements_publish_three_words():
    from eprecon_amd import _lib, back_project as BP
    lv = raster("all")
    coords, origin, vs, feats, kr, mv = _args(lv)
    n = coords.shape[0]
    half = n // 2 + 3                                       # (not a multiple of the tile or of the count workgroup)
    coords = coords.clone()
    coords[half:, 0] = 1
    feats2 = torch.cat([feats, feats.flip(0)], dim=1).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    pend = BP.run_async(coords, origin.repeat(2, 1), vs, feats2, kr.repeat(1, 2, 1, 1).contiguous(), mv, VAR, min_valid_per_batch=0)
    res = pend.result()
    torch.cuda.synchronize()
    dev = pend.n_valid_dev.tolist()
    assert isinstance(pend._read, _lib.MailboxRead) and pend._read.from_mailbox and pend._read.slot.words == 3
    assert pend._read.result() == dev == [n, half, n - half]
    assert res["n_valid_per_batch"] == dev[1:]


def test_one_tile():
    from eprecon_amd import _lib
    res, counts, dev, read = variance_call(raster("all", drop=24 ** 3 - 10))
    assert isinstance(read, _lib.MailboxRead) and read.from_mailbox and counts == dev == [10, 10]
    assert res["n_valid"] == 10


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("cap", [TILES_24 + 1, TILES_24, TILES_24 - 1])     # tiles = cap - 1, cap, cap + 1
def test_both_publishers_around_the_fold_cap(cap, whole, monkeypatch):
    """at and below the cap the gather folds the scan in (its last workgroup publishes; a count half publishes through the early
    scan, which must leave the tile totals raw); one tile above, the scan launch publishes"""
    from eprecon_amd import _lib
    want = variance_call(raster("window"), whole=True)
    res, counts, dev, read = variance_call(raster("window"), whole=whole, fold=cap, monkeypatch=monkeypatch)
    assert isinstance(read, _lib.MailboxRead) and read.from_mailbox and counts == dev == want[2]
    same_bits([_host(res)], [_host(want[0])])


def test_an_empty_list_takes_the_copy_path():
    from eprecon_amd import _lib
    lv = raster("all")
    lv["coords"] = lv["coords"][:0]
    for whole in (False, True):
        res, counts, dev, read = variance_call(lv, whole=whole)
        assert isinstance(read, _lib.PinnedRead) and counts == dev == [0, 0] and res is None


def test_count_half_on_a_side_stream_is_read_before_the_gather_is_queued():
    from eprecon_amd import _lib
    want = variance_call(raster("window"), whole=True)
    res, counts, dev, read = variance_call(raster("window"), side=True, read_early=True)
    assert isinstance(read, _lib.MailboxRead) and counts == dev == want[2]
    same_bits([_host(res)], [_host(want[0])])


def _three_levels():
    from eprecon_amd import back_project as BP
    levels = [level(4, 80, 6, 8, 2, drop=0), level(8, 40, 12, 16, 0, drop=0), level(16, 24, 24, 32, 0, drop=0)]
    args = [_args(lv) for lv in levels]
    handles = BP.prepare_levels_async(args)
    pends = [BP.run_async(*a[:3], hd.nhwc, *a[4:], hold_read=True, counted=hd) for a, hd in zip(args, handles)]
    read = BP.PendingLevels(pends, handles)
    out = [_host(r) for r in read.results()]
    torch.cuda.synchronize()
    return out, read, [p.n_valid_dev.tolist() for p in pends]


def test_three_levels_read_one_slot_each(monkeypatch):
    switch(monkeypatch, True)
    on, read, dev = _three_levels()
    assert read._read is None and all(m.from_mailbox for m in read._slots)
    assert [m.result() for m in read._slots] == dev
    switch(monkeypatch, False)
    off, read_off, dev_off = _three_levels()
    assert read_off._read is not None and dev_off == dev
    same_bits(on, off)
    assert on[1]["n_valid"] == 8 ** 3 and on[2]["n_valid"] == 16 ** 3        # (min_view 0: every voxel)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("case", ["no mark", "every mark", "threshold"])
def test_selection_on_a_12_cubed_grid(case, dense, monkeypatch):
    from eprecon_amd import _lib, grid_ops as GO, sparse as SP
    xyz = np.argwhere(np.ones((12, 12, 12), bool)) * 2
    coords = _dev(np.concatenate([np.zeros((len(xyz), 1), int), xyz], 1).astype(np.int32))
    t = float(np.log(0.3 / 0.7))                            # sigmoid(t) = 0.3, the threshold
    if case == "threshold":     # logits on both sides of the threshold: above it in the cells with x < 16, below elsewhere
        logit = np.where(xyz[:, 0] < 16, t + 1e-3, t - 1e-3).astype(np.float32)
    else:
        logit = np.full(len(xyz), 5.0 if case == "every mark" else -5.0, np.float32)
    logit = _dev(logit)

    def select(on):
        switch(monkeypatch, on)
        dm = SP.DenseMap(SP.VoxelSet(coords, 2, dims=(12, 12, 12)), (12, 12, 12)) if dense else None
        torch.cuda.synchronize()
        _lib.take_deferred(None)                            # (the map's own off-grid check is not what is under test)
        pend = GO.init_select_async(logit, coords, 1, dim=6, cell=4, dense=dm)
        assert isinstance(pend._read, _lib.MailboxRead if on else _lib.PinnedRead)
        sel, per_batch = pend.result()
        assert not on or pend._read.from_mailbox
        return sel.cpu().numpy(), per_batch

    got, want = select(True), select(False)
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes() and got[0].shape[0] == got[1][0]
    assert got[1][0] == {"no mark": 0, "every mark": 6 ** 3}.get(case, got[1][0]) and (case != "threshold" or 0 < got[1][0] < 6 ** 3)


def _short_read(k):
    """a back-projection of the raster's first k entries that every camera sees: n_valid = k"""
    from eprecon_amd import back_project as BP
    if "lv" not in _short:
        _short["lv"] = _args(raster("all", mv=1))
    coords, origin, vs, feats, kr, mv = _short["lv"]
    return BP.run_async(coords[:k], origin, vs, feats, kr, mv, VAR, min_valid_per_batch=0)


_short = {}


def test_ring_wraps_around():
    from eprecon_amd import _lib
    assert ring_is_idle()
    slots, seqs = [], {}
    for i in range(200):
        k = 1 + (i * 37) % 500
        pend = _short_read(k)
        assert isinstance(pend._read, _lib.MailboxRead)
        s = pend._read.slot
        assert s.seq != 0 and s.seq > seqs.get(s.index, 0)                 # rises per slot
        seqs[s.index] = s.seq
        slots.append(s.index)
        assert pend.result()["n_valid"] == k and pend._read.from_mailbox
    assert len(set(slots)) == 64 and len(slots) > 3 * 64                    # every slot, several times over
    assert ring_is_idle()


def test_dropped_reads_give_their_slots_back():
    from eprecon_amd import _lib
    assert ring_is_idle()
    for i in range(70):
        pend = _short_read(20 + i)     # never read: its slot drains until its publisher has stored, and then is free again
        del pend
    pend = _short_read(7)              # (a slot, or the copy path while the 70 are still draining: right either way)
    assert pend.result()["n_valid"] == 7
    del pend
    assert ring_is_idle()
    pend = _short_read(9)
    assert isinstance(pend._read, _lib.MailboxRead) and pend.result()["n_valid"] == 9 and pend._read.from_mailbox


def test_the_65th_held_read_takes_the_copy_path():
    from eprecon_amd import _lib
    assert ring_is_idle()
    held = [_short_read(100 + i) for i in range(65)]
    assert all(isinstance(p._read, _lib.MailboxRead) for p in held[:64]) and isinstance(held[64]._read, _lib.PinnedRead)
    assert _lib.load().eprecon_mailbox_free_slots() == 0
    assert [p.result()["n_valid"] for p in held] == [100 + i for i in range(65)]
    del held
    assert ring_is_idle()


def test_wait_times_out_on_a_slot_nobody_publishes():
    """host-only waiting: no kernel is involved"""
    import ctypes
    import time
    from eprecon_amd import _lib
    lib = _lib.load()
    assert ring_is_idle()
    slot, out = _lib.MailboxSlot(), (ctypes.c_int32 * 2)()
    assert lib.eprecon_mailbox_acquire(2, ctypes.byref(slot)) == _lib.EPRECON_OK and slot.seq != 0
    t0 = time.perf_counter()
    assert lib.eprecon_mailbox_wait(ctypes.byref(slot), 1000, out) == _lib.EPRECON_ERR_TIMEOUT
    assert 1e-3 <= time.perf_counter() - t0 < 0.5
    assert lib.eprecon_mailbox_release(ctypes.byref(slot)) == _lib.EPRECON_OK          # (never armed: free at once)
    assert lib.eprecon_mailbox_release(ctypes.byref(slot)) == -1                       # (and only once)
    assert lib.eprecon_mailbox_free_slots() == 64
    assert lib.eprecon_mailbox_acquire(16, ctypes.byref(slot)) == _lib.EPRECON_EMPTY   # more than a slot holds: the copy path


def test_a_pending_deferred_check_is_verified_through_the_fallback():
    from eprecon_amd import _lib
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    _lib.defer_check(one, 1, "a check that holds")
    pend = _short_read(5)
    assert isinstance(pend._read, _lib.PinnedRead)          # not stranded: this read takes it along
    assert pend.result()["n_valid"] == 5 and not _lib.has_deferred()
    _lib.defer_check(one, 0, "a check that fails")
    pend = _short_read(5)
    with pytest.raises(_lib.EpreconError, match="a check that fails"):
        pend.result()
    pend = _short_read(6)                                   # nothing pending any more: the mailbox again
    assert isinstance(pend._read, _lib.MailboxRead) and pend.result()["n_valid"] == 6


def _same_step(a, b):
    assert list(a) == list(b) and a["init"] is not None
    assert torch.equal(a["stage0_coords"], b["stage0_coords"])
    for x, y in zip(a["init"], b["init"]):
        assert torch.equal(x, y)
    for lvl in ("bp24", "bp48", "bp96"):
        assert (a[lvl] is None) == (b[lvl] is None)
        if a[lvl] is not None:
            assert a[lvl]["n_valid"] == b[lvl]["n_valid"] and a[lvl]["n_valid_per_batch"] == b[lvl]["n_valid_per_batch"]
            for k in ("feats", "coords", "count"):
                assert torch.equal(a[lvl][k], b[lvl][k]), (lvl, k)


@pytest.fixture(scope="module")
def small_step():
    from eprecon_amd.fragment_step import Cfg2Step
    steps = {}

    def get(graph):
        if graph not in steps:
            steps[graph] = Cfg2Step(seed=0, height=128, width=160, n_vox=(24, 24, 24))
            steps[graph].init_net.use_hip_graph = graph
        return steps[graph]
    yield get
    steps.clear()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("defer", [False, True])
def test_a_whole_step_on_a_small_volume(defer, graph, small_step, monkeypatch):
    from eprecon_amd import _lib
    from eprecon_amd import occupancy_initialization as OI
    from eprecon_amd import sparse as SP
    monkeypatch.setattr(OI, "INIT_MIN_VALID", 100)          # (12^3 cells: as tests/test_bp_levels_gpu.py's whole step)
    monkeypatch.setattr(SP, "DENSE_MIN_FILL", 0.1)
    step = small_step(graph)

    def three_steps(on):
        switch(monkeypatch, on)
        step.defer_reads = defer
        reads0 = _lib.HOST_READS
        outs = [dict(step.run()) for _ in range(3)]
        if defer:
            assert outs[0] == {}
            outs = outs[1:] + [dict(step.flush())]
        torch.cuda.synchronize()
        step.defer_reads = False
        return outs, _lib.HOST_READS - reads0

    assert ring_is_idle()
    want, reads_off = three_steps(False)
    assert _lib.load().eprecon_mailbox_free_slots() == 64   # (switch off: no slot was touched)
    got, reads_on = three_steps(True)
    assert reads_on == reads_off == 3 * 3                   # the three host round trips of a step stay three
    for g, w in zip(got, want):
        _same_step(g, w)
    assert ring_is_idle()


CHILD = """
import sys, hashlib
sys.path[:0] = [{root!r}, {tests!r}]
import torch
from eprecon_amd import _lib, back_project as BP
from test_count_mailbox_gpu import raster, variance_call
assert _lib.load().eprecon_count_mailbox() == {want}
assert (_lib.mailbox_read(2) is not None) == bool({want})
res, counts, dev, read = variance_call(raster("window"))
assert isinstance(read, _lib.MailboxRead if {want} else _lib.PinnedRead) and counts == dev
print("DIGEST", counts, hashlib.sha256(res["feats"].cpu().numpy().tobytes() + res["coords"].cpu().numpy().tobytes()).hexdigest())
"""


def test_the_environment_switch_restores_the_copies(tmp_path):
    """EPRECON_COUNT_MAILBOX=0 is read when the library is loaded: a child process of its own, one small variance call"""
    import hashlib
    res, counts, dev, read = variance_call(raster("window"))
    want = f"DIGEST {counts} " + hashlib.sha256(res["feats"].cpu().numpy().tobytes() + res["coords"].cpu().numpy().tobytes()).hexdigest()
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), want=0))
    out = subprocess.run([sys.executable, str(script)], env={**os.environ, "EPRECON_COUNT_MAILBOX": "0"}, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert want in out.stdout

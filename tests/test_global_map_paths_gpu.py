"""The two host paths of the global map (csrc/global_map*.hip) on the branches their shared steps own: reallocation inside the
replace step, an empty map, an empty fragment, kept == 0, kept == size, a ground-truth twin that appends nothing.

A walk of seven 24^3 fragments is run once on the queued stage call (GlobalMap.stage_begin -> read -> update) and once on the
separate blocking calls (crop_union, gathers, target_fuse, update), on fresh maps with ground truth attached.  After every
fragment the two runs are compared byte for byte and both against oracle/gru_fusion.py (identity fusion, the reference's row
order cat([old[outside], new])).  The oracle alone is checked, on the CPU, to produce every event the walk is built for; the
GPU tests assert the same events on the handles, so a later edit of the walk cannot pass by skipping one."""
import ctypes

import numpy as np
import pytest

from oracle import gru_fusion as OGF

DIM, C, CHV = 24, 3, 2
# relative origin per fragment: 16 voxels along x each, except 1 (the origin of 0: the whole map is inside), 5 (far from every
# row) and 6 (back where 5 would have been)
RELS = [(0, 0, 0), (0, 0, 0), (16, 0, 0), (32, 0, 0), (48, 0, 0), (64, 500, -500), (64, 0, 0)]
EMPTY_FRAGMENT, BLANK_GT, FAR = 3, 4, 5


def walk():
    rng = np.random.default_rng(2015)
    frags = []
    for k, rel in enumerate(RELS):
        xyz = np.argwhere(rng.random((DIM, DIM, DIM)) < 0.5)                     # ~6,900 rows, ~5,900 of them active
        rng.shuffle(xyz)
        if k == EMPTY_FRAGMENT:
            xyz = xyz[:0]
        vals = rng.standard_normal((len(xyz), C)).astype(np.float32)
        vals[rng.random(len(xyz)) < 0.15] = 0.0                                   # all-zero rows do not activate a voxel
        tsdf = np.clip(rng.standard_normal((DIM, DIM, DIM)) * 0.8, -1, 1).astype(np.float32)
        occ = (np.abs(tsdf) < 0.999) & (rng.random((DIM, DIM, DIM)) < 0.5)
        if k == BLANK_GT:                                                         # every cell overwritten by |tsdf| = 1
            tsdf, occ = np.ones_like(tsdf), np.ones_like(occ)
        frags.append({"coords": np.concatenate([np.zeros((len(xyz), 1), np.int64), xyz], 1).astype(np.int32), "values": vals,
                      "tsdf": tsdf, "occ": occ, "rel": np.array(rel, np.int64)})
    return frags


@pytest.fixture(scope="module")
def reference():
    """the oracle's walk, computed once: per fragment the result dict plus both maps before and after, and the stamps the
    handle keeps beside the rows (fragment + 1 for the rows a fragment appended; carried by the compaction)"""
    frags = walk()
    st = OGF.ScaleState(C, np.zeros(3, np.float32))
    stamps = np.zeros(0, np.int32)
    steps = []
    for k, fr in enumerate(frags):
        before = {"C": st.C, "F": st.F, "tC": st.tC, "tF": st.tF}
        # base_voxel = 1: the origin in voxels IS the relative origin (no rounding of a metric origin in between)
        r = OGF.fuse_fragment(st, fr["coords"], fr["values"], fr["rel"].astype(np.float32), fr["tsdf"], fr["occ"], 1, DIM, base_voxel=1.0)
        assert np.array_equal(r["rel"], fr["rel"])
        t_inside = ((before["tC"] - fr["rel"] >= 0) & (before["tC"] - fr["rel"] < DIM)).all(1)
        stamps = np.concatenate([stamps[~r["valid"]], np.full(len(r["updated"]), k + 1, np.int32)])
        steps.append({"r": r, "before": before, "C": st.C, "F": st.F, "tC": st.tC, "tF": st.tF, "stamps": stamps,
                      "kept": int((~r["valid"]).sum()), "t_kept": int((~t_inside).sum()),
                      "t_new": len(st.tC) - int((~t_inside).sum())})
    return frags, steps


def check_events(frags, steps, sizes, t_sizes, kept):
    """the six events, on row counts: sizes[k] / t_sizes[k] = rows of the feature map / the twin BEFORE fragment k (one more entry
    for the end), kept[k] = feature rows outside fragment k's volume; taken from the oracle by the CPU test and from the handles
    (size, and size minus the rows the crop reported inside) by the GPU test"""
    # 1. the first fragment goes into empty maps
    assert sizes[0] == 0 and t_sizes[0] == 0 and sizes[1] > 0 and t_sizes[1] > 0
    # 2. the feature map crosses 4,096 rows and LATER 8,192 (two reallocations inside the replace step, the second with live rows
    #    to carry over); the twin crosses 4,096
    first = next(k for k in range(len(steps)) if sizes[k] <= 4096 < sizes[k + 1])
    assert any(sizes[k] <= 8192 < sizes[k + 1] for k in range(first + 1, len(steps)))
    assert any(t_sizes[k] <= 4096 < t_sizes[k + 1] for k in range(len(steps)))
    # 3. an empty fragment: the union is exactly the map rows inside the volume
    k = EMPTY_FRAGMENT
    r, b = steps[k]["r"], steps[k]["before"]
    assert len(frags[k]["coords"]) == 0 and 0 < len(r["updated"]) == sizes[k] - kept[k]
    assert sorted(map(tuple, r["updated"] + r["rel"])) == sorted(map(tuple, b["C"][r["valid"]]))
    # 4. the same origin as the predecessor while the whole map is inside the volume: nothing is kept
    assert tuple(RELS[1]) == tuple(RELS[0]) and sizes[1] > 0 and kept[1] == 0
    # 5. an origin far from every row: everything is kept, in both maps
    assert kept[FAR] == sizes[FAR] > 8192 and steps[FAR]["t_kept"] == t_sizes[FAR] > 0
    # 6. ground truth without a cell of |tsdf| < 1: the twin appends nothing (and drops the rows it had inside the volume)
    assert steps[BLANK_GT]["t_new"] == 0 and 0 < t_sizes[BLANK_GT + 1] == steps[BLANK_GT]["t_kept"] < t_sizes[BLANK_GT]
    # and the ordinary case in between: some rows kept, some replaced
    assert 0 < kept[2] < sizes[2] and 0 < kept[6] < sizes[6]


def test_oracle_walk_contains_every_event(reference):
    frags, steps = reference
    sizes = [len(s["before"]["C"]) for s in steps] + [len(steps[-1]["C"])]
    t_sizes = [len(s["before"]["tC"]) for s in steps] + [len(steps[-1]["tC"])]
    check_events(frags, steps, sizes, t_sizes, [s["kept"] for s in steps])
    assert all(5000 < (f["values"] != 0).any(1).sum() < 7000 for k, f in enumerate(frags) if k != EMPTY_FRAGMENT)


def run_walk(frags, staged):
    """-> per fragment: dict of host arrays (outputs, both maps, stamps) and the row counts before the fragment"""
    import torch
    from eprecon_amd.global_map import GlobalMap
    from eprecon_amd.gru_fusion import gather_rows
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gm, tm = GlobalMap(C, dev), GlobalMap(1, dev)
    w2ac = np.eye(4, dtype=np.float32)
    w2ac[:3, :3] = np.array([[0.8, 0.6, 0], [-0.6, 0.8, 0], [0, 0, 1]], np.float32)
    origin, w2ac = up(np.array([-0.96, 0.2, -0.4], np.float32)), up(w2ac)
    out = []
    for k, fr in enumerate(frags):
        sizes = (gm.size, tm.size)
        gm.set_fragment(k)
        cur_c, cur_f, rel = up(fr["coords"]), up(fr["values"]), fr["rel"].tolist()
        tsdf, occ = up(fr["tsdf"]), up(fr["occ"])
        chi = C - CHV
        if staged:
            st = gm.stage_begin(tm, cur_c, cur_f, DIM, 1, rel, tsdf, occ, origin, w2ac, 0.04, 0.04, CHV).read()
            updated, hx_v, hx_i, tsdf_t, inside = st.updated, st.hx_v, st.hx_i, st.tsdf_target, st.n_inside
        else:
            updated, src_cur, src_glob, inside = gm.crop_union(cur_c, cur_f, DIM, 1, rel)
            n_u = updated.shape[0]
            hx_v = torch.empty((n_u, 2 * CHV), dtype=torch.float32, device=dev)
            hx_i = torch.empty((n_u, 2 * chi), dtype=torch.float32, device=dev)
            gm.gather(src_glob, 0, CHV, hx_v[:, :CHV])
            gm.gather(src_glob, CHV, chi, hx_i[:, :chi])
            gather_rows(cur_f[:, :CHV], src_cur, CHV, out=hx_v[:, CHV:])
            gather_rows(cur_f[:, CHV:], src_cur, chi, out=hx_i[:, chi:])
            tsdf_t = tm.target_fuse(tsdf, occ, DIM, rel, updated)
        values = torch.cat([hx_v[:, CHV:], hx_i[:, chi:]], 1).contiguous()        # identity fusion: the fragment's rows
        gm.update(updated, values)
        (mc, mf), (tc, tf) = gm.export(), tm.export()
        got = {"updated": updated, "values": values, "h": torch.cat([hx_v[:, :CHV], hx_i[:, :chi]], 1), "tsdf_target": tsdf_t,
               "occ_target": tsdf_t.abs() < 1, "C": mc, "F": mf, "tC": tc, "tF": tf, "stamps": gm.stamps()}
        got = {name: t.cpu().numpy() for name, t in got.items()}
        got.update(sizes=sizes, inside=inside)
        out.append(got)
    out.append({"sizes": (gm.size, tm.size)})
    return out


@pytest.mark.gpu
def test_walk_on_both_paths_and_against_the_oracle(reference):
    frags, steps = reference
    a, b = run_walk(frags, staged=True), run_walk(frags, staged=False)
    for run in (a, b):
        check_events(frags, steps, [g["sizes"][0] for g in run], [g["sizes"][1] for g in run],
                     [g["sizes"][0] - g["inside"] for g in run[:-1]])
    for k, (x, y, s) in enumerate(zip(a, b, steps)):
        r = s["r"]
        for name in ("updated", "values", "h", "tsdf_target", "occ_target", "C", "F", "tC", "tF", "stamps"):
            assert x[name].dtype == y[name].dtype and x[name].shape == y[name].shape, (k, name)
            assert x[name].tobytes() == y[name].tobytes(), (k, name)
        assert x["inside"] == y["inside"] == int(r["valid"].sum())
        for name, want in (("updated", r["updated"]), ("values", r["fused"]), ("h", r["global_values"]), ("tsdf_target", r["tsdf_target"]),
                           ("occ_target", r["occ_target"]), ("C", s["C"]), ("F", s["F"]), ("tC", s["tC"]), ("tF", s["tF"]),
                           ("stamps", s["stamps"])):
            assert x[name].shape == want.shape and np.array_equal(x[name], want), (k, name)


@pytest.mark.gpu
def test_pending_crop_state_machine():
    """update needs a crop whose count the host holds; commit needs a queued stage; a refused call leaves the map as it was"""
    import torch
    from eprecon_amd import _lib
    from eprecon_amd.global_map import GlobalMap
    dev = torch.device("cuda")
    rng = np.random.default_rng(5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gm = GlobalMap(C, dev)
    rows = np.unique(rng.integers(0, 12, (200, 3)), axis=0).astype(np.int32)
    feats = rng.standard_normal((len(rows), C)).astype(np.float32)
    gm.set(up(rows), up(feats))

    def unchanged():
        c, f = gm.export()
        return gm.size == len(rows) and np.array_equal(c.cpu().numpy(), rows) and np.array_equal(f.cpu().numpy(), feats)

    upd, vals = up(np.zeros((4, 3), np.int32)), up(np.ones((4, C), np.float32))
    with pytest.raises(_lib.EpreconError):                                        # no crop pending
        gm.update(upd, vals)
    assert unchanged()
    counts = (ctypes.c_int32 * 8)(4, 0, 0, 0, 0, 0, 0, 0)
    rc = _lib.load().eprecon_gru_stage_commit_async(gm._h, None, ctypes.cast(counts, ctypes.c_void_p), _lib.current_stream())
    assert rc == -1 and unchanged()                                               # EPRECON_ERR_ARG: no stage was begun
    cur = np.concatenate([np.zeros((4, 1), np.int32), np.arange(12, dtype=np.int32).reshape(4, 3)], 1)
    st = gm.stage_begin(None, up(cur), up(np.ones((4, C), np.float32)), 12, 1, [0, 0, 0], None, None,
                        up(np.zeros(3, np.float32)), up(np.eye(4, dtype=np.float32)), 0.04, 0.04, CHV)
    with pytest.raises(_lib.EpreconError):                                        # pending, its count still on the device
        gm.update(upd, vals)
    assert unchanged()
    st.read()                                                                     # the refused calls did not disturb the crop
    gm.update(st.updated, torch.ones((st.n, C), device=dev))
    assert gm.size == st.n and st.n_inside == len(rows)                           # (the whole map was inside the 12^3 volume)

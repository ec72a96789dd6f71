"""Restatement of the panoptic scoring rules with Python sets, dicts and loops in int64 / float64.  It shares
no code with eprecon_amd/panoptic_score.py: labels are Python tuples per site, the table is filled one site at a time, the
voxel domain enumerates the lattice cell by cell.

A site's prediction is None (nothing predicted) or a segment key (class, instance); its ground truth is None (no ground
truth here), "void" or a segment key.  A stuff class has instance 0 in its key.
"""
import math

import numpy as np

MAPPING = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
VALID = MAPPING[1:]
STUFF = (1, 2)


def _key(cls, ins):
    return (int(cls), 0) if int(cls) in STUFF else (int(cls), int(ins))


def pred_labels(class_index, instance, mapping=MAPPING):
    """class indices of the network -> per site None or a key"""
    out = []
    for s, i in zip(np.asarray(class_index).reshape(-1).tolist(), np.asarray(instance).reshape(-1).tolist()):
        c = mapping[int(s)] if mapping is not None else int(s)
        out.append(None if c == 0 or c not in VALID else _key(c, i))
    return out


def gt_labels(sem, instance):
    """ScanNet ids -> per site "void" or a key"""
    return ["void" if int(s) not in VALID else _key(s, i)
            for s, i in zip(np.asarray(sem).reshape(-1).tolist(), np.asarray(instance).reshape(-1).tolist())]


def contingency(pred, gt):
    """-> (M int64[P + 1, G + 2], predicted keys ascending, ground-truth keys ascending)"""
    assert len(pred) == len(gt)
    pkeys = sorted({p for p in pred if p is not None})
    gkeys = sorted({g for g in gt if g is not None and g != "void"})
    row, col = {k: r for r, k in enumerate(pkeys)}, {k: r for r, k in enumerate(gkeys)}
    P, G = len(pkeys), len(gkeys)
    M = np.zeros((P + 1, G + 2), np.int64)
    for p, g in zip(pred, gt):
        M[P if p is None else row[p], G + 1 if g is None else (G if g == "void" else col[g])] += 1
    return M, pkeys, gkeys


def table_of_ranks(pred_rank, gt_rank, n_pred, n_gt):
    """the table of two rank lists, one site at a time -> (M, sites skipped because a rank is outside its range)"""
    M, skipped = np.zeros((n_pred + 1, n_gt + 2), np.int64), 0
    for p, g in zip(np.asarray(pred_rank).reshape(-1).tolist(), np.asarray(gt_rank).reshape(-1).tolist()):
        if not (-1 <= p < n_pred and -1 <= g <= n_gt):
            skipped += 1
            continue
        M[n_pred if p == -1 else p, n_gt + 1 if g == -1 else g] += 1
    return M, skipped


def match(M, pred_classes, gt_classes, threshold=0.5):
    """-> {class: [tp, fp, fn, iou_sum]} over VALID, list of (p, g, iou), set of ignored predicted ranks"""
    P, G = len(pred_classes), len(gt_classes)
    assert M.shape == (P + 1, G + 2)
    cand = []
    for p in range(P):
        size_p = sum(int(M[p, c]) for c in range(G + 2))
        for g in range(G):
            if pred_classes[p] != gt_classes[g] or M[p, g] == 0:
                continue
            size_g = sum(int(M[r, g]) for r in range(P + 1))
            iou = float(int(M[p, g])) / float(size_p + size_g - int(M[p, g]) - int(M[p, G]))
            if iou > threshold:
                cand.append((-iou, g, p))
    used_p, used_g, taken = set(), set(), []
    for neg, g, p in sorted(cand):
        if p not in used_p and g not in used_g:
            used_p.add(p), used_g.add(g)
            taken.append((p, g, -neg))
    ignored = {p for p in range(P) if p not in used_p and int(M[p, G]) / sum(int(v) for v in M[p]) > 0.5}
    per = {c: [0, 0, 0, 0.0] for c in VALID}
    for p, g, iou in taken:
        per[int(pred_classes[p])][0] += 1
        per[int(pred_classes[p])][3] += iou
    for p in range(P):
        if p not in used_p and p not in ignored:
            per[int(pred_classes[p])][1] += 1
    for g in range(G):
        if g not in used_g:
            per[int(gt_classes[g])][2] += 1
    return per, taken, ignored


def semantic_counts(pred, gt):
    """from the sites, not from the table -> {class: [tp, fp, fn]} over VALID"""
    out = {c: [0, 0, 0] for c in VALID}
    for p, g in zip(pred, gt):
        if g == "void":
            continue
        pc, gc = (None if p is None else p[0]), (None if g is None else g[0])
        if pc is not None and pc == gc:
            out[pc][0] += 1
        else:
            if pc is not None:
                out[pc][1] += 1
            if gc is not None:
                out[gc][2] += 1
    return out


def score(pred, gt, threshold=0.5):
    """one scene from its site labels -> {"M", "pred_keys", "gt_keys", "per" {class: [tp, fp, fn, iou_sum]}, "sem"
    {class: [tp, fp, fn]}, "matches", "ignored"}"""
    M, pkeys, gkeys = contingency(pred, gt)
    per, taken, ignored = match(M, [k[0] for k in pkeys], [k[0] for k in gkeys], threshold)
    return {"M": M, "pred_keys": pkeys, "gt_keys": gkeys, "per": per, "sem": semantic_counts(pred, gt), "matches": taken,
            "ignored": ignored}


def summary(scenes, threshold=0.5):
    """pooled over the scenes (results of `score`), in the layout PanopticScore.summary() returns"""
    out = {"threshold": float(threshold), "scenes": len(scenes), "classes": {}}
    groups = {"all": [], "things": [], "stuff": []}
    ious = []
    for c in VALID:
        tp = sum(s["per"][c][0] for s in scenes)
        fp = sum(s["per"][c][1] for s in scenes)
        fn = sum(s["per"][c][2] for s in scenes)
        iou_sum = math.fsum(s["per"][c][3] for s in scenes)
        s_tp, s_fp, s_fn = (sum(s["sem"][c][k] for s in scenes) for k in range(3))
        row = {"tp": tp, "fp": fp, "fn": fn, "iou_sum": iou_sum, "pq": None, "sq": None, "rq": None, "sem_tp": s_tp,
               "sem_fp": s_fp, "sem_fn": s_fn, "iou": None}
        if tp + fp + fn > 0:
            row["pq"] = iou_sum / (tp + 0.5 * fp + 0.5 * fn)
            row["sq"] = iou_sum / tp if tp else 0.0
            row["rq"] = tp / (tp + 0.5 * fp + 0.5 * fn)
            groups["all"].append(row)
            groups["stuff" if c in STUFF else "things"].append(row)
        if s_tp + s_fp + s_fn > 0:
            row["iou"] = s_tp / (s_tp + s_fp + s_fn)
            ious.append(row["iou"])
        out["classes"][str(c)] = row
    for name, rows in groups.items():
        out[name] = {"n": len(rows)}
        for k in ("pq", "sq", "rq"):
            out[name][k] = math.fsum(r[k] for r in rows) / len(rows) if rows else None
    out["miou"] = math.fsum(ious) / len(ious) if ious else None
    return out


def assert_tables_equal(tables, scene, tol=1e-12):
    """a SceneTables of the module against a `score` of this file: every integer exactly, the IoU sums to `tol`"""
    assert tables.counts.dtype == np.int64 and tables.counts.shape == scene["M"].shape, (tables.counts.shape, scene["M"].shape)
    assert (tables.counts == scene["M"]).all(), (tables.counts, scene["M"])
    assert tables.classes == tuple(VALID)
    if tables.pred_keys is not None:
        assert [tuple(k) for k in tables.pred_keys.tolist()] == scene["pred_keys"]
        assert [tuple(k) for k in tables.gt_keys.tolist()] == scene["gt_keys"]
    for k, c in enumerate(tables.classes):
        assert [int(tables.tp[k]), int(tables.fp[k]), int(tables.fn[k])] == scene["per"][c][:3], c
        assert abs(tables.iou_sum[k] - scene["per"][c][3]) <= tol, c
        assert [int(tables.sem_tp[k]), int(tables.sem_fp[k]), int(tables.sem_fn[k])] == scene["sem"][c], c
    assert sorted((p, g) for p, g, _ in tables.matches) == sorted((p, g) for p, g, _ in scene["matches"])
    assert set(tables.ignored) == scene["ignored"]


def assert_summaries_equal(got, want, tol=1e-12):
    """integers and None exactly, floats to `tol` (exact rationals; the float64 error of a few hundred terms in [0, 1])"""
    assert type(got) is type(want) or {type(got), type(want)} <= {int, float}, (got, want)
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        for k in want:
            assert_summaries_equal(got[k], want[k], tol)
    elif isinstance(want, float) or isinstance(got, float):
        assert abs(got - want) <= tol, (got, want)
    else:
        assert got == want, (got, want)


# ------------------------------------------------------------------------------------------------------------ voxel domain

def _axis(n_p, o_p, vs_p, n_g, o_g, vs_g, guard):
    """one axis -> (first k, last k of the lattice, {k: ground-truth cell j or None}).  k runs generously past both boxes;
    with `guard`, no site may lie within that many cells of a rounding decision."""
    o_p, o_g = np.float64(np.float32(o_p)), np.float64(np.float32(o_g))
    near = int(math.floor((o_g - o_p) / vs_p))
    cell = {}
    for k in range(min(-4, near - 4), max(n_p, near + n_g) + 5):
        t = (o_p + np.float64(k) * np.float64(vs_p) - o_g) / np.float64(vs_g) + np.float64(0.5)
        if guard is not None:
            assert abs(t - round(t)) > guard, (k, t)
        j = int(math.floor(t))
        cell[k] = j if 0 <= j < n_g else None
    hit = [k for k, j in cell.items() if j is not None]
    assert sorted(cell[k] for k in hit) == list(range(n_g)), "sites and ground-truth cells do not correspond one to one"
    return min(0, min(hit)), max(n_p - 1, max(hit)), cell


def voxel_labels(pred_sem, pred_ins, origin_p, vs_p, gt_tsdf, gt_sem, gt_ins, origin_g, vs_g, gt_surface=1.0, mapping=MAPPING,
                 guard=None):
    """lattice enumeration -> (pred labels, ground-truth labels) per site, x slowest and z fastest"""
    pred_sem, pred_ins, gt_tsdf, gt_sem, gt_ins = (np.asarray(a) for a in (pred_sem, pred_ins, gt_tsdf, gt_sem, gt_ins))
    axes = [_axis(pred_sem.shape[a], origin_p[a], vs_p, gt_sem.shape[a], origin_g[a], vs_g, guard) for a in range(3)]
    pred, gt = [], []
    for x in range(axes[0][0], axes[0][1] + 1):
        for y in range(axes[1][0], axes[1][1] + 1):
            for z in range(axes[2][0], axes[2][1] + 1):
                k = (x, y, z)
                if all(0 <= k[a] < pred_sem.shape[a] for a in range(3)):
                    pred.extend(pred_labels([pred_sem[k]], [pred_ins[k]], mapping))
                else:
                    pred.append(None)
                j = tuple(axes[a][2][k[a]] for a in range(3))
                if None in j or not np.abs(np.float32(gt_tsdf[j])) < np.float32(gt_surface):
                    gt.append(None)
                else:
                    gt.extend(gt_labels([gt_sem[j]], [gt_ins[j]]))
    return pred, gt


# ------------------------------------------------------------------------------------------------------ the worked strip

def strip():
    """the 40 sites of the issue's table -> (pred labels, gt labels)"""
    gt = [(1, 0)] * 10 + [(5, 3)] * 10 + [(5, 4)] * 6 + ["void"] * 6 + [None] * 8
    pred = [None] * 40
    for lo, hi, key in ((0, 11, (1, 0)), (12, 19, (5, 7)), (22, 23, (5, 8)), (26, 30, (7, 9)), (32, 35, (7, 10))):
        for s in range(lo, hi + 1):
            pred[s] = key
    return pred, gt

"""Panoptic scoring of a saved scene: PQ, SQ, RQ per class (all / things / stuff) and semantic IoU / mIoU.

    python -m eprecon_amd.panoptic_score --pred DIR --scenes FILE (--gt DIR | --info DIR) [--threshold 0.5] [--out FILE]
    python -m eprecon_amd.panoptic_score --pred DIR --scenes FILE --views DATA_PATH --info DIR --gt_mesh DIR [--every 10]
                                         [--size W H]

--pred holds the <scene>.npz files SaveScene wrote (either form).  With --info DIR the sites are the vertices of
DIR/<scene>_{vert,sem_label,ins_label}.npy (the ScanNet benchmark's domain: the prediction at a vertex is transfer_labels
of the saved scene).  With --gt DIR the sites are the cells of the prediction's own lattice, scored against
DIR/<scene>/{tsdf_info.pkl, full_tsdf_layer0, full_semantic_layer_interpolate0, full_instance_layer_interpolate0}
(generate_gt's files), so that geometry errors cost IoU.  With --views DATA_PATH the sites are the pixels of every
--every-th frame of DATA_PATH/<scene> (pose/, intrinsic/): the predicted mesh with its vertex ids and the labelled
ground-truth mesh --gt_mesh/<scene>_vh_clean_2.ply (labels: --info) are both rendered into those cameras
(eprecon_amd/render.py), which weighs a surface by how much of the video saw it.

The reference ships no scoring code; the rules (segments, void, the contingency table, matching, the figures) are this
project's and are written down in DESIGN.md §5b.  What runs on the device is the count of sites per (predicted segment,
ground-truth segment) pair (csrc/panoptic_score.hip); `finish` turns that small table into the figures on the host in
int64 / float64.  A `score_*` call issues one blocking read of its own (the flags, both key lists and the table in one
transfer); the two `torch.unique` calls behind the segment tables wait for their output sizes besides.

EPRECON_PC_LDS=0 (tests / timing): the kernels never sum the table per workgroup in LDS first; every add goes straight
to memory, as it does for a table above 8,192 entries.  The tables are the same integers.
"""
import argparse
import ctypes
import json
import os
import pickle
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import need_device
from .generate_gt import load_panoptic_points
from .generate_semantic_instance import SCANNET20_MAPPING, brick_masks, c_i32, mapping_list, query_labels
from .scene_io import LABEL_KEYS, read_ply, read_scene_list, scene_volumes
from .scene_fusion import STUFF_IDS

VALID_CLASSES = SCANNET20_MAPPING[1:]      # models/criterion.py:112
MAX_TABLE = 1 << 22
_KEY_SHIFT, _INS_BIAS = 32, 1 << 31


# ------------------------------------------------------------------------------------------------------- segments (device)

def _segment_table(semantic, instance, mapping, stuff_ids, valid_classes, absent_zero):
    """-> (rank, classes, keys, bad): segment_table plus a device flag (or None): a class index outside the mapping"""
    need_device(semantic, instance)
    if semantic.shape != instance.shape:
        raise ValueError(f"semantic {tuple(semantic.shape)} and instance {tuple(instance.shape)} differ in shape")
    dev = semantic.device
    sem, ins = semantic.to(torch.int64), instance.to(torch.int32).to(torch.int64)
    bad = None
    if mapping is not None:
        m = torch.tensor(mapping_list(mapping), dtype=torch.int64, device=dev)
        out = (sem < 0) | (sem >= m.numel())
        sem = torch.where(out, torch.zeros_like(sem), m[sem.clamp(0, m.numel() - 1)])
        bad = out.any()
    if absent_zero is None:
        absent_zero = mapping is not None
    valid = torch.isin(sem, torch.tensor([int(c) for c in valid_classes], dtype=torch.int64, device=dev))
    stuff = torch.isin(sem, torch.tensor([int(c) for c in stuff_ids], dtype=torch.int64, device=dev))
    key = (sem << _KEY_SHIFT) + torch.where(stuff, torch.zeros_like(ins), ins) + _INS_BIAS
    keys = torch.unique(key[valid])                   # ascending (class, instance)
    n = keys.numel()
    rank = torch.searchsorted(keys, key) if n else torch.zeros_like(key)
    rank = torch.where(valid, rank, torch.full_like(rank, n))
    if absent_zero:
        rank = torch.where(sem == 0, torch.full_like(rank, -1), rank)
    return rank.to(torch.int32), (keys >> _KEY_SHIFT).to(torch.int32), keys, bad


def segment_table(semantic, instance, mapping=None, stuff_ids=STUFF_IDS, valid_classes=VALID_CLASSES, absent_zero=None):
    """Label tensors of one shape on the device -> (rank int32 of that shape, classes int32[n], keys int64[n]).

    `mapping` (prediction side) takes class indices to ids first.  The sites of a stuff class form one segment, whatever
    their instance id; elsewhere a segment is one (class, instance) pair.  Segments are ranked 0..n-1 in ascending (class,
    instance) order; keys[r] = class << 32 | (instance + 2^31) (instance ids as int32, 0 for stuff).  A site whose class is
    not in valid_classes is void: rank n.  With absent_zero (default: when a mapping is given) class 0 is "nothing here":
    rank -1.  ValueError for a class index outside the mapping (one host read, only with a mapping)."""
    rank, classes, keys, bad = _segment_table(semantic, instance, mapping, stuff_ids, valid_classes, absent_zero)
    if bad is not None and _lib.read_counts(bad.to(torch.int32))[0]:
        raise ValueError(f"semantic values outside [0, {len(mapping_list(mapping))})")
    return rank, classes, keys


def key_pairs(keys):
    """keys of segment_table (host or device) -> int64[n,2] (class, instance) on the host"""
    k = np.asarray(keys.detach().cpu().numpy() if isinstance(keys, torch.Tensor) else keys, np.int64).reshape(-1)
    return np.stack([k >> _KEY_SHIFT, (k & (2 * _INS_BIAS - 1)) - _INS_BIAS], axis=1)


# ----------------------------------------------------------------------------------------------------- contingency (device)

def _table_buffers(n_pred, n_gt, dev):
    n_pred, n_gt = int(n_pred), int(n_gt)
    if n_pred < 0 or n_gt < 0:
        raise ValueError(f"segment counts must not be negative, got {n_pred}, {n_gt}")
    if (n_pred + 1) * (n_gt + 2) > MAX_TABLE:      # (the C entry refuses it too; no allocation of that size first)
        raise _lib.EpreconError(f"contingency table of {n_pred + 1} x {n_gt + 2} entries: more than 2^22 is unsupported (-3)")
    return (torch.empty((n_pred + 1, n_gt + 2), dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int32, device=dev))


def _launch_pair_counts(pred_rank, gt_rank, n_pred, n_gt):
    need_device(pred_rank, gt_rank)
    lib = _lib.load()
    p, g = (t.to(torch.int32).contiguous().reshape(-1) for t in (pred_rank, gt_rank))
    if p.numel() != g.numel():
        raise ValueError(f"{p.numel()} predicted and {g.numel()} ground-truth sites")
    counts, status = _table_buffers(n_pred, n_gt, p.device)
    _lib.check(lib.eprecon_pair_count_async(_lib.ptr(p), _lib.ptr(g), p.numel(), int(n_pred), int(n_gt), _lib.ptr(counts),
                                            _lib.ptr(status), _lib.current_stream()), "eprecon_pair_count_async")
    return counts, status


def _range_error(counts, n_pred, n_gt):
    err = ValueError(f"a rank outside [-1, {n_pred}) (predicted) or [-1, {n_gt}] (ground truth); such sites were not counted")
    err.counts = counts
    return err


def pair_counts(pred_rank, gt_rank, n_pred, n_gt):
    """Ranks of segment_table (any shape, the same number of sites) -> M int64[n_pred + 1, n_gt + 2] on the device:
    M[p, g] = sites in predicted segment p and ground-truth segment g; row n_pred: no prediction (rank -1); column n_gt:
    void; column n_gt + 1: no ground truth (rank -1).  One host read (the range flag): ValueError when a rank lies outside
    its range; such sites are left out and the table of the others is on the error as `.counts`."""
    counts, status = _launch_pair_counts(pred_rank, gt_rank, n_pred, n_gt)
    if _lib.read_counts(status)[0]:
        raise _range_error(counts, n_pred, n_gt)
    return counts


def _lattice(dims_p, origin_p, vs_p, dims_g, origin_g, vs_g):
    """-> (lo int[3], dims int[3]) of the site lattice in cells of the prediction's grid: per axis from min(0, the first k
    whose ground-truth cell lies inside) to max(X_p - 1, the last such k), with the kernel's own float64 arithmetic"""
    lo, dims = [], []
    for a in range(3):
        op, og = np.float64(np.float32(origin_p[a])), np.float64(np.float32(origin_g[a]))
        k0 = int(np.floor((og - op) / vs_p))
        k = np.arange(k0 - 2, k0 + int(dims_g[a]) + 3, dtype=np.int64)
        j = np.floor((op + k.astype(np.float64) * np.float64(vs_p) - og) / np.float64(vs_g) + 0.5)
        inside = k[(j >= 0) & (j < int(dims_g[a]))]
        first = min(0, int(inside.min())) if inside.size else 0
        last = max(int(dims_p[a]) - 1, int(inside.max())) if inside.size else int(dims_p[a]) - 1
        lo.append(first)
        dims.append(last - first + 1)
    return lo, dims


def _launch_voxel_pair_counts(pred_rank, origin_p, vs_p, gt_rank, gt_tsdf, origin_g, vs_g, gt_surface, n_pred, n_gt):
    need_device(pred_rank, gt_rank, gt_tsdf)
    lib = _lib.load()
    p, g = pred_rank.to(torch.int32).contiguous(), gt_rank.to(torch.int32).contiguous()
    t = gt_tsdf.to(torch.float32).contiguous()
    if p.dim() != 3 or g.dim() != 3 or g.shape != t.shape or 0 in p.shape or 0 in g.shape:
        raise ValueError(f"expected [X,Y,Z] volumes, got {tuple(p.shape)}, {tuple(g.shape)}, {tuple(t.shape)}")
    vs_p, vs_g = float(vs_p), float(vs_g)
    if not (vs_p > 0.0 and vs_g > 0.0) or abs(vs_p - vs_g) > 1e-9 * max(vs_p, vs_g):
        raise ValueError(f"voxel sizes {vs_p!r} (prediction) and {vs_g!r} (ground truth) must be positive and agree to 1e-9")
    origin_p, origin_g = (np.asarray(o, np.float32).reshape(3) for o in (origin_p, origin_g))
    lo, dims = _lattice(p.shape, origin_p, vs_p, g.shape, origin_g, vs_g)
    if int(np.prod(dims, dtype=np.int64)) >= 1 << 31:
        raise ValueError(f"a site lattice of {dims} cells (2^31 or more) is unsupported")
    counts, status = _table_buffers(n_pred, n_gt, p.device)
    keep = [c_i32(v) for v in (tuple(p.shape), tuple(g.shape), lo, dims)]
    o_p, o_g = (ctypes.c_float * 3)(*origin_p.tolist()), (ctypes.c_float * 3)(*origin_g.tolist())
    _lib.check(lib.eprecon_voxel_pair_count_async(
        _lib.ptr(p), _lib.ptr(g), _lib.ptr(t), keep[0][1], keep[1][1], ctypes.cast(o_p, ctypes.c_void_p),
        ctypes.cast(o_g, ctypes.c_void_p), vs_p, vs_g, float(gt_surface), keep[2][1], keep[3][1], int(n_pred), int(n_gt),
        _lib.ptr(counts), _lib.ptr(status), _lib.current_stream()), "eprecon_voxel_pair_count_async")
    return counts, status


# -------------------------------------------------------------------------------------------------------- the figures (host)

@dataclass
class SceneTables:
    """one scene: the contingency table, both sides' segments, and what `finish` made of them (arrays follow `classes`)"""
    counts: np.ndarray                 # M int64[P + 1, G + 2]
    pred_classes: np.ndarray           # int64[P]
    gt_classes: np.ndarray             # int64[G]
    threshold: float
    classes: tuple
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    iou_sum: np.ndarray                # float64
    sem_tp: np.ndarray
    sem_fp: np.ndarray
    sem_fn: np.ndarray
    matches: list = field(default_factory=list)     # (predicted rank, ground-truth rank, IoU) of every TP
    ignored: list = field(default_factory=list)     # predicted ranks left out of FP: more than half on void
    pred_keys: np.ndarray = None       # int64[P,2] (class, instance), when the caller knows them
    gt_keys: np.ndarray = None


def finish(M, pred_classes, gt_classes, threshold=0.5, valid_classes=VALID_CLASSES):
    """Contingency table int64[P + 1, G + 2] and the class of every predicted / ground-truth segment -> SceneTables.
    Host only, int64 and float64: IoU(p, g) = M[p,g] / (|p| + |g| - M[p,g] - M[p,void]); candidates have
    one class and IoU > threshold; they are taken in the order IoU descending, ground-truth rank, predicted rank while
    both segments are free; an unmatched prediction with more than half its sites on void is ignored."""
    M = np.asarray(M, np.int64)
    pc, gc = np.asarray(pred_classes, np.int64).reshape(-1), np.asarray(gt_classes, np.int64).reshape(-1)
    P, G = pc.size, gc.size
    if M.shape != (P + 1, G + 2):
        raise ValueError(f"table {M.shape} for {P} predicted and {G} ground-truth segments: expected {(P + 1, G + 2)}")
    classes = tuple(int(c) for c in valid_classes)
    psize, gsize, pvoid = M[:P].sum(axis=1), M[:, :G].sum(axis=0), M[:P, G]
    inter = M[:P, :G]
    pi, gi = np.nonzero((pc[:, None] == gc[None, :]) & (inter > 0))
    m = inter[pi, gi]
    iou = m.astype(np.float64) / (psize[pi] + gsize[gi] - m - pvoid[pi]).astype(np.float64)
    keep = iou > threshold
    pi, gi, iou = pi[keep], gi[keep], iou[keep]
    p_free, g_free = np.ones(P, bool), np.ones(G, bool)
    matches = []
    for t in np.lexsort((pi, gi, -iou)):
        if p_free[pi[t]] and g_free[gi[t]]:
            p_free[pi[t]] = g_free[gi[t]] = False
            matches.append((int(pi[t]), int(gi[t]), float(iou[t])))
    ignored = p_free & (2 * pvoid > psize)
    n = len(classes)
    tp, fp, fn = (np.zeros(n, np.int64) for _ in range(3))
    iou_sum = np.zeros(n, np.float64)
    sem_tp, sem_fp, sem_fn = (np.zeros(n, np.int64) for _ in range(3))
    for k, c in enumerate(classes):
        rows, cols = pc == c, gc == c
        for p, g, v in matches:
            if pc[p] == c:
                tp[k] += 1
                iou_sum[k] += v
        fp[k] = int((p_free & ~ignored & rows).sum())
        fn[k] = int((g_free & cols).sum())
        sem_tp[k] = M[:P][rows][:, :G][:, cols].sum()
        sem_fp[k] = M[:P][rows][:, :G][:, ~cols].sum() + M[:P][rows][:, G + 1].sum()
        sem_fn[k] = M[:P][~rows][:, :G][:, cols].sum() + M[P, :G][cols].sum()
    return SceneTables(M, pc, gc, float(threshold), classes, tp, fp, fn, iou_sum, sem_tp, sem_fp, sem_fn, matches,
                       np.flatnonzero(ignored).tolist())


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


class PanopticScore:
    """Accumulates scenes: TP, FP, FN and the IoU sum per class are summed over the scenes first, then divided."""

    def __init__(self, stuff_ids=STUFF_IDS):
        self.stuff_ids = tuple(int(c) for c in stuff_ids)
        self.classes = self.threshold = None
        self.n_scenes = 0

    def add(self, tables):
        if self.classes is None:
            self.classes, self.threshold = tables.classes, tables.threshold
            self.tp, self.fp, self.fn, self.sem_tp, self.sem_fp, self.sem_fn = (np.zeros(len(self.classes), np.int64) for _ in range(6))
            self.iou_sum = np.zeros(len(self.classes), np.float64)
        elif tables.classes != self.classes or tables.threshold != self.threshold:
            raise ValueError("scenes scored with different classes or thresholds do not add up")
        for name in ("tp", "fp", "fn", "iou_sum", "sem_tp", "sem_fp", "sem_fn"):
            setattr(self, name, getattr(self, name) + getattr(tables, name))
        self.n_scenes += 1
        return self

    def summary(self):
        """{'threshold', 'scenes', 'classes': {id: tp, fp, fn, iou_sum, pq, sq, rq, sem_tp, sem_fp, sem_fn, iou}, 'all' /
        'things' / 'stuff': {pq, sq, rq, n} (means over the n classes with TP + FP + FN > 0; None without one), 'miou' (mean
        over the classes with tp + fp + fn > 0; None without one)}.  A class that occurs nowhere has pq, sq, rq, iou None."""
        out = {"threshold": self.threshold, "scenes": self.n_scenes, "classes": {}}
        groups = {"all": [], "things": [], "stuff": []}
        ious = []
        for k, c in enumerate(self.classes or ()):
            tp, fp, fn = int(self.tp[k]), int(self.fp[k]), int(self.fn[k])
            s_tp, s_fp, s_fn = int(self.sem_tp[k]), int(self.sem_fp[k]), int(self.sem_fn[k])
            row = {"tp": tp, "fp": fp, "fn": fn, "iou_sum": float(self.iou_sum[k]), "pq": None, "sq": None, "rq": None,
                   "sem_tp": s_tp, "sem_fp": s_fp, "sem_fn": s_fn, "iou": None}
            if tp + fp + fn > 0:
                den = tp + 0.5 * fp + 0.5 * fn
                row.update(pq=float(self.iou_sum[k]) / den, sq=_ratio(self.iou_sum[k], tp), rq=tp / den)
                for g in ("all", "stuff" if c in self.stuff_ids else "things"):
                    groups[g].append(row)
            if s_tp + s_fp + s_fn > 0:
                row["iou"] = s_tp / (s_tp + s_fp + s_fn)
                ious.append(row["iou"])
            out["classes"][str(c)] = row
        for g, rows in groups.items():
            out[g] = {"n": len(rows)}
            for key in ("pq", "sq", "rq"):
                out[g][key] = float(np.mean([r[key] for r in rows])) if rows else None
        out["miou"] = float(np.mean(ious)) if ious else None
        return out

    def write(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(self.summary(), fh, indent=1)
        return path


def format_table(summary):
    """one table in the style of evaluation.visualize: a line per class that occurs, then all / things / stuff and mIoU"""
    f = lambda v: "  nan" if v is None else "%0.3f" % v
    lines = ["%10s %5s %5s %5s %5s %5s %5s %5s" % ("class", "PQ", "SQ", "RQ", "IoU", "TP", "FP", "FN")]
    for c, r in summary["classes"].items():
        if r["pq"] is not None or r["iou"] is not None:
            lines.append("%10s %s %s %s %s %5d %5d %5d" % (c, f(r["pq"]), f(r["sq"]), f(r["rq"]), f(r["iou"]), r["tp"], r["fp"], r["fn"]))
    for g in ("all", "things", "stuff"):
        lines.append("%10s %s %s %s" % (g, f(summary[g]["pq"]), f(summary[g]["sq"]), f(summary[g]["rq"])))
    lines.append("%10s %s" % ("mIoU", f(summary["miou"])))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------ scoring

def _read_tables(counts, status, bad, pred_keys, gt_keys, threshold, valid_classes, what):
    """THE host read of a scene: the flags, both key lists and the table in one transfer -> SceneTables"""
    P, G = pred_keys.numel(), gt_keys.numel()
    flag = torch.zeros(1, dtype=torch.int64, device=counts.device) if bad is None else bad.to(torch.int64).reshape(1)
    host = np.array(_lib.read_counts(torch.cat([status.to(torch.int64), flag, pred_keys, gt_keys, counts.reshape(-1)])), np.int64)
    if host[2]:
        raise ValueError(f"{what}: predicted semantic values outside the mapping")
    M = host[3 + P + G:].reshape(P + 1, G + 2)
    if host[0]:
        raise _range_error(M, P, G)
    pk, gk = key_pairs(host[3:3 + P]), key_pairs(host[3 + P:3 + P + G])
    tables = finish(M, pk[:, 0], gk[:, 0], threshold, valid_classes)
    tables.pred_keys, tables.gt_keys = pk, gk
    return tables


def _pred_table(pred_sem, pred_ins, mapping, stuff_ids, valid_classes):
    """prediction side: class 0 is "no prediction"; a class outside valid_classes (none with the default mapping) too"""
    rank, _, keys, bad = _segment_table(pred_sem, pred_ins, mapping, stuff_ids, valid_classes, True)
    return torch.where(rank == keys.numel(), torch.full_like(rank, -1), rank), keys, bad


def score_sites(pred_sem, pred_ins, gt_sem, gt_ins, mapping=SCANNET20_MAPPING, threshold=0.5, stuff_ids=STUFF_IDS,
                valid_classes=VALID_CLASSES):
    """Labels of N sites on the device -> SceneTables.  pred_sem: class indices taken through `mapping` (None: ids already);
    0 = no prediction.  gt_sem: ScanNet ids; a class outside valid_classes (0 included) is void.  One host read."""
    need_device(pred_sem, pred_ins, gt_sem, gt_ins)
    if pred_sem.numel() != gt_sem.numel():
        raise ValueError(f"{pred_sem.numel()} predicted and {gt_sem.numel()} ground-truth sites")
    p_rank, p_keys, bad = _pred_table(pred_sem.reshape(-1), pred_ins.reshape(-1), mapping, stuff_ids, valid_classes)
    g_rank, _, g_keys, _ = _segment_table(gt_sem.reshape(-1), gt_ins.reshape(-1), None, stuff_ids, valid_classes, False)
    counts, status = _launch_pair_counts(p_rank, g_rank, p_keys.numel(), g_keys.numel())
    return _read_tables(counts, status, bad, p_keys, g_keys, threshold, valid_classes, "score_sites")


def score_volumes(pred_sem, pred_ins, pred_origin, pred_voxel, gt_tsdf, gt_sem, gt_ins, gt_origin, gt_voxel, gt_surface=1.0,
                  mapping=SCANNET20_MAPPING, threshold=0.5, stuff_ids=STUFF_IDS, valid_classes=VALID_CLASSES):
    """The voxel domain on device volumes [X,Y,Z]; origins are taken as float32 like the files', voxel sizes as float64.
    The sites are the cells of the prediction's lattice over the union of both boxes; ground truth is present where
    |tsdf| < gt_surface (compared in float32).  One host read."""
    need_device(pred_sem, pred_ins, gt_tsdf, gt_sem, gt_ins)
    if gt_sem.shape != gt_tsdf.shape or gt_ins.shape != gt_tsdf.shape:
        raise ValueError(f"ground-truth volumes differ in shape: {tuple(gt_tsdf.shape)}, {tuple(gt_sem.shape)}, {tuple(gt_ins.shape)}")
    p_rank, p_keys, bad = _pred_table(pred_sem, pred_ins, mapping, stuff_ids, valid_classes)
    tsdf = gt_tsdf.to(torch.float32)
    present = tsdf.abs() < torch.tensor(float(gt_surface), dtype=torch.float32, device=tsdf.device)
    # (a segment is made of PRESENT cells: the others are void here, and the kernel never reads their rank)
    g_rank, _, g_keys, _ = _segment_table(torch.where(present, gt_sem.to(torch.int64), 0), gt_ins, None, stuff_ids, valid_classes, False)
    counts, status = _launch_voxel_pair_counts(p_rank, pred_origin, pred_voxel, g_rank, tsdf, gt_origin, gt_voxel, gt_surface,
                                               p_keys.numel(), g_keys.numel())
    return _read_tables(counts, status, bad, p_keys, g_keys, threshold, valid_classes, "score_volumes")


def _warn_empty(scene):
    print(f"[eprecon_amd] warning: No labelled voxel for scene {scene}")


def score_vertices(pred_npz, info_dir, scene, mapping=SCANNET20_MAPPING, threshold=0.5, stuff_ids=STUFF_IDS,
                   valid_classes=VALID_CLASSES, device=None):
    """The vertex domain: <info_dir>/<scene>_{vert,sem_label,ins_label}.npy against transfer_labels of the saved scene
    `pred_npz` at those vertices.  A scene with no labelled voxel scores as all-FN, with a warning.  Two host reads: the
    transfer's own (class range, site count) and the tables."""
    device = torch.device(device if device is not None else "cuda")
    sem, ins, origin, voxel_size = scene_volumes(pred_npz, device, LABEL_KEYS)
    verts, gt_sem, gt_ins = load_panoptic_points(info_dir, scene)
    masks, n_sites = brick_masks(sem, mapping)
    if n_sites == 0:
        _warn_empty(scene)
    out = query_labels(masks, sem, ins, origin, voxel_size, torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(device), mapping, 2)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64).reshape(-1)).to(device)
    return score_sites(out["semantic"], out["instance"], to_dev(gt_sem), to_dev(gt_ins), None, threshold, stuff_ids, valid_classes)


def _arr0(path):
    with np.load(path) as z:
        return z["arr_0"]


def score_voxels(pred_npz, gt_scene_dir, gt_surface=1.0, mapping=SCANNET20_MAPPING, threshold=0.5, stuff_ids=STUFF_IDS,
                 valid_classes=VALID_CLASSES, device=None):
    """The voxel domain: the saved scene `pred_npz` against generate_gt's files of <gt_scene_dir>: tsdf_info.pkl,
    full_tsdf_layer0.npz, full_semantic_layer_interpolate0.npz, full_instance_layer_interpolate0.npz.  ValueError when
    the two voxel sizes differ by more than 1e-9 relative or the lattice has 2^31 sites or more."""
    device = torch.device(device if device is not None else "cuda")
    sem, ins, origin, voxel_size = scene_volumes(pred_npz, device, LABEL_KEYS)
    with open(os.path.join(gt_scene_dir, "tsdf_info.pkl"), "rb") as fh:
        info = pickle.load(fh)
    tsdf = torch.from_numpy(np.ascontiguousarray(_arr0(os.path.join(gt_scene_dir, "full_tsdf_layer0.npz")), np.float32)).to(device)
    gt_sem, gt_ins = (torch.from_numpy(np.ascontiguousarray(_arr0(os.path.join(gt_scene_dir, f"full_{k}_layer_interpolate0.npz")))
                                       .astype(np.int32)).to(device) for k in LABEL_KEYS)
    tables = score_volumes(sem, ins, origin, voxel_size, tsdf, gt_sem, gt_ins, np.asarray(info["vol_origin"], np.float32).reshape(3),
                           float(info["voxel_size"]), gt_surface, mapping, threshold, stuff_ids, valid_classes)
    if tables.pred_classes.size == 0:
        _warn_empty(os.path.basename(os.path.normpath(gt_scene_dir)))
    return tables


def score_pixels(pred_npz, gt_mesh_path, info_dir, scene, K, poses, height, width, mapping=SCANNET20_MAPPING, threshold=0.5,
                 stuff_ids=STUFF_IDS, valid_classes=VALID_CLASSES, device=None, chunk=32, **raster):
    """The pixel domain: the mesh of the saved scene `pred_npz` with its vertex ids against the mesh `gt_mesh_path`
    (<scene>_vh_clean_2.ply) labelled at its vertices by <info_dir>/<scene>_{sem_label,ins_label}.npy, both rendered into
    the cameras K [3,3], poses [V,4,4] at height x width (render.visibility's **raster: znear, zfar, cull_back,
    pixel_center).  Both vertex sets are ranked once; every pixel takes the rank of the nearest corner of the triangle it
    sees, -1 where a side shows nothing (no prediction / no ground truth).  The pairs are counted per chunk of views and
    the tables added on the device; the sites are all pixels of the given frames.  ValueError when the label files and
    the mesh differ in vertex count.  One host read of its own (the tables)."""
    from . import render as RD
    device = torch.device(device if device is not None else "cuda")
    verts, faces, vsem, vins = RD.scene_mesh(pred_npz, device)
    gt_verts, gt_faces = read_ply(gt_mesh_path)
    _, gt_sem, gt_ins = load_panoptic_points(info_dir, scene)
    if len(gt_sem) != len(gt_verts) or len(gt_ins) != len(gt_verts):
        raise ValueError(f"{scene}: {len(gt_verts)} vertices in {gt_mesh_path}, {len(gt_sem)} semantic and {len(gt_ins)} instance "
                         f"labels in {info_dir}")
    to_dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(device)
    gt_verts, gt_faces = to_dev(gt_verts, np.float32), to_dev(gt_faces, np.int32)
    p_rank, p_keys, bad = _pred_table(vsem, vins, mapping, stuff_ids, valid_classes)
    g_rank, _, g_keys, _ = _segment_table(to_dev(gt_sem, np.int64).reshape(-1), to_dev(gt_ins, np.int64).reshape(-1), None,
                                          stuff_ids, valid_classes, False)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    pc = raster.get("pixel_center", 0.5)
    counts, status = _table_buffers(p_keys.numel(), g_keys.numel(), device)
    counts.zero_()
    status.zero_()
    chunk = max(int(chunk), 1)
    for s in range(0, len(poses), chunk):
        images = []
        for v, f, rank in ((verts, faces, p_rank), (gt_verts, gt_faces, g_rank)):
            vis = RD.visibility(v, f, K, poses[s:s + chunk], height, width, **raster)
            images.append(RD.resolve(vis, v, f, K, poses[s:s + chunk], labels=(rank,), backgrounds=(-1,), pixel_center=pc,
                                     outputs=())["labels"][0])
        c, st = _launch_pair_counts(images[0], images[1], p_keys.numel(), g_keys.numel())
        counts += c
        status |= st
    return _read_tables(counts, status, bad, p_keys, g_keys, threshold, valid_classes, "score_pixels")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="panoptic quality (PQ, SQ, RQ) and semantic IoU of saved scenes")
    ap.add_argument("--pred", required=True, help="directory of the <scene>.npz files SaveScene wrote")
    ap.add_argument("--scenes", required=True, help="text file, one scene name per line")
    # (--info names the vertex domain on its own and the labels of the pixel domain next to --views, so it cannot sit in
    # the exclusive group with --views; the rules the group used to state are checked below)
    domain = ap.add_mutually_exclusive_group()
    domain.add_argument("--gt", help="voxel domain: directory of generate_gt's <scene>/ directories")
    domain.add_argument("--views", metavar="DATA_PATH", help="pixel domain: ScanNet-layout scenes <scene>/pose, intrinsic; "
                        "needs --info (the vertex labels) and --gt_mesh")
    ap.add_argument("--info", help="vertex domain: directory of <scene>_{vert,sem_label,ins_label}.npy")
    ap.add_argument("--gt_mesh", help="pixel domain: directory of the <scene>_vh_clean_2.ply meshes")
    ap.add_argument("--every", default=10, type=int, help="pixel domain: every n-th frame (default 10)")
    ap.add_argument("--size", default=[640, 480], type=int, nargs=2, metavar=("W", "H"), help="pixel domain: image size")
    ap.add_argument("--threshold", default=0.5, type=float, help="a pair matches above this IoU (default 0.5)")
    ap.add_argument("--gt_surface", default=1.0, type=float, help="voxel domain: ground truth is present where |tsdf| is below this")
    ap.add_argument("--out", default=None, help="write the summary as JSON here")
    args = ap.parse_args(argv)
    if args.views is not None:
        if args.info is None or args.gt_mesh is None:
            ap.error("--views needs --info and --gt_mesh")
    elif args.gt is not None and args.info is not None:
        ap.error("argument --info: not allowed with argument --gt")
    elif args.gt is None and args.info is None:
        ap.error("one of the arguments --gt --info --views is required")
    elif args.gt_mesh is not None:
        ap.error("--gt_mesh belongs to --views")
    return args


def main(argv=None):
    args = parse_args(argv)
    score = PanopticScore()
    for scene in read_scene_list(args.scenes):
        npz = os.path.join(args.pred, scene + ".npz")
        if args.views is not None:
            from .render import scene_views
            _, k, poses = scene_views(args.views, scene, args.every, tuple(args.size))
            score.add(score_pixels(npz, os.path.join(args.gt_mesh, scene + "_vh_clean_2.ply"), args.info, scene, k, poses,
                                   args.size[1], args.size[0], threshold=args.threshold))
        elif args.gt is not None:
            score.add(score_voxels(npz, os.path.join(args.gt, scene), gt_surface=args.gt_surface, threshold=args.threshold))
        else:
            score.add(score_vertices(npz, args.info, scene, threshold=args.threshold))
    print(format_table(score.summary()))
    if args.out:
        score.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

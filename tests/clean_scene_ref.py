"""The clean-up rule of DESIGN.md §5b restated on the host with no code of the package: a dict from coordinate to row and a
breadth-first search whose adjacency is spelled out from the coordinate difference.  tests/test_clean_scene_host.py checks
it on cases written out by hand; tests/test_clean_scene_gpu.py holds eprecon_amd.clean_scene to it element for element."""
from collections import deque

import numpy as np

REPORT_KEYS = ("rows_in", "rows_removed", "components", "components_removed", "segment_components_cleared", "rows_cleared",
               "instances_split")


def adjacent(a, b, connectivity):
    d = [abs(int(p) - int(q)) for p, q in zip(a, b)]
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    return any(d) and max(d) <= 1 and sum(d) <= limit


def components_ref(coords, keys=None, connectivity=26):
    """coords int[M,3] (pairwise distinct), keys int[M] or None -> label int32[M]: the smallest row of the row's component,
    -1 for a row with a negative key"""
    coords = [tuple(int(v) for v in c) for c in np.asarray(coords).reshape(-1, 3)]
    m = len(coords)
    keys = [0] * m if keys is None else [int(k) for k in keys]
    row_of = {}
    for i, c in enumerate(coords):
        if c in row_of:
            raise ValueError(f"rows {row_of[c]} and {i} have the same coordinates")
        row_of[c] = i
    offsets = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
               if adjacent((dx, dy, dz), (0, 0, 0), connectivity)]
    assert len(offsets) == connectivity
    label = [-1] * m
    for start in range(m):                      # ascending: the first row to reach a component is its smallest
        if keys[start] < 0 or label[start] >= 0:
            continue
        label[start] = start
        queue = deque([start])
        while queue:
            i = queue.popleft()
            x, y, z = coords[i]
            for dx, dy, dz in offsets:
                j = row_of.get((x + dx, y + dy, z + dz))
                if j is not None and label[j] < 0 and keys[j] == keys[start]:
                    label[j] = start
                    queue.append(j)
    return np.array(label, np.int32).reshape(m)


def _sizes(label, member):
    sizes = {}
    for i in range(len(label)):
        if member[i]:
            sizes[int(label[i])] = sizes.get(int(label[i]), 0) + 1
    return sizes


def clean_rows_ref(coords, tsdf, semantic, instance, min_voxels=0, keep_largest=0, min_segment_voxels=0, split_instances=False,
                   connectivity=26):
    """numpy rows -> (coords, tsdf, semantic, instance, report) by the rule of DESIGN.md §5b"""
    coords, tsdf = np.asarray(coords).reshape(-1, 3), np.asarray(tsdf)
    semantic, instance = np.array(semantic), np.array(instance)
    m = len(coords)
    report = dict.fromkeys(REPORT_KEYS, 0)
    report["rows_in"] = m
    # geometry pass
    geo = [bool(t < 1) for t in tsdf]
    label = components_ref(coords, [0 if g else -1 for g in geo], connectivity)
    sizes = _sizes(label, geo)
    if keep_largest > 0:
        kept = set(sorted(sizes, key=lambda r: (-sizes[r], r))[:keep_largest])
    else:
        kept = {r for r, s in sizes.items() if s >= min_voxels}
    keep = np.array([not geo[i] or int(label[i]) in kept for i in range(m)], bool).reshape(m)
    report["components"], report["components_removed"] = len(sizes), len(sizes) - len(kept)
    report["rows_removed"] = int((~keep).sum())
    coords, tsdf, semantic, instance = coords[keep], tsdf[keep], semantic[keep], instance[keep]
    # segment pass
    n = len(coords)
    seg = [bool(s > 0) for s in semantic]
    pairs = sorted({(int(semantic[i]), int(instance[i])) for i in range(n) if seg[i]})
    keys = [pairs.index((int(semantic[i]), int(instance[i]))) if seg[i] else -1 for i in range(n)]
    label = components_ref(coords, keys, connectivity)
    sizes = _sizes(label, seg)
    small = {r for r, s in sizes.items() if s < min_segment_voxels}
    for i in range(n):
        if seg[i] and int(label[i]) in small:
            semantic[i] = 0
            instance[i] = 0
            report["rows_cleared"] += 1
    report["segment_components_cleared"] = len(small)
    if split_instances and n:
        by_pair = {}
        for r in sorted(sizes):
            if r not in small and instance[r] > 0:
                by_pair.setdefault(keys[r], []).append(r)
        losers = []
        for roots in by_pair.values():
            winner = min(roots, key=lambda r: (-sizes[r], r))
            losers += [r for r in roots if r != winner]
        base = max(int(instance.max()), 0)
        fresh = {r: base + 1 + j for j, r in enumerate(sorted(losers))}
        for i in range(n):
            if seg[i] and int(label[i]) in fresh:
                instance[i] = fresh[int(label[i])]
        report["instances_split"] = len(losers)
    return coords, tsdf, semantic, instance, report

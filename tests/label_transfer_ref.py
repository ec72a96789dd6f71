"""float64 numpy oracle of the panoptic export (eprecon_amd/generate_semantic_instance.py, csrc/label_transfer.hip).

The arithmetic is the kernels' contract, written as numpy evaluates it — every operation rounded on its own:
    site  = idx * float64(voxel_size) + float32(origin)              (numpy promotes the sum to float64)
    d2    = (dx * dx + dy * dy) + dz * dz,   d = float64(vertex) - site
    winner: the smallest d2, among equal ones the smallest linear cell index (x * Y + y) * Z + z
and the vote is the reference's literal Counter(...).most_common(1).
"""
from collections import Counter

import numpy as np

SCANNET20 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


def sites(semantic, origin, voxel_size, mapping=SCANNET20):
    """-> (linear index int64[S] ascending, world coordinates float64[S,3]) of the cells whose mapped class is not 0"""
    semantic = np.asarray(semantic)
    mapped = np.asarray(mapping)[semantic.reshape(-1).astype(int)]
    lin = np.flatnonzero(mapped != 0)
    idx = np.stack(np.unravel_index(lin, semantic.shape), axis=-1)
    return lin, idx * np.float64(voxel_size) + np.asarray(origin, np.float32)


def brute_force(semantic, instance, origin, voxel_size, vertices, mapping=SCANNET20, chunk=256):
    """-> dict: index int32[N] (-1 without a site), dist float32[N], d2 float64[N], second float64[N] (the d2 of the
    nearest site other than the winner, inf when there is none), semantic / instance int64[N] (0 without a site)"""
    semantic, instance = np.asarray(semantic), np.asarray(instance)
    q = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    n = q.shape[0]
    lin, xyz = sites(semantic, origin, voxel_size, mapping)
    out = {"index": np.full(n, -1, np.int32), "d2": np.full(n, np.inf), "second": np.full(n, np.inf),
           "semantic": np.zeros(n, np.int64), "instance": np.zeros(n, np.int64)}
    if lin.size and n:
        for s in range(0, n, chunk):
            d = q[s:s + chunk, None, :] - xyz[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            k = np.argmin(d2, axis=1)                      # (the first minimum: the sites are in linear-index order)
            rows = np.arange(d2.shape[0])
            out["index"][s:s + chunk] = lin[k]
            out["d2"][s:s + chunk] = d2[rows, k]
            if lin.size > 1:
                d2[rows, k] = np.inf
                out["second"][s:s + chunk] = d2.min(axis=1)
        mapped = np.asarray(mapping)[semantic.reshape(-1).astype(int)]
        out["semantic"] = mapped[out["index"]].astype(np.int64)
        out["instance"] = instance.reshape(-1)[out["index"]].astype(np.int64)
    out["dist"] = np.sqrt(out["d2"]).astype(np.float32)
    return out


def minima(semantic, origin, voxel_size, vertex, mapping=SCANNET20):
    """linear indices of ALL the sites at the smallest d2 from one vertex (the exact-tie tests)"""
    lin, xyz = sites(semantic, origin, voxel_size, mapping)
    d = np.asarray(vertex, np.float32).astype(np.float64)[None, :] - xyz
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return lin[d2 == d2.min()]


def vote(mapped_semantic, mapped_instance):
    """tools/generate_semantic_instance.py:62-77 -> (ids ascending, class per id, vertex count per id)"""
    sem, ins = np.asarray(mapped_semantic).reshape(-1), np.asarray(mapped_instance).reshape(-1)
    ids = np.unique(ins).astype(int)
    classes, counts = [], []
    for instance_id in ids:
        counter = Counter(sem[ins == instance_id].tolist())
        classes.append(counter.most_common(1)[0][0])
        counts.append(int((ins == instance_id).sum()))
    return ids, np.array(classes, np.int64), np.array(counts, np.int64)


# A constructed tie: instance 40 has classes 9 and 3 with two vertices each and 9 is seen first, so most_common(1) gives 9 (a
# "smallest class id" rule gives 3); instance 0, seen last, has a clear majority.  Instance ids non-contiguous, 0 among them.
TIE_SEM = np.array([9, 3, 3, 9, 5, 4, 4], np.int64)
TIE_INS = np.array([40, 40, 40, 40, 0, 0, 0], np.int64)

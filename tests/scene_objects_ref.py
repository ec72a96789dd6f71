"""Restatement of the object-inventory rule with Python loops, Python integers and fractions.  It shares no
code with eprecon_amd/scene_objects.py: the segments are re-derived from (class, instance) with the stuff rule, the table is
filled one row at a time in Python ints, the centroid is a Fraction rounded once, the extents are plain float64 numpy.

A row's label is None (it does not take part) or a segment key (class, instance); a stuff class has instance 0 in its key.
"""
import math
from fractions import Fraction

import numpy as np

MAPPING = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
VALID = MAPPING[1:]
STUFF = (1, 2)
LIMIT = 2 ** 19 - 2
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
COLUMNS = 16


def labels(semantic, instance, tsdf, mapping=MAPPING, surface=1.0):
    """per row None or a key: the row takes part when |tsdf| < surface in float32 and its class maps to a valid id"""
    out = []
    for s, i, t in zip(np.asarray(semantic).reshape(-1).tolist(), np.asarray(instance).reshape(-1).tolist(),
                       np.asarray(tsdf, np.float32).reshape(-1)):
        if mapping is not None and not 0 <= int(s) < len(mapping):
            raise ValueError("class index outside the mapping")
        c = mapping[int(s)] if mapping is not None else int(s)
        near = bool(np.abs(np.float32(t)) < np.float32(surface))
        out.append(((c, 0) if c in STUFF else (c, int(i))) if near and c in VALID else None)
    return out


def ranks(row_labels):
    """-> (rank per row, -1 for None; the keys in ascending (class, instance) order)"""
    keys = sorted({k for k in row_labels if k is not None})
    where = {k: r for r, k in enumerate(keys)}
    return [-1 if k is None else where[k] for k in row_labels], keys


def identity_row():
    return [0] * 10 + [INT32_MAX] * 3 + [INT32_MIN] * 3


def _takes_part(r, xyz, n):
    """-> (takes part, status bits): the rank is looked at first"""
    if r == -1 or r == n:
        return False, 0
    if not 0 <= r < n:
        return False, 1
    if any(abs(k) > LIMIT for k in xyz):
        return False, 2
    return True, 0


def moments(coords, rank, n):
    """-> (table: n rows of 16 Python ints, status word)"""
    table, status = [identity_row() for _ in range(n)], 0
    if n == 0:
        return table, 0
    for (x, y, z), r in zip(np.asarray(coords, np.int64).reshape(-1, 3).tolist(), np.asarray(rank).reshape(-1).tolist()):
        ok, bits = _takes_part(r, (x, y, z), n)
        status |= bits
        if not ok:
            continue
        t = table[r]
        t[0] += 1
        for a, k in enumerate((x, y, z)):
            t[1 + a] += k
            t[10 + a] = min(t[10 + a], k)
            t[13 + a] = max(t[13 + a], k)
        for a, p in enumerate((x * x, x * y, x * z, y * y, y * z, z * z)):
            t[4 + a] += p
    return table, status


def table_array(table):
    return np.array(table, np.int64).reshape(-1, COLUMNS)


def extents(coords, rank, n, dirs):
    """-> (float64[n,4] = (min u, max u, min v, max v), status word); a zero is +0"""
    coords, rank = np.asarray(coords, np.int64).reshape(-1, 3), np.asarray(rank).reshape(-1)
    ext, status = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf]), (n, 1)).reshape(n, 4), 0
    if n == 0:
        return ext, 0
    member = [[] for _ in range(n)]
    for i, r in enumerate(rank.tolist()):
        ok, bits = _takes_part(r, coords[i].tolist(), n)
        status |= bits
        if ok:
            member[r].append(i)
    for r, rows in enumerate(member):
        if not rows:
            continue
        x, y = coords[rows, 0].astype(np.float64), coords[rows, 1].astype(np.float64)
        c, s = np.float64(dirs[r][0]), np.float64(dirs[r][1])
        u = x * c + y * s
        v = y * c - x * s
        ext[r] = [u.min() + 0.0, u.max() + 0.0, v.min() + 0.0, v.max() + 0.0]
    return ext, status


def heading(t):
    n, sx, sy, sxx, sxy, syy = t[0], t[1], t[2], t[4], t[5], t[7]
    A = n * sxx - sx ** 2
    B = n * syy - sy ** 2
    C = n * sxy - sx * sy
    if C == 0 and A == B:
        return 0.0
    return 0.5 * math.atan2(float(2 * C), float(A - B))


def directions(table):
    out = []
    for t in table:
        th = heading([int(v) for v in t]) if int(t[0]) > 0 else 0.0
        out.append((math.cos(th), math.sin(th)))
    return np.array(out, np.float64).reshape(-1, 2)


def records(table, ext, keys, origin, voxel_size, min_voxels=1):
    """table: rows of ints, ext float64[n,4] or None, keys: (class, instance) per segment -> the records"""
    o = [float(np.float64(np.float32(v))) for v in origin]
    vs = float(voxel_size)
    out = []
    for r, (t, key) in enumerate(zip(table, keys)):
        t = [int(v) for v in t]
        n = t[0]
        if n < max(min_voxels, 1):
            continue
        rec = {"id": r, "class_id": int(key[0]), "instance": int(key[1]), "voxels": n}
        rec["centroid"] = [o[a] + float(Fraction(t[1 + a], n)) * vs for a in range(3)]
        rec["aabb_min"] = [o[a] + (t[10 + a] - 0.5) * vs for a in range(3)]
        rec["aabb_max"] = [o[a] + (t[13 + a] + 0.5) * vs for a in range(3)]
        if ext is not None:
            th = heading(t)
            c, s = math.cos(th), math.sin(th)
            u0, u1, v0, v1 = (float(v) for v in ext[r])
            cu, cv, cz = (u0 + u1) / 2, (v0 + v1) / 2, (float(t[12]) + float(t[15])) / 2
            rec["heading"] = th
            rec["obb_centre"] = [o[0] + vs * (c * cu - s * cv), o[1] + vs * (s * cu + c * cv), o[2] + vs * cz]
            rec["obb_size"] = [((u1 - u0) + 1) * vs, ((v1 - v0) + 1) * vs, ((float(t[15]) - float(t[12])) + 1) * vs]
        out.append(rec)
    return out


def scene(coords, tsdf, semantic, instance, origin, voxel_size, mapping=MAPPING, surface=1.0, min_voxels=1, oriented=True):
    rank, keys = ranks(labels(semantic, instance, tsdf, mapping, surface))
    table, status = moments(coords, rank, len(keys))
    assert status == 0
    ext = extents(coords, rank, len(keys), directions(table))[0] if oriented else None
    return records(table, ext, keys, origin, voxel_size, min_voxels)

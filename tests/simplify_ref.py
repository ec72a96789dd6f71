"""The mesh simplification rule of DESIGN.md §5b restated with Python loops, dicts and float64 numpy.  Shares no code with
eprecon_amd/: the tests hold eprecon_amd/simplify.py (csrc/mesh_simplify.hip) to what this file computes.

    out = simplify(vertices, faces, cell, semantic=None, instance=None, colors=None, origin=None, regularize=1e-3)

out: cluster int64[N]; per cluster cells int64[K,3], positions f64[K,3], means f64[K,3] (absolute), normals f32[K,3], rgb
u8[K,3] or None, cluster_semantic / cluster_instance int64[K] or None, written bool[K], fragile bool[K]; kept (the input
indices of the surviving faces), faces int64[F,3] re-indexed, vertices f64[V,3]; report; and `quadrics`, per cluster the
tuple (A, b, c0, lam, m) relative to the centre of its cell, for `energy`.

fragile[k]: the clip of step 4 is continuous except where the mean sits on a face of the box and the step towards the
minimiser runs along that face: then the sign of a component that is zero in exact arithmetic decides between t = 0 and
t > 0.  A cluster is marked when, on some axis, both |x* - m| and the distance of m to the nearer face are below 1e-9 cell
while the step is longer than 1e-9 cell on another axis.
"""
import math

import numpy as np


def cells_of(vertices, cell, origin=None):
    o = np.zeros(3, np.float64) if origin is None else np.asarray(origin, np.float64).reshape(3)
    return np.floor((np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3) - o) / np.float64(cell)).astype(np.int64)


def energy(q, x):
    """xT A x - 2 bT x + c0 + lam |x - m|^2 at x (relative to the cell's centre)"""
    a, b, c0, lam, m = q
    x = np.asarray(x, np.float64)
    return float(x @ a @ x - 2.0 * (b @ x) + c0 + lam * ((x - m) @ (x - m)))


def represent(a, b, m, half, regularize):
    """-> (position relative to the centre, x*, lam, fragile)"""
    trace = a[0, 0] + a[1, 1] + a[2, 2]
    lam = regularize * trace / 3.0
    x = m.copy()
    if trace > 0.0:
        x = np.linalg.solve(a + lam * np.eye(3), b + lam * m)
    t = 1.0
    for ax in range(3):
        d = x[ax] - m[ax]
        if d > 0.0:
            t = min(t, (half - m[ax]) / d)
        elif d < 0.0:
            t = min(t, (-half - m[ax]) / d)
    t = max(t, 0.0)
    p = np.clip(m + t * (x - m), -half, half)
    tiny = 1e-9 * 2.0 * half
    step = np.abs(x - m)
    fragile = any(step[ax] < tiny and min(abs(half - m[ax]), abs(-half - m[ax])) < tiny and max(step[(ax + 1) % 3], step[(ax + 2) % 3]) > tiny
                  for ax in range(3))
    return p, x, lam, fragile


def simplify(vertices, faces, cell, semantic=None, instance=None, colors=None, origin=None, regularize=1e-3):
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n, m = len(v), len(f)
    if m and (f.min() < 0 or f.max() >= n):
        raise ValueError("a face index outside [0, N)")
    if not np.isfinite(v).all():
        raise ValueError("a vertex that is not finite")
    cell = float(cell)
    o = np.zeros(3, np.float64) if origin is None else np.asarray(origin, np.float64).reshape(3)
    cells = cells_of(vertices, cell, o)
    sem = np.zeros(n, np.int64) if semantic is None else np.asarray(semantic, np.int64)
    ins = np.zeros(n, np.int64) if instance is None else np.asarray(instance, np.int64)

    # 2. clusters: the ranks of (cx, cy, cz, semantic, instance)
    keys = [(int(cells[i, 0]), int(cells[i, 1]), int(cells[i, 2]), int(sem[i]), int(ins[i])) for i in range(n)]
    rank = {key: r for r, key in enumerate(sorted(set(keys)))}
    cluster = np.array([rank[key] for key in keys], np.int64)
    k = len(rank)
    by_rank = sorted(rank, key=rank.get)
    members = [[] for _ in range(k)]
    for i in range(n):
        members[cluster[i]].append(i)
    corners = [[] for _ in range(k)]
    for fi in range(m):
        for c in range(3):
            corners[cluster[f[fi, c]]].append(fi)        # (ascending 3 f + c)

    # 3. n = (b - a) x (c - a) of every face from the vertices as they are, in Python floats
    face_n, face_len = [], []
    for fi in range(m):
        pa, pb, pc = ([float(x) for x in v[f[fi, c]]] for c in range(3))
        e1, e2 = [pb[a] - pa[a] for a in range(3)], [pc[a] - pa[a] for a in range(3)]
        nx, ny, nz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        face_n.append(np.array([nx, ny, nz]))
        face_len.append(math.sqrt(nx * nx + ny * ny + nz * nz))

    half = 0.5 * cell
    positions, means, normals = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3), np.float32)
    rgb = None if colors is None else np.zeros((k, 3), np.uint8)
    fragile = np.zeros(k, bool)
    quadrics = []
    for r in range(k):
        centre = o + (np.array(by_rank[r][:3], np.float64) + 0.5) * cell
        mean = np.zeros(3)
        for i in members[r]:
            mean = mean + (v[i] - centre)
        mean = mean / len(members[r])
        a, b, c0, nsum = np.zeros((3, 3)), np.zeros(3), 0.0, np.zeros(3)
        for fi in corners[r]:
            nrm, length = face_n[fi], face_len[fi]
            if length == 0.0:
                continue
            pa = v[f[fi, 0]] - centre
            u, w = nrm / length, length / 2.0
            d = -float(u @ pa)
            a = a + w * np.outer(u, u)
            b = b + (-w * d) * u
            c0 = c0 + w * d * d
            nsum = nsum + nrm
        p, _, lam, fragile[r] = represent(a, b, mean, half, float(regularize))
        positions[r], means[r] = centre + p, centre + mean
        quadrics.append((a, b, c0, lam, mean))
        nl = math.sqrt(nsum[0] * nsum[0] + nsum[1] * nsum[1] + nsum[2] * nsum[2])
        normals[r] = (nsum / nl).astype(np.float32) if nl > 0.0 else 0.0
        if colors is not None:
            count = len(members[r])
            for ch in range(3):
                total = sum(int(colors[i][ch]) for i in members[r])
                rgb[r, ch] = (2 * total + count) // (2 * count)

    # 6. faces
    seen, kept, degenerate, duplicate = set(), [], 0, 0
    for fi in range(m):
        t = tuple(int(cluster[f[fi, c]]) for c in range(3))
        if len(set(t)) < 3:
            degenerate += 1
        elif tuple(sorted(t)) in seen:
            duplicate += 1
        else:
            seen.add(tuple(sorted(t)))
            kept.append(fi)
    # 7. vertices
    written = np.zeros(k, bool)
    for fi in kept:
        written[cluster[f[fi]]] = True
    new_id = np.cumsum(written) - 1
    out_faces = np.array([[new_id[cluster[f[fi, c]]] for c in range(3)] for fi in kept], np.int64).reshape(-1, 3)
    shift = max((float(np.linalg.norm(v[i] - positions[cluster[i]])) for i in range(n)), default=0.0)
    report = {"vertices_in": n, "faces_in": m, "clusters": k, "vertices_out": int(written.sum()), "faces_out": len(kept),
              "faces_degenerate": degenerate, "faces_duplicate": duplicate, "max_shift": shift}
    label = lambda which, given: None if given is None else np.array([key[which] for key in by_rank], np.int64)
    return {"cluster": cluster, "cells": np.array([key[:3] for key in by_rank], np.int64).reshape(-1, 3), "positions": positions, "means": means,
            "normals": normals, "rgb": rgb, "cluster_semantic": label(3, semantic), "cluster_instance": label(4, instance),
            "written": written, "fragile": fragile, "kept": np.array(kept, np.int64), "faces": out_faces,
            "vertices": positions[written], "report": report, "quadrics": quadrics}

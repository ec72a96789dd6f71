"""float64 restatement of vertex colouring (eprecon_amd/colorize.py, csrc/mesh_colorize.hip; the rule of DESIGN.md §5b) — a
test helper that shares no code with the package: Python loops over vertices and views, one (vertex, view) pair at a time.

Per pair, everything in float64 with sums associated (a x + b y) + c z:
    q = w2c p, z = q.z, kept only if znear <= z <= zfar;
    (u_d, v_d) = (K_vis q) (1 / z), cd = floor(u_d - pixel_center + 0.5), rd likewise, inside the visibility buffer; the word
    there is a hit (upper word < 0x7F800000, the face index below n_faces, its corners in range) and z <= D + tolerance;
    n = (b - a) x (c - a) of that face in the camera frame, |n| > 0, cos = |n . q| / (|n| |q|) >= min_cos;
    (u_c, v_c) = (K_color q) (1 / z), x = u_c - pixel_center, y likewise, 0 <= x <= Wc - 1, 0 <= y <= Hc - 1;
    x0 = min(floor(x), Wc - 2), fx = x - x0 (the same for y), the bilinear value of the four bytes per channel;
    w = cos / z^2; acc += (w r, w g, w b, w), seen += 1.
Finish: min(255, floor(acc_c / acc_w + 0.5)) where seen >= min_views (and acc_w > 0), else the fallback colour.

Next to acc, seen and rgb comes a mask of the vertices LEFT OUT of a comparison because float64 cannot decide them: some view
has a keep / reject comparison, the argument of a floor or a pixel boundary within `eps` (relative to max(1, |a|, |b|)), or
a final channel is within `round_eps` of x.5.
"""
import math
import struct

import numpy as np

EPS = 1e-9
ROUND_EPS = 1e-6
INF_BITS = 0x7F800000


def _close(a, b, eps):
    return abs(a - b) <= eps * max(1.0, abs(a), abs(b))


def _near_integer(a, eps):
    return abs(a - math.floor(a + 0.5)) <= eps * max(1.0, abs(a))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _camera(m, p):
    return tuple(((m[r][0] * p[0] + m[r][1] * p[1]) + m[r][2] * p[2]) + m[r][3] for r in range(3))


def _project(k, q):
    iz = 1.0 / q[2]
    return (((k[0][0] * q[0] + k[0][1] * q[1]) + k[0][2] * q[2]) * iz, ((k[1][0] * q[0] + k[1][1] * q[1]) + k[1][2] * q[2]) * iz)


def pair(p, m, verts, faces, k_color, k_vis, frame, vis, pc, znear, zfar, tolerance, min_cos, eps=EPS):
    """one (vertex, view): p the vertex (three floats), m the world -> camera rows, frame u8[Hc,Wc,3], vis u64[Hd,Wd] ->
    (None or (w r, w g, w b, w), undecided)"""
    q = _camera(m, p)
    z = q[2]
    und = _close(z, znear, eps) or _close(z, zfar, eps)
    if not (znear <= z <= zfar):
        return None, und
    hd, wd = vis.shape
    ud, vd = _project(k_vis, q)
    au, av = ud - pc + 0.5, vd - pc + 0.5
    und = und or _near_integer(au, eps) or _near_integer(av, eps)
    cd, rd = math.floor(au), math.floor(av)
    if not (0 <= cd <= wd - 1 and 0 <= rd <= hd - 1):
        return None, und
    word = int(vis[rd, cd])
    bits, tri = word >> 32, word & 0xFFFFFFFF
    if not (bits < INF_BITS and tri < len(faces)):
        return None, und
    ids = [int(t) for t in faces[tri]]
    if any(t < 0 or t >= len(verts) for t in ids):
        return None, und
    depth = struct.unpack("<f", struct.pack("<I", bits))[0]
    und = und or _close(z, depth + tolerance, eps)
    if not (z <= depth + tolerance):
        return None, und
    a, b, c = (_camera(m, verts[t]) for t in ids)
    u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    w = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    n = _cross(u, w)
    nlen = math.sqrt(_dot(n, n))
    scale = math.sqrt(_dot(u, u)) * math.sqrt(_dot(w, w))
    if not nlen > 0.0:
        return None, und                      # (a face with two equal corners: n is exactly 0)
    und = und or nlen <= eps * scale
    cosine = abs(_dot(n, q)) / (nlen * math.sqrt(_dot(q, q)))
    und = und or _close(cosine, min_cos, eps)
    if not cosine >= min_cos:
        return None, und
    hc, wc = frame.shape[:2]
    uc, vc = _project(k_color, q)
    x, y = uc - pc, vc - pc
    und = und or _close(x, 0.0, eps) or _close(x, wc - 1.0, eps) or _close(y, 0.0, eps) or _close(y, hc - 1.0, eps)
    if not (0.0 <= x <= wc - 1 and 0.0 <= y <= hc - 1):
        return None, und
    und = und or _near_integer(x, eps) or _near_integer(y, eps)
    x0, y0 = min(math.floor(x), wc - 2), min(math.floor(y), hc - 2)
    fx, fy = x - x0, y - y0
    weight = cosine / (z * z)
    out = []
    for ch in range(3):
        top = (1.0 - fx) * float(frame[y0, x0, ch]) + fx * float(frame[y0, x0 + 1, ch])
        bottom = (1.0 - fx) * float(frame[y0 + 1, x0, ch]) + fx * float(frame[y0 + 1, x0 + 1, ch])
        out.append(weight * ((1.0 - fy) * top + fy * bottom))
    return (out[0], out[1], out[2], weight), und


def colorize(verts, faces, k_color, k_vis, poses, frames, vis, pixel_center=0.5, znear=0.05, zfar=100.0, tolerance=0.04,
             min_cos=0.1, min_views=1, fallback=(153, 153, 153), eps=EPS, round_eps=ROUND_EPS):
    """verts [N,3] (read as float32), faces [M,3], poses [V,4,4] camera -> world, frames u8[V,Hc,Wc,3], vis u64[V,Hd,Wd] ->
    {acc f64[N,4], seen int32[N], rgb u8[N,3], value f64[N,3] (the channels before rounding, nan where the fallback is
    taken), undecided bool[N]}; pixel_center, znear, zfar are taken as float32 values, as the entry takes them"""
    verts = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3).tolist()
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    k_color, k_vis = np.asarray(k_color, np.float64).tolist(), np.asarray(k_vis, np.float64).tolist()
    w2c = [np.linalg.inv(np.asarray(p, np.float64))[:3, :4].tolist() for p in np.asarray(poses, np.float64).reshape(-1, 4, 4)]
    frames, vis = np.asarray(frames, np.uint8), np.asarray(vis).view(np.uint64)
    pc, zn, zf = float(np.float32(pixel_center)), float(np.float32(znear)), float(np.float32(zfar))
    n = len(verts)
    acc, seen = np.zeros((n, 4), np.float64), np.zeros(n, np.int32)
    rgb, value, undecided = np.zeros((n, 3), np.uint8), np.full((n, 3), np.nan), np.zeros(n, bool)
    for i, p in enumerate(verts):
        s = [0.0, 0.0, 0.0, 0.0]
        for v, m in enumerate(w2c):
            got, und = pair(p, m, verts, faces, k_color, k_vis, frames[v], vis[v], pc, zn, zf, float(tolerance), float(min_cos), eps)
            undecided[i] |= und
            if got is not None:
                s = [s[k] + got[k] for k in range(4)]
                seen[i] += 1
        acc[i] = s
        if seen[i] >= min_views and s[3] > 0.0:
            for ch in range(3):
                val = s[ch] / s[3]
                value[i, ch] = val
                rgb[i, ch] = int(min(255.0, math.floor(val + 0.5)))
                undecided[i] |= abs(val + 0.5 - math.floor(val + 0.5 + 0.5)) <= round_eps
        else:
            rgb[i] = fallback
    return {"acc": acc, "seen": seen, "rgb": rgb, "value": value, "undecided": undecided}


def pack_visibility(depth, face):
    """depth f64[...] (0 = no hit), face int[...] (-1) -> the u64 words of a visibility buffer: fp32 depth bits << 32 | face"""
    bits = np.asarray(depth, np.float32).view(np.uint32).astype(np.uint64)
    words = (bits << np.uint64(32)) | np.asarray(np.maximum(face, 0), np.uint64)
    return np.where(np.asarray(face) >= 0, words, np.uint64(0xFFFFFFFFFFFFFFFF))

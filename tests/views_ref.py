"""numpy restatement of the view preparation (the 8-bit bilinear resize of a colour frame, the depth conversion): the
independent reference of tests/test_views_host.py and tests/test_views_gpu.py.  It shares no code with eprecon_amd.

The resize is two passes of integer arithmetic, horizontal first, each pass rounded to uint8:

    scale = in / out, fs = max(scale, 1), support = fs, ksize = 2 * ceil(support) + 1
    centre = (xx + 0.5) * scale
    xmin = max(int(centre - support + 0.5), 0), xmax = min(int(centre + support + 0.5), in), n = xmax - xmin
    w[x] = max(0, 1 - |(x + xmin - centre + 0.5) / fs|), divided by their sum (accumulated in index order)
    k[x] = int(0.5 + w[x] * 2^22)
    out = clamp((2^21 + sum pixel * k) >> 22, 0, 255)

Rows above and below the frame (`pad_top`, `pad_bottom`) are black.
"""
import math

import numpy as np

PRECISION_BITS = 22


def coefficients(n_in, n_out):
    """-> (bounds int32[n_out, 2] = (xmin, n), k int32[n_out, ksize]) of one axis, float64 on the host"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        centre = (xx + 0.5) * scale
        xmin = max(int(centre - support + 0.5), 0)
        xmax = min(int(centre + support + 0.5), n_in)
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - centre + 0.5) / fs)) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        for x in range(n):
            k[xx, x] = int(0.5 + (w[x] / total) * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return bounds, k


def _pass(img, bounds, k):
    """the resampling along axis 1 of uint8[R, n_in, C] -> uint8[R, n_out, C]"""
    out = np.zeros((img.shape[0], bounds.shape[0], img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (src[:, xmin:xmin + n] * k[xx, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, out_hw, pad_top=0, pad_bottom=0):
    """uint8[H, W, 3] -> uint8[h, w, 3]: the frame between pad_top and pad_bottom black rows, resized"""
    h, w = out_hw
    canvas = np.zeros((pad_top + img.shape[0] + pad_bottom,) + img.shape[1:], np.uint8)
    canvas[pad_top:pad_top + img.shape[0]] = img
    rows = _pass(canvas, *coefficients(canvas.shape[1], w))
    return _pass(rows.transpose(1, 0, 2), *coefficients(canvas.shape[0], h)).transpose(1, 0, 2)


def prepare_views(frames, out_hw, pad_top=0, pad_bottom=0):
    """uint8[V, H, W, 3] -> f32[V, 3, h, w]"""
    out = np.stack([resize(f, out_hw, pad_top, pad_bottom) for f in frames])
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)).astype(np.float32)


def depth_to_metres(depth_mm, max_depth=3.0):
    """uint16 millimetres -> float32 metres, values beyond max_depth zeroed (the reference's read_depth)"""
    d = depth_mm.astype(np.float32)
    d /= 1000.
    d[d > max_depth] = 0
    return d

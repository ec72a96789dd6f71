"""Writes tests/golden/views.npz: colour strips and what PIL's resize(BILINEAR) makes of them (PIL only; run by hand).

    python tests/golden/make_views_golden.py

Two strips at the production ratio of a 1296 x 968 ScanNet frame resized to 640 x 480 (81 / 40 = 1296 / 640 = 2.025, the
second one standing between 2 + 2 black rows as such a frame does on its 1296 x 972 canvas), and one upscaling case.
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# name: (height, width, pad_top, pad_bottom, out_h, out_w)
CASES = {"strip": (81, 1296, 0, 0, 40, 640), "strip_padded": (77, 1296, 2, 2, 40, 640), "upscale": (30, 40, 0, 0, 48, 64)}


def frame(rng, h, w):
    """a smooth colour field with texture, edges and saturated patches, uint8[h, w, 3]"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 120 * np.sin(x / 37.0 + y / 11.0), 127 + 120 * np.cos(x / 23.0 - y / 7.0), (x * 3 + y * 5) % 256], -1)
    img += rng.normal(0, 25, img.shape)
    img[:, w // 3:w // 3 + 5] = 255
    img[h // 2:h // 2 + 2] = 0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20)
    out = {}
    for name, (h, w, top, bottom, out_h, out_w) in CASES.items():
        # one frame per case keeps the file under 1 MB (the texture does not compress); the channels are resampled
        # independently, so a test gets a second, different view by reversing the channels of both arrays
        f = frame(rng, h, w)
        canvas = Image.new("RGB", (w, top + h + bottom))
        canvas.paste(Image.fromarray(f), (0, top))
        out[name + "/frame"] = f
        out[name + "/pad"] = np.array([top, bottom], np.int32)
        out[name + "/resized"] = np.asarray(canvas.resize((out_w, out_h), Image.BILINEAR))
    path = os.path.join(HERE, "views.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

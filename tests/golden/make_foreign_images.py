"""Regenerates the committed fixtures tests/golden/foreign.{png,tiff,jpg,exr}: one small RGBA picture written by other
libraries than this repository's own writers -- libpng, libtiff and libjpeg through Pillow -- and as an uncompressed half-float
RGBA OpenEXR file (channels stored A B G R) by the byte-level writer of the tests (tests/helpers.py make_exr), which follows the
file-format description independently of the library's reader. tests/test_image_formats.py decodes them with the library.

    python tests/golden/make_foreign_images.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.helpers import make_exr  # noqa: E402


def picture(w=48, h=32):
    """Smooth gradients, a disc and a ramp of transparency: every channel varies, no noise (JPEG decoders agree on it)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    r = x / (w - 1)
    g = y / (h - 1)
    b = 0.5 + 0.5 * np.cos(np.hypot(x - w / 2, y - h / 2) / 5.0)
    a = np.where(np.hypot(x - w / 3, y - h / 2) < h / 3, 1.0, 0.4 + 0.6 * r)
    return np.round(np.stack([r, g, b, a], axis=-1) * 255.0).astype(np.uint8)


def main():
    rgba = picture()
    im = Image.fromarray(rgba, "RGBA")
    for ext, fmt in (("png", "PNG"), ("tiff", "TIFF")):
        im.save(os.path.join(HERE, "foreign." + ext), fmt)
    buf = io.BytesIO()
    im.convert("RGB").save(buf, "JPEG", quality=90)
    open(os.path.join(HERE, "foreign.jpg"), "wb").write(buf.getvalue())
    f = rgba.astype(np.float32) / 255.0
    planes = {c: np.ascontiguousarray(f[:, :, i]).astype(np.float16) for i, c in enumerate("RGBA")}
    open(os.path.join(HERE, "foreign.exr"), "wb").write(make_exr(planes, 0))


if __name__ == "__main__":
    main()

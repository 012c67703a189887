"""Writes tests/golden/g17_cls_resize.npz: small uint8 images, crop boxes, and what Pillow itself makes of them -- `Image.crop(box).resize((ow, oh), BILINEAR)`.
tests/test_cls_augment_cpu.py holds frostnet_amd.cls_augment.resize_crop bit-equal to these, so the comparison with Pillow never turns into a skip where Pillow is
absent.  Needs Pillow (generated with 12.2); nothing else in the project does.

    python tools/gen_cls_resize_golden.py
"""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (image h, image w, box x0, y0, w, h, output w, h): every image at most 64 pixels a side
CASES = [
    (37, 53, 0, 0, 53, 37, 224, 224),          # up-scale
    (64, 64, 0, 0, 64, 64, 64, 64),            # identity: both passes skipped by Pillow
    (64, 48, 0, 0, 48, 64, 30, 40),            # scale in (1, 2)
    (64, 64, 0, 0, 64, 64, 24, 20),            # scale > 2, different per axis
    (1, 1, 0, 0, 1, 1, 8, 8),
    (3, 64, 0, 0, 64, 3, 16, 16),              # a thin strip: up in one axis, down by 4 in the other
    (32, 64, 0, 0, 64, 32, 40, 32),            # one axis unchanged
    (64, 64, 5, 9, 41, 33, 32, 32),            # a crop inside the image: the filter's support is clipped to the crop
    (64, 64, 23, 0, 41, 64, 7, 7),             # touching the right and the top border; scale > 4
    (64, 64, 0, 31, 17, 33, 32, 32),           # touching the left and the bottom border; up in x, about 1 in y
]


def main():
    rng = np.random.default_rng(1717)
    out = {"cases": np.asarray(CASES, dtype=np.int32)}
    for i, (h, w, x0, y0, cw, ch, ow, oh) in enumerate(CASES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).crop((x0, y0, x0 + cw, y0 + ch)).resize((ow, oh), Image.BILINEAR))
        assert ref.shape == (oh, ow, 3) and ref.dtype == np.uint8
        out[f"img{i}"], out[f"ref{i}"] = img, ref
    path = os.path.join(ROOT, "tests", "golden", "g17_cls_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Generate tests/golden/g19_seg_augment.npz by RUNNING the reference's segmentation transforms (dev container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_seg_augment.py

Imports Semantic_Segmentation/utilities/data_transforms.py through tools/refshim.py and drives the reference's own `Compose` in both recipe orders
(data_loader/segmentation/voc.py: RandomFlip, RandomScale, RandomCrop, Normalize; cityscapes.py: RandomScale, RandomCrop, RandomFlip, Normalize) and both validation
recipes, with `random.random` / `random.randint` of that module replaced by a scripted sequence.  The fixture holds DATA only, per case: the picture and the label
map that went in, the decisions the run took as the words of a frostnet_amd.seg_augment plan record (grid, window offset, mirror: the grid is what
`Image.resize` was asked for, observed, not recomputed), and the picture and label tensors the reference returned.
"""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
from PIL import Image

import refshim
from frostnet_amd import seg_augment as S

OUT = os.path.join(ROOT, "tests", "golden", "g19_seg_augment.npz")


class Script:
    """Stands in for the `random` module of data_transforms.py: random() and randint() hand out what the case wrote down, and keep what they were asked."""

    def __init__(self, units, ints):
        self.units, self.ints, self.asked = list(units), list(ints), []

    def random(self):
        return self.units.pop(0)

    def randint(self, a, b):
        v = self.ints.pop(0)
        assert a <= v <= b, (a, v, b)
        self.asked.append((a, b, v))
        return v


def picture(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def label_map(rng, h, w, palette):
    """Blocks of classes 0 .. 20 with 255 (ignore) scattered in: mode L, or mode P with a palette as the PASCAL VOC annotation files have one."""
    lab = np.kron(rng.integers(0, 21, ((h + 2) // 3, (w + 3) // 4)), np.ones((3, 4), dtype=np.int64))[:h, :w].astype(np.uint8)
    lab[rng.random((h, w)) < 0.08] = 255
    lab[0, 0] = 255
    img = Image.fromarray(lab, mode="L")
    if palette:
        img = Image.fromarray(lab, mode="P")
        img.putpalette([(i * 7) % 256 for i in range(768)])
    return lab, img


# name, order, (h, w), scale, crop (w, h), palette, units (in the order the recipe draws them), ints (row offset, column offset)
TRAIN = [
    ("voc_s1_flip", "voc", (24, 32), (0.5, 2.0), (20, 17), False, [0.1, 0.5], [5, 9]),
    ("voc_half_pad_w", "voc", (24, 32), (0.5, 2.0), (20, 10), False, [0.9, 0.0], [1, 0]),
    ("voc_half_pad_both_odd_1", "voc", (24, 32), (0.5, 2.0), (20, 17), False, [0.7, 0.0], [1, 0]),
    ("voc_half_pad_both_odd_0_flip", "voc", (24, 32), (0.5, 2.0), (20, 17), False, [0.2, 0.0], [0, 0]),
    ("city_s2_flip", "city", (10, 15), (2.0, 2.0), (20, 12), False, [0.4, 0.3], [7, 9]),
    ("city_s1_equal", "city", (17, 20), (0.5, 2.0), (20, 17), False, [0.5, 0.8], []),
    ("city_half_pad_w_odd_1_flip", "city", (15, 23), (0.5, 2.0), (19, 8), False, [0.0, 0.1], [0, 1]),
    ("voc_palette_flip", "voc", (23, 31), (0.5, 1.0), (15, 12), True, [0.3, 0.3], [2, 3]),
    ("city_palette_flip", "city", (21, 19), (0.5, 2.0), (20, 20), True, [0.77, 0.45], [6, 4]),
    ("voc_s2_pad_both", "voc", (8, 6), (2.0, 2.0), (20, 20), False, [0.6, 0.5], []),
]
# name, (h, w), size (w, h) or None, palette
EVAL = [
    ("val_voc_down", (24, 32), (20, 15), True),
    ("val_voc_up", (10, 9), (17, 20), False),
    ("val_city", (12, 16), None, False),
]


def main():
    T = refshim.load_seg_transforms()
    rng = np.random.default_rng(19)
    asked_sizes = []
    resize = Image.Image.resize

    def watched(self, size, *a, **k):
        asked_sizes.append(tuple(size))
        return resize(self, size, *a, **k)

    Image.Image.resize = watched
    arrs, names = {}, []
    try:
        for name, order, (h, w), scale, crop, palette, units, ints in TRAIN:
            img, (lab, lab_img) = picture(rng, h, w), label_map(rng, h, w, palette)
            T.random = script = Script(units, ints)
            scale_crop = [T.RandomScale(scale=scale), T.RandomCrop(crop_size=crop)]
            recipe = T.Compose([T.RandomFlip()] + scale_crop + [T.Normalize()] if order == "voc" else scale_crop + [T.RandomFlip(), T.Normalize()])
            del asked_sizes[:]
            flip_unit = units[0] if order == "voc" else units[1]
            x, t = recipe(Image.fromarray(img), lab_img)
            assert not script.units and not script.ints and len(asked_sizes) == 2 and asked_sizes[0] == asked_sizes[1]
            rw, rh = asked_sizes[0]
            pw, ph = S._pad(crop[0], rw), S._pad(crop[1], rh)
            (_, _, i), (_, _, j) = script.asked if script.asked else ((0, 0, 0), (0, 0, 0))
            flags = S.F_LANCZOS | (S.F_FLIP_FIRST if order == "voc" else 0) | (S.F_MIRROR if flip_unit < 0.5 else 0)
            plan = np.array([flags, rw, rh, j - pw, i - ph, pw, ph, 0], dtype=np.int32)
            names.append(name)
            arrs.update({f"{name}_img": img, f"{name}_lab": lab, f"{name}_plan": plan, f"{name}_crop": np.array(crop, dtype=np.int32),
                         f"{name}_x": x.numpy(), f"{name}_t": t.numpy().astype(np.uint8)})
            assert int(t.max()) <= 255 and tuple(x.shape) == (3, crop[1], crop[0])
            print(f"{name:32s} grid {rw} x {rh} pads {pw} {ph} offset {j - pw} {i - ph} asked {script.asked} flags {flags}")
        for name, (h, w), size, palette in EVAL:
            img, (lab, lab_img) = picture(rng, h, w), label_map(rng, h, w, palette)
            recipe = T.Compose(([T.Resize(size=size)] if size is not None else []) + [T.Normalize()])
            x, t = recipe(Image.fromarray(img), lab_img)
            rw, rh = size if size is not None else (w, h)
            plan = np.array([S.F_TRIANGLE if size is not None else 0, rw, rh, 0, 0, 0, 0, 0], dtype=np.int32)
            names.append(name)
            arrs.update({f"{name}_img": img, f"{name}_lab": lab, f"{name}_plan": plan, f"{name}_crop": np.array((rw, rh), dtype=np.int32),
                         f"{name}_x": x.numpy(), f"{name}_t": t.numpy().astype(np.uint8)})
            print(f"{name:32s} grid {rw} x {rh}")
    finally:
        Image.Image.resize = resize
    arrs["names"] = np.asarray(names)
    arrs["meta_pillow_version"] = np.asarray(Image.__version__ if hasattr(Image, "__version__") else "")
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

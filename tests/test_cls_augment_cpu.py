"""The CPU definition of the classifier's input pipeline (frostnet_amd/cls_augment.py), which is the yardstick of tests/test_gpu_cls_augment.py: the resampler against
Pillow itself (a golden file made by tools/gen_cls_resize_golden.py, and live Pillow where it imports), the crop decisions against known answers and torchvision's
rules, the validation plan, the output arithmetic, and the whole call."""
import math

import numpy as np
import pytest
import torch

from frostnet_amd import augment as A
from frostnet_amd import cls_augment as CA


def _sizes(rows):
    return torch.tensor(rows, dtype=torch.int32)


# ---- the resampler ---------------------------------------------------------------------------------------------------------------------------------------
def test_resize_equals_pillow_golden_bit_for_bit(golden):
    g = golden("g17_cls_resize")
    cases = g["cases"].tolist()
    assert len(cases) == 10
    for i, (h, w, x0, y0, cw, ch, ow, oh) in enumerate(cases):
        img, ref = g[f"img{i}"], g[f"ref{i}"]
        assert img.shape == (h, w, 3) and ref.shape == (oh, ow, 3)
        got = CA.resize_crop(img[y0:y0 + ch, x0:x0 + cw], ow, oh)
        diff = int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
        print(f"[golden case {i}: {ch}x{cw} -> {oh}x{ow}] max |definition - Pillow| = {diff}")
        assert np.array_equal(got, ref), (i, diff)


# (h, w) -> (oh, ow): up-scale, identity, scale in (1, 2), scale > 2, 1x1, a strip, one axis unchanged, and the two production shapes
LIVE = [(37, 53, 224, 224), (224, 224, 224, 224), (300, 250, 224, 224), (700, 600, 224, 224), (1, 1, 8, 8), (3, 700, 16, 16), (224, 300, 224, 224),
        (375, 500, 224, 224), (480, 640, 256, 341)]


def test_resize_equals_live_pillow_on_larger_shapes():
    Image = pytest.importorskip("PIL.Image")          # the golden test above carries the comparison where Pillow is absent
    rng = np.random.default_rng(5)
    for h, w, oh, ow in LIVE:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(CA.resize_crop(img, ow, oh), ref), (h, w, oh, ow)
    # a window of the validation grid equals the same window of the whole resize
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((341, 256), Image.BILINEAR))[16:240, 58:282]
    assert np.array_equal(CA.resize_crop(img, 341, 256, 58, 16, 224, 224), ref)


def test_coefficients_are_pillows_fixed_point():
    """Identity: one tap of 2^22.  2x down-scale: the triangle (1, 3, 3, 1) / 8 inside the image."""
    xmin, c = CA.resample_coeffs(8, 8, 0, 8)
    assert xmin.tolist() == list(range(8)) and (c[:, 0] == 1 << 22).all() and (c[:, 1:] == 0).all()
    xmin, c = CA.resample_coeffs(16, 8, 2, 1)
    assert xmin.tolist() == [3] and c[0].tolist() == [1 << 19, 3 << 19, 3 << 19, 1 << 19, 0]


# ---- the crop decisions ----------------------------------------------------------------------------------------------------------------------------------
def test_exp_polynomial_against_libm():
    """Derived bound: 13 multiply-add pairs, each rounding relative 2^-53 of a partial sum below e^0.29 -> about 4e-15; asserted at 1e-14."""
    lo, hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
    worst = max(abs(CA.exp_poly(lo + (hi - lo) * k / 10000.0) / math.exp(lo + (hi - lo) * k / 10000.0) - 1.0) for k in range(10001))
    print(f"[exp_poly] max relative error on 10001 points = {worst:.3e}")
    assert worst <= 1e-14


def test_plan_known_answers_under_a_fixed_seed():
    aug = CA.ClassificationAugmentation(seed=1)
    plan = aug.plan(_sizes([[375, 500], [8, 64], [1, 1], [64, 8]]))
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (4, CA.PLAN_WORDS)
    assert plan.tolist() == [[0, 168, 33, 302, 331, 224, 224, 0, 0, 2, 0, 0],
                             [3, 26, 0, 11, 8, 224, 224, 0, 0, 10, 0, 0],          # the fallback of a 8 x 64 (h x w) image: h = 8, w = rint(8 * 4/3) = 11, centred
                             [0, 0, 0, 1, 1, 224, 224, 0, 0, 2, 0, 0],
                             [2, 0, 26, 8, 11, 224, 224, 0, 0, 10, 0, 0]]
    assert aug.images_seen() == 4


def test_accepted_rects_follow_torchvisions_rules():
    rng = np.random.default_rng(3)
    sizes = _sizes(rng.integers(1, 600, (400, 2)).tolist())
    aug = CA.ClassificationAugmentation(seed=99)
    p = aug.plan(sizes).numpy().astype(np.int64)
    h0, w0 = sizes[:, 0].numpy(), sizes[:, 1].numpy()
    x0, y0, w, h = p[:, CA.P_X0], p[:, CA.P_Y0], p[:, CA.P_W], p[:, CA.P_H]
    assert (x0 >= 0).all() and (y0 >= 0).all() and (w >= 1).all() and (h >= 1).all() and (x0 + w <= w0).all() and (y0 + h <= h0).all()
    acc = (p[:, CA.P_FLAGS] & CA.F_FALLBACK) == 0
    assert acc.sum() > 200 and (~acc).sum() > 0
    assert ((p[:, CA.P_TRIES] >= 1) & (p[:, CA.P_TRIES] <= CA.TRIALS)).all() and (p[~acc, CA.P_TRIES] == CA.TRIALS).all()
    # w = rint(sqrt(t a)), h = rint(sqrt(t / a)): each within 1/2 of its real value, so (w - 1/2) / (h + 1/2) <= a <= (w + 1/2) / (h - 1/2) with a in [3/4, 4/3]
    wa, ha = w[acc].astype(np.float64), h[acc].astype(np.float64)
    assert ((wa - 0.5) / (ha + 0.5) <= 4.0 / 3.0 + 1e-12).all() and ((wa + 0.5) / np.maximum(ha - 0.5, 1e-300) >= 3.0 / 4.0 - 1e-12).all()
    # ... and the area within the scale bounds, with the same slack
    area = (h0 * w0)[acc].astype(np.float64)
    assert ((wa - 0.5) * (ha - 0.5) <= area * 1.0 + 1e-9).all() and ((wa + 0.5) * (ha + 0.5) >= area * 0.08 - 1e-9).all()
    assert len(set((p[:, CA.P_FLAGS] & CA.F_MIRROR).tolist())) == 2
    assert (p[:, CA.P_RW] == 224).all() and (p[:, CA.P_RH] == 224).all() and (p[:, CA.P_OX] == 0).all() and (p[:, CA.P_OY] == 0).all()


def test_fallback_rects():
    """scale = (0.5, 1) on an 8 x 64 image: every trial's h = sqrt(>= 256 / a) >= 13.8 > 8 fails, whatever is drawn."""
    aug = CA.ClassificationAugmentation(scale=(0.5, 1.0), seed=7)
    p = aug.plan(_sizes([[8, 64]] * 5 + [[64, 8]] * 5)).numpy()
    assert (p[:, CA.P_FLAGS] & CA.F_FALLBACK).all() and (p[:, CA.P_TRIES] == 10).all()
    assert (p[:5, CA.P_X0:CA.P_H + 1] == [26, 0, 11, 8]).all()          # in_ratio 8 > 4/3: h = h0, w = rint(8 * 4/3) = 11, X0 = (64 - 11) // 2
    assert (p[5:, CA.P_X0:CA.P_H + 1] == [0, 26, 8, 11]).all()          # in_ratio 1/8 < 3/4: w = w0, h = rint(8 / (3/4)) = 11
    # a ratio range that excludes the image's own ratio on neither side: the whole image (scale > 1 makes every trial fail)
    p = CA.ClassificationAugmentation(scale=(1.5, 2.0), seed=7).plan(_sizes([[30, 40]])).numpy()
    assert p[0, CA.P_FLAGS] & CA.F_FALLBACK and p[0, CA.P_X0:CA.P_H + 1].tolist() == [0, 0, 40, 30]
    # 1 x 1: the only rect there is
    p = CA.ClassificationAugmentation(seed=5).plan(_sizes([[1, 1]] * 20)).numpy()
    assert (p[:, CA.P_X0:CA.P_H + 1] == [0, 0, 1, 1]).all()


def test_stream_is_its_own_and_resumes():
    assert CA.STREAM_TAG != A.STREAM_TAG and CA.STREAM_TAG != 0x53534441
    a, b = CA._Draws(5, 9), A._Draws(5, 9)
    assert [a.word() for _ in range(8)] != [b.word() for _ in range(8)]
    sizes = _sizes([[100, 120], [300, 200], [50, 50]])
    one = CA.ClassificationAugmentation(seed=11)
    first = one.plan(sizes)
    state = one.state_dict()
    assert state == {"seed": 11, "images_seen": 3}
    second = one.plan(sizes)
    two = CA.ClassificationAugmentation(seed=0)
    two.load_state_dict(state)
    assert torch.equal(two.plan(sizes), second) and not torch.equal(first, second)
    # the ordinal, not the call, carries the position: one call on six images = two calls on three
    both = CA.ClassificationAugmentation(seed=11).plan(torch.cat([sizes, sizes]))
    assert torch.equal(both, torch.cat([first, second]))
    assert CA.ClassificationAugmentation(seed=None).seed == A.default_seed() & A._M64


# ---- the validation plan ---------------------------------------------------------------------------------------------------------------------------------
def test_eval_plan():
    t = CA.ClassificationEvalTransform()
    p = t.plan(_sizes([[480, 640], [640, 480], [300, 300], [375, 500]])).tolist()
    assert p[0] == [0, 0, 0, 640, 480, 341, 256, 58, 16, 0, 0, 0]          # round(58.5) = 58: half to even
    assert p[1] == [0, 0, 0, 480, 640, 256, 341, 16, 58, 0, 0, 0]
    assert p[2] == [0, 0, 0, 300, 300, 256, 256, 16, 16, 0, 0, 0]
    assert p[3] == [0, 0, 0, 500, 375, 341, 256, 58, 16, 0, 0, 0]
    assert [CA._half_even(d) for d in (0, 1, 2, 3, 117, 119, 32)] == [round(d / 2) for d in (0, 1, 2, 3, 117, 119, 32)] == [0, 0, 1, 2, 58, 60, 16]
    p = CA.ClassificationEvalTransform(size=32, resize=36).plan(_sizes([[50, 101]])).tolist()
    assert p[0][CA.P_RW] == int(36 * 101 / 50) == 72 and p[0][CA.P_RH] == 36 and p[0][CA.P_OX] == 20 and p[0][CA.P_OY] == 2
    with pytest.raises(ValueError):
        CA.ClassificationEvalTransform(size=224, resize=200)


# ---- the output ------------------------------------------------------------------------------------------------------------------------------------------
def test_table_is_totensor_and_normalize_in_fp32():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    tab = torch.from_numpy(CA.norm_table(mean, std))
    v = torch.arange(256, dtype=torch.float32)
    for c in range(3):
        want = v.div(255).sub(mean[c]).div(std[c])
        assert want.dtype == torch.float32 and torch.equal(tab[c].view(torch.int32), want.view(torch.int32)), c


def _batch(sentinel):
    """Three images in 48 x 56 slots whose padding holds a sentinel."""
    rng = np.random.default_rng(21)
    dims = [(48, 40), (30, 56), (17, 23)]
    images = np.full((3, 48, 56, 3), sentinel, dtype=np.uint8)
    for i, (h, w) in enumerate(dims):
        images[i, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return torch.from_numpy(images), _sizes(dims)


def test_whole_call_mirror_layout_and_padding():
    images, sizes = _batch(0)
    images255, _ = _batch(255)
    aug = CA.ClassificationAugmentation(size=20, seed=4)
    x = aug(images, sizes)
    plan = aug.last_plan
    assert x.dtype == torch.float32 and tuple(x.shape) == (3, 3, 20, 20) and x.is_contiguous()
    # the padding of a slot influences nothing
    assert torch.equal(aug.apply(images255, sizes, plan), x)
    # pixel for pixel: crop, resize, table
    tab = CA.norm_table(aug.mean, aug.std)
    for i in range(3):
        x0, y0, w, h = plan[i, CA.P_X0:CA.P_H + 1].tolist()
        win = CA.resize_crop(images[i, y0:y0 + h, x0:x0 + w].numpy(), 20, 20)
        if int(plan[i, CA.P_FLAGS]) & CA.F_MIRROR:
            win = win[:, ::-1]
        for c in range(3):
            assert np.array_equal(x[i, c].numpy(), tab[c][win[..., c]])
    # the mirror acts on the resized window
    flipped = plan.clone()
    flipped[:, CA.P_FLAGS] ^= CA.F_MIRROR
    assert torch.equal(aug.apply(images, sizes, flipped), x.flip(3))
    # channels-last: the same values in the other memory format
    cl = CA.ClassificationAugmentation(size=20, seed=4, channels_last=True)
    y = cl(images, sizes)
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, x) and torch.equal(cl.last_plan, plan)
    # the validation transform: the central window of the whole image's resize
    ev = CA.ClassificationEvalTransform(size=20, resize=24)
    z = ev(images, sizes)
    assert torch.equal(ev(images255, sizes), z) and tuple(z.shape) == (3, 3, 20, 20)
    grid = CA.resize_crop(images[1, :30, :56].numpy(), 24 * 56 // 30, 24)
    ox = CA._half_even(24 * 56 // 30 - 20)
    assert np.array_equal(z[1, 0].numpy(), tab[0][grid[2:22, ox:ox + 20, 0]])
    # size 32 (the CIFAR recipes) is a size like any other
    assert tuple(CA.ClassificationAugmentation(size=32, seed=1)(images, sizes).shape) == (3, 3, 32, 32)


def test_argument_errors():
    images, sizes = _batch(0)
    aug = CA.ClassificationAugmentation(size=16, seed=1)
    for bad in ((images.float(), sizes), (images[0], sizes), (images, sizes.long()), (images, sizes[:2]), (images[..., :2], sizes)):
        with pytest.raises(ValueError):
            aug(*bad)
        with pytest.raises(ValueError):
            CA.ClassificationEvalTransform(size=16, resize=16)(*bad)
    with pytest.raises(ValueError):
        aug(images, _sizes([[49, 40], [30, 56], [17, 23]]))          # a size beyond its slot
    plan = aug.plan(sizes)
    plan[0, CA.P_W] = 57
    with pytest.raises(ValueError):
        aug.apply(images, sizes, plan)                                # a rect beyond its image
    for kw in (dict(size=0), dict(scale=(0.5, 0.1)), dict(ratio=(0.1, 1.0)), dict(std=(1.0, 0.0, 1.0)), dict(mean=(1.0, 2.0))):
        with pytest.raises(ValueError):
            CA.ClassificationAugmentation(**kw)
    assert aug.images_seen() == 3


def test_public_names():
    import frostnet_amd
    assert frostnet_amd.ClassificationAugmentation is CA.ClassificationAugmentation and frostnet_amd.ClassificationEvalTransform is CA.ClassificationEvalTransform
    assert CA.PLAN_WORDS == 12 and (CA.P_FLAGS, CA.P_X0, CA.P_Y0, CA.P_W, CA.P_H, CA.P_RW, CA.P_RH, CA.P_OX, CA.P_OY, CA.P_TRIES) == tuple(range(10))

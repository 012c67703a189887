"""The CPU definition of the batch augmentation (frostnet_amd/augment.py on CPU tensors), which is the yardstick of tests/test_gpu_augment.py.  The reference module
(Object_Detection/utils/augmentations.py) imports cv2 and torchvision, neither of which this project's tests can use, so there is no recorded reference output
for it: the definition is pinned here by known answers, by Pillow where Pillow computes the same thing (bilinear up-scaling), by round trips of the colour
conversions, by hand-applied formulas for every switch, by geometry constructed so that the answer is the source itself, and by the properties the sampler's
output must have."""
import numpy as np
import pytest
import torch

from frostnet_amd import augment as A

f32 = np.float32
EPS = f32(1.1920928955078125e-07)


def _plan(sizes, **words):
    """identity_plan with some words replaced: name -> value (one for all images), floats for the fp32 words."""
    plan = A.identity_plan(sizes)
    for name, v in words.items():
        w = getattr(A, "P_" + name.upper())
        if w in A.FLOAT_WORDS:
            plan.view(torch.float32)[:, w] = float(v)
        else:
            plan[:, w] = int(v)
    return plan


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _apply(img, size, plan_words, mean=(104, 117, 123)):
    images, sizes = A.pad_images([img])
    return A.SSDAugmentation(size=size, mean=mean, seed=0).apply(images, sizes, _plan(sizes, **plan_words))[0].numpy()


# ---- the test's own scalar restatement of OpenCV's float colour conversions ------------------------------------------------------------------------------
def _to_hsv(b, g, r):
    v = max(r, g, b)
    diff = f32(v - min(r, g, b))
    s = f32(diff / f32(abs(v) + EPS))
    d = f32(f32(60) / f32(diff + EPS))
    if v == r:
        h = f32(f32(g - b) * d)
    elif v == g:
        h = f32(f32(f32(b - r) * d) + f32(120))
    else:
        h = f32(f32(f32(r - g) * d) + f32(240))
    if h < 0:
        h = f32(h + f32(360))
    return h, s, v


def _to_bgr(h, s, v):
    h = f32(h * f32(1.0 / 60.0))
    if h < 0:
        h = f32(h + f32(6))
    if h >= 6:
        h = f32(h - f32(6))
    sector = int(np.floor(h))
    f = f32(h - f32(sector))
    one = f32(1)
    tab = (v, f32(v * f32(one - s)), f32(v * f32(one - f32(s * f))), f32(v * f32(one - f32(s * f32(one - f)))))
    ib, ig, ir = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))[sector]
    return tab[ib], tab[ig], tab[ir]


def _hand(img, mean, delta=0.0, pre=1.0, post=1.0, sat=1.0, hue=0.0, perm=(0, 1, 2), hsv=True):
    """The photometric chain applied by hand, pixel by pixel, minus the mean: [3, h, w]."""
    out = np.zeros(img.shape, dtype=np.float32)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            b, g, r = (f32(f32(f32(c) + f32(delta)) * f32(pre)) for c in img[y, x])
            if hsv:
                h, s, v = _to_hsv(b, g, r)
                s = f32(s * f32(sat))
                h = f32(h + f32(hue))
                if h > 360:
                    h = f32(h - f32(360))
                if h < 0:
                    h = f32(h + f32(360))
                b, g, r = _to_bgr(h, s, v)
            px = [f32(c * f32(post)) for c in (b, g, r)]
            out[y, x] = [px[perm[0]], px[perm[1]], px[perm[2]]]
    return (out - np.asarray(mean, dtype=np.float32)).transpose(2, 0, 1)


# ---- pixels --------------------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_known_answer():
    """Source [[0, 10], [20, 30]] to 4 x 4: source coordinates -0.25, 0.25, 0.75, 1.25 per axis, clamped, i.e. the weights (1, 0), (.75, .25), (.25, .75), (0, 1)."""
    src = np.array([[0, 10], [20, 30]], dtype=np.uint8)
    out = _apply(np.repeat(src[:, :, None], 3, 2), 4, {}, mean=(0, 0, 0))
    wts = np.array([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1]], dtype=np.float32)
    want = (wts @ src.astype(np.float32) @ wts.T).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == (3, 4, 4)
    for c in range(3):
        assert np.array_equal(out[c], want), (out[c], want)


@pytest.mark.parametrize("hw", [(5, 7), (3, 3)])
@pytest.mark.parametrize("size", [8, 16, 32])
def test_upscaling_matches_pillow(hw, size):
    """Pillow's BILINEAR on mode-F images is the same convention when up-scaling (it antialiases when down-scaling, so it is no yardstick there).
    Bound 6.1e-5 = 4 ulp at 255: three lerps of three roundings each here against Pillow's single rounding."""
    Image = pytest.importorskip("PIL.Image")
    img = _img(hw[0], hw[1], 11 + size)
    out = _apply(img, size, {}, mean=(0, 0, 0))
    for c in range(3):
        ref = np.asarray(Image.fromarray(img[:, :, c].astype(np.float32), "F").resize((size, size), Image.BILINEAR))
        d = float(np.abs(out[c] - ref).max())
        print(f"[pillow {hw} -> {size} ch {c}] max |d| = {d:.3e}")
        assert d <= 6.1e-5, d


def test_base_transform_is_apply_under_the_identity_plan():
    imgs = [_img(9, 14, 1), _img(20, 6, 2)]
    images, sizes = A.pad_images(imgs)
    assert tuple(images.shape) == (2, 20, 14, 3) and sizes.tolist() == [[9, 14], [20, 6]] and int(images[0, 9:].sum()) == 0
    x = A.BaseTransform(12)(images, sizes)
    y = A.SSDAugmentation(12, seed=1).apply(images, sizes, A.identity_plan(sizes))
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, 3, 12, 12) and x.is_contiguous() and torch.equal(x, y)
    z = A.BaseTransform(12, channels_last=True)(images, sizes)
    assert z.is_contiguous(memory_format=torch.channels_last) and torch.equal(x, z)
    # the pixels outside an image's own extent never matter
    images[0, 9:] = 255
    images[0, :, 14:] = 255
    assert torch.equal(A.BaseTransform(12)(images, sizes), x)


# ---- colour ----------------------------------------------------------------------------------------------------------------------------------------------
def test_hsv_round_trip():
    """100 000 integer triples in [0, 255]: HSV -> BGR of BGR -> HSV within 1e-3 (2.0e-4 measured; the slack covers the two FLT_EPSILON-regularised divisions on other
    seeds).  Grey triples come back exactly."""
    p = np.random.default_rng(5).integers(0, 256, (100000, 3)).astype(np.float32)
    back = np.stack(A.hsv_to_bgr(*A.bgr_to_hsv(p[:, 0], p[:, 1], p[:, 2])), 1)
    d = float(np.abs(back - p).max())
    print(f"[hsv round trip] max |d| = {d:.3e}")
    assert back.dtype == np.float32 and d <= 1e-3, d
    grey = np.repeat(np.arange(256, dtype=np.float32)[:, None], 3, 1)
    assert np.array_equal(np.stack(A.hsv_to_bgr(*A.bgr_to_hsv(grey[:, 0], grey[:, 1], grey[:, 2])), 1), grey)
    # the vectorised conversions are the scalar restatement of this file
    for b, g, r in p[:200]:
        assert tuple(float(v[0]) for v in A.bgr_to_hsv(*(np.array([c]) for c in (b, g, r)))) == tuple(float(v) for v in _to_hsv(b, g, r))


MEAN = (104, 117, 123)
SWITCHES = {
    "brightness": (dict(delta=-20.5), dict(delta=-20.5, hsv=False)),
    "contrast_first": (dict(alpha_pre=1.37), dict(pre=1.37, hsv=False)),
    "contrast_last": (dict(alpha_post=0.61), dict(post=0.61, hsv=False)),
    "round_trip_alone": (dict(flags=A.F_HSV), dict()),
    "saturation": (dict(flags=A.F_HSV, sat=1.43), dict(sat=1.43)),
    "hue_up": (dict(flags=A.F_HSV, hue=17.5), dict(hue=17.5)),
    "hue_down": (dict(flags=A.F_HSV, hue=-17.5), dict(hue=-17.5)),
    "all_contrast_first": (dict(flags=A.F_HSV, delta=12.25, alpha_pre=0.8, sat=0.7, hue=9.0, perm=3), dict(delta=12.25, pre=0.8, sat=0.7, hue=9.0, perm=A.PERMS[3])),
    "all_contrast_last": (dict(flags=A.F_HSV, delta=-31.0, alpha_post=1.45, sat=1.2, hue=-11.0, perm=4), dict(delta=-31.0, post=1.45, sat=1.2, hue=-11.0, perm=A.PERMS[4])),
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_each_photometric_switch_alone(name):
    """A 4 x 4 image at size 4 is a 1:1 resize: the taps are the pixels, so the output is the chain applied by hand."""
    img = _img(4, 4, 21)
    img[0, 0], img[0, 1] = (20, 10, 250), (10, 20, 250)          # hues 357.5 and 2.5 degrees: + 17.5 wraps the first above 360, - 17.5 takes the second below 0
    words, hand = SWITCHES[name]
    if name in ("hue_up", "hue_down"):
        h0, h1 = float(_to_hsv(*map(f32, img[0, 0]))[0]), float(_to_hsv(*map(f32, img[0, 1]))[0])
        assert (h0 + 17.5 > 360 and name == "hue_up") or (h1 - 17.5 < 0 and name == "hue_down"), (h0, h1)
    assert np.array_equal(_apply(img, 4, words, MEAN), _hand(img, MEAN, **hand))


@pytest.mark.parametrize("perm", range(6))
def test_every_channel_permutation(perm):
    img = _img(4, 4, 22)
    want = img.astype(np.float32)[:, :, list(A.PERMS[perm])] - np.asarray(MEAN, dtype=np.float32)
    assert np.array_equal(_apply(img, 4, dict(perm=perm), MEAN), want.transpose(2, 0, 1))


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------------------
def _canvas(img, cw, ch, px, py, mean):
    c = np.empty((ch, cw, 3), dtype=np.float32)
    c[:] = np.asarray(mean, dtype=np.float32)
    c[py:py + img.shape[0], px:px + img.shape[1]] = img
    return c - np.asarray(mean, dtype=np.float32)


def test_geometry_by_construction():
    """Canvas 20 x 30 (h x w), a 10 x 10 image pasted at column 4, row 7, a 12 x 12 rect that overhangs the paste to the left and below, output size = the rect's
    extent: the output is the canvas's window: source - mean inside the paste, exactly 0 outside; mirrored, it is the flipped window."""
    img = _img(10, 10, 31)
    can = _canvas(img, 30, 20, 4, 7, MEAN)
    geo = dict(canvas_w=30, canvas_h=20, paste_x=4, paste_y=7, x1=1, y1=8, x2=13, y2=20, mode=5)
    out = _apply(img, 12, geo, MEAN)
    want = can[8:20, 1:13].transpose(2, 0, 1)
    assert np.array_equal(out, want)
    assert np.all(out[:, :, :3] == 0) and np.all(out[:, 9:, :] == 0) and np.any(out[:, :9, 3:] != 0)
    assert np.array_equal(_apply(img, 12, dict(geo, flags=A.F_MIRROR), MEAN), want[:, :, ::-1])
    # the photometric chain touches the pasted pixels only: the surround is the undistorted mean
    dist = _apply(img, 12, dict(geo, delta=30.0), MEAN)
    assert np.all(dist[:, :, :3] == 0) and np.all(dist[:, 9:, :] == 0) and np.array_equal(dist[:, :9, 3:], out[:, :9, 3:] + f32(30))


def test_rect_one_past_the_canvas_is_the_clipped_rect():
    """int(left + w) can be W + 1 (and int(top + h) H + 1): numpy slicing clips, so the crop is the clipped rect."""
    img = _img(10, 10, 32)
    a = _apply(img, 7, dict(x1=3, y1=2, x2=11, y2=11, mode=5), MEAN)
    b = _apply(img, 7, dict(x1=3, y1=2, x2=10, y2=10, mode=5), MEAN)
    assert np.array_equal(a, b)
    assert np.array_equal(_apply(img, 7, dict(x1=3, y1=3, x2=11, y2=10, mode=5), MEAN), (img[3:10, 3:10].astype(np.float32) - np.asarray(MEAN, dtype=np.float32)).transpose(2, 0, 1))


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------------------------
def _rec(h, w, **words):
    return _plan(torch.tensor([[h, w]], dtype=torch.int32), **words)[0].numpy()


def test_boxes_by_hand():
    h, w = 100, 200
    boxes = np.array([[0.1, 0.2, 0.3, 0.6, 7], [0.5, 0.5, 0.9, 0.9, 2], [0.0, 0.0, 0.2, 0.2, 4]], dtype=np.float32)
    valid = np.array([True, True, False])
    # identity: percent of the image again
    out, keep = A.boxes_under_plan(_rec(h, w), h, w, boxes, valid)
    assert keep.tolist() == [True, True, False] and np.allclose(out[:2], boxes[:2], atol=1e-7) and not out[2].any()
    # expand offset: canvas 400 x 300 (w x h), paste at (50, 30), mode 0 -> (x * 200 + 50) / 400, (y * 100 + 30) / 300
    out, keep = A.boxes_under_plan(_rec(h, w, canvas_w=400, canvas_h=300, paste_x=50, paste_y=30, x2=400, y2=300), h, w, boxes, valid)
    assert np.allclose(out[0], [70 / 400, 50 / 300, 110 / 400, 90 / 300, 7], atol=1e-7) and keep.tolist() == [True, True, False]
    # a crop: rect (30, 10, 130, 90).  Box 0 = (20, 20, 60, 60), centre (40, 40) inside: clipped to x1 = 30 -> (0, 10, 30, 50) / (100, 80).  Box 1 = (100, 50, 180, 90),
    # centre (140, 70): outside (140 > 130) -> dropped, and its row stays in place as zeros
    out, keep = A.boxes_under_plan(_rec(h, w, mode=2, x1=30, y1=10, x2=130, y2=90), h, w, boxes, valid)
    assert keep.tolist() == [True, False, False] and np.allclose(out[0], [0, 10 / 80, 30 / 100, 50 / 80, 7], atol=1e-7) and not out[1:].any()
    # strict inequalities: box 0's centre (40, 40) exactly on the rect's left edge, then its top edge, right edge, bottom edge
    for rect in ((40, 10, 130, 90), (30, 40, 130, 90), (30, 10, 40, 90), (30, 10, 130, 40)):
        assert not A.boxes_under_plan(_rec(h, w, mode=1, x1=rect[0], y1=rect[1], x2=rect[2], y2=rect[3]), h, w, boxes, valid)[1][0], rect
    assert A.boxes_under_plan(_rec(h, w, mode=1, x1=39, y1=39, x2=41, y2=41), h, w, boxes, valid)[1][0]
    # mirror in the crop: x1' = cw - x2, x2' = cw - x1
    out, _ = A.boxes_under_plan(_rec(h, w, mode=2, x1=30, y1=10, x2=130, y2=90, flags=A.F_MIRROR), h, w, boxes, valid)
    assert np.allclose(out[0], [70 / 100, 10 / 80, 100 / 100, 50 / 80, 7], atol=1e-7)
    # a rect one past the canvas: boxes are clipped to the UNCLIPPED rect (x2 = 201), percent by the CLIPPED extent (200 - 120 = 80 wide, 100 - 30 = 70 high).
    # Box 1 = (100, 50, 180, 90), centre (140, 70): clipped to x1 = 120 -> (0, 20, 60, 60)
    wide = np.array([[0.5, 0.5, 1.01, 1.02, 2]], dtype=np.float32)          # (100, 50, 202, 102): x2 clips to 201, y2 to 101
    out, keep = A.boxes_under_plan(_rec(h, w, mode=3, x1=120, y1=30, x2=201, y2=101), h, w, wide, np.array([True]))
    assert keep[0] and np.allclose(out[0], [0, 20 / 70, 81 / 80, 71 / 70, 2], atol=1e-6)
    # mode 0 keeps every valid box unclipped, whatever its centre
    out, keep = A.boxes_under_plan(_rec(h, w), h, w, np.array([[1.2, 1.2, 1.4, 1.4, 1]], dtype=np.float32), np.array([True]))
    assert keep[0] and np.allclose(out[0], [1.2, 1.2, 1.4, 1.4, 1], atol=1e-6)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------------------
def _scene(n, g, seed, lo=32, hi=500):
    """n images of random size in [lo, hi]^2 with 1 .. g valid boxes each, inside the image."""
    r = np.random.default_rng(seed)
    sizes = r.integers(lo, hi + 1, (n, 2)).astype(np.int32)
    c, half = r.uniform(0.1, 0.9, (n, g, 2)), r.uniform(0.02, 0.3, (n, g, 2))
    boxes = np.concatenate([np.clip(c - half, 0, 1), np.clip(c + half, 0, 1), r.integers(0, 20, (n, g, 1))], 2).astype(np.float32)
    valid = np.arange(g)[None, :] < r.integers(1, g + 1, (n, 1))
    return torch.from_numpy(sizes), torch.from_numpy(boxes), torch.from_numpy(valid)


@pytest.fixture(scope="module")
def sampled():
    sizes, boxes, valid = _scene(4096, 8, 77)
    plan, bo, vo = A.SSDAugmentation(size=64, seed=2024).plan(sizes, boxes, valid)
    return sizes.numpy(), boxes.numpy(), valid.numpy(), plan.numpy(), bo.numpy(), vo.numpy()


def test_plan_sampler_properties(sampled):
    sizes, boxes, valid, plan, bo, vo = sampled
    fl = plan.view(np.float32)
    flags = plan[:, A.P_FLAGS]
    for bit in (A.F_BRIGHT, A.F_CONTRAST_FIRST, A.F_CONTRAST, A.F_SAT, A.F_HUE, A.F_NOISE, A.F_EXPAND, A.F_MIRROR):
        share = float(((flags & bit) != 0).mean())
        print(f"[coin {bit}] share {share:.4f}")
        assert abs(share - 0.5) <= 0.039, (bit, share)          # 5 sigma of a fair coin at n = 4096
    assert np.all((flags & A.F_HSV) != 0)
    on = lambda bit: (flags & bit) != 0
    assert np.all(np.abs(fl[:, A.P_DELTA]) <= 32) and np.all(fl[~on(A.F_BRIGHT), A.P_DELTA] == 0) and np.any(fl[:, A.P_DELTA] < -16) and np.any(fl[:, A.P_DELTA] > 16)
    alpha = fl[:, A.P_ALPHA_PRE] * fl[:, A.P_ALPHA_POST]
    first = on(A.F_CONTRAST_FIRST)
    assert np.all(fl[~first, A.P_ALPHA_PRE] == 1) and np.all(fl[first, A.P_ALPHA_POST] == 1) and np.all(alpha[~on(A.F_CONTRAST)] == 1)
    assert np.all((alpha >= 0.5) & (alpha <= 1.5)) and alpha.min() < 0.6 and alpha.max() > 1.4
    assert np.all((fl[:, A.P_SAT] >= 0.5) & (fl[:, A.P_SAT] <= 1.5)) and np.all(fl[~on(A.F_SAT), A.P_SAT] == 1)
    assert np.all(np.abs(fl[:, A.P_HUE]) <= 18) and np.all(fl[~on(A.F_HUE), A.P_HUE] == 0) and np.abs(fl[:, A.P_HUE]).max() > 16
    perm = plan[:, A.P_PERM]
    assert np.all((perm >= 0) & (perm <= 5)) and np.all(perm[~on(A.F_NOISE)] == 0) and set(perm[on(A.F_NOISE)].tolist()) == set(range(6))
    # Expand
    ex = on(A.F_EXPAND)
    h0, w0 = sizes[:, 0], sizes[:, 1]
    W, H, px, py, ratio = plan[:, A.P_CANVAS_W], plan[:, A.P_CANVAS_H], plan[:, A.P_PASTE_X], plan[:, A.P_PASTE_Y], fl[:, A.P_RATIO]
    assert np.all(W[~ex] == w0[~ex]) and np.all(H[~ex] == h0[~ex]) and np.all(px[~ex] == 0) and np.all(py[~ex] == 0) and np.all(ratio[~ex] == 1)
    assert np.all((ratio >= 1) & (ratio <= 4)) and ratio.max() > 3.5
    assert np.all(W == (w0.astype(np.float32) * ratio).astype(np.int32)) and np.all(H == (h0.astype(np.float32) * ratio).astype(np.int32))
    assert np.all((px >= 0) & (px + w0 <= W) & (py >= 0) & (py + h0 <= H))
    # RandomSampleCrop
    mode, rounds = plan[:, A.P_MODE], plan[:, A.P_ROUNDS]
    assert np.all((mode >= 0) & (mode <= 5)) and np.all((rounds >= 1) & (rounds <= A.MAX_ROUNDS)) and set(mode.tolist()) == set(range(6))
    z = mode == 0
    assert np.all(plan[z, A.P_X1] == 0) and np.all(plan[z, A.P_Y1] == 0) and np.all(plan[z, A.P_X2] == W[z]) and np.all(plan[z, A.P_Y2] == H[z])
    assert np.array_equal(vo[z], valid[z])
    dw, dh = fl[:, A.P_DRAWN_W], fl[:, A.P_DRAWN_H]
    Wf, Hf = W.astype(np.float32), H.astype(np.float32)
    nz = ~z
    assert np.all(f32(0.3) * Wf[nz] <= dw[nz]) and np.all(dw[nz] <= Wf[nz]) and np.all(f32(0.3) * Hf[nz] <= dh[nz]) and np.all(dh[nz] <= Hf[nz])
    q = dh[nz] / dw[nz]
    assert np.all((q >= 0.5) & (q <= 2))
    x1, y1, x2, y2 = (plan[:, k] for k in (A.P_X1, A.P_Y1, A.P_X2, A.P_Y2))
    assert np.all((x1 >= 0) & (y1 >= 0) & (x2 <= W + 1) & (y2 <= H + 1) & (x2 > x1) & (y2 > y1))
    # at least one valid box centre strictly inside, in the definition's fp32 arithmetic: x (w, h), + the paste offset, (a + b) / 2
    wf, hf = w0.astype(np.float32)[:, None], h0.astype(np.float32)[:, None]
    cx = ((boxes[:, :, 0] * wf + px.astype(np.float32)[:, None]) + (boxes[:, :, 2] * wf + px.astype(np.float32)[:, None])) * f32(0.5)
    cy = ((boxes[:, :, 1] * hf + py.astype(np.float32)[:, None]) + (boxes[:, :, 3] * hf + py.astype(np.float32)[:, None])) * f32(0.5)
    assert cx.dtype == np.float32
    inside = valid & (x1[:, None] < cx) & (y1[:, None] < cy) & (x2[:, None] > cx) & (y2[:, None] > cy)
    assert np.all(inside[nz].any(1)) and np.array_equal(vo[nz], inside[nz])
    assert np.all(vo.any(1) == valid.any(1)) and valid.any(1).all()          # valid_out is never all-false where valid had a true
    assert not np.any(vo & ~valid) and not bo[~vo].any()
    # surviving boxes lie in the crop: [0, 1] up to the one-past-the-canvas column / row
    kept = bo[vo & nz[:, None]]
    assert np.all(kept[:, :4] >= 0) and np.all(kept[:, :4] <= 1.04) and np.all(kept[:, 2] >= kept[:, 0]) and np.all(kept[:, 3] >= kept[:, 1])
    assert np.array_equal(bo[vo][:, 4], boxes[vo][:, 4])


def test_an_image_without_a_valid_box_takes_mode_0():
    sizes, boxes, valid = _scene(64, 3, 5)
    valid[:] = False
    plan, bo, vo = A.SSDAugmentation(size=32, seed=9).plan(sizes, boxes, valid)
    assert np.all(plan[:, A.P_MODE].numpy() == 0) and np.all(plan[:, A.P_ROUNDS].numpy() == 0) and not vo.any() and not bo.any()


def test_a_box_that_no_rect_can_hold_takes_mode_0_for_256_seeds():
    """`rect[0] < cx` can never hold for a centre at or left of the canvas's origin, so every constrained trial fails and the image ends in mode 0: by a mode-0 draw or by
    the cap of 64 rounds.  On the canvas the centre of a box is (cx w + paste_x, cy h + paste_y): Expand moves a centre at fraction (0, 0) to the paste offset, which a
    rect CAN hold.  So the centre-(0, 0) box is checked in two parts: un-expanded (paste offset (0, 0)) it takes mode 0 for every seed that does not expand, and where
    a non-zero mode was accepted the paste offset is strictly inside the rect; a box centred at fraction (-4, -4) stays left of the origin under every expansion
    (paste_x < 3 w) and takes mode 0 for every one of the 256 seeds."""
    sizes = torch.tensor([[120, 90]], dtype=torch.int32)
    valid = torch.tensor([[True]])
    at_origin = torch.tensor([[[-0.1, -0.2, 0.1, 0.2, 3]]], dtype=torch.float32)
    far_left = torch.tensor([[[-4.5, -4.5, -3.5, -3.5, 3]]], dtype=torch.float32)
    plain = capped = 0
    for seed in range(256):
        plan, bo, vo = (t.numpy()[0] for t in A.SSDAugmentation(size=32, seed=seed).plan(sizes, at_origin, valid))
        if (plan[A.P_PASTE_X], plan[A.P_PASTE_Y]) == (0, 0):
            plain += 1
            assert plan[A.P_MODE] == 0 and 1 <= plan[A.P_ROUNDS] <= A.MAX_ROUNDS and vo[0], (seed, plan)
        elif plan[A.P_MODE]:
            assert plan[A.P_X1] < plan[A.P_PASTE_X] < plan[A.P_X2] and plan[A.P_Y1] < plan[A.P_PASTE_Y] < plan[A.P_Y2], (seed, plan)
        plan, bo, vo = (t.numpy()[0] for t in A.SSDAugmentation(size=32, seed=seed).plan(sizes, far_left, valid))
        assert plan[A.P_MODE] == 0 and 1 <= plan[A.P_ROUNDS] <= A.MAX_ROUNDS and vo[0], (seed, plan)
        capped += int(plan[A.P_ROUNDS] == A.MAX_ROUNDS)
    assert plain >= 96, plain          # about half the seeds do not expand (5 sigma below 128 is 88)
    print(f"[(0, 0) centre] {plain} of 256 seeds un-expanded; far-left box: {capped} seeds reached the cap of {A.MAX_ROUNDS} rounds")


# ---- the stream ------------------------------------------------------------------------------------------------------------------------------------------
def test_stream_and_state_dict():
    sizes, boxes, valid = _scene(6, 4, 8)
    images = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (6, 500, 500, 3), dtype=np.uint8))
    a, b = A.SSDAugmentation(size=24, seed=41), A.SSDAugmentation(size=24, seed=41)
    xa, ba, va = a(images, sizes, boxes, valid)
    xb, bb, vb = b(images, sizes, boxes, valid)
    assert torch.equal(a.last_plan, b.last_plan) and torch.equal(xa, xb) and torch.equal(ba, bb) and torch.equal(va, vb)          # same seed, same plan
    assert a.images_seen() == 6 and a.state_dict() == {"seed": 41, "images_seen": 6}
    xa2 = a(images, sizes, boxes, valid)[0]
    assert not torch.equal(a.last_plan, b.last_plan) and not torch.equal(xa2, xa)                                                  # the stream advances
    assert not torch.equal(A.SSDAugmentation(size=24, seed=42).plan(sizes, boxes, valid)[0], b.last_plan)                         # another seed, another plan
    # after N images the next call equals a fresh object at images seen = N; the ordinal is per image: a batch split in two draws the same plans
    c = A.SSDAugmentation(size=24, seed=41)
    c.load_state_dict({"seed": 41, "images_seen": 6})
    assert torch.equal(c.plan(sizes, boxes, valid)[0], a.last_plan)
    d = A.SSDAugmentation(size=24, seed=41)
    halves = [d.plan(sizes[s], boxes[s], valid[s])[0] for s in (slice(0, 2), slice(2, 6))]
    assert torch.equal(torch.cat(halves), b.last_plan)
    e = A.SSDAugmentation(size=24, seed=0)
    e.load_state_dict(a.state_dict())
    assert e.state_dict() == a.state_dict() == {"seed": 41, "images_seen": 12}
    assert torch.equal(e.plan(sizes, boxes, valid)[0], a.plan(sizes, boxes, valid)[0])
    # seed=None: torch's seed
    torch.manual_seed(1234)
    s1 = A.SSDAugmentation(size=24).seed
    torch.manual_seed(1235)
    assert A.SSDAugmentation(size=24).seed != s1


def test_philox_known_answer():
    """Random123's known-answer vectors for Philox4x32-10."""
    assert A.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert A.philox4x32_10((0xffffffff,) * 4, (0xffffffff, 0xffffffff)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert A.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_argument_errors():
    images, sizes = A.pad_images([_img(8, 8, 1)])
    boxes, valid = torch.zeros(1, 2, 5), torch.zeros(1, 2, dtype=torch.bool)
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError):
            A.SSDAugmentation(size=bad)
    aug = A.SSDAugmentation(size=8, seed=1)
    for args in ((images.float(), sizes, boxes, valid), (images, sizes.long(), boxes, valid), (images, sizes, boxes.double(), valid), (images, sizes, boxes, valid.int()),
                 (images[0], sizes, boxes, valid), (images, sizes, boxes[:, :, :4], valid), (images, sizes, boxes, valid[:, :1]),
                 (images, torch.tensor([[9, 8]], dtype=torch.int32), boxes, valid), (images, torch.tensor([[0, 8]], dtype=torch.int32), boxes, valid)):
        with pytest.raises(ValueError):
            aug(*args)
    with pytest.raises(ValueError):
        aug.apply(images, sizes, torch.zeros(1, A.PLAN_WORDS - 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        A.pad_images([np.zeros((4, 4), dtype=np.uint8)])
    assert aug.images_seen() == 0

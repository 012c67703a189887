"""SSD training-time augmentation of whole batches: the first line of the reference's detection recipe, `SSDAugmentation(cfg['min_dim'], MEANS)`
(Object_Detection/utils/augmentations.py:400-417, used at qtrainval.py:109) and the eval-time `BaseTransform` (data/__init__.py:30-43).  uint8 BGR batch in,
the network's fp32 input and the padded targets of `MultiBoxLoss` out.  On device tensors two HIP kernels do the work (csrc/frost_augment.hip) without any host
synchronisation; on CPU tensors the same classes run the definition below in numpy, which is the yardstick of every GPU test.

The work is split in two.  `plan` takes every random decision of the reference's pipeline, in the reference's order, and writes one fixed-size record per image
(PLAN_WORDS 32-bit words, layout in include/frost_hip.h) together with the transformed boxes; `apply` is a pure function of (images, sizes, plan): per output
pixel four taps of a bilinear resize, each tap mirrored, offset into the canvas, photometrically distorted (or the undistorted mean outside the pasted image),
then the mean is subtracted.  All arithmetic of both halves is fp32 in a fixed written order, so the device and this file agree word for word.

What is restated, and what is defined here because the reference lacks it:
  * RandomSampleCrop (augmentations.py:208-309) as written, quirks included -- see `_plan_one`.
  * Two added definitions: an image without a valid box takes mode 0 (the reference raises on an empty overlap array), and the outer `while True` is bounded at
    MAX_ROUNDS = 64 mode draws, then mode 0 (a round ends the loop with probability >= 1/6, so the cap changes an outcome with probability <= (5/6)^64 = 8.6e-6).
  * The colour conversions are OpenCV's float BGR<->HSV formulas written out (`bgr_to_hsv`, `hsv_to_bgr`), the resize is OpenCV's INTER_LINEAR convention
    without antialiasing.  The reference module imports cv2 and torchvision; neither is available to this project's tests, so equality with OpenCV's own
    binaries is NOT measured anywhere: this file is the restatement, pinned by tests/test_augment_cpu.py (known answers, Pillow for up-scaling, round trips).
  * Randomness is Philox4x32-10 (the library's generator): key = seed, counter = (image ordinal low, image ordinal high, draw block, STREAM_TAG); draw k of an
    image is word k & 3 of block k >> 2.  u = (word >> 8) * 2^-24, a coin is the top bit, a choice among k is the high 32 bits of word * k,
    uniform(a, b) = a + (b - a) * u.  Image ordinal = images seen so far + index in the batch."""
import numpy as np
import torch

PLAN_WORDS = 24          # FROST_AUG_PLAN_WORDS
# word indices of a plan record (FROST_AUG_* of include/frost_hip.h); F = fp32 bits, I = int32
P_FLAGS, P_DELTA, P_ALPHA_PRE, P_ALPHA_POST, P_SAT, P_HUE, P_PERM, P_RATIO = 0, 1, 2, 3, 4, 5, 6, 7
P_PASTE_X, P_PASTE_Y, P_CANVAS_W, P_CANVAS_H, P_MODE, P_ROUNDS = 8, 9, 10, 11, 12, 13
P_X1, P_Y1, P_X2, P_Y2, P_DRAWN_W, P_DRAWN_H = 14, 15, 16, 17, 18, 19
FLOAT_WORDS = (P_DELTA, P_ALPHA_PRE, P_ALPHA_POST, P_SAT, P_HUE, P_RATIO, P_DRAWN_W, P_DRAWN_H)
# flag bits: the coins as drawn (F_EXPAND = the image was expanded, i.e. the reference's randint(2) came up 0), and F_HSV = the BGR -> HSV -> BGR round trip runs
F_BRIGHT, F_CONTRAST_FIRST, F_CONTRAST, F_SAT, F_HUE, F_NOISE, F_EXPAND, F_MIRROR, F_HSV = 1, 2, 4, 8, 16, 32, 64, 128, 256
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))          # RandomLightingNoise.perms: out[c] = in[PERMS[i][c]]
HSV_SECTORS = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))    # (b, g, r) indices into {v, v(1-s), v(1-sf), v(1-s(1-f))} per hue sector
MAX_ROUNDS, TRIALS = 64, 50
STREAM_TAG = 0x53534441                                                            # "SSDA": the counter word that keeps this stream apart from the library's others
MAX_G = 1024                                                                       # FROST_AUG_MAX_G: box rows of one image
MAX_SIZE = 4096
f32 = np.float32
EPS = f32(1.1920928955078125e-07)                                                  # FLT_EPSILON
_M64 = 0xFFFFFFFFFFFFFFFF


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python ints: counter c = (c0, c1, c2, c3), key k = (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


class _Draws:
    """The draw sequence of one image."""

    def __init__(self, seed, ordinal):
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.ord = (ordinal & 0xFFFFFFFF, (ordinal >> 32) & 0xFFFFFFFF)
        self.n, self.block, self.words = 0, -1, None

    def word(self):
        b = self.n >> 2
        if b != self.block:
            self.words, self.block = philox4x32_10((self.ord[0], self.ord[1], b, STREAM_TAG), self.key), b
        w = self.words[self.n & 3]
        self.n += 1
        return w

    def coin(self):
        return self.word() >> 31

    def choice(self, k):
        return (self.word() * k) >> 32

    def uniform(self, a, b):
        u = f32(self.word() >> 8) * f32(2.0 ** -24)
        return f32(a + f32(f32(b - a) * u))


def default_seed():
    """seed=None: torch's seed mixed with the data-parallel rank (runner.dropout_seed's rule), so the ranks of one job augment their shards differently."""
    from .runner import dropout_seed
    return dropout_seed()


def identity_plan(sizes):
    """[N, PLAN_WORDS] int32 on sizes' device: every factor neutral, no colour round trip, no expand, crop = the whole image, no mirror."""
    if not isinstance(sizes, torch.Tensor) or sizes.dim() != 2 or sizes.size(1) != 2 or sizes.dtype != torch.int32:
        raise ValueError("identity_plan: sizes must be [N, 2] int32 (h, w)")
    out = torch.zeros(sizes.size(0), PLAN_WORDS, dtype=torch.int32, device=sizes.device)          # fills and strided copies only: no host transfer on the device
    fl = out.view(torch.float32)
    for word in (P_ALPHA_PRE, P_ALPHA_POST, P_SAT, P_RATIO):
        fl[:, word] = 1.0
    for word, col in ((P_CANVAS_W, 1), (P_CANVAS_H, 0), (P_X2, 1), (P_Y2, 0)):
        out[:, word] = sizes[:, col]
    return out


def pad_images(images):
    """list of HxWx3 uint8 arrays / tensors -> (images uint8 [N, Hmax, Wmax, 3] with each image in the top-left corner of its slot, sizes int32 [N, 2] = (h, w)):
    the image half of a collate function (ssdlite.pad_targets is the target half)."""
    ts = [torch.as_tensor(np.ascontiguousarray(i)) if not isinstance(i, torch.Tensor) else i for i in images]
    if not ts or any(t.dim() != 3 or t.size(2) != 3 or t.dtype != torch.uint8 or t.size(0) < 1 or t.size(1) < 1 for t in ts):
        raise ValueError("pad_images: a non-empty list of HxWx3 uint8 images expected")
    out = torch.zeros(len(ts), max(t.size(0) for t in ts), max(t.size(1) for t in ts), 3, dtype=torch.uint8)
    for i, t in enumerate(ts):
        out[i, :t.size(0), :t.size(1)] = t
    return out, torch.tensor([[t.size(0), t.size(1)] for t in ts], dtype=torch.int32)


# ---- the definition: colour ----------------------------------------------------------------------------------------------------------------------------
def bgr_to_hsv(b, g, r):
    """OpenCV's float BGR -> HSV (H in degrees) on fp32 arrays."""
    v = np.maximum(np.maximum(r, g), b)
    diff = f32(v - np.minimum(np.minimum(r, g), b))
    s = f32(diff / f32(np.abs(v) + EPS))
    d = f32(f32(60.0) / f32(diff + EPS))
    h = np.where(v == r, f32(f32(g - b) * d), np.where(v == g, f32(f32(f32(b - r) * d) + f32(120.0)), f32(f32(f32(r - g) * d) + f32(240.0))))
    h = np.where(h < 0, f32(h + f32(360.0)), h)
    return f32(h), s, f32(v)


def hsv_to_bgr(h, s, v):
    """OpenCV's float HSV -> BGR on fp32 arrays: one + 6 if negative, one - 6 if >= 6."""
    h = f32(h * f32(1.0 / 60.0))
    h = np.where(h < 0, f32(h + f32(6.0)), h)
    h = np.where(h >= 6, f32(h - f32(6.0)), h)
    fl = np.floor(h)
    f = f32(h - fl)
    sector = np.clip(fl, 0, 5).astype(np.int64)          # the clip never acts on finite input; it keeps the table index in range whatever comes in
    one = f32(1.0)
    tab = np.stack([v, f32(v * f32(one - s)), f32(v * f32(one - f32(s * f))), f32(v * f32(one - f32(s * f32(one - f))))])
    idx = np.asarray(HSV_SECTORS, dtype=np.int64)[sector]          # [..., 3]
    pick = lambda k: np.take_along_axis(tab, idx[..., k][None], 0)[0]
    return f32(pick(0)), f32(pick(1)), f32(pick(2))


def photometric(px, rec):
    """The photometric chain of one plan record on fp32 BGR pixels [..., 3]; nothing is clipped anywhere (the reference clips nothing)."""
    fl = rec.view(np.float32)
    x = f32(px.astype(np.float32) + fl[P_DELTA])
    x = f32(x * fl[P_ALPHA_PRE])
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    if int(rec[P_FLAGS]) & F_HSV:
        h, s, v = bgr_to_hsv(b, g, r)
        s = f32(s * fl[P_SAT])
        h = f32(h + fl[P_HUE])
        h = np.where(h > 360, f32(h - f32(360.0)), h)
        h = np.where(h < 0, f32(h + f32(360.0)), h)
        b, g, r = hsv_to_bgr(h, s, v)
    x = f32(np.stack([b, g, r], -1) * fl[P_ALPHA_POST])
    return np.ascontiguousarray(x[..., list(PERMS[int(rec[P_PERM])])])


# ---- the definition: pixels ----------------------------------------------------------------------------------------------------------------------------
def _taps(extent, size):
    """OpenCV INTER_LINEAR: src = (dst + 0.5) * (extent / size) - 0.5, i0 = floor, both taps clamped to [0, extent - 1]."""
    scale = f32(f32(extent) / f32(size))
    src = f32(f32(f32(np.arange(size, dtype=np.float32) + f32(0.5)) * scale) - f32(0.5))
    fl = np.floor(src)
    frac = f32(src - fl)
    i0 = fl.astype(np.int64)
    return np.clip(i0, 0, extent - 1), np.clip(i0 + 1, 0, extent - 1), frac


def _apply_one(img, h, w, rec, size, mean):
    """One image: uint8 slot [Hmax, Wmax, 3], its size, its plan record -> fp32 [3, size, size]."""
    D = photometric(img[:h, :w], rec)
    cw_, ch_ = int(rec[P_CANVAS_W]), int(rec[P_CANVAS_H])
    x1, y1 = int(rec[P_X1]), int(rec[P_Y1])
    cw, ch = max(min(int(rec[P_X2]), cw_) - x1, 1), max(min(int(rec[P_Y2]), ch_) - y1, 1)          # the crop's pixels are the rect clipped to the canvas
    tx0, tx1, fx = _taps(cw, size)
    ty0, ty1, fy = _taps(ch, size)
    if int(rec[P_FLAGS]) & F_MIRROR:
        tx0, tx1 = cw - 1 - tx0, cw - 1 - tx1
    px, py = int(rec[P_PASTE_X]), int(rec[P_PASTE_Y])
    m = np.asarray(mean, dtype=np.float32)

    def tap(ty, tx):
        sy, sx = y1 + ty - py, x1 + tx - px
        inside = ((sy >= 0) & (sy < h))[:, None] & ((sx >= 0) & (sx < w))[None, :]
        v = D[np.clip(sy, 0, h - 1)[:, None], np.clip(sx, 0, w - 1)[None, :]]
        return np.where(inside[..., None], v, m)          # outside the pasted image: the mean, undistorted (Expand runs after PhotometricDistort)

    one = f32(1.0)
    wx0, wx1 = f32(one - fx)[None, :, None], fx[None, :, None]
    wy0, wy1 = f32(one - fy)[:, None, None], fy[:, None, None]
    top = f32(f32(tap(ty0, tx0) * wx0) + f32(tap(ty0, tx1) * wx1))
    bot = f32(f32(tap(ty1, tx0) * wx0) + f32(tap(ty1, tx1) * wx1))
    out = f32(f32(f32(top * wy0) + f32(bot * wy1)) - m)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out.transpose(2, 0, 1))


# ---- the definition: decisions and boxes ---------------------------------------------------------------------------------------------------------------
def _plan_one(seed, ordinal, h0, w0, boxes, valid):
    """One image: (plan record int32 [PLAN_WORDS], boxes_out [G, 5], valid_out [G]).  The decisions in the reference's order (augmentations.py:404-414)."""
    rng = _Draws(seed, ordinal)
    rec = np.zeros(PLAN_WORDS, dtype=np.int32)
    fl = rec.view(np.float32)
    flags = F_HSV          # both orders of PhotometricDistort.pd convert to HSV and back, whatever the coins say (:378-395)
    delta, alpha, sat, hue = f32(0), f32(1), f32(1), f32(0)
    if rng.coin():                                        # RandomBrightness (:185-195)
        flags |= F_BRIGHT
        delta = rng.uniform(f32(-32), f32(32))
    if rng.coin():                                        # PhotometricDistort: randint(2) true = pd[:-1], contrast before HSV (:392-395)
        flags |= F_CONTRAST_FIRST
        if rng.coin():                                    # RandomContrast (:170-182)
            flags |= F_CONTRAST
            alpha = rng.uniform(f32(0.5), f32(1.5))
    if rng.coin():                                        # RandomSaturation (:114-125)
        flags |= F_SAT
        sat = rng.uniform(f32(0.5), f32(1.5))
    if rng.coin():                                        # RandomHue (:128-138)
        flags |= F_HUE
        hue = rng.uniform(f32(-18), f32(18))
    if not flags & F_CONTRAST_FIRST and rng.coin():
        flags |= F_CONTRAST
        alpha = rng.uniform(f32(0.5), f32(1.5))
    perm = 0
    if rng.coin():                                        # RandomLightingNoise (:141-152)
        flags |= F_NOISE
        perm = rng.choice(6)
    W, H = int(w0), int(h0)
    wf, hf = f32(w0), f32(h0)
    ratio, px, py = f32(1), 0, 0
    if not rng.coin():                                    # Expand (:312-337): randint(2) TRUE returns the image unchanged
        flags |= F_EXPAND
        ratio = rng.uniform(f32(1), f32(4))
        left = rng.uniform(f32(0), f32(f32(wf * ratio) - wf))
        top = rng.uniform(f32(0), f32(f32(hf * ratio) - hf))
        W, H = int(f32(wf * ratio)), int(f32(hf * ratio))
        px, py = int(left), int(top)
    rec[P_PASTE_X], rec[P_PASTE_Y] = px, py
    cx, cy = _canvas_boxes(rec, h0, w0, boxes)[4:]
    # RandomSampleCrop (:208-309), as written:
    #  * line 269's reject test is `overlap.min() < min_iou and max_iou < overlap.max()` with max_iou = inf in all six options: never true.  The IoU thresholds have no
    #    effect, only the mode (uniform over six, mode 0 = the whole image) and the centre test matter; the IoU is not computed.
    #  * `random.uniform(width - w)` is numpy's uniform(low=width - w, high=1.0): left = (W - w) + (1 - (W - w)) u.  int(left + w) can exceed W by one: the crop's pixels
    #    are the rect clipped to the canvas (numpy slicing), the boxes are clipped to the UNCLIPPED rect, percent coordinates and the mirror use the clipped extent.
    #  * a trial that fails the aspect test consumes only its two size draws.
    #  * a trial is accepted iff at least one valid box has its centre strictly inside the rect; the other boxes are dropped.
    mode, rounds, rect, dw, dh = 0, 0, (0, 0, W, H), f32(0), f32(0)
    Wf, Hf = f32(W), f32(H)
    if valid.any():                                       # (added definition: no valid box -> mode 0, no draws)
        done = False
        while rounds < MAX_ROUNDS and not done:           # (added definition: at most MAX_ROUNDS mode draws, then mode 0)
            rounds += 1
            m = rng.choice(6)
            if m == 0:
                break
            for _ in range(TRIALS):
                w = rng.uniform(f32(f32(0.3) * Wf), Wf)
                h = rng.uniform(f32(f32(0.3) * Hf), Hf)
                q = f32(h / w)
                if q < f32(0.5) or q > f32(2):
                    continue
                left = rng.uniform(f32(Wf - w), f32(1))
                top = rng.uniform(f32(Hf - h), f32(1))
                r = (int(left), int(top), int(f32(left + w)), int(f32(top + h)))
                inside = valid & (f32(r[0]) < cx) & (f32(r[1]) < cy) & (f32(r[2]) > cx) & (f32(r[3]) > cy)
                if inside.any():
                    mode, rect, dw, dh, done = m, r, w, h, True
                    break
    if rng.coin():                                        # RandomMirror (:340-347)
        flags |= F_MIRROR
    rec[P_FLAGS], rec[P_PERM], rec[P_PASTE_X], rec[P_PASTE_Y], rec[P_CANVAS_W], rec[P_CANVAS_H], rec[P_MODE], rec[P_ROUNDS] = flags, perm, px, py, W, H, mode, rounds
    rec[P_X1:P_Y2 + 1] = rect
    cf = bool(flags & F_CONTRAST_FIRST)
    fl[P_DELTA], fl[P_ALPHA_PRE], fl[P_ALPHA_POST], fl[P_SAT], fl[P_HUE], fl[P_RATIO] = delta, alpha if cf else f32(1), f32(1) if cf else alpha, sat, hue, ratio
    fl[P_DRAWN_W], fl[P_DRAWN_H] = dw, dh
    out, keep = boxes_under_plan(rec, h0, w0, boxes, valid)
    return rec, out, keep


def _canvas_boxes(rec, h0, w0, boxes):
    """ToAbsoluteCoords and Expand's offset: corners and centres of every row on the canvas."""
    b = boxes.astype(np.float32)
    wf, hf, px, py = f32(w0), f32(h0), f32(int(rec[P_PASTE_X])), f32(int(rec[P_PASTE_Y]))
    bx1, by1, bx2, by2 = f32(f32(b[:, 0] * wf) + px), f32(f32(b[:, 1] * hf) + py), f32(f32(b[:, 2] * wf) + px), f32(f32(b[:, 3] * hf) + py)
    return bx1, by1, bx2, by2, f32(f32(bx1 + bx2) * f32(0.5)), f32(f32(by1 + by2) * f32(0.5))


def boxes_under_plan(rec, h0, w0, boxes, valid):
    """The targets of one image under one plan record: (boxes_out [G, 5], valid_out [G]).  In order: x (w, h); + the paste offset; in a non-zero mode the centre mask,
    the clip to the UNCLIPPED rect; - rect[:2]; the mirror x1' = cw - x2, x2' = cw - x1; / (cw, ch) with cw, ch the CLIPPED crop's extent.  Survivors keep their rows."""
    bx1, by1, bx2, by2, cx, cy = _canvas_boxes(rec, h0, w0, boxes)
    rect = [int(v) for v in rec[P_X1:P_Y2 + 1]]
    rx1, ry1, rx2, ry2 = (f32(v) for v in rect)
    keep = valid.copy()
    if int(rec[P_MODE]):
        keep = valid & (rx1 < cx) & (ry1 < cy) & (rx2 > cx) & (ry2 > cy)
        bx1, by1, bx2, by2 = np.maximum(bx1, rx1), np.maximum(by1, ry1), np.minimum(bx2, rx2), np.minimum(by2, ry2)
    bx1, by1, bx2, by2 = f32(bx1 - rx1), f32(by1 - ry1), f32(bx2 - rx1), f32(by2 - ry1)
    cwf = f32(max(min(rect[2], int(rec[P_CANVAS_W])) - rect[0], 1))
    chf = f32(max(min(rect[3], int(rec[P_CANVAS_H])) - rect[1], 1))
    if int(rec[P_FLAGS]) & F_MIRROR:
        bx1, bx2 = f32(cwf - bx2), f32(cwf - bx1)
    out = np.stack([f32(bx1 / cwf), f32(by1 / chf), f32(bx2 / cwf), f32(by2 / chf), boxes[:, 4].astype(np.float32)], 1).astype(np.float32)
    out[~keep] = 0
    return out, keep


# ---- the public classes --------------------------------------------------------------------------------------------------------------------------------
def _check_images(who, images, sizes):
    if not isinstance(images, torch.Tensor) or not isinstance(sizes, torch.Tensor):
        raise ValueError(f"{who}: tensors expected")
    if images.dim() != 4 or images.size(3) != 3 or images.dtype != torch.uint8 or images.size(0) < 1 or images.size(1) < 1 or images.size(2) < 1:
        raise ValueError(f"{who}: images must be [N, Hmax, Wmax, 3] uint8")
    _check_sizes(who, sizes, images.size(0), images.device)
    if sizes.device.type == "cpu":          # a device tensor is trusted: reading it would synchronise
        s = sizes.numpy()
        if (s < 1).any() or (s[:, 0] > images.size(1)).any() or (s[:, 1] > images.size(2)).any():
            raise ValueError(f"{who}: every sizes row must lie in [1, Hmax] x [1, Wmax]")


def _check_sizes(who, sizes, n, device):
    if not isinstance(sizes, torch.Tensor) or tuple(sizes.shape) != (n, 2) or sizes.dtype != torch.int32:
        raise ValueError(f"{who}: sizes must be [N, 2] int32 (h, w)")
    if sizes.device != device:
        raise ValueError(f"{who}: tensors on different devices")


def _apply(size, mean, channels_last, images, sizes, plan):
    _check_images("apply", images, sizes)
    n = images.size(0)
    if not isinstance(plan, torch.Tensor) or tuple(plan.shape) != (n, PLAN_WORDS) or plan.dtype != torch.int32 or plan.device != images.device:
        raise ValueError(f"apply: plan must be [N, {PLAN_WORDS}] int32 on the images' device")
    if images.device.type == "cpu":
        im, sz, pl = images.numpy(), sizes.numpy(), plan.numpy()
        x = torch.from_numpy(np.stack([_apply_one(im[i], int(sz[i, 0]), int(sz[i, 1]), pl[i], size, mean) for i in range(n)]))
        return x.contiguous(memory_format=torch.channels_last) if channels_last else x
    from ._lib import call, ptr, stream
    x = torch.empty(n, 3, size, size, dtype=torch.float32, device=images.device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    call("frost_aug_apply", ptr(images.contiguous()), ptr(sizes.contiguous()), ptr(plan.contiguous()), n, images.size(1), images.size(2), size,
         mean[0], mean[1], mean[2], int(channels_last), ptr(x), stream())
    return x


def _check_ctor(who, size, mean):
    if int(size) != size or not 1 <= size <= MAX_SIZE:
        raise ValueError(f"{who}: size outside 1 .. {MAX_SIZE}")
    mean = tuple(float(m) for m in mean)
    if len(mean) != 3:
        raise ValueError(f"{who}: mean is one value per BGR channel")
    return int(size), mean


class BaseTransform:
    """The eval-time transform (reference data/__init__.py:30-43): resize to size x size, subtract the mean.  `__call__(images, sizes) -> x`."""

    def __init__(self, size=512, mean=(104, 117, 123), channels_last=False):
        self.size, self.mean = _check_ctor("BaseTransform", size, mean)
        self.channels_last = bool(channels_last)

    def __call__(self, images, sizes):
        _check_images("BaseTransform", images, sizes)
        return _apply(self.size, self.mean, self.channels_last, images, sizes, identity_plan(sizes))


class SSDAugmentation:
    """`__call__(images, sizes, boxes, valid) -> (x, boxes_out, valid_out)`:
      images uint8 [N, Hmax, Wmax, 3] BGR, each image in the top-left corner of its slot; sizes int32 [N, 2] = (h, w); boxes fp32 [N, G, 5] rows (x1, y1, x2, y2 as
      fractions of the image, label); valid bool [N, G] (ssdlite.pad_targets' format).
      x fp32 [N, 3, size, size], contiguous or (channels_last=True) in torch.channels_last memory format; boxes_out / valid_out in the input's shapes: surviving boxes
      stay in their rows (the matching's "later ground truth wins" depends on order), dropped rows are zeros with valid_out False.
    `plan(sizes, boxes, valid) -> (plan, boxes_out, valid_out)` and `apply(images, sizes, plan) -> x` are the two halves; `last_plan` keeps the plan of the last call.
    The stream position {seed, images seen} is part of `state_dict()`.  On the device it lives in a two-word tensor that the plan launch reads and a one-thread kernel
    advances behind it: nothing synchronises with the host, and a replayed HIP graph of `__call__` draws fresh decisions."""

    def __init__(self, size=512, mean=(104, 117, 123), seed=None, channels_last=False):
        self.size, self.mean = _check_ctor("SSDAugmentation", size, mean)
        self.channels_last = bool(channels_last)
        self.seed = (default_seed() if seed is None else int(seed)) & _M64
        self._seen = 0            # the position of the CPU path, and the initial value of the device word
        self._state = None        # device: int64 {seed, images seen}
        self.last_plan = None

    # ---- stream ----
    def _device_state(self, device):
        if self._state is None or self._state.device != device:
            s = self.seed - (1 << 64) if self.seed >= 1 << 63 else self.seed
            self._state = torch.tensor([s, self.images_seen()], dtype=torch.int64).to(device)
        return self._state

    def images_seen(self):
        """Host value of the images-seen word (a device read when the state lives on the device)."""
        return int(self._state[1].item()) if self._state is not None else self._seen

    def state_dict(self):
        return {"seed": self.seed, "images_seen": self.images_seen()}

    def load_state_dict(self, state):
        """Restores {seed, images seen}; the device words are written IN PLACE, so a HIP graph captured earlier continues from the restored position."""
        self.seed, self._seen = int(state["seed"]) & _M64, int(state["images_seen"])
        if self._state is not None:
            s = self.seed - (1 << 64) if self.seed >= 1 << 63 else self.seed
            self._state.copy_(torch.tensor([s, self._seen], dtype=torch.int64))

    # ---- the two halves ----
    def plan(self, sizes, boxes, valid):
        if not isinstance(boxes, torch.Tensor) or not isinstance(valid, torch.Tensor) or not isinstance(sizes, torch.Tensor):
            raise ValueError("SSDAugmentation.plan: tensors expected")
        if boxes.dim() != 3 or boxes.size(2) != 5 or boxes.dtype != torch.float32 or boxes.size(0) < 1:
            raise ValueError("SSDAugmentation.plan: boxes must be [N, G, 5] float32")
        n, g = boxes.size(0), boxes.size(1)
        if not 1 <= g <= MAX_G:
            raise ValueError(f"SSDAugmentation.plan: G = {g} outside 1 .. {MAX_G}")
        if tuple(valid.shape) != (n, g) or valid.dtype != torch.bool:
            raise ValueError("SSDAugmentation.plan: valid must be [N, G] bool")
        _check_sizes("SSDAugmentation.plan", sizes, n, boxes.device)
        if valid.device != boxes.device:
            raise ValueError("SSDAugmentation.plan: tensors on different devices")
        if boxes.device.type == "cpu":
            sz, bx, vl = sizes.numpy(), boxes.numpy(), valid.numpy()
            if (sz < 1).any():
                raise ValueError("SSDAugmentation.plan: every sizes row must be >= 1")
            rows = [_plan_one(self.seed, self._seen + i, int(sz[i, 0]), int(sz[i, 1]), bx[i], vl[i]) for i in range(n)]
            self._seen += n
            return tuple(torch.from_numpy(np.stack([r[k] for r in rows])) for k in range(3))
        from ._lib import call, ptr, stream
        state = self._device_state(boxes.device)
        plan = torch.empty(n, PLAN_WORDS, dtype=torch.int32, device=boxes.device)
        boxes_out, valid_out = torch.empty_like(boxes, memory_format=torch.contiguous_format), torch.empty_like(valid, memory_format=torch.contiguous_format)
        call("frost_aug_plan", ptr(sizes.contiguous()), ptr(boxes.contiguous()), ptr(valid.contiguous()), n, g, ptr(state), ptr(plan), ptr(boxes_out),
             ptr(valid_out), stream())
        return plan, boxes_out, valid_out

    def apply(self, images, sizes, plan):
        return _apply(self.size, self.mean, self.channels_last, images, sizes, plan)

    def __call__(self, images, sizes, boxes, valid):
        _check_images("SSDAugmentation", images, sizes)
        if isinstance(boxes, torch.Tensor) and (boxes.device != images.device or boxes.size(0) != images.size(0)):
            raise ValueError("SSDAugmentation: images and boxes disagree in device or batch size")
        plan, boxes_out, valid_out = self.plan(sizes, boxes, valid)
        self.last_plan = plan
        return self.apply(images, sizes, plan), boxes_out, valid_out

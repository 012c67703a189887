"""The classifier's input pipeline on whole batches: the reference's training recipe `RandomResizedCrop(224)` -> `RandomHorizontalFlip()` -> `ToTensor()` ->
`Normalize(mean, std)` and its validation recipe `Resize(256)` -> `CenterCrop(224)` -> `ToTensor()` -> `Normalize` (Classification/utils/data_functions.py:23-42),
which it runs with torchvision on PIL images, one image at a time on the host.  uint8 batch in (`augment.pad_images`' format), the network's fp32 input out.  On
device tensors three HIP entries do the work (csrc/frost_caug.hip) without any host synchronisation; on CPU tensors the same classes run the definition below in
numpy, which is the yardstick of every GPU test.

As in augment.py the work is split in two.  `plan` takes every random decision and writes one fixed-size int32 record per image (PLAN_WORDS words, FROST_CAUG_* of
include/frost_hip.h): the crop rect in the source, the grid RW x RH the crop is resized to, and the offset of the size x size output window in that grid.  `apply`
is a pure function of (images, sizes, plan).

What is restated:
  * `RandomResizedCrop.get_params` of torchvision: up to TRIALS = 10 trials of (area fraction, log-uniform aspect), then the central fallback.  All of it fp64 in the
    written order; sqrt and / are correctly rounded on both sides, exp is NOT a libm call but `exp_poly`, a fixed Horner sequence, identical here and in the kernel.
    Added definition: the fallback's rounded side is clamped into [1, side] (with ratio bounds that straddle 1, as the defaults do, the clamp never acts).
  * `Resize` + `CenterCrop` of torchvision: shorter side -> resize, longer side -> resize * long // short; the window starts at round_half_even((grid - size) / 2).
  * The resize is Pillow's antialiased two-pass resampler with the triangle filter (ImagingResample, BILINEAR): fp64 weights normalised per output index, turned into
    22-bit fixed-point coefficients, horizontal pass into a uint8 intermediate, then the vertical pass.  torchvision crops first, so the filter's support is clipped to
    the crop.  tests/test_cls_augment_cpu.py holds `resize_crop` bit-equal to Pillow itself (tests/golden/g17_cls_resize.npz, and live Pillow where it imports).
  * The mirror acts on the resized window; `ToTensor` + `Normalize` is a 3 x 256 table of ((fp32(v) / 255) - mean_c) / std_c, every operation rounded to fp32.
  * Randomness is the library's Philox4x32-10 with augment._Draws' conventions and a stream tag of its own."""
import math

import numpy as np
import torch

from . import augment as _A
from .augment import MAX_SIZE, _M64, _check_images, _check_sizes, default_seed, philox4x32_10

PLAN_WORDS = 12          # FROST_CAUG_PLAN_WORDS
# word indices of a plan record (FROST_CAUG_* of include/frost_hip.h), all int32
P_FLAGS, P_X0, P_Y0, P_W, P_H, P_RW, P_RH, P_OX, P_OY, P_TRIES = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
F_MIRROR, F_FALLBACK = 1, 2
TRIALS = 10
STREAM_TAG = 0x43524F50          # "CROP": keeps this Philox stream apart from the detector's (augment.STREAM_TAG) and the library's others
PRECISION_BITS = 22              # Pillow: 32 - 8 - 2
EXP_DEGREE = 13
EXP_COEF = tuple(1.0 / math.factorial(k) for k in range(EXP_DEGREE + 1))          # k! < 2^53: each a correctly rounded quotient of two exact doubles
f32 = np.float32


class _Draws(_A._Draws):
    """augment._Draws on this module's stream, with the fp64 unit draw of the crop's trials."""

    def word(self):
        b = self.n >> 2
        if b != self.block:
            self.words, self.block = philox4x32_10((self.ord[0], self.ord[1], b, STREAM_TAG), self.key), b
        w = self.words[self.n & 3]
        self.n += 1
        return w

    def unit(self):
        return float(self.word() >> 8) * 2.0 ** -24


def exp_poly(t):
    """exp(t) for |t| <= log(4/3): Horner over the Taylor coefficients to degree 13, 13 multiplies and 13 adds in fp64.  Truncation 0.29^14 / 14! = 3e-19, rounding
    about 2 * 13 * 2^-53 * e^0.29 = 4e-15 relative: tests assert <= 1e-14 against math.exp."""
    r = EXP_COEF[EXP_DEGREE]
    for k in range(EXP_DEGREE - 1, -1, -1):
        r = r * t + EXP_COEF[k]
    return r


def _rint(v):
    return int(round(v))          # Python's round: half to even, as rint under the default rounding mode


# ---- the definition: decisions -------------------------------------------------------------------------------------------------------------------------
def _plan_one(seed, ordinal, h0, w0, size, scale, logr, ratio):
    """One image: the plan record int32 [PLAN_WORDS] of RandomResizedCrop.get_params + RandomHorizontalFlip."""
    rng = _Draws(seed, ordinal)
    rec = np.zeros(PLAN_WORDS, dtype=np.int32)
    area = float(h0 * w0)
    flags, tries, rect = 0, 0, None
    for _ in range(TRIALS):
        tries += 1
        target = area * (scale[0] + (scale[1] - scale[0]) * rng.unit())
        aspect = exp_poly(logr[0] + (logr[1] - logr[0]) * rng.unit())
        w, h = _rint(math.sqrt(target * aspect)), _rint(math.sqrt(target / aspect))
        if 0 < w <= w0 and 0 < h <= h0:
            y0 = rng.choice(h0 - h + 1)
            rect = (rng.choice(w0 - w + 1), y0, w, h)
            break
    if rect is None:
        flags |= F_FALLBACK
        in_ratio = float(w0) / float(h0)
        if in_ratio < ratio[0]:
            w, h = w0, min(max(_rint(float(w0) / ratio[0]), 1), h0)
        elif in_ratio > ratio[1]:
            h, w = h0, min(max(_rint(float(h0) * ratio[1]), 1), w0)
        else:
            w, h = w0, h0
        rect = ((w0 - w) // 2, (h0 - h) // 2, w, h)
    if rng.coin():
        flags |= F_MIRROR
    rec[P_FLAGS], rec[P_TRIES] = flags, tries
    rec[P_X0:P_H + 1] = rect
    rec[P_RW], rec[P_RH] = size, size
    return rec


def _half_even(d):
    """round(d / 2) for an integer d >= 0, half to even."""
    return (d + ((d >> 1) & 1)) >> 1


def _eval_plan_one(h0, w0, size, resize):
    """Resize(resize) + CenterCrop(size): the whole image, the grid that keeps the aspect with the shorter side at `resize`, the central window."""
    rec = np.zeros(PLAN_WORDS, dtype=np.int32)
    rw, rh = (resize, resize * h0 // w0) if w0 <= h0 else (resize * w0 // h0, resize)
    rec[P_W], rec[P_H], rec[P_RW], rec[P_RH], rec[P_OX], rec[P_OY] = w0, h0, rw, rh, _half_even(rw - size), _half_even(rh - size)
    return rec


# ---- the definition: pixels ----------------------------------------------------------------------------------------------------------------------------
def resample_coeffs(n_in, n_out, first, count):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter, for output indices first .. first + count - 1 of a resize n_in -> n_out:
    (xmin [count] int64, coef [count, K] int64 with zeros behind each index's last tap).  fp64, in Pillow's order."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    k = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # the C cast: towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    x = np.arange(k, dtype=np.int64)[None, :]
    a = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((x < (xmax - xmin)[:, None]) & (a < 1.0), 1.0 - a, 0.0)
    ww = np.zeros(count, dtype=np.float64)
    for j in range(k):                                                          # ascending x, as Pillow sums (a zero behind the last tap changes nothing)
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    return xmin, (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)


def _pass(src, xmin, coef):
    """One resampling pass along axis 1 of src uint8 [R, n_in, 3] -> uint8 [R, count, 3]."""
    idx = np.minimum(xmin[:, None] + np.arange(coef.shape[1], dtype=np.int64)[None, :], src.shape[1] - 1)          # a tap past the last one has coefficient 0
    acc = (1 << (PRECISION_BITS - 1)) + (src[:, idx].astype(np.int64) * coef[None, :, :, None]).sum(2)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_crop(crop, rw, rh, ox=0, oy=0, out_w=None, out_h=None):
    """uint8 [h, w, 3] -> the out_h x out_w window at (ox, oy) of `Image.resize((rw, rh), BILINEAR)` of the crop: horizontal pass first, uint8 intermediate."""
    out_w, out_h = rw - ox if out_w is None else out_w, rh - oy if out_h is None else out_h
    ymin, cy = resample_coeffs(crop.shape[0], rh, oy, out_h)
    xmin, cx = resample_coeffs(crop.shape[1], rw, ox, out_w)
    mid = _pass(crop, xmin, cx)
    return np.ascontiguousarray(_pass(mid.transpose(1, 0, 2), ymin, cy).transpose(1, 0, 2))


def norm_table(mean, std):
    """fp32 [3, 256]: ToTensor + Normalize of every byte value per channel, each operation rounded to fp32."""
    v = np.arange(256, dtype=np.float32)[None, :]
    m, s = np.asarray(mean, dtype=np.float32)[:, None], np.asarray(std, dtype=np.float32)[:, None]
    return f32(f32(f32(v / f32(255.0)) - m) / s)


def _apply_one(img, rec, size, table):
    x0, y0, w, h = (int(v) for v in rec[P_X0:P_H + 1])
    win = resize_crop(img[y0:y0 + h, x0:x0 + w], int(rec[P_RW]), int(rec[P_RH]), int(rec[P_OX]), int(rec[P_OY]), size, size)
    if int(rec[P_FLAGS]) & F_MIRROR:
        win = win[:, ::-1]
    return np.stack([table[c][win[..., c]] for c in range(3)])


# ---- the public classes --------------------------------------------------------------------------------------------------------------------------------
def _check_ctor(who, size, mean, std):
    if int(size) != size or not 1 <= size <= MAX_SIZE:
        raise ValueError(f"{who}: size outside 1 .. {MAX_SIZE}")
    mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError(f"{who}: mean and std are one value per channel, std non-zero")
    return int(size), mean, std


def _apply(who, size, mean, std, channels_last, images, sizes, plan):
    _check_images(who, images, sizes)
    n = images.size(0)
    if not isinstance(plan, torch.Tensor) or tuple(plan.shape) != (n, PLAN_WORDS) or plan.dtype != torch.int32 or plan.device != images.device:
        raise ValueError(f"{who}: plan must be [N, {PLAN_WORDS}] int32 on the images' device")
    if images.device.type == "cpu":
        im, sz, pl = images.numpy(), sizes.numpy(), plan.numpy().astype(np.int64)
        bad = (pl[:, P_X0] < 0) | (pl[:, P_Y0] < 0) | (pl[:, P_W] < 1) | (pl[:, P_H] < 1) | (pl[:, P_X0] + pl[:, P_W] > sz[:, 1]) | (pl[:, P_Y0] + pl[:, P_H] > sz[:, 0]) \
            | (pl[:, P_OX] < 0) | (pl[:, P_OY] < 0) | (pl[:, P_OX] + size > pl[:, P_RW]) | (pl[:, P_OY] + size > pl[:, P_RH])
        if bad.any():
            raise ValueError(f"{who}: a plan record's rect leaves its image, or its window leaves the resize grid")
        table = norm_table(mean, std)
        x = torch.from_numpy(np.stack([_apply_one(im[i], pl[i], size, table) for i in range(n)]))
        return x.contiguous(memory_format=torch.channels_last) if channels_last else x
    from ._lib import call, ptr, stream
    x = torch.empty(n, 3, size, size, dtype=torch.float32, device=images.device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    call("frost_caug_apply", ptr(images.contiguous()), ptr(sizes.contiguous()), ptr(plan.contiguous()), n, images.size(1), images.size(2), size,
         mean[0], mean[1], mean[2], std[0], std[1], std[2], int(channels_last), ptr(x), stream())
    return x


class ClassificationEvalTransform:
    """`Resize(resize)` -> `CenterCrop(size)` -> `ToTensor()` -> `Normalize(mean, std)` of a batch.  `__call__(images, sizes) -> x`: images uint8 [N, Hmax, Wmax, 3], each
    image in the top-left corner of its slot (augment.pad_images), sizes int32 [N, 2] = (h, w); x fp32 [N, 3, size, size], contiguous or channels-last."""

    def __init__(self, size=224, resize=256, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels_last=False):
        self.size, self.mean, self.std = _check_ctor("ClassificationEvalTransform", size, mean, std)
        if int(resize) != resize or not self.size <= resize <= MAX_SIZE:
            raise ValueError(f"ClassificationEvalTransform: resize outside size .. {MAX_SIZE}")
        self.resize, self.channels_last = int(resize), bool(channels_last)

    def plan(self, sizes):
        if not isinstance(sizes, torch.Tensor) or sizes.dim() != 2 or sizes.size(0) < 1:
            raise ValueError("ClassificationEvalTransform.plan: sizes must be [N, 2] int32 (h, w)")
        _check_sizes("ClassificationEvalTransform.plan", sizes, sizes.size(0), sizes.device)
        if sizes.device.type == "cpu":
            sz = sizes.numpy()
            if (sz < 1).any():
                raise ValueError("ClassificationEvalTransform.plan: every sizes row must be >= 1")
            return torch.from_numpy(np.stack([_eval_plan_one(int(h), int(w), self.size, self.resize) for h, w in sz]))
        from ._lib import call, ptr, stream
        plan = torch.empty(sizes.size(0), PLAN_WORDS, dtype=torch.int32, device=sizes.device)
        call("frost_caug_eval_plan", ptr(sizes.contiguous()), sizes.size(0), self.size, self.resize, ptr(plan), stream())
        return plan

    def __call__(self, images, sizes):
        _check_images("ClassificationEvalTransform", images, sizes)
        return _apply("ClassificationEvalTransform", self.size, self.mean, self.std, self.channels_last, images, sizes, self.plan(sizes))


class ClassificationAugmentation:
    """`RandomResizedCrop(size, scale, ratio)` -> `RandomHorizontalFlip()` -> `ToTensor()` -> `Normalize(mean, std)` of a batch.  `__call__(images, sizes) -> x` in
    ClassificationEvalTransform's formats.  `plan(sizes) -> plan` and `apply(images, sizes, plan) -> x` are the two halves; `last_plan` keeps the plan of the last call.
    The stream position {seed, images seen} is part of `state_dict()`.  On the device it lives in a two-word tensor that the plan launch reads and a one-thread kernel
    advances behind it: nothing synchronises with the host, and a replayed HIP graph of `__call__` draws fresh crops."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), seed=None, channels_last=False):
        self.size, self.mean, self.std = _check_ctor("ClassificationAugmentation", size, mean, std)
        self.scale, self.ratio = tuple(float(s) for s in scale), tuple(float(r) for r in ratio)
        if len(self.scale) != 2 or len(self.ratio) != 2 or not 0 < self.scale[0] <= self.scale[1] or not 0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError("ClassificationAugmentation: scale and ratio are (min, max) with 0 < min <= max")
        if self.ratio[0] < 0.5 or self.ratio[1] > 2.0:          # exp_poly's truncation at |t| = log 2 is 0.7^14 / 14! = 7e-14; beyond that it grows quickly
            raise ValueError("ClassificationAugmentation: ratio outside 1/2 .. 2")
        self.logr = (math.log(self.ratio[0]), math.log(self.ratio[1]))          # once, on the host; the kernel receives the two doubles
        self.channels_last = bool(channels_last)
        self.seed = (default_seed() if seed is None else int(seed)) & _M64
        self._seen = 0            # the position of the CPU path, and the initial value of the device word
        self._state = None        # device: int64 {seed, images seen}
        self.last_plan = None

    # ---- stream ----
    def _signed_seed(self):
        return self.seed - (1 << 64) if self.seed >= 1 << 63 else self.seed

    def _device_state(self, device):
        if self._state is None or self._state.device != device:
            self._state = torch.tensor([self._signed_seed(), self.images_seen()], dtype=torch.int64).to(device)
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
            self._state.copy_(torch.tensor([self._signed_seed(), self._seen], dtype=torch.int64))

    # ---- the two halves ----
    def plan(self, sizes):
        if not isinstance(sizes, torch.Tensor) or sizes.dim() != 2 or sizes.size(0) < 1:
            raise ValueError("ClassificationAugmentation.plan: sizes must be [N, 2] int32 (h, w)")
        n = sizes.size(0)
        _check_sizes("ClassificationAugmentation.plan", sizes, n, sizes.device)
        if sizes.device.type == "cpu":
            sz = sizes.numpy()
            if (sz < 1).any():
                raise ValueError("ClassificationAugmentation.plan: every sizes row must be >= 1")
            rows = [_plan_one(self.seed, self._seen + i, int(sz[i, 0]), int(sz[i, 1]), self.size, self.scale, self.logr, self.ratio) for i in range(n)]
            self._seen += n
            return torch.from_numpy(np.stack(rows))
        from ._lib import call, ptr, stream
        state = self._device_state(sizes.device)
        plan = torch.empty(n, PLAN_WORDS, dtype=torch.int32, device=sizes.device)
        call("frost_caug_plan", ptr(sizes.contiguous()), n, self.size, self.scale[0], self.scale[1], self.logr[0], self.logr[1], self.ratio[0], self.ratio[1],
             ptr(state), ptr(plan), stream())
        return plan

    def apply(self, images, sizes, plan):
        return _apply("ClassificationAugmentation.apply", self.size, self.mean, self.std, self.channels_last, images, sizes, plan)

    def __call__(self, images, sizes):
        _check_images("ClassificationAugmentation", images, sizes)
        plan = self.plan(sizes)
        self.last_plan = plan
        return self.apply(images, sizes, plan)

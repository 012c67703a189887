"""The segmentation input pipeline on whole batches: the reference's training recipes `RandomFlip` -> `RandomScale` -> `RandomCrop` -> `Normalize` (PASCAL VOC) and
`RandomScale` -> `RandomCrop` -> `RandomFlip` -> `Normalize` (Cityscapes), and its validation recipes `Resize` -> `Normalize` and `Normalize` alone
(Semantic_Segmentation/utilities/data_transforms.py, composed in data_loader/segmentation/voc.py and cityscapes.py), which it runs on PIL images, one pair at a time on
the host.  uint8 pictures and uint8 label maps in (`pad_pairs`' format), the network's fp32 input and the criterion's target out.  On device tensors the HIP entries of
csrc/frost_saug.hip do the work without any host synchronisation; on CPU tensors the same classes run the definition below in numpy, which is the yardstick of every
GPU test.

As in cls_augment.py the work is split in two.  `plan` takes every random decision and writes one fixed-size int32 record per image (PLAN_WORDS words, FROST_SAUG_* of
include/frost_hip.h): the flags (mirror, which side of the resize the mirror acts on, the filter), the grid RW x RH the whole picture is resized to, and the offset
(OX, OY) of the crop window in that grid.  The offset may be negative and the window may pass the grid's far edges: whatever lies outside the grid is padding
(byte 0 in the picture, `ignore_idx` in the label map), which is how `RandomCrop`'s `Pad` is carried.  `apply` is a pure function of (images, labels, sizes, plan).

What is restated:
  * `RandomScale`: s log-uniform in [s0, s1]; the new size is (round(w s), round(h s)).  Ours: s = exp_poly(ln s0 + u (ln s1 - ln s0)) with cls_augment's written-out
    exp, the rounding half to even, the sides clamped into [1, 2 MAX_SIZE].
  * The picture's resize is Pillow's antialiased two-pass resampler with the Lanczos filter (`Image.ANTIALIAS`, today `Image.LANCZOS`): sinc(x) sinc(x / 3) on
    [-3, 3), fp64 weights summed in ascending order and normalised, 22-bit fixed point with Pillow's separate rounding of NEGATIVE weights, a uint8 intermediate
    between the horizontal and the vertical pass.  sin is NOT a libm call but `sin_pi`, a fixed fp64 sequence, identical here and in the kernel;
    tests/test_seg_augment_cpu.py holds the coefficient tables equal to the libm ones and `resize_lanczos` bit-equal to Pillow itself.
  * The label's resize is Pillow's nearest-neighbour transform, whose index table is filled by REPEATED ADDITION (xo = a / 2; idx = (int) xo; xo += a with
    a = n_in / n_out): the closed form (int)((x + 0.5) a) differs from it on about a fifth of all size pairs.
  * `RandomCrop`: pad = max(0, (1 + crop - side) // 2) on both sides of an axis, then a uniform window of the padded grid; `RandomFlip`: a left-right mirror of both
    planes; `Normalize`: cls_augment.norm_table, the label as int64 (or uint8).
  * Validation: `Resize(size)` is the triangle filter (`Image.BILINEAR`, cls_augment.resample_coeffs) to exactly (w, h) and nearest for the label.
  * Randomness is the library's Philox4x32-10 with augment._Draws' conventions and a stream tag of its own; every image uses exactly one block of four words:
    scale unit, row offset, column offset, coin."""
import math

import numpy as np
import torch

from . import augment as _A
from .augment import MAX_SIZE, _M64, _check_images, default_seed, philox4x32_10
from .cls_augment import PRECISION_BITS, _check_ctor, _pass, _rint, exp_poly, norm_table, resample_coeffs

PLAN_WORDS = 8           # FROST_SAUG_PLAN_WORDS
# word indices of a plan record (FROST_SAUG_* of include/frost_hip.h), all int32
P_FLAGS, P_RW, P_RH, P_OX, P_OY, P_PADW, P_PADH = 0, 1, 2, 3, 4, 5, 6
F_MIRROR, F_FLIP_FIRST, F_LANCZOS, F_TRIANGLE = 1, 2, 4, 8          # neither filter bit: no resize, the grid IS the image
MAX_GRID = 2 * MAX_SIZE          # a side of the resize grid, and the largest |offset| of the window
STREAM_TAG = 0x53454741          # "SEGA": keeps this Philox stream apart from the classifier's, the detector's and the library's others
PI = float.fromhex("0x1.921fb54442d18p+1")
# (-1)^k / (2k + 1)!, k = 0 .. 11, each the correctly rounded quotient 1 / float((2k + 1)!), written as the bits the kernel holds too
SIN_COEF = tuple(float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19", "-0x1.ae64567f544e4p-26",
    "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49", "-0x1.2f49b46814157p-57", "0x1.71b8ef6dcf572p-66", "-0x1.761b413163819p-75"))
f32 = np.float32


class _Draws(_A._Draws):
    """augment._Draws on this module's stream, with the fp64 unit draw of the scale."""

    def word(self):
        b = self.n >> 2
        if b != self.block:
            self.words, self.block = philox4x32_10((self.ord[0], self.ord[1], b, STREAM_TAG), self.key), b
        w = self.words[self.n & 3]
        self.n += 1
        return w

    def unit(self):
        return float(self.word() >> 8) * 2.0 ** -24


# ---- the definition: the two resamplers ----------------------------------------------------------------------------------------------------------------
def sin_pi(x):
    """sin(pi x) in a fixed fp64 sequence (scalar or array): x = n + r with n = rint(x), t = pi r, Horner over the odd Taylor terms of t up to degree 23 in t^2
    (11 multiplies and 11 adds), times t, negated for odd n.  Truncation (pi / 2)^25 / 25! = 5e-21; rounding about 1e-15 absolute."""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x)
    t = PI * (x - n)
    t2 = t * t
    p = np.full_like(t, SIN_COEF[11])
    for k in range(10, -1, -1):
        p = p * t2 + SIN_COEF[k]
    s = p * t
    s = np.where(np.fmod(n, 2.0) != 0.0, -s, s)
    return float(s) if s.ndim == 0 else s


def lanczos_coeffs(n_in, n_out, first=0, count=None, sin=sin_pi):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the Lanczos filter, for output indices first .. first + count - 1 of a resize n_in -> n_out:
    (xmin [count] int64, coef [count, K] int64 with zeros behind each index's last tap).  fp64, in Pillow's order.  `sin(x)` returns sin(pi x) of an array."""
    count = n_out - first if count is None else count
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support, ss = 3.0 * fs, 1.0 / fs
    k = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # the C cast: towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    x = np.arange(k, dtype=np.int64)[None, :]
    a = ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    a3 = a / 3.0

    def sinc(v):
        d = np.where(v == 0.0, 1.0, v * PI)
        return np.where(v == 0.0, 1.0, sin(v) / d)

    w = np.where((x < (xmax - xmin)[:, None]) & (a >= -3.0) & (a < 3.0), sinc(a) * sinc(a3), 0.0)
    ww = np.zeros(count, dtype=np.float64)
    for j in range(k):                                                          # ascending x, as Pillow sums (a zero behind the last tap changes nothing)
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    one = float(1 << PRECISION_BITS)
    return xmin, np.where(w < 0.0, -0.5 + w * one, 0.5 + w * one).astype(np.int64)          # Pillow rounds a negative weight away from zero too


def nearest_index(n_in, n_out, count=None):
    """Pillow's nearest-neighbour source index of output indices 0 .. count - 1 of a resize n_in -> n_out (ImagingScaleAffine): int64 [count], accumulated."""
    count = n_out if count is None else count
    a = float(n_in) / float(n_out)
    xo = 0.5 * a
    out = np.empty(count, dtype=np.int64)
    for x in range(count):
        out[x] = min(int(xo), n_in - 1)
        xo = xo + a
    return out


def _coeffs(filt, n_in, n_out, first, count):
    return lanczos_coeffs(n_in, n_out, first, count) if filt == F_LANCZOS else resample_coeffs(n_in, n_out, first, count)


def _resize_window(src, filt, rw, rh, x0, x1, y0, y1):
    """uint8 [h, w, 3] -> columns x0 .. x1 - 1, rows y0 .. y1 - 1 of `Image.resize((rw, rh), filter)`: horizontal pass first, uint8 intermediate."""
    ymin, cy = _coeffs(filt, src.shape[0], rh, y0, y1 - y0)
    xmin, cx = _coeffs(filt, src.shape[1], rw, x0, x1 - x0)
    mid = _pass(src, xmin, cx)
    return np.ascontiguousarray(_pass(mid.transpose(1, 0, 2), ymin, cy).transpose(1, 0, 2))


def resize_lanczos(img, rw, rh):
    """uint8 [h, w, 3] -> `Image.resize((rw, rh), Image.LANCZOS)` as uint8 [rh, rw, 3]."""
    img = np.ascontiguousarray(img)
    return _resize_window(img, F_LANCZOS, int(rw), int(rh), 0, int(rw), 0, int(rh))


def _apply_one(img, lab, rec, cw, ch, table, ignore_idx):
    flags, rw, rh, ox, oy = (int(v) for v in rec[:P_OY + 1])
    mirror, first = bool(flags & F_MIRROR), bool(flags & F_FLIP_FIRST)
    filt = flags & (F_LANCZOS | F_TRIANGLE)
    if mirror and first:
        img, lab = img[:, ::-1], lab[:, ::-1]
    pic, tgt = np.zeros((ch, cw, 3), dtype=np.uint8), np.full((ch, cw), ignore_idx, dtype=np.uint8)
    x0, x1, y0, y1 = max(ox, 0), min(ox + cw, rw), max(oy, 0), min(oy + ch, rh)          # the window's part of the grid
    if x0 < x1 and y0 < y1:
        if filt:
            pic[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = _resize_window(np.ascontiguousarray(img), filt, rw, rh, x0, x1, y0, y1)
        else:
            pic[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = img[y0:y1, x0:x1]
        iy, ix = nearest_index(lab.shape[0], rh, y1)[y0:], nearest_index(lab.shape[1], rw, x1)[x0:]
        tgt[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = lab[iy[:, None], ix[None, :]]
    if mirror and not first:
        pic, tgt = pic[:, ::-1], tgt[:, ::-1]
    return np.stack([table[c][pic[..., c]] for c in range(3)]), np.ascontiguousarray(tgt)


# ---- the definition: decisions -------------------------------------------------------------------------------------------------------------------------
def _pad(crop, side):
    """RandomCrop: max(0, int((1 + crop - side) / 2)) on each side of the axis."""
    return max(0, (1 + crop - side) >> 1)


def _plan_one(seed, ordinal, h0, w0, cw, ch, logs, flip_first):
    """One image: the plan record int32 [PLAN_WORDS] of RandomScale + RandomCrop + RandomFlip.  Four words, in this order for both recipes."""
    rng = _Draws(seed, ordinal)
    rec = np.zeros(PLAN_WORDS, dtype=np.int32)
    s = exp_poly(logs[0] + rng.unit() * (logs[1] - logs[0]))
    rw, rh = min(max(_rint(float(w0) * s), 1), MAX_GRID), min(max(_rint(float(h0) * s), 1), MAX_GRID)
    pw, ph = _pad(cw, rw), _pad(ch, rh)
    oy = rng.choice(rh + 2 * ph - ch + 1) - ph
    ox = rng.choice(rw + 2 * pw - cw + 1) - pw
    flags = F_LANCZOS | (F_FLIP_FIRST if flip_first else 0) | (F_MIRROR if rng.coin() else 0)
    rec[:] = (flags, rw, rh, ox, oy, pw, ph, 0)
    return rec


# ---- the public interface ------------------------------------------------------------------------------------------------------------------------------
def pad_pairs(images, labels):
    """lists of HxWx3 uint8 pictures and HxW uint8 label maps -> (images uint8 [N, Hmax, Wmax, 3], labels uint8 [N, Hmax, Wmax], sizes int32 [N, 2] = (h, w)), each
    pair in the top-left corner of its slot: a collate function's work."""
    im = [torch.as_tensor(np.ascontiguousarray(i)) if not isinstance(i, torch.Tensor) else i for i in images]
    lb = [torch.as_tensor(np.ascontiguousarray(i)) if not isinstance(i, torch.Tensor) else i for i in labels]
    if not im or len(im) != len(lb) or any(t.dim() != 3 or t.size(2) != 3 or t.dtype != torch.uint8 or t.size(0) < 1 or t.size(1) < 1 for t in im) \
            or any(g.dim() != 2 or g.dtype != torch.uint8 or tuple(g.shape) != tuple(t.shape[:2]) for t, g in zip(im, lb)):
        raise ValueError("pad_pairs: equally long, non-empty lists of HxWx3 uint8 pictures and HxW uint8 label maps of the same extents expected")
    hmax, wmax = max(t.size(0) for t in im), max(t.size(1) for t in im)
    oi, ol = torch.zeros(len(im), hmax, wmax, 3, dtype=torch.uint8), torch.zeros(len(im), hmax, wmax, dtype=torch.uint8)
    for i, (t, g) in enumerate(zip(im, lb)):
        oi[i, :t.size(0), :t.size(1)] = t
        ol[i, :t.size(0), :t.size(1)] = g
    return oi, ol, torch.tensor([[t.size(0), t.size(1)] for t in im], dtype=torch.int32)


def _check_crop(who, crop_size):
    cs = (crop_size, crop_size) if isinstance(crop_size, (int, np.integer)) else tuple(crop_size)
    if len(cs) != 2 or any(int(c) != c or not 1 <= c <= MAX_SIZE for c in cs):
        raise ValueError(f"{who}: crop_size is (w, h) or one int, each side in 1 .. {MAX_SIZE}")
    return int(cs[0]), int(cs[1])


def _check_common(who, ignore_idx, mean, std, target_dtype):
    _, mean, std = _check_ctor(who, 1, mean, std)
    if int(ignore_idx) != ignore_idx or not 0 <= ignore_idx <= 255:
        raise ValueError(f"{who}: ignore_idx outside 0 .. 255")
    if target_dtype not in (torch.int64, torch.uint8):
        raise ValueError(f"{who}: target_dtype is torch.int64 or torch.uint8")
    return int(ignore_idx), mean, std


def _check_pairs(who, images, labels, sizes):
    _check_images(who, images, sizes)
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or tuple(labels.shape) != tuple(images.shape[:3]) or labels.device != images.device:
        raise ValueError(f"{who}: labels must be [N, Hmax, Wmax] uint8 on the images' device")


def _apply(who, cw, ch, ignore_idx, mean, std, channels_last, target_dtype, images, labels, sizes, plan):
    _check_pairs(who, images, labels, sizes)
    n = images.size(0)
    if not isinstance(plan, torch.Tensor) or tuple(plan.shape) != (n, PLAN_WORDS) or plan.dtype != torch.int32 or plan.device != images.device:
        raise ValueError(f"{who}: plan must be [N, {PLAN_WORDS}] int32 on the images' device")
    if images.device.type == "cpu":
        im, lb, sz, pl = images.numpy(), labels.numpy(), sizes.numpy(), plan.numpy().astype(np.int64)
        filt = pl[:, P_FLAGS] & (F_LANCZOS | F_TRIANGLE)
        bad = (pl[:, P_FLAGS] < 0) | (pl[:, P_FLAGS] > 15) | (filt == (F_LANCZOS | F_TRIANGLE)) | (pl[:, P_RW] < 1) | (pl[:, P_RH] < 1) | (pl[:, P_RW] > MAX_GRID) \
            | (pl[:, P_RH] > MAX_GRID) | (np.abs(pl[:, P_OX]) > MAX_GRID) | (np.abs(pl[:, P_OY]) > MAX_GRID) \
            | ((filt == 0) & ((pl[:, P_RW] != sz[:, 1]) | (pl[:, P_RH] != sz[:, 0])))
        if bad.any():
            raise ValueError(f"{who}: a plan record's flags, grid or offset are out of range, or a record without a filter has a grid other than its image")
        table = norm_table(mean, std)
        outs = [_apply_one(im[i, :sz[i, 0], :sz[i, 1]], lb[i, :sz[i, 0], :sz[i, 1]], pl[i], cw, ch, table, ignore_idx) for i in range(n)]
        x, t = torch.from_numpy(np.stack([o[0] for o in outs])), torch.from_numpy(np.stack([o[1] for o in outs])).to(target_dtype)
        return (x.contiguous(memory_format=torch.channels_last) if channels_last else x), t
    from ._lib import call, ptr, stream
    dev = images.device
    x = torch.empty(n, 3, ch, cw, dtype=torch.float32, device=dev, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    t = torch.empty(n, ch, cw, dtype=target_dtype, device=dev)
    tables = torch.empty(n, cw + ch, dtype=torch.int32, device=dev)          # the window's entries of the two nearest-neighbour index tables
    call("frost_saug_apply", ptr(images.contiguous()), ptr(labels.contiguous()), ptr(sizes.contiguous()), ptr(plan.contiguous()), n, images.size(1), images.size(2),
         cw, ch, mean[0], mean[1], mean[2], std[0], std[1], std[2], ignore_idx, int(channels_last), int(target_dtype == torch.int64), 7, ptr(tables), ptr(x), ptr(t),
         stream())
    return x, t


class SegmentationEvalTransform:
    """`Resize(size)` -> `Normalize` (size = (w, h): PASCAL VOC) or `Normalize` alone (size = None: Cityscapes; every image has to fill its slot) of a batch.
    `__call__(images, labels, sizes) -> (x, target)`: images uint8 [N, Hmax, Wmax, 3], labels uint8 [N, Hmax, Wmax], sizes int32 [N, 2] = (h, w) (`pad_pairs`);
    x fp32 [N, 3, h, w], contiguous or channels-last, target [N, h, w] int64 or uint8."""

    def __init__(self, size=None, ignore_idx=255, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels_last=False, target_dtype=torch.int64):
        who = "SegmentationEvalTransform"
        self.size = None if size is None else _check_crop(who, size)
        self.ignore_idx, self.mean, self.std = _check_common(who, ignore_idx, mean, std, target_dtype)
        self.channels_last, self.target_dtype = bool(channels_last), target_dtype

    def plan(self, sizes):
        if not isinstance(sizes, torch.Tensor) or sizes.dim() != 2 or sizes.size(0) < 1:
            raise ValueError("SegmentationEvalTransform.plan: sizes must be [N, 2] int32 (h, w)")
        n = sizes.size(0)
        _A._check_sizes("SegmentationEvalTransform.plan", sizes, n, sizes.device)
        w, h = self.size if self.size is not None else (0, 0)
        if sizes.device.type == "cpu":
            sz = sizes.numpy()
            if (sz < 1).any():
                raise ValueError("SegmentationEvalTransform.plan: every sizes row must be >= 1")
            plan = np.zeros((n, PLAN_WORDS), dtype=np.int32)
            if self.size is None:
                plan[:, P_RW], plan[:, P_RH] = sz[:, 1], sz[:, 0]
            else:
                plan[:, P_FLAGS], plan[:, P_RW], plan[:, P_RH] = F_TRIANGLE, w, h
            return torch.from_numpy(plan)
        from ._lib import call, ptr, stream
        plan = torch.empty(n, PLAN_WORDS, dtype=torch.int32, device=sizes.device)
        call("frost_saug_eval_plan", ptr(sizes.contiguous()), n, w, h, ptr(plan), stream())
        return plan

    def apply(self, images, labels, sizes, plan):
        who = "SegmentationEvalTransform.apply"
        _check_pairs(who, images, labels, sizes)
        if self.size is None and sizes.device.type == "cpu" and bool(((sizes[:, 0] != images.size(1)) | (sizes[:, 1] != images.size(2))).any()):
            raise ValueError(f"{who}: without a size every image has to fill its slot")
        cw, ch = self.size if self.size is not None else (images.size(2), images.size(1))
        if cw > MAX_SIZE or ch > MAX_SIZE:
            raise ValueError(f"{who}: a side above {MAX_SIZE}")
        return _apply(who, cw, ch, self.ignore_idx, self.mean, self.std, self.channels_last, self.target_dtype, images, labels, sizes, plan)

    def __call__(self, images, labels, sizes):
        _check_pairs("SegmentationEvalTransform", images, labels, sizes)
        return self.apply(images, labels, sizes, self.plan(sizes))


class SegmentationAugmentation:
    """`RandomScale(scale)` -> `RandomCrop(crop_size)` -> `Normalize` of a batch with `RandomFlip` in front of them (flip_first=True, the PASCAL VOC order: the mirror
    acts on the source, in front of both resizes) or behind the crop (flip_first=False, the Cityscapes order).  `__call__(images, labels, sizes) -> (x, target)` in
    SegmentationEvalTransform's formats, (h, w) = crop_size[::-1].  `plan(sizes) -> plan` and `apply(images, labels, sizes, plan) -> (x, target)` are the two halves;
    `last_plan` keeps the plan of the last call.  The stream position {seed, images seen} is part of `state_dict()`.  On the device it lives in a two-word tensor that
    the plan launch reads and a one-thread kernel advances behind it: nothing synchronises with the host, and a replayed HIP graph of `__call__` draws fresh crops."""

    def __init__(self, crop_size, scale=(0.5, 1.0), flip_first=True, ignore_idx=255, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), seed=None,
                 channels_last=False, target_dtype=torch.int64):
        who = "SegmentationAugmentation"
        self.crop_size = _check_crop(who, crop_size)
        self.ignore_idx, self.mean, self.std = _check_common(who, ignore_idx, mean, std, target_dtype)
        self.scale = tuple(float(s) for s in scale)
        if len(self.scale) != 2 or not 0.5 <= self.scale[0] <= self.scale[1] <= 2.0:          # exp_poly's stated domain: |t| <= log 2
            raise ValueError(f"{who}: scale is (min, max) with 1/2 <= min <= max <= 2")
        self.logs = (math.log(self.scale[0]), math.log(self.scale[1]))          # once, on the host; the kernel receives the two doubles
        self.flip_first, self.channels_last, self.target_dtype = bool(flip_first), bool(channels_last), target_dtype
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
        who = "SegmentationAugmentation.plan"
        if not isinstance(sizes, torch.Tensor) or sizes.dim() != 2 or sizes.size(0) < 1:
            raise ValueError(f"{who}: sizes must be [N, 2] int32 (h, w)")
        n = sizes.size(0)
        _A._check_sizes(who, sizes, n, sizes.device)
        cw, ch = self.crop_size
        if sizes.device.type == "cpu":
            sz = sizes.numpy()
            if (sz < 1).any():
                raise ValueError(f"{who}: every sizes row must be >= 1")
            rows = [_plan_one(self.seed, self._seen + i, int(sz[i, 0]), int(sz[i, 1]), cw, ch, self.logs, self.flip_first) for i in range(n)]
            self._seen += n
            return torch.from_numpy(np.stack(rows))
        from ._lib import call, ptr, stream
        state = self._device_state(sizes.device)
        plan = torch.empty(n, PLAN_WORDS, dtype=torch.int32, device=sizes.device)
        call("frost_saug_plan", ptr(sizes.contiguous()), n, cw, ch, self.logs[0], self.logs[1], int(self.flip_first), ptr(state), ptr(plan), stream())
        return plan

    def apply(self, images, labels, sizes, plan):
        cw, ch = self.crop_size
        return _apply("SegmentationAugmentation.apply", cw, ch, self.ignore_idx, self.mean, self.std, self.channels_last, self.target_dtype, images, labels, sizes,
                      plan)

    def __call__(self, images, labels, sizes):
        _check_pairs("SegmentationAugmentation", images, labels, sizes)
        plan = self.plan(sizes)
        self.last_plan = plan
        return self.apply(images, labels, sizes, plan)

"""Segmentation criterion and mean-IoU meter on the device (csrc/frost_seg.hip), with the reference's surface:
`SegmentationLoss` (Semantic_Segmentation/loss_fns/segmentation_loss.py, loss_type 'ce') and `SegMeter` (utilities/metrics/segmentation_miou.py: MIOU plus
the two AverageMeters of utilities/train_eval_seg.py).  The reference's models end in `F.interpolate(out, size, mode='bilinear', align_corners=True)`; here the
criterion takes the LOW-resolution logits and upsamples inside the kernel, so nothing of the label resolution times the class count ever exists in memory.

`seg_reference` is the definition in plain torch ops: the CPU path of both classes, and what the device tests compare against (fp64 the reference, fp32 the yardstick).
"""
import torch

from . import _lib as L

IGNORE = 255


def _axis(n_in, n_out, dtype, device):
    """Source index pair and weight of every destination index: s = dst (in - 1) / (out - 1) (0 when out == 1), i0 = floor(s) held to in - 2, f = s - i0."""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    s = torch.arange(n_out, dtype=dtype, device=device) * torch.tensor(scale, dtype=dtype, device=device)
    i0 = s.floor().clamp(max=max(n_in - 2, 0)).long()
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)


def upsample_reference(x, size):
    """bilinear(x -> size), align_corners=True, horizontally first and then vertically (torch's association); the identity when the sizes are equal."""
    h, w = x.shape[-2:]
    H, W = size
    if (H, W) == (h, w):
        return x
    x0, x1, fx = _axis(w, W, x.dtype, x.device)
    y0, y1, fy = _axis(h, H, x.dtype, x.device)
    xw = (1 - fx) * x[..., x0] + fx * x[..., x1]
    fy = fy[:, None]
    return (1 - fy) * xw[..., y0, :] + fy * xw[..., y1, :]


def _check(x, t, n_classes=None):
    if x.dim() != 4 or t.dim() != 3 or t.size(0) != x.size(0):
        raise ValueError(f"segmentation: expected (N, C, h, w) logits and (N, H, W) targets, got {tuple(x.shape)} and {tuple(t.shape)}")
    if t.dtype not in (torch.int64, torch.uint8):
        raise ValueError(f"segmentation: targets are int64 or uint8 class indices, got {t.dtype}")
    c = x.size(1)
    if not 2 <= c <= 255:
        raise ValueError(f"segmentation: 2 <= classes <= 255 (255 is the ignore label), got {c}")
    if n_classes is not None and c != n_classes:
        raise ValueError(f"segmentation: logits have {c} classes, expected {n_classes}")
    if t.size(1) < x.size(2) or t.size(2) < x.size(3):
        raise ValueError(f"segmentation: the target {tuple(t.shape[1:])} is smaller than the logits {tuple(x.shape[2:])}")


def _loss_torch(x, t, wt):
    """(differentiable loss, upsampled logits, valid mask, clamped target)."""
    c = x.size(1)
    u = upsample_reference(x, t.shape[1:])
    tl = t.long()
    valid = tl < c                                   # 255 (ignore) and every other out-of-range label
    tc = torch.where(valid, tl, torch.zeros_like(tl))
    w = torch.ones(c, dtype=x.dtype, device=x.device) if wt is None else wt.to(x.dtype)
    wv = w[tc] * valid.to(x.dtype)
    nll = torch.logsumexp(u, 1) - u.gather(1, tc[:, None]).squeeze(1)
    return (wv * nll).sum() / wv.sum(), u, valid, tc


def _counts_torch(u, valid, tc, tl):
    c = u.size(1)
    pred = u.argmax(1)                               # the first of equal maxima
    p, m = pred[valid], tc[valid]
    return (torch.bincount(m[p == m], minlength=c), torch.bincount(p, minlength=c), torch.bincount(m, minlength=c),
            int((~valid & (tl != IGNORE)).sum()))


def seg_reference(x, t, wt=None, size=None):
    """The definition of frost_seg_forward in the dtype of `x`: (loss, dx, area_inter, area_pred, area_mask).  `size` defaults to the target's."""
    _check(x, t)
    if size is not None and tuple(size) != tuple(t.shape[1:]):
        raise ValueError("seg_reference: size must be the target's size")
    xr = x.detach().clone().requires_grad_(True)
    loss, u, valid, tc = _loss_torch(xr, t, wt)
    dx = torch.autograd.grad(loss, xr)[0] if bool(valid.any()) and float(loss.detach()) == float(loss.detach()) else torch.zeros_like(xr)
    inter, pred, mask, _ = _counts_torch(u.detach(), valid, tc, t.long())
    return loss.detach(), dx, inter, pred, mask


class SegMeter:
    """Running per-class pixel counts and mean IoU.  The state is one int64 device tensor {area_inter [C], area_pred [C], area_mask [C], batches, bad_targets}
    that the criterion's launch (or `update`) adds to; `compute` is the only host read.

    Difference from the reference: it keeps `inter` and `union + 1e-6` per batch as fp32 histograms in fp32 running sums, which stop being exact past 2^24 pixels
    per class, and adds its 1e-6 once per batch in fp32.  Here the counts are exact 64-bit integers and mean IoU is
    mean_c inter_c / (union_c + 1e-6 * batches + 1e-10) * 100 evaluated in fp64."""

    def __init__(self, num_classes=21, device="cuda"):
        if not 2 <= num_classes <= 255:
            raise ValueError("SegMeter: 2 <= num_classes <= 255")
        self.num_classes = num_classes
        self.device = torch.device(device)
        self.state = torch.zeros(3 * num_classes + 2, dtype=torch.int64, device=self.device)
        self._ws = None

    def workspace(self):
        if self._ws is None:
            self._ws = torch.zeros(L.load_library().frost_seg_workspace_bytes(), dtype=torch.uint8, device=self.device)
        return self._ws

    def reset(self):
        self.state.zero_()                           # an asynchronous memset on the current stream

    def update(self, logits, target):
        """Counts only (no loss, no gradient): for use without a criterion."""
        if isinstance(logits, (tuple, list)):
            logits = logits[0]
        _check(logits, target, self.num_classes)
        if logits.is_cuda:
            _launch(logits.detach(), target, None, self, self.workspace(), False, False)
        else:
            self._update_reference(logits.detach(), target)

    def _update_reference(self, logits, target):
        c = self.num_classes
        tl = target.long()
        valid = tl < c
        tc = torch.where(valid, tl, torch.zeros_like(tl))
        inter, pred, mask, bad = _counts_torch(upsample_reference(logits.float(), target.shape[1:]), valid, tc, tl)
        self.state[:3 * c] += torch.cat([inter, pred, mask]).to(self.state.device)
        self.state[3 * c] += 1
        self.state[3 * c + 1] += bad

    def _host(self):
        s = self.state.cpu()
        if int(s[-1]) > 0:
            raise ValueError(f"SegMeter: {int(s[-1])} target pixels held a label >= {self.num_classes} other than {IGNORE}")
        return s

    def areas(self):
        """(area_inter, area_pred, area_mask) as int64 CPU vectors."""
        s, c = self._host(), self.num_classes
        return s[:c].clone(), s[c:2 * c].clone(), s[2 * c:3 * c].clone()

    def compute(self):
        s, c = self._host(), self.num_classes
        inter, pred, mask, batches = s[:c].double(), s[c:2 * c].double(), s[2 * c:3 * c].double(), float(s[3 * c])
        return float((inter / ((pred + mask - inter) + 1e-6 * batches + 1e-10)).mean() * 100.0)


def _launch(x, t, wt, meter, ws, want_loss, want_dx):
    """One frost_seg_forward call on the current stream -> (loss [1] or None, dx or None)."""
    if x.dtype != torch.float32:
        x = x.float()
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.contiguous()
    t = t.contiguous()
    if t.device != x.device:
        raise ValueError("segmentation: logits and targets live on different devices")
    n, c, h, w = x.shape
    loss = torch.empty(1, dtype=torch.float32, device=x.device) if want_loss else None
    dx = torch.empty_like(x) if want_dx else None
    if dx is not None and dx.stride() != x.stride():
        raise RuntimeError("segmentation: the gradient buffer does not share the layout of the logits")
    sn, sc, sh, sw = x.stride()
    L.call("frost_seg_forward", L.ptr(x), n, c, h, w, sn, sc, sh, sw, L.ptr(t), 8 if t.dtype == torch.int64 else 1, t.size(1), t.size(2),
           L.ptr(wt), L.ptr(loss), L.ptr(dx), L.ptr(meter.state) if meter is not None else None, L.ptr(ws), L.stream())
    return loss, dx


class _SegLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, crit, meter):
        loss, dx = _launch(logits.detach(), target, crit._weights(logits.device), meter, crit._workspace(logits.device), True, ctx.needs_input_grad[0])
        ctx.save_for_backward(dx)
        ctx.in_dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.in_dtype), None, None, None


class SegmentationLoss(torch.nn.Module):
    """The reference's `SegmentationLoss` for loss_type 'ce': `CrossEntropyLoss(ignore_index=255, weight=class_wts)` over (N, C, h, w) logits and (N, H, W)
    targets (int64 or uint8), H >= h, W >= w.  Logits smaller than the target are upsampled (bilinear, align_corners=True) inside the kernel: hand it the head's
    stride-8 output, not the interpolated one.  A tuple of two outputs gives the sum of the two losses.  Loss and gradient come from one launch (capturable, works
    under `torch.no_grad()`); with `meter=` the same launch adds the batch (of `inputs[0]` for a tuple) to that `SegMeter`.  CPU tensors take `seg_reference`'s ops."""

    def __init__(self, n_classes=21, loss_type="ce", device="cuda", ignore_idx=255, class_wts=None, meter=None):
        super().__init__()
        if loss_type != "ce":
            raise NotImplementedError(f"SegmentationLoss: loss_type {loss_type!r} is not implemented (only 'ce')")
        if ignore_idx != IGNORE:
            raise NotImplementedError("SegmentationLoss: the ignore label is 255")
        if not 2 <= n_classes <= 255:
            raise ValueError("SegmentationLoss: 2 <= n_classes <= 255")
        if class_wts is not None and tuple(class_wts.shape) != (n_classes,):
            raise ValueError("SegmentationLoss: class_wts must have n_classes entries")
        self.n_classes, self.loss_type, self.device, self.ignore_idx = n_classes, loss_type, device, ignore_idx
        self.class_wts = None if class_wts is None else class_wts.detach().float()
        self.meter = meter
        self._wt_dev, self._ws = {}, {}

    def _weights(self, device):
        if self.class_wts is None:
            return None
        if device not in self._wt_dev:
            self._wt_dev[device] = self.class_wts.to(device).contiguous()
        return self._wt_dev[device]

    def _workspace(self, device):
        if device not in self._ws:
            self._ws[device] = torch.zeros(L.load_library().frost_seg_workspace_bytes(), dtype=torch.uint8, device=device)
        return self._ws[device]

    def _one(self, x, target, meter):
        _check(x, target, self.n_classes)
        if x.is_cuda:
            return _SegLossFunction.apply(x, target, self, meter)
        if meter is not None:
            meter._update_reference(x.detach(), target)
        return _loss_torch(x, target, self.class_wts)[0]

    def forward(self, inputs, target):
        if isinstance(inputs, (tuple, list)):
            if len(inputs) != 2:
                raise ValueError("SegmentationLoss: a tuple of outputs has two entries")
            return self._one(inputs[0], target, self.meter) + self._one(inputs[1], target, None)
        return self._one(inputs, target, self.meter)

"""FrostNet + Lite R-ASPP segmentation network in float mode.

The reference's segmentation networks (Semantic_Segmentation/model/mobilenetv3.py) put a Lite R-ASPP head (model/layers/LRASPP.py) on a MobileNet backbone; it has
no FrostNet segmentation model and its FrostNet ignores `dilated`.  This is the project's own composition: the FrostNet trunk that already trains in float mode, taps
at x2 (stride 8) and x5 (stride 32), and the reference's head with its mathematics unchanged:

    feat1 = b0(c4)                                               ConvBNReLU(in_channels, 128, 1)
    feat2 = bilinear(b1(c4) -> c4's size, align_corners=True)    AvgPool2d -> ConvBN(in_channels, 128, 1) -> hard sigmoid
    out   = project(bilinear(feat1 * feat2 -> c1's size, align_corners=True)) + auxlayer(c1)

`forward` returns the stride-8 logits: `seg.SegmentationLoss` / `SegMeter` upsample inside their kernel.  `upsample=True` returns the reference's full-size output
(seg.upsample_reference in torch ops), the one deviation of the surface.  On the CPU the stock modules run (the definition the device tests compare against); on the
GPU the float model runs on the float HIP kernels plus csrc/frost_seghead.hip (frostnet_amd.float_train.FloatSegRunner).  QAT of the segmentation model is not built."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .frostnet import _SETTINGS, CascadePreExBottleneck, ConvBN, ConvBNReLU, _FrostBase, _make_divisible
from .seg import upsample_reference

HEAD_CHANNELS = 256 // 2
# AvgPool2d (kernel, stride) of b1: the reference's own at stride 16; at stride 32 the map is half as large each way (513^2: 17^2 -> 2 x 2, as the reference's 33^2 -> 2 x 2)
POOL_DEFAULTS = {("pascal", 16): (25, 8), ("city", 16): (37, 12), ("pascal", 32): (13, 4), ("city", 32): (19, 6)}


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class Hsigmoid(nn.Module):
    """The reference's `_Hsigmoid` in float mode: relu6(v + 3) * (1 / 6)."""

    def forward(self, x):
        return F.relu6(x + 3.0) * (1 / 6)


class _LRASPP(nn.Module):
    def __init__(self, in_channels, pool_kernel, pool_stride):
        super().__init__()
        self.b0 = ConvBNReLU(in_channels, HEAD_CHANNELS, 1)
        self.b1 = nn.Sequential(nn.AvgPool2d(pool_kernel, pool_stride), ConvBN(in_channels, HEAD_CHANNELS, 1), Hsigmoid())


def check_pool_fits(h, w, kernel):
    if h < kernel[0] or w < kernel[1]:
        raise ValueError(f"LRASPPHead: the c4 map {h} x {w} is smaller than the pool window {kernel[0]} x {kernel[1]}")


class LRASPPHead(nn.Module):
    """Lite R-ASPP head: `_LRASPP` + `_Head` of model/layers/LRASPP.py and `project` / `auxlayer` / the add of MobileNetV3Seg.forward.  forward(c1, c4) -> logits at
    c1's resolution.  Parameters in registration order: lr_aspp.b0, lr_aspp.b1[1], project, auxlayer."""

    def __init__(self, nclass, in_channels, inter_channels, dataset="pascal", pool_kernel=None, pool_stride=None, c4_stride=32):
        super().__init__()
        if not 2 <= nclass <= 255:
            raise ValueError(f"LRASPPHead: 2 <= nclass <= 255 (the criterion's range), got {nclass}")
        key = ("city" if dataset == "city" else "pascal", int(c4_stride))
        if (pool_kernel is None or pool_stride is None) and key not in POOL_DEFAULTS:
            raise ValueError(f"LRASPPHead: no default pool window for c4_stride = {c4_stride}: pass pool_kernel and pool_stride")
        self.pool_kernel = _pair(pool_kernel if pool_kernel is not None else POOL_DEFAULTS[key][0])
        self.pool_stride = _pair(pool_stride if pool_stride is not None else POOL_DEFAULTS[key][1])
        self.nclass, self.in_channels, self.inter_channels = int(nclass), int(in_channels), int(inter_channels)
        self.lr_aspp = _LRASPP(in_channels, self.pool_kernel, self.pool_stride)
        self.project = nn.Conv2d(HEAD_CHANNELS, nclass, 1, 1)
        self.auxlayer = nn.Conv2d(inter_channels, nclass, 1, 1)

    def forward(self, c1, c4):
        check_pool_fits(c4.shape[2], c4.shape[3], self.pool_kernel)
        feat1 = self.lr_aspp.b0(c4)
        feat2 = F.interpolate(self.lr_aspp.b1(c4), c4.shape[2:], mode="bilinear", align_corners=True)
        z = F.interpolate(feat1 * feat2, c1.shape[2:], mode="bilinear", align_corners=True)
        return self.project(z) + self.auxlayer(c1)


class FrostNetSeg(_FrostBase):
    """FrostNet trunk (held flat: conv1, layer1 .. layer5, like SSDLiteFrostNet) + LRASPPHead on x2 (stride 8) and x5 (stride 32).  forward(x) -> stride-8 logits
    [N, nclass, ceil(h / 8), ceil(w / 8)], or with `upsample=True` the logits interpolated to x's size.  `float_precision` ('bf16' default | 'fp32') selects the
    activation storage of the device path, as on the classifier and the detector."""

    def __init__(self, nclass=21, mode="large", width_mult=1.0, dataset="pascal", upsample=False, bottleneck=CascadePreExBottleneck, **head_kw):
        super().__init__()
        self.quantized = False
        self.nclass, self.mode, self.upsample = int(nclass), mode, bool(upsample)
        self.in_channels = _make_divisible(int(32 * min(1.0, width_mult)))
        self.conv1 = ConvBNReLU(3, self.in_channels, 3, 2, 1)
        chans = []
        for i, st in enumerate(_SETTINGS[mode]):
            setattr(self, f"layer{i + 1}", self._make_layer(bottleneck, st, width_mult, 1))
            chans.append(self.in_channels)
        self.head = LRASPPHead(nclass, chans[4], chans[1], dataset=dataset, **head_kw)
        self._init_weights()

    def _is_fused(self):
        return not isinstance(self.conv1.conv[1], nn.BatchNorm2d)

    def forward(self, x):
        if x.is_cuda:
            out = self.hip_runner().forward(x)
        else:
            c1 = self.layer2(self.layer1(self.conv1(x)))
            out = self.head(c1, self.layer5(self.layer4(self.layer3(c1))))
        return upsample_reference(out, tuple(x.shape[2:])) if self.upsample else out

    def hip_runner(self):
        """FloatSegRunner bound to this tree; rebuilt when the float precision or the parameters change."""
        if self._is_qat_prepared() or self._is_ptq_prepared() or self._is_fused():
            raise NotImplementedError("FrostNetSeg: segmentation QAT is not built yet -- the device path runs the float (un-fused, not prepared) model only")
        r = self.__dict__.get("_hip_runner")
        want = getattr(self, "float_precision", None)
        if r is not None and want is not None and r.precision != want:
            r = None
        if r is None or r.model is not self or not r.still_valid():
            from .float_train import FloatSegRunner
            r = FloatSegRunner(self)
            r.is_qat = False
            self.__dict__["_hip_runner"] = r
        return r


def _factory(mode, width):
    def make(nclass=21, **kw):
        return FrostNetSeg(nclass=nclass, mode=mode, width_mult=width, **kw)
    return make


frostnet_seg_large_1_0 = _factory("large", 1.0)
frostnet_seg_base_1_0 = _factory("base", 1.0)
frostnet_seg_small_1_0 = _factory("small", 1.0)
for _f, _n in ((frostnet_seg_large_1_0, "large"), (frostnet_seg_base_1_0, "base"), (frostnet_seg_small_1_0, "small")):
    _f.__name__ = _f.__qualname__ = f"frostnet_seg_{_n}_1_0"
    _f.__doc__ = f"FrostNetSeg(mode='{_n}', width_mult=1.0)"

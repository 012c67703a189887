"""SSDLite detector on the FrostNet feature backbone -- BASELINE.json config c5 ("SSDLite-FrostNet backbone 512x512 QAT detection").

The reference never wired FrostNet into its detector (Object_Detection/ssd_qmv2.py hard-codes MobileNetV2 @300), so this is the
composition SURVEY N3 asks for, following the reference's conventions:
  * one QuantStub at the image, one DeQuantStub per prediction map (ssd_qmv2.py:205-216,249-252);
  * sources = backbone stages at strides 8 / 16 / 32 (x2, x3, x5 of frostnet_features.py:342-352) + extra stages at 64 / 128 / 256;
  * SSDLite form (MobileNetV2 paper, sec. 6.3): every regular conv of the SSD extras / prediction layers becomes depthwise 3x3 + pointwise 1x1 --
    exactly the two conv kinds the Frost bottleneck is made of, so the whole detector runs on the fake-quantised HIP engine
    (ConvBNReLU / ConvBN of frostnet.py:14-60, BN in every layer like the reference's `ConvBN` head layers, ssd_qmv2.py:56-77);
  * both phases of the reference's detection recipe run on the device: the float model (the StatAssist warm-up, Object_Detection/qtrainval.py:187-238,
    or a whole `--quant False` run) trains on the float kernels (frostnet_amd.float_train.FloatSSDRunner), then fuse_model() + prepare_qat
    (harness.statassist_qat_switch) hands the same parameters to the fake-quant engine (frostnet_amd.runner.SSDRunner); on the CPU the stock modules run;
  * PriorBox (layers/functions/prior_box.py:28-55) and MultiBoxLoss (layers/modules/multibox_loss.py:48-117, layers/box_utils.py:71-139)
    restated in vectorised, device-agnostic torch (they are the caller's loss, not conv math) and pinned to the reference by goldens.
Class-score maps are padded to a multiple of 8 channels (the HIP backward's channel granularity); the padding is sliced off before the loss.
The test phase -- softmax, box decoding, per-class top-k and NMS (layers/functions/detection.py:14-66) -- is `Detect` / `SSDLiteFrostNet.detect`, two HIP
kernels on the device (csrc/frost_detect.hip)."""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .frostnet import _SETTINGS, CascadePreExBottleneck, ConvBN, ConvBNReLU, _FrostBase, _make_divisible

# 512x512 analogue of the reference's SSD300 VOC table (data/config.py:18-34): same aspect ratios / variances, sizes scaled by 512/300
SSD512_VOC = dict(num_classes=21, min_dim=512, feature_maps=[64, 32, 16, 8, 4, 2], steps=[8, 16, 32, 64, 128, 256],
                  min_sizes=[51, 102, 189, 276, 363, 450], max_sizes=[102, 189, 276, 363, 450, 537],
                  aspect_ratios=[[2], [2, 3], [2, 3], [2, 3], [2], [2]], variance=[0.1, 0.2], clip=True, name="VOC")


def ssd_cfg_for(res):
    """SSD512_VOC rescaled to a square input of `res` pixels (tests / rehearsals at a smaller resolution): the feature maps follow the network's
    stride-8 ... stride-256 sources (ceil division: every stride-2 conv has padding 1), the box sizes keep their fraction of the image."""
    if res == 512:
        return dict(SSD512_VOC)
    cfg = dict(SSD512_VOC, min_dim=res, feature_maps=[-(-res // s) for s in SSD512_VOC["steps"]])
    cfg["min_sizes"] = [v * res / 512.0 for v in SSD512_VOC["min_sizes"]]
    cfg["max_sizes"] = [v * res / 512.0 for v in SSD512_VOC["max_sizes"]]
    return cfg


def prior_boxes(cfg):
    """PriorBox.get_prior (layers/functions/prior_box.py:28-55): [sum_k f_k^2 * (2 + 2*len(ar_k)), 4] boxes (cx, cy, w, h) in [0, 1]."""
    size = cfg["min_dim"]
    out = []
    for k, f in enumerate(cfg["feature_maps"]):
        f_k = size / cfg["steps"][k]
        s_k = cfg["min_sizes"][k] / size
        s_kp = math.sqrt(s_k * (cfg["max_sizes"][k] / size))
        wh = [(s_k, s_k), (s_kp, s_kp)]
        for ar in cfg["aspect_ratios"][k]:
            r = math.sqrt(ar)
            wh += [(s_k * r, s_k / r), (s_k / r, s_k * r)]
        c = (torch.arange(f, dtype=torch.float64) + 0.5) / f_k
        cy, cx = torch.meshgrid(c, c, indexing="ij")                        # row-major: i (y) outer, j (x) inner, like product(range(f), repeat=2)
        whs = torch.tensor(wh, dtype=torch.float64)
        box = torch.cat([cx.reshape(-1, 1, 1).expand(-1, len(wh), 1), cy.reshape(-1, 1, 1).expand(-1, len(wh), 1),
                         whs.unsqueeze(0).expand(f * f, -1, -1)], 2)
        out.append(box.reshape(-1, 4))
    out = torch.cat(out).to(torch.float32)
    return out.clamp_(0, 1) if cfg["clip"] else out


def pad_targets(targets, device):
    """Ragged ground truth (list of [n_i, 5] rows x1, y1, x2, y2, label) -> (boxes [N, K, 5], valid [N, K]) with K = max n_i.  The row counts are
    host knowledge (tensor shapes), so this is one concatenation and one gather on the device -- no per-image work, no synchronisation."""
    lens = [int(t.size(0)) for t in targets]
    k = max(1, max(lens))
    flat = torch.cat([t.reshape(-1, 5).to(device) for t in targets] + [torch.zeros(1, 5, device=device)])     # last row = the padding row
    idx = torch.full((len(lens), k), flat.size(0) - 1, dtype=torch.long)
    off = 0
    for i, n in enumerate(lens):
        idx[i, :n] = torch.arange(off, off + n)
        off += n
    valid = torch.tensor([[j < n for j in range(k)] for n in lens], dtype=torch.bool)
    return flat[idx.to(device)], valid.to(device)


def match_priors(threshold, truths, valid, priors, variances, labels):
    """layers/box_utils.py:71-139 `match` + `encode`, for the whole batch at once: every ground-truth box keeps its best prior, every prior takes
    its best ground truth; overlap < threshold -> background (label 0).  truths [N,K,4], valid [N,K], labels [N,K] -> (loc_t [N,P,4], conf_t [N,P]).
    Padding rows overlap nothing (-1) and write to a spare column P."""
    n, k, P = truths.size(0), truths.size(1), priors.size(0)
    pp = torch.cat([priors[:, :2] - priors[:, 2:] / 2, priors[:, :2] + priors[:, 2:] / 2], 1)                 # point_form
    lt = torch.max(truths[:, :, None, :2], pp[None, None, :, :2])
    rb = torch.min(truths[:, :, None, 2:], pp[None, None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(3)
    area_t = ((truths[..., 2] - truths[..., 0]) * (truths[..., 3] - truths[..., 1]))[:, :, None]
    area_p = ((pp[:, 2] - pp[:, 0]) * (pp[:, 3] - pp[:, 1]))[None, None, :]
    ov = torch.where(valid[:, :, None], inter / (area_t + area_p - inter), inter.new_full((), -1.0))          # jaccard [N,K,P]
    best_prior_idx = torch.where(valid, ov.argmax(2), torch.full_like(ov[:, :, 0], P, dtype=torch.long))      # [N,K]
    bto, bti = ov.max(1)                                                                                      # [N,P]
    bto = torch.cat([bto, bto.new_zeros(n, 1)], 1).scatter_(1, best_prior_idx, 2.0)
    bti = torch.cat([bti, bti.new_zeros(n, 1)], 1)
    for j in range(k):                                      # (sequential on purpose: a later ground truth wins a shared prior, as in the reference)
        bti.scatter_(1, best_prior_idx[:, j:j + 1], j)
    bto, bti = bto[:, :P], bti[:, :P]
    matched = truths.gather(1, bti[:, :, None].expand(-1, -1, 4))
    conf = torch.where(bto < threshold, torch.zeros_like(bti), labels.gather(1, bti).long() + 1)
    g_cxcy = ((matched[..., :2] + matched[..., 2:]) / 2 - priors[None, :, :2]) / (variances[0] * priors[None, :, 2:])
    g_wh = torch.log((matched[..., 2:] - matched[..., :2]) / priors[None, :, 2:]) / variances[1]
    return torch.cat([g_cxcy, g_wh], 2), conf


_MBOX_HIP = os.environ.get("FROST_MBOX_HIP", "1") != "0"          # dev switch: the loss as HIP kernels on the device (default) or as torch stages


class _MBoxFunction(torch.autograd.Function):
    """MultiBoxLoss forward + backward on the device (csrc/frost_mbox.hip): (loss_l, loss_c) = f(loc, conf); nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, loc, conf, priors, boxes, valid, threshold, negpos, variance):
        from ._lib import call, load_library, ptr, stream
        lib = load_library()
        n, p, c, k = loc.size(0), loc.size(1), conf.size(2), boxes.size(1)
        dev = loc.device
        loc_c, conf_c = loc.detach().contiguous().float(), conf.detach().contiguous().float()
        pri = priors.detach().contiguous().float()
        bx = boxes.detach().contiguous().float()
        vd = valid.detach().contiguous().to(torch.uint8) if valid.dtype != torch.bool else valid.detach().contiguous()
        bto = torch.empty(n, p, dtype=torch.float32, device=dev)
        bti = torch.empty(n, p, dtype=torch.int32, device=dev)
        loc_t = torch.empty(n, p, 4, dtype=torch.float32, device=dev)
        conf_t = torch.empty(n, p, dtype=torch.int32, device=dev)
        lc = torch.empty(n, p, dtype=torch.float32, device=dev)
        sel = torch.empty(n, p, dtype=torch.uint8, device=dev)
        num_pos = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.zeros(lib.frost_mbox_workspace_floats(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("frost_mbox_forward", ptr(loc_c), ptr(conf_c), ptr(pri), ptr(bx), ptr(vd), n, p, c, k, float(threshold), int(negpos), float(variance[0]), float(variance[1]),
                 ptr(bto), ptr(bti), ptr(loc_t), ptr(conf_t), ptr(lc), ptr(sel), ptr(num_pos), ptr(out), stream())
        ctx.save_for_backward(loc_c, conf_c, loc_t, conf_t, sel, out)
        ctx.conf_t, ctx.num_pos = conf_t, num_pos          # (tests read the matching)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l, g_c):
        from ._lib import call, ptr, stream
        loc, conf, loc_t, conf_t, sel, out = ctx.saved_tensors
        n, p, c = conf.shape
        dloc, dconf = torch.empty_like(loc), torch.empty_like(conf)
        gl = g_l.contiguous().float() if g_l is not None else None
        gc = g_c.contiguous().float() if g_c is not None else None
        with torch.cuda.device(loc.device):
            call("frost_mbox_backward", ptr(loc), ptr(conf), ptr(loc_t), ptr(conf_t), ptr(sel), ptr(out), ptr(gl), ptr(gc), n, p, c, ptr(dloc), ptr(dconf), stream())
        return dloc, dconf, None, None, None, None, None, None


class MultiBoxLoss(nn.Module):
    """SSD loss (layers/modules/multibox_loss.py:48-117): smooth-L1 on the matched priors + cross-entropy on positives and the hardest
    negatives (3:1), both divided by the number of positives.  forward((loc [N,P,4], conf [N,P,C], priors [P,4]), targets) with targets the
    reference's list of [n_i,5], or pad_targets(...) of it made ahead of time.  Fixed shapes and no host synchronisation throughout (masked sums
    instead of boolean gathers), so the loss records into a HIP graph with the rest of the step."""

    def __init__(self, num_classes, overlap_thresh=0.5, neg_pos=3, variance=(0.1, 0.2)):
        super().__init__()
        self.num_classes, self.threshold, self.negpos_ratio, self.variance = num_classes, overlap_thresh, neg_pos, variance

    def forward(self, predictions, targets):
        loc_data, conf_data, priors = predictions
        num, num_priors = loc_data.size(0), loc_data.size(1)
        priors = priors[:num_priors].to(loc_data.device)
        boxes, valid = targets if isinstance(targets, tuple) else pad_targets(targets, loc_data.device)
        if loc_data.is_cuda and _MBOX_HIP:
            # the device path: matching, per-prior loss, hard negative mining and both gradients as four HIP kernels (csrc/frost_mbox.hip); the torch stages below
            # are the CPU definition (and the yardstick of tests/test_gpu_detect.py)
            return _MBoxFunction.apply(loc_data, conf_data, priors, boxes, valid, self.threshold, self.negpos_ratio, self.variance)
        return self.forward_torch(loc_data, conf_data, priors, boxes, valid)

    def forward_torch(self, loc_data, conf_data, priors, boxes, valid):
        """The loss as batched torch stages (the restatement of multibox_loss.py:48-117 pinned to the reference's goldens, tests/test_oracle_golden.py G11)."""
        with torch.no_grad():
            loc_t, conf_t = match_priors(self.threshold, boxes[..., :4], valid, priors, self.variance, boxes[..., 4])
            pos = conf_t > 0
            num_pos = pos.long().sum(1, keepdim=True)
        zero = loc_data.new_zeros(())
        loss_l = torch.where(pos[:, :, None], F.smooth_l1_loss(loc_data, loc_t, reduction="none"), zero).sum()
        # per-prior classification loss: log-sum-exp minus the target's score (== cross-entropy; the reference's max-shifted log_sum_exp)
        lc = torch.logsumexp(conf_data, 2) - conf_data.gather(2, conf_t[:, :, None]).squeeze(2)
        with torch.no_grad():                                   # hard negative mining: rank the non-positive priors by their loss
            _, loss_idx = lc.detach().masked_fill(pos, 0).sort(1, descending=True)
            _, idx_rank = loss_idx.sort(1)
            num_neg = torch.clamp(self.negpos_ratio * num_pos, max=pos.size(1) - 1)
            sel = pos | (idx_rank < num_neg)
        loss_c = torch.where(sel, lc, zero).sum()
        n = num_pos.sum().to(loss_l.dtype)
        return loss_l / n, loss_c / n


_DETECT_HIP = os.environ.get("FROST_DETECT_HIP", "1") != "0"      # dev switch: the Detect layer as HIP kernels on the device (default) or as torch stages


class Detect(nn.Module):
    """The SSD test-phase output layer: nn.Softmax + Detect of the reference (Object_Detection/ssd_qmv2.py:290-292,320-327,
    layers/functions/detection.py:14-66, decode: layers/box_utils.py:140-158).  forward(loc [N,P,4], conf [N,P,C] LOGITS, priors [P,4] (cx, cy, w, h)) ->
    out [N, num_classes, top_k, 5] fp32.  For every image n and class c != bkg_label:
      1. s_p = softmax(conf[n, p, :])[c];
      2. box_p = decode(loc[n, p], prior_p) in the reference's operation order (cxcy = p.cxcy + l[:2] * v0 * p.wh, wh = p.wh * exp(l[2:] * v1),
         x1y1 = cxcy - wh / 2, x2y2 = wh + x1y1);
      3. candidates are the priors with s_p > conf_thresh (a NaN score is never a candidate);
      4. they are ordered by score descending, EQUAL SCORES BY THE LOWER PRIOR INDEX FIRST (the reference's torch.sort leaves ties unspecified; quantised
         models tie in quantity, so the order is defined here), and the first top_k stay;
      5. greedy NMS in that order on box * min_dim: a candidate is kept iff its IoU with every earlier kept box is <= nms_thresh,
         IoU = inter / (area_a + area_b - inter) with the intersection's width and height clamped at 0 (torchvision.ops.nms's rule; the reference's own
         box_utils.nms applies the same criterion with a differently rounded union);
      6. out[n, c, r] = (score, x1, y1, x2, y2) of the r-th kept candidate with the UNSCALED box; every other row, and the plane out[:, bkg_label], is zero.
    detection.py:68-71 (a rank filter across classes) writes into a temporary and has no effect in the reference; it is not reproduced.
    After a forward, `last_counts` [N, num_classes] int32 holds the number of kept rows.  No parameters, no buffers, no state_dict keys.  On the device the
    layer is two HIP kernels (csrc/frost_detect.hip): fixed launch shapes and no host synchronisation, so it records into a HIP graph; forward_torch is the
    CPU definition and the yardstick of tests/test_gpu_detect_post.py."""

    def __init__(self, num_classes, bkg_label=0, top_k=200, conf_thresh=0.01, nms_thresh=0.45, variance=(0.1, 0.2), min_dim=512):
        super().__init__()
        if nms_thresh <= 0:
            raise ValueError("nms_threshold must be non negative.")
        if top_k < 1:
            raise ValueError("top_k must be at least 1")
        self.num_classes, self.bkg_label, self.top_k = int(num_classes), int(bkg_label), int(top_k)
        self.conf_thresh, self.nms_thresh, self.variance, self.min_dim = float(conf_thresh), float(nms_thresh), tuple(variance), float(min_dim)
        self.last_counts = None

    def forward(self, loc, conf, priors):
        priors = priors[:loc.size(1)].to(loc.device)
        if loc.is_cuda and _DETECT_HIP:
            return self.forward_hip(loc, conf, priors)
        return self.forward_torch(loc, conf, priors)

    def _check(self, loc, conf, priors):
        n, p = loc.size(0), loc.size(1)
        if loc.dim() != 3 or loc.size(2) != 4 or tuple(conf.shape) != (n, p, self.num_classes) or tuple(priors.shape) != (p, 4):
            raise ValueError(f"Detect: loc {tuple(loc.shape)} / conf {tuple(conf.shape)} / priors {tuple(priors.shape)} are not [N,P,4] / [N,P,{self.num_classes}] / [P,4]")

    @torch.no_grad()
    def forward_hip(self, loc, conf, priors):
        from ._lib import call, load_library, ptr, stream
        self._check(loc, conf, priors)
        cap = load_library().frost_detect_max_top_k()
        if self.top_k > cap:
            raise ValueError(f"Detect: top_k = {self.top_k} exceeds the HIP kernel's cap of {cap} (one thread per candidate of an (image, class) pair)")
        n, p, c, dev = loc.size(0), loc.size(1), self.num_classes, loc.device
        loc_c, conf_c, pri = loc.detach().contiguous().float(), conf.detach().contiguous().float(), priors.detach().contiguous().float()
        scores = torch.empty(n, c, p, dtype=torch.float32, device=dev)          # class-major scores and decoded boxes: work buffers of the two kernels
        boxes = torch.empty(n, p, 4, dtype=torch.float32, device=dev)
        out = torch.empty(n, c, self.top_k, 5, dtype=torch.float32, device=dev)  # (every element is written by the kernel: no clearing pass)
        counts = torch.empty(n, c, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            call("frost_detect_forward", ptr(loc_c), ptr(conf_c), ptr(pri), n, p, c, self.bkg_label, self.top_k, self.conf_thresh, self.nms_thresh,
                 float(self.variance[0]), float(self.variance[1]), self.min_dim, ptr(scores), ptr(boxes), ptr(out), ptr(counts), stream())
        self.last_counts = counts
        return out

    @torch.no_grad()
    def forward_torch(self, loc, conf, priors):
        """The layer as batched torch stages on any device: one stable sort per (image, class) row, a [K, K] IoU table, K masked steps of the greedy scan,
        one scatter -- fixed shapes, no boolean-mask gather."""
        self._check(loc, conf, priors)
        loc, conf, priors = loc.float(), conf.float(), priors.float()
        n, p, c = loc.size(0), loc.size(1), self.num_classes
        k = min(self.top_k, p)
        v0, v1 = self.variance
        cxcy = priors[None, :, :2] + loc[..., :2] * v0 * priors[None, :, 2:]
        wh = priors[None, :, 2:] * torch.exp(loc[..., 2:] * v1)
        x1y1 = cxcy - wh / 2
        boxes = torch.cat([x1y1, wh + x1y1], 2)                                                   # [N,P,4]
        scores = torch.softmax(conf, 2).transpose(1, 2)                                           # [N,C,P]
        cand = scores > self.conf_thresh                                                          # (NaN > t is False)
        cand[:, self.bkg_label] = False
        key = torch.where(cand, scores, scores.new_full((), -math.inf))
        val, idx = torch.sort(key, dim=2, descending=True, stable=True)                           # stable: equal scores keep the lower prior index first
        val, idx = val[..., :k], idx[..., :k]
        valid = cand.gather(2, idx)                                                               # [N,C,K] (candidates sort in front of the -inf fill)
        bx = boxes[:, None].expand(n, c, p, 4).gather(2, idx[..., None].expand(n, c, k, 4))        # [N,C,K,4]
        sb = bx * self.min_dim
        area = (sb[..., 2] - sb[..., 0]) * (sb[..., 3] - sb[..., 1])
        lt = torch.max(sb[:, :, :, None, :2], sb[:, :, None, :, :2])
        rb = torch.min(sb[:, :, :, None, 2:], sb[:, :, None, :, 2:])
        whi = (rb - lt).clamp(min=0)
        inter = whi[..., 0] * whi[..., 1]
        over = ~(inter / (area[..., :, None] + area[..., None, :] - inter) <= self.nms_thresh)    # [N,C,K,K]: row i suppresses column j
        del lt, rb, whi, inter
        gone = ~valid
        keep = torch.zeros_like(valid)
        for i in range(k):                                                                        # greedy scan: K dependent, batched steps
            ki = ~gone[..., i]
            keep[..., i] = ki
            gone = gone | (ki[..., None] & over[..., i, :])
        keep &= valid
        counts = keep.sum(2)
        slot = torch.where(keep, keep.long().cumsum(2) - 1, torch.full_like(idx, self.top_k))     # dropped rows go to a spare slot
        rows = torch.cat([val[..., None], bx], 3)
        out = loc.new_zeros(n, c, self.top_k + 1, 5).scatter_(2, slot[..., None].expand(n, c, k, 5), rows)[:, :, :self.top_k].contiguous()
        self.last_counts = counts.to(torch.int32)
        return out


class ExtraBlock(nn.Module):
    """SSDLite extra stage: 1x1 (-> c/2) -> depthwise 3x3 stride 2 -> 1x1 (-> c), ReLU after each (the reference applies F.relu after every
    extra layer, ssd_qmv2.py:240-243)."""

    def __init__(self, cin, cout):
        super().__init__()
        mid = cout // 2
        self.pw1 = ConvBNReLU(cin, mid, 1)
        self.dw = ConvBNReLU(mid, mid, 3, 2, 1, 1, groups=mid)
        self.pw2 = ConvBNReLU(mid, cout, 1)

    def forward(self, x):
        return self.pw2(self.dw(self.pw1(x)))


class SepHead(nn.Module):
    """SSDLite prediction layer: depthwise 3x3 + BN + ReLU, then 1x1 + BN (linear), like the reference's ConvBN head layers but separable."""

    def __init__(self, cin, cout):
        super().__init__()
        self.dw = ConvBNReLU(cin, cin, 3, 1, 1, 1, groups=cin)
        self.pw = ConvBN(cin, cout, 1)

    def forward(self, x):
        return self.pw(self.dw(x))


class SSDLiteFrostNet(_FrostBase):
    ANCHORS = [4, 6, 6, 6, 4, 4]
    EXTRAS = [512, 256, 256]

    def __init__(self, num_classes=21, mode="large", width_mult=1.0, cfg=None, bottleneck=CascadePreExBottleneck):
        super().__init__()
        self.quantized = True
        self.num_classes, self.cfg = num_classes, dict(cfg or SSD512_VOC)
        l1, l2, l3, l4, l5 = _SETTINGS[mode]
        self.in_channels = _make_divisible(int(32 * min(1.0, width_mult)))
        self.conv1 = ConvBNReLU(3, self.in_channels, 3, 2, 1)
        chans = []
        for i, st in enumerate((l1, l2, l3, l4, l5)):
            setattr(self, f"layer{i + 1}", self._make_layer(bottleneck, st, width_mult, 1))
            chans.append(self.in_channels)
        src = [chans[1], chans[2], chans[4]]
        self.extras = nn.ModuleList()
        cin = chans[4]
        for c in self.EXTRAS:
            self.extras.append(ExtraBlock(cin, c))
            src.append(c)
            cin = c
        self.source_channels = src
        self.conf_pad = [(a * num_classes + 7) // 8 * 8 for a in self.ANCHORS]
        self.loc = nn.ModuleList([SepHead(c, a * 4) for c, a in zip(src, self.ANCHORS)])
        self.conf = nn.ModuleList([SepHead(c, p) for c, p in zip(src, self.conf_pad)])
        self.quant = torch.quantization.QuantStub()
        self.dequant = torch.quantization.DeQuantStub()
        self._init_weights()
        self.register_buffer("priors", prior_boxes(self.cfg), persistent=False)

    def _assemble(self, maps):
        """12 dequantised NCHW maps [loc0, conf0, loc1, ...] -> (loc [N,P,4], conf [N,P,C], priors)."""
        n = maps[0].size(0)
        loc = torch.cat([m.permute(0, 2, 3, 1).reshape(n, -1) for m in maps[0::2]], 1).view(n, -1, 4)
        conf = torch.cat([m.permute(0, 2, 3, 1)[..., : a * self.num_classes].reshape(n, -1) for m, a in zip(maps[1::2], self.ANCHORS)], 1)
        return loc, conf.view(n, -1, self.num_classes), self.priors

    def forward(self, x):
        if x.is_cuda:
            r = self.hip_runner()
            if r.is_qat:
                return self._assemble(r.forward_maps(x))
            loc, conf = r.forward(x)            # the float model: (loc, conf) gathered on the device in _assemble's order
            return loc, conf, self.priors
        x = self.conv1(self.quant(x))
        sources = []
        for i in range(5):
            x = getattr(self, f"layer{i + 1}")(x)
            if i in (1, 2, 4):
                sources.append(x)
        for e in self.extras:
            x = e(x)
            sources.append(x)
        maps = []
        for s, l, c in zip(sources, self.loc, self.conf):
            maps += [self.dequant(l(s)), self.dequant(c(s))]
        return self._assemble(maps)

    def detect(self, x, top_k=200, conf_thresh=0.01, nms_thresh=0.45):
        """Detections of a batch of images: Detect(...)(*self(x)) -> [N, num_classes, top_k, 5] rows (score, x1, y1, x2, y2), the reference's test phase
        (ssd_qmv2.py:320-327).  Eval mode only; runs without autograd; float (bf16 / fp32), QAT-prepared and hip_convert()-ed models alike.  The Detect layer
        is built on first use and kept outside the module tree (it has no state; state_dict() is unchanged)."""
        if self.training:
            raise RuntimeError("SSDLiteFrostNet.detect() is the test phase: call model.eval() first")
        d = self._detect_layer(top_k, conf_thresh, nms_thresh)
        with torch.no_grad():
            loc, conf, priors = self(x)
            return d(loc, conf, priors)

    def _detect_layer(self, top_k, conf_thresh, nms_thresh):
        key = (int(top_k), float(conf_thresh), float(nms_thresh))
        d = self.__dict__.get("_detect")
        if d is None or d[0] != key:
            d = (key, Detect(self.num_classes, 0, top_k, conf_thresh, nms_thresh, tuple(self.cfg["variance"]), self.cfg["min_dim"]))
            self.__dict__["_detect"] = d
        return d[1]

    def _bf16_runner(self):
        if self._is_qat_prepared():
            raise RuntimeError("hip_infer_bf16 is the float model's inference path; a QAT-prepared model runs model(x)")
        inf = self.__dict__.get("_bf16_infer")
        if inf is None or inf.device != next(self.parameters()).device:
            from .infer import Bf16SSDInference
            inf = Bf16SSDInference(self)
            self.__dict__["_bf16_infer"] = inf
        return inf

    def hip_infer_bf16(self, x):
        """bf16 inference of the float (un-fused, not QAT-prepared) detector on the HIP inference kernels -> (loc [N,P,4], conf [N,P,C], priors): eval-mode
        BatchNorm folded once per state of the parameters, NHWC bf16 activations, fp32 accumulation, the trunk on the fused bottleneck kernels, both heads of
        a source in one launch that stores fp32 in _assemble's order.  See frostnet_amd.infer.Bf16SSDInference."""
        loc, conf = self._bf16_runner()(x)
        return loc, conf, self.priors

    def hip_detect_bf16(self, x, top_k=200, conf_thresh=0.01, nms_thresh=0.45):
        """detect() on the bf16 inference path: Detect(...)(*hip_infer_bf16(x)) -> [N, num_classes, top_k, 5] with the Detect object detect() caches
        (`last_counts` as there).  After one eager call (it measures the per-bottleneck kernel choice and folds the weights) the whole call records into a
        HIP graph on a static input: no host synchronisation, no host-to-device copy."""
        if self.training:
            raise RuntimeError("bf16 inference is the eval-mode graph: call model.eval() first")
        d = self._detect_layer(top_k, conf_thresh, nms_thresh)
        with torch.no_grad():
            return d(*self.hip_infer_bf16(x))

    def hip_infer_int8(self, x):
        """Inference of the hip_convert()-ed detector -> (loc [N,P,4], conf [N,P,C], priors), bit-equal to model(x): the heads of every source store their
        dequantised fp32 values straight in _assemble's order (frostnet_amd.runner.SSDRunner.infer_converted; FROST_CVT_HEAD selects fused heads / layer launches); model(x) itself keeps the twelve-map form."""
        if not self._is_qat_prepared() or not self.__dict__.get("_hip_converted", False):
            raise RuntimeError("hip_infer_int8 is the converted detector's inference path: call hip_convert() on the QAT-prepared model first")
        if self.training:
            raise RuntimeError("int8 inference is the eval-mode graph: call model.eval() first")
        with torch.no_grad():
            loc, conf = self.hip_runner().infer_converted(x)
        return loc, conf, self.priors

    def hip_detect_int8(self, x, top_k=200, conf_thresh=0.01, nms_thresh=0.45):
        """detect() on the converted detector's inference path: Detect(...)(*hip_infer_int8(x)) -> [N, num_classes, top_k, 5] with the Detect object detect() caches
        (`last_counts` as there); equal to model.detect(x) bit for bit.  After one eager call the whole call records into a HIP graph on a static input."""
        if not self._is_qat_prepared() or not self.__dict__.get("_hip_converted", False):
            raise RuntimeError("hip_detect_int8 is the converted detector's inference path: call hip_convert() on the QAT-prepared model first")
        if self.training:
            raise RuntimeError("int8 inference is the eval-mode graph: call model.eval() first")
        d = self._detect_layer(top_k, conf_thresh, nms_thresh)
        with torch.no_grad():
            return d(*self.hip_infer_int8(x))

    def hip_runner(self):
        """The device executor: SSDRunner (fake-quant) for the QAT-prepared model, FloatSSDRunner for the float model (StatAssist warm-up / float
        training, `float_precision` 'bf16' | 'fp32'); rebuilt when the mode, the float precision or the parameters change."""
        qat = self._is_qat_prepared()
        r = self.__dict__.get("_hip_runner")
        want = getattr(self, "float_precision", None)
        if r is not None and not qat and want is not None and getattr(r, "precision", want) != want:
            r = None
        if r is None or r.model is not self or r.is_qat != qat or not r.still_valid():
            if qat:
                from .runner import SSDRunner
                r = SSDRunner(self)
            else:
                from .float_train import FloatSSDRunner
                r = FloatSSDRunner(self)
            r.is_qat = qat
            self.__dict__["_hip_runner"] = r
        return r

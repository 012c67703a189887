"""PASCAL VOC mean-AP scoring of the detector's test-phase tensor: the third phase of the reference's detection recipe (Object_Detection/qeval_convert.py:177-396,
`test_net` / `voc_eval` / `voc_ap`, called from the training loop at qtrainval.py:314).  On device tensors the evaluator state lives in device memory and is
advanced by HIP kernels (csrc/frost_voceval.hip); on CPU tensors the same definition runs in numpy and is the yardstick of every GPU test."""
import numpy as np
import torch

FLAG_IGNORED, FLAG_TP, FLAG_FP = 0, 1, 2
ORD_BITS = 30
ORD_MASK = (1 << ORD_BITS) - 1
MAX_K = 1024          # VOC_MAXK of csrc/frost_voceval.hip: detection rows of one (image, class)
MAX_G = 1024          # VOC_MAXG: ground-truth rows of one image
EPS64 = 2.220446049250313e-16


def pad_difficult(flags, device):
    """Ragged difficult flags (one 1-D sequence per image) -> [N, G] bool with G = max(1, longest), the companion of ssdlite.pad_targets."""
    g = max(1, max(len(f) for f in flags))
    out = torch.zeros(len(flags), g, dtype=torch.bool)
    for i, f in enumerate(flags):
        if len(f):
            out[i, :len(f)] = torch.as_tensor(f, dtype=torch.bool)
    return out.to(device)


def pack_records(score, ordinal, flag):
    """score fp32 > 0, ordinal < 2^30, flag 0 / 1 / 2 -> uint64 records (see VOCEvaluator)."""
    bits = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).astype(np.uint64)
    inv = (~np.asarray(ordinal, dtype=np.uint64)) & np.uint64(ORD_MASK)
    return (bits << np.uint64(32)) | (inv << np.uint64(2)) | np.asarray(flag, dtype=np.uint64)


def ap_from_flags(flags, npos, use_07_metric):
    """AP of one class from the flags of its records in rank order: (ap, rec, prec), fp64 in the reference's operation order (qeval_convert.py:177-208,332-339)."""
    tp = np.cumsum((flags == FLAG_TP).astype(np.float64))
    fp = np.cumsum((flags == FLAG_FP).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, EPS64)
    if use_07_metric:
        ap = 0.0
        for i in range(11):
            t = i * 0.1
            sel = rec >= t
            p = float(np.max(prec[sel])) if sel.any() else 0.0
            ap = ap + p / 11.0
        return ap, rec, prec
    if npos == 0:
        return float("nan"), rec, prec          # rec is 0 / 0 everywhere: the reference's sum is NaN
    env = np.maximum.accumulate(prec[::-1])[::-1]
    ap, prev = 0.0, 0.0
    for r in np.nonzero(flags == FLAG_TP)[0]:
        ap += (rec[r] - prev) * env[r]
        prev = rec[r]
    return ap, rec, prec


class VOCEvaluator:
    """Per-class average precision and mean AP of detections against ground truth, by the PASCAL VOC rules as the reference evaluates them.

    One `update(detections, gt, difficult, valid, sizes=None)` feeds a batch:
      detections [N, C, K, 5] fp32 rows (score, x1, y1, x2, y2) as `Detect` writes them; gt [N, G, 5] fp32 rows (x1, y1, x2, y2, label); difficult [N, G] and
      valid [N, G] bool; sizes [N, 2] fp32 (w, h) or None for 1.  `label` is the training-target label, which numbers the non-background classes from 0: its
      class index is `label` when label < bkg_label and `label + 1` otherwise (label + 1 for bkg_label = 0).

    Per image n and class c != bkg_label:
      1. a detection is a row with score > 0 (qeval_convert.py:373);
      2. its box is b = (x1 w, y1 h, x2 w, y2 h) + det_offset in fp32; ground-truth boxes are taken as given, in the same pixel frame;
      3. against every valid ground-truth row of class c of that image, in fp32 and in this order: iw = max(min(g.x2, b.x2) - max(g.x1, b.x1), 0), ih alike,
         inter = iw ih, IoU = inter / ((b.x2 - b.x1)(b.y2 - b.y1) + (g.x2 - g.x1)(g.y2 - g.y1) - inter), no "+ 1" (:308-318); jmax = the first index of the
         largest IoU (a NaN IoU is never the largest);
      4. no ground truth of the class, or not IoU[jmax] > ovthresh -> FP; else jmax difficult -> ignored (neither TP nor FP, never marks the box taken); else the
         highest-ranked detection of this (image, class) pointing at jmax -> TP, every later one -> FP;
      5. npos[c] += the valid, non-difficult ground-truth rows of class c.
    Rank within a class over the whole evaluation: score descending, equal scores by the lower ordinal = image_ordinal * top_k + row first, image_ordinal counting
    images in the order they were fed.  The tie rule is this project's: the reference's np.argsort is unstable on ties.  The reference walks the ranked list once
    with per-image `det` flags; jmax does not depend on those flags, so that walk equals rule 4 applied per (image, class), which is what runs in parallel.

    Per class with at least one detection, in fp64 in the reference's operation order: tp / fp cumulative along the rank, rec = tp / npos,
    prec = tp / max(tp + fp, 2^-52); use_07_metric: ap = sum over i = 0..10 of max(prec[rec >= i * 0.1], or 0) / 11 accumulated in that order; otherwise the
    area under the precision envelope (:193-207): every TP at rank r adds (rec[r] - rec_prev) * max(prec[r:]).  npos = 0 gives 0.0 under the 07 metric and NaN
    under the area metric, which is what the reference's arithmetic yields.  A class without any detection scores -1, the reference's sentinel (:340-343).
    mean_ap is the plain mean over the non-background classes, sentinels (and NaN) included, as do_python_eval prints it (:162,174); ap[bkg_label] is NaN and is
    not part of the mean.

    Two deliberate deviations from the reference: (a) scores are not rounded to 3 decimals nor coordinates to 1 -- artefacts of the VOCdevkit text files the
    reference round-trips through; (b) det_offset defaults to 0: the reference adds 1 to every detection coordinate when it writes the file (:137) while its
    ground truth is xml - 1 (:92-95), so it scores detections shifted by one pixel; det_offset=1.0 reproduces that.

    State: per class a row of `capacity` (default max_images * top_k) 64-bit records  score bits << 32 | (~ordinal & 0x3FFFFFFF) << 2 | flag  (0 ignored, 1 TP,
    2 FP; scores are positive floats, so "larger record" is "earlier rank" and the flag travels with it; empty slots are 0), a cursor and npos per class, the
    number of images seen and an overflow word.  A full row, or more than max_images images, drops records, sets the overflow word and makes compute() raise.
    On the device update() is one C-ABI call without host synchronisation or data-dependent allocation (it records into a HIP graph; the image count advances on
    the device); compute() sorts the rows once (torch.sort), runs frost_voc_ap and returns device tensors.  Raising on overflow needs the overflow
    word on the host: that is compute()'s one host read of its own; compute(check_overflow=False) makes none and leaves the word to the caller, who reads
    overflowed() together with the results (harness.val_detector: one read per evaluation)."""

    def __init__(self, num_classes=21, bkg_label=0, ovthresh=0.5, use_07_metric=True, det_offset=0.0, max_images=4952, top_k=200, capacity=None, device=None):
        if num_classes < 2 or not 0 <= bkg_label < num_classes:
            raise ValueError("VOCEvaluator: num_classes >= 2 and 0 <= bkg_label < num_classes")
        if top_k < 1 or top_k > MAX_K:
            raise ValueError(f"VOCEvaluator: top_k outside 1 .. {MAX_K}")
        if max_images < 1 or max_images * top_k > 1 << ORD_BITS:
            raise ValueError("VOCEvaluator: max_images * top_k must not exceed 2^30 (the ordinal field of a record)")
        self.num_classes, self.bkg_label, self.ovthresh, self.use_07_metric = int(num_classes), int(bkg_label), float(ovthresh), bool(use_07_metric)
        self.det_offset, self.max_images, self.top_k = float(det_offset), int(max_images), int(top_k)
        self.capacity = int(capacity) if capacity is not None else self.max_images * self.top_k
        if not 1 <= self.capacity <= 1 << ORD_BITS:
            raise ValueError("VOCEvaluator: capacity outside 1 .. 2^30")
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.reset()

    # ---- state ---------------------------------------------------------------------------------------------------------------------------------------
    def reset(self):
        C = self.num_classes
        if self.device.type == "cpu":
            self._rows = [[] for _ in range(C)]
            self._cursor = np.zeros(C, dtype=np.int64)
            self._npos = np.zeros(C, dtype=np.int64)
            self._seen, self._overflow = 0, 0
        elif getattr(self, "_records", None) is None:
            self._records = torch.empty(C, self.capacity, dtype=torch.int64, device=self.device)
            self._ctr = torch.empty(2 * C + 2, dtype=torch.int32, device=self.device)          # cursor [C], npos [C], images seen, overflow
        if self.device.type != "cpu":
            from ._lib import call, ptr, stream
            call("frost_voc_reset", ptr(self._records), ptr(self._ctr), C, self.capacity, stream())

    def _check(self, detections, gt, difficult, valid, sizes):
        ts = [detections, gt, difficult, valid] + ([sizes] if sizes is not None else [])
        if any(not isinstance(t, torch.Tensor) for t in ts):
            raise ValueError("VOCEvaluator.update: tensors expected")
        if any(t.device != detections.device for t in ts):
            raise ValueError("VOCEvaluator.update: tensors on different devices")
        if detections.device.type != self.device.type or (self.device.index is not None and detections.device != self.device):
            raise ValueError(f"VOCEvaluator.update: tensors on {detections.device}, evaluator state on {self.device}")
        if detections.dim() != 4 or detections.size(1) != self.num_classes or detections.size(3) != 5 or detections.dtype != torch.float32:
            raise ValueError("VOCEvaluator.update: detections must be [N, num_classes, K, 5] float32")
        n, k = detections.size(0), detections.size(2)
        if k < 1 or k > self.top_k:
            raise ValueError(f"VOCEvaluator.update: K = {k} outside 1 .. top_k = {self.top_k}")
        if gt.dim() != 3 or gt.size(0) != n or gt.size(2) != 5 or gt.dtype != torch.float32:
            raise ValueError("VOCEvaluator.update: gt must be [N, G, 5] float32")
        g = gt.size(1)
        if g < 1 or g > MAX_G:
            raise ValueError(f"VOCEvaluator.update: G = {g} outside 1 .. {MAX_G}")
        for name, t in (("difficult", difficult), ("valid", valid)):
            if tuple(t.shape) != (n, g) or t.dtype != torch.bool:
                raise ValueError(f"VOCEvaluator.update: {name} must be [N, G] bool")
        if sizes is not None and (tuple(sizes.shape) != (n, 2) or sizes.dtype != torch.float32):
            raise ValueError("VOCEvaluator.update: sizes must be [N, 2] float32")
        return n, k, g

    def update(self, detections, gt, difficult, valid, sizes=None):
        n, k, g = self._check(detections, gt, difficult, valid, sizes)
        if n == 0:
            return
        if self.device.type == "cpu":
            return self._update_cpu(detections.numpy(), gt.numpy(), difficult.numpy(), valid.numpy(), None if sizes is None else sizes.numpy())
        from ._lib import call, ptr, stream
        det, gtc, dif, val = detections.contiguous(), gt.contiguous(), difficult.contiguous(), valid.contiguous()
        call("frost_voc_update", ptr(det), ptr(gtc), ptr(dif), ptr(val), ptr(sizes.contiguous()) if sizes is not None else None, n, self.num_classes, k, g,
             self.bkg_label, self.ovthresh, self.det_offset, self.top_k, self.max_images, self.capacity, ptr(self._records), ptr(self._ctr), stream())

    def _update_cpu(self, det, gt, difficult, valid, sizes):
        f32 = np.float32
        C, K = self.num_classes, det.shape[2]
        off, thr = f32(self.det_offset), f32(self.ovthresh)
        labels = gt[..., 4].astype(np.int64)
        cls_of = np.where(labels < self.bkg_label, labels, labels + 1)
        for n in range(det.shape[0]):
            img = self._seen + n
            if img >= self.max_images:
                self._overflow = 1
                continue
            w, h = (f32(sizes[n, 0]), f32(sizes[n, 1])) if sizes is not None else (f32(1), f32(1))
            for c in range(C):
                if c == self.bkg_label:
                    continue
                gi = np.nonzero(valid[n] & (cls_of[n] == c))[0]
                G = gt[n, gi, :4].astype(f32)
                gdiff = difficult[n, gi]
                self._npos[c] += int((~gdiff).sum())
                rows = np.nonzero(det[n, c, :, 0] > 0)[0]
                if rows.size == 0:
                    continue
                d = det[n, c, rows].astype(f32)
                score = d[:, 0]
                bx1, by1, bx2, by2 = d[:, 1] * w + off, d[:, 2] * h + off, d[:, 3] * w + off, d[:, 4] * h + off
                ordinal = img * self.top_k + rows
                flags = np.full(rows.size, FLAG_FP, dtype=np.uint64)
                if gi.size:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        iw = np.maximum(np.minimum(G[None, :, 2], bx2[:, None]) - np.maximum(G[None, :, 0], bx1[:, None]), f32(0))
                        ih = np.maximum(np.minimum(G[None, :, 3], by2[:, None]) - np.maximum(G[None, :, 1], by1[:, None]), f32(0))
                        inter = iw * ih
                        iou = inter / (((bx2 - bx1) * (by2 - by1))[:, None] + ((G[:, 2] - G[:, 0]) * (G[:, 3] - G[:, 1]))[None, :] - inter)
                    assert iou.dtype == np.float32
                    iou = np.where(np.isnan(iou), f32(-np.inf), iou)
                    jmax = np.argmax(iou, axis=1)
                    passed = iou[np.arange(rows.size), jmax] > thr
                    key = pack_records(score, ordinal, 0)
                    for j in np.unique(jmax[passed]):
                        sel = np.nonzero(passed & (jmax == j))[0]
                        if gdiff[j]:
                            flags[sel] = FLAG_IGNORED
                        else:
                            flags[sel[np.argmax(key[sel])]] = FLAG_TP
                recs = pack_records(score, ordinal, flags)
                room = max(0, self.capacity - int(self._cursor[c]))
                if recs.size > room:
                    self._overflow = 1
                self._cursor[c] += recs.size
                if room:
                    self._rows[c].append(recs[:room])
        self._seen += det.shape[0]

    # ---- results --------------------------------------------------------------------------------------------------------------------------------------
    def sorted_records(self):
        """[C, capacity] int64: every class's records in rank order (descending), empty slots 0 at the end."""
        if self.device.type != "cpu":
            return torch.sort(self._records, dim=1, descending=True)[0]
        out = np.zeros((self.num_classes, self.capacity), dtype=np.uint64)
        for c, rows in enumerate(self._rows):
            if rows:
                r = np.sort(np.concatenate(rows))[::-1]
                out[c, :r.size] = r
        return torch.from_numpy(out.view(np.int64))

    def pr_curve(self, c):
        """CPU state only: (rec, prec) of class c along the rank, as the reference's voc_eval returns them."""
        r = self.sorted_records().numpy().view(np.uint64)[c]
        r = r[r != 0]
        _, rec, prec = ap_from_flags(r & np.uint64(3), int(self._npos[c]), self.use_07_metric)
        return rec, prec

    OVERFLOW_MSG = "VOCEvaluator: record storage overflowed (capacity or max_images too small): the evaluation is incomplete"

    def overflowed(self):
        """0-d tensor on the evaluator's device: non-zero when records were dropped."""
        return torch.tensor(self._overflow) if self.device.type == "cpu" else self._ctr[2 * self.num_classes + 1]

    def compute(self, check_overflow=True):
        """dict: ap [C] fp64, mean_ap fp64 scalar, npos / ndet / tp / fp / ignored [C] int64 -- tensors on the evaluator's device.  check_overflow=False leaves
        the overflow word unread (no host read at all here): the caller reads overflowed() together with the results, as harness.val_detector does."""
        C = self.num_classes
        fg = torch.tensor([c for c in range(C) if c != self.bkg_label], dtype=torch.int64, device=self.device)
        if self.device.type == "cpu":
            if check_overflow and self._overflow:
                raise RuntimeError(self.OVERFLOW_MSG)
            recs = self.sorted_records().numpy().view(np.uint64)
            ap = np.full(C, np.nan, dtype=np.float64)
            cnt = np.zeros((5, C), dtype=np.int64)
            for c in range(C):
                if c == self.bkg_label:
                    continue
                r = recs[c][recs[c] != 0]
                fl = r & np.uint64(3)
                cnt[:, c] = [self._npos[c], r.size, (fl == FLAG_TP).sum(), (fl == FLAG_FP).sum(), (fl == FLAG_IGNORED).sum()]
                ap[c] = ap_from_flags(fl, int(self._npos[c]), self.use_07_metric)[0] if r.size else -1.0
            ap_t, cnt_t = torch.from_numpy(ap), torch.from_numpy(cnt)
        else:
            from ._lib import call, ptr, stream
            srt = self.sorted_records()
            ap_t = torch.empty(C, dtype=torch.float64, device=self.device)
            cnt_t = torch.empty(5, C, dtype=torch.int64, device=self.device)
            call("frost_voc_ap", ptr(srt), ptr(self._ctr), C, self.capacity, self.bkg_label, int(self.use_07_metric), ptr(ap_t), ptr(cnt_t), stream())
            if check_overflow and int(self._ctr[2 * C + 1]) != 0:          # the call's one host read of its own
                raise RuntimeError(self.OVERFLOW_MSG)
        out = dict(ap=ap_t, mean_ap=ap_t.index_select(0, fg).mean())
        for i, name in enumerate(("npos", "ndet", "tp", "fp", "ignored")):
            out[name] = cnt_t[i]
        return out

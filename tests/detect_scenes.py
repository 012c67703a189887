"""Synthetic detection scenes with DECISION MARGINS for the Detect layer's tests and for tools/gen_golden.py g15 (a plain helper module, not a conftest).

Random logits carry no margins: adjacent scores tie and sit 1e-8 from the confidence threshold, so any two fp32 implementations flip decisions on them.  A scene is
  * background priors: seeded noise (oracle.frost_oracle.synth) with +11 on the background logit, every foreground score far below 0.01;
  * a few ground-truth boxes per image from three classes: every prior with IoU > 0.2 to a box gets loc = encode(box) + jitter and the row
    (background 0, other classes -7, the box's class 3 * IoU - 1.5 + 0.8 * z), scores over about 0.2 .. 0.8; the class logits of one (image, class) are then
    spread at least 1e-3 apart in sorted order (the score is a monotone function of that logit alone, so adjacent scores cannot tie);
and it is accepted only if, measured in fp64 on the definition,
  1. every foreground score is >= 1e-3 away from conf_thresh,
  2. adjacent scores among the first top_k + 1 candidates of every (image, class) differ by >= 1e-5,
  3. every pairwise IoU inside each top-top_k set is >= 1e-5 away from nms_thresh
(about 30 x the fp32 rounding of a softmax / an IoU, ~3e-7).  find_scene() searches seeds deterministically."""
import zlib

import numpy as np
import torch

from oracle.frost_oracle import synth

M_THRESH, M_GAP, M_IOU = 1e-3, 1e-5, 1e-5
BKG_OFFSET, OTHER_LOGIT, LOGIT_STEP = 11.0, -7.0, 1e-3


def crc(*arrs):
    v = 0
    for a in arrs:
        v = zlib.crc32(np.ascontiguousarray(a).tobytes(), v)
    return np.uint32(v)


def background(n, p, c, seed):
    """Seeded background predictions: loc [n,p,4], conf [n,p,c] with the background logit raised by 11."""
    loc = synth((n, p, 4), 2 * seed + 15000) * np.float32(0.5)
    conf = synth((n, p, c), 2 * seed + 15001)
    conf[..., 0] += np.float32(BKG_OFFSET)
    return loc, conf


def assemble(n, p, c, seed, obj_idx, obj_loc, obj_conf):
    """Background of `seed` with the object rows (flat index image * p + prior) written over it."""
    loc, conf = background(n, p, c, seed)
    loc.reshape(-1, 4)[obj_idx] = obj_loc
    conf.reshape(-1, c)[obj_idx] = obj_conf
    return loc, conf


def _iou_np(box, pp):
    iw = np.clip(np.minimum(box[2], pp[:, 2]) - np.maximum(box[0], pp[:, 0]), 0, None)
    ih = np.clip(np.minimum(box[3], pp[:, 3]) - np.maximum(box[1], pp[:, 1]), 0, None)
    inter = iw * ih
    return inter / ((box[2] - box[0]) * (box[3] - box[1]) + (pp[:, 2] - pp[:, 0]) * (pp[:, 3] - pp[:, 1]) - inter)


def object_rows(priors, n, c, seed, variance=(0.1, 0.2), jitter=(1.0, 0.5)):
    """Ground-truth boxes of the scene `seed` and the prediction rows of the priors they claim -> (obj_idx [M] int64, obj_loc [M,4], obj_conf [M,c]) fp32."""
    pri = np.asarray(priors, dtype=np.float64)
    p = pri.shape[0]
    pp = np.concatenate([pri[:, :2] - pri[:, 2:] / 2, pri[:, :2] + pri[:, 2:] / 2], 1)
    rng = np.random.Generator(np.random.PCG64(7919 * seed + 13))
    classes = np.sort(rng.choice(np.arange(1, c), size=min(3, c - 1), replace=False))
    idx_all, loc_all, conf_all = [], [], []
    for i in range(n):
        k = 3 + int(rng.integers(0, 3))
        ctr = rng.random((k, 2)) * 0.6 + 0.2
        wh = rng.random((k, 2)) * 0.35 + 0.15
        lab = np.full(k, classes[0]) if i == 0 else classes[rng.integers(0, len(classes), k)]      # image 0: one crowded class
        best, owner = np.full(p, 0.2), np.full(p, -1)
        for j in range(k):
            ov = _iou_np(np.concatenate([ctr[j] - wh[j] / 2, ctr[j] + wh[j] / 2]), pp)
            take = ov > best
            best[take], owner[take] = ov[take], j
        sel = np.nonzero(owner >= 0)[0]
        j = owner[sel]
        z = rng.standard_normal((sel.size, 5))
        g_c = (ctr[j] - pri[sel, :2]) / (variance[0] * pri[sel, 2:]) + jitter[0] * z[:, 0:2]
        g_wh = np.log(wh[j] / pri[sel, 2:]) / variance[1] + jitter[1] * z[:, 2:4]
        logit = 3.0 * best[sel] - 1.5 + 0.8 * np.clip(z[:, 4], -2.0, 2.0)
        for cl in np.unique(lab[j]):                                 # per (image, class): sorted logits at least LOGIT_STEP apart
            m = np.nonzero(lab[j] == cl)[0]
            o = m[np.argsort(logit[m], kind="stable")]
            ramp = np.arange(o.size) * LOGIT_STEP
            logit[o] = np.maximum.accumulate(logit[o] - ramp) + ramp
        rows = np.full((sel.size, c), OTHER_LOGIT)
        rows[:, 0] = 0.0
        rows[np.arange(sel.size), lab[j]] = logit
        idx_all.append(i * p + sel)
        loc_all.append(np.concatenate([g_c, g_wh], 1))
        conf_all.append(rows)
    return np.concatenate(idx_all).astype(np.int64), np.concatenate(loc_all).astype(np.float32), np.concatenate(conf_all).astype(np.float32)


def measure(loc, conf, priors, top_k, min_dim, conf_thresh=0.01, nms_thresh=0.45, variance=(0.1, 0.2), bkg=0):
    """The three margins and the coverage counts of a scene, in fp64 on the definition (softmax, decode, score order, IoU on box * min_dim)."""
    loc, conf, pri = (torch.as_tensor(np.asarray(a)).double() for a in (loc, conf, priors))
    n, p, c = conf.shape
    sc = torch.softmax(conf, 2).transpose(1, 2).clone()                 # [n,c,p]
    sc[:, bkg] = 0.0
    fg = torch.ones(c, dtype=torch.bool)
    fg[bkg] = False
    m_thresh = float((sc[:, fg] - conf_thresh).abs().min())
    cxcy = pri[None, :, :2] + loc[..., :2] * variance[0] * pri[None, :, 2:]
    wh = pri[None, :, 2:] * torch.exp(loc[..., 2:] * variance[1])
    x1y1 = cxcy - wh / 2
    boxes = torch.cat([x1y1, wh + x1y1], 2) * min_dim
    ncand = (sc > conf_thresh).sum(2)                                    # [n,c]
    m_gap, m_iou, removed, kept_max = np.inf, np.inf, 0.0, 0
    for i, cl in torch.nonzero(ncand > 0).tolist():
        s, order = torch.sort(sc[i, cl], descending=True, stable=True)
        k1 = min(int(ncand[i, cl]), top_k + 1)
        if k1 > 1:
            m_gap = min(m_gap, float((s[:k1 - 1] - s[1:k1]).min()))
        k = min(k1, top_k)
        b = boxes[i, order[:k]]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        whi = (torch.min(b[:, None, 2:], b[None, :, 2:]) - torch.max(b[:, None, :2], b[None, :, :2])).clamp(min=0)
        inter = whi[..., 0] * whi[..., 1]
        iou = inter / (area[:, None] + area[None, :] - inter)
        if k > 1:
            off = ~torch.eye(k, dtype=torch.bool)
            m_iou = min(m_iou, float((iou[off] - nms_thresh).abs().min()))
        gone = torch.zeros(k, dtype=torch.bool)
        kept = 0
        for r in range(k):
            if not gone[r]:
                kept += 1
                gone |= iou[r] > nms_thresh
        removed, kept_max = max(removed, 1.0 - kept / k), max(kept_max, kept)
    nfg = int(fg.sum())
    return dict(m_thresh=m_thresh, m_gap=float(m_gap), m_iou=float(m_iou), ncand=ncand.numpy(), pairs_over_top_k=int((ncand[:, fg] > top_k).sum()),
                pairs_empty=int((ncand[:, fg] == 0).sum()), pairs=n * nfg, max_removed_fraction=float(removed), max_kept=int(kept_max))


def accepted(m):
    return m["m_thresh"] >= M_THRESH and m["m_gap"] >= M_GAP and m["m_iou"] >= M_IOU


def find_scene(priors, n, c, top_k, min_dim, seed0, tries=32, require=None):
    """The first seed in seed0 .. seed0 + tries - 1 whose scene holds all three margins (and `require(measurement)`, if given) ->
    (loc, conf, info) as fp32 numpy arrays and dict(seed, obj_idx, obj_loc, obj_conf, measurement...).  Raises if none qualifies."""
    pri = np.asarray(priors, dtype=np.float32)
    seen = []
    for seed in range(seed0, seed0 + tries):
        oi, ol, oc = object_rows(pri, n, c, seed)
        loc, conf = assemble(n, pri.shape[0], c, seed, oi, ol, oc)
        m = measure(loc, conf, pri, top_k, min_dim)
        seen.append((seed, m["m_thresh"], m["m_gap"], m["m_iou"]))
        if accepted(m) and (require is None or require(m)):
            return loc, conf, dict(m, seed=seed, obj_idx=oi, obj_loc=ol, obj_conf=oc)
    raise AssertionError(f"no scene with decision margins among {tries} seeds from {seed0}: (seed, thresh, gap, iou) = {seen}")

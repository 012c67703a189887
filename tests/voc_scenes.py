"""Synthetic evaluation scenes for the VOC mean-AP evaluator whose every decision carries a margin, so that the reference (which round-trips detections through
'%.3f' / '%.1f' text and computes IoU in fp64), the CPU definition (fp32 IoU) and the HIP kernels must agree without exceptions:
  * scores are distinct multiples of 0.001 in (0.01, 1) within a class (over all images of the scene): the text round trip keeps them, the rank has no ties;
  * pixel coordinates are multiples of 0.5, and a detection row is redrawn unless fp32(fp32(p / w) * w) is exactly p for each of its coordinates: the
    evaluator's scaled box is then the drawn box, bit for bit (products of such coordinates below 2^12 are exact in fp32 as well);
  * every IoU of a detection with a ground-truth box of its class in its image is >= M_IOU away from ovthresh, and wherever the best IoU passes, the runner-up is
    >= M_IOU below it (fp64; a box identical to the best one is exempt when the scene asks for duplicated ground truth: the lowest index must win then).
build() draws one scene from a seed and asserts all of this; find() searches seeds until the coverage the caller requires is there as well."""
import numpy as np

M_IOU = 1e-4
SIZES = ((500.0, 375.0), (333.0, 500.0), (480.0, 364.0))          # (w, h): none a power of two


def _iou64(d, g):
    iw = np.maximum(np.minimum(g[:, 2], d[2]) - np.maximum(g[:, 0], d[0]), 0.0)
    ih = np.maximum(np.minimum(g[:, 3], d[3]) - np.maximum(g[:, 1], d[1]), 0.0)
    inter = iw * ih
    return inter / ((d[2] - d[0]) * (d[3] - d[1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter)


def _half(rng, lo, hi):
    return float(rng.integers(int(np.ceil(lo * 2)), int(np.floor(hi * 2)) + 1)) / 2.0


def _lossless(p, w):
    x = np.float32(np.float32(p) / np.float32(w))
    return float(np.float32(x * np.float32(w))) == p


def build(seed, N=6, C=5, K=40, G=8, bkg=0, ovthresh=0.5, offset=1.0, fill=0.5, no_gt=False, dup_gt=False):
    """-> (det [N, C, K, 5] fp32, gt [N, G, 5] fp32, difficult [N, G] bool, valid [N, G] bool, sizes [N, 2] fp32, info).  Detection boxes are stored normalised
    (pixel / size, before `offset`); ground truth is in the pixel frame the evaluator compares in (detection pixel + offset)."""
    rng = np.random.default_rng(seed)
    fg = [c for c in range(C) if c != bkg]
    gt_only = fg[-1] if len(fg) >= 3 else None          # ground truth, never a detection
    det_only = fg[-2] if len(fg) >= 3 else None         # detections, never ground truth
    det = np.zeros((N, C, K, 5), dtype=np.float32)
    gt = np.zeros((N, G, 5), dtype=np.float32)
    difficult, valid = np.zeros((N, G), dtype=bool), np.zeros((N, G), dtype=bool)
    sizes = np.array([SIZES[n % len(SIZES)] for n in range(N)], dtype=np.float32)
    pool = {c: list(rng.permutation(np.arange(11, 1000))) for c in fg}
    cov = dict(tp=0, dup=0, near=0, difficult_twice=0, redrawn=0, rows=0, partial_class=0, gt_only=0, det_only=0, image_without_gt=0, twin_first=0, twin_last=0, sizes=len({tuple(s) for s in sizes.tolist()}))
    m_thr, m_gap = np.inf, np.inf
    for n in range(N):
        w, h = float(sizes[n, 0]), float(sizes[n, 1])
        # -- ground truth: some rows of the G, scattered (the holes stay invalid)
        boxes = {c: [] for c in fg}
        if not no_gt and not (N >= 2 and n == N - 1):
            rows = sorted(rng.choice(G, size=max(1, int(rng.integers((G + 1) // 2, G + 1))), replace=False).tolist()) if G > 1 else [0]
            if dup_gt:
                rows = list(range(G))          # every row valid: the copy sits G - 1 rows behind its original
            for i, g in enumerate(rows):
                c = fg[int(rng.integers(0, len(fg)))]
                if c == det_only:
                    c = fg[0]
                if dup_gt and i > 0 and i == len(rows) - 1:
                    # the last row repeats the first one, and exactly one of the two is difficult -- the original in odd images, the copy in even ones: a detection
                    # of that box is TP / FP or ignored depending on which of the two equal IoUs is taken, so the records show whether the lowest index won
                    src = rows[0]
                    gt[n, g] = gt[n, src]
                    difficult[n, src], difficult[n, g] = n % 2 == 1, n % 2 == 0
                    c = [k for k in fg if (k if k < bkg else k - 1) == int(gt[n, src, 4])][0]
                else:
                    bw, bh = _half(rng, 40, 160), _half(rng, 40, 160)
                    x1, y1 = _half(rng, 8, w - bw - 8), _half(rng, 8, h - bh - 8)
                    gt[n, g] = (x1, y1, x1 + bw, y1 + bh, c if c < bkg else c - 1)
                    difficult[n, g] = rng.random() < 0.25
                valid[n, g] = True
                boxes[c].append(g)
        else:
            cov["image_without_gt"] += 1
        for c in fg:
            if c == gt_only:
                cov["gt_only"] += len(boxes[c])
                continue
            if c != det_only and len(fg) >= 2 and (n + c) % 3 == 0:
                cov["partial_class"] += 1          # this class has no detection in this image
                continue
            gsel = np.array(boxes[c], dtype=np.int64)
            gb = gt[n, gsel, :4].astype(np.float64)
            plan = []
            for j in range(len(gsel)):
                plan += [("hit", j)] * int(rng.integers(0, 4)) + [("near", j)] * int(rng.integers(0, 2))
            target = max(1, int(K * fill)) if K > 1 else 1
            target = min(target, K, len(pool[c]) // max(1, N - n))
            plan = plan[:target] + [("free", -1)] * max(0, target - len(plan))
            slots = sorted(rng.choice(K, size=len(plan), replace=False).tolist())
            hits = {}
            for (kind, j), r in zip(plan, slots):
                for attempt in range(200):
                    if kind == "free" or attempt >= 100:          # a planned row that cannot be placed (image border) becomes a free one
                        bw, bh = _half(rng, 20, 200), _half(rng, 20, 200)
                        x1, y1 = _half(rng, 1, w - bw - 2), _half(rng, 1, h - bh - 2)
                        p = np.array([x1, y1, x1 + bw, y1 + bh])
                    else:
                        g0 = gb[j] - offset
                        if kind == "hit":
                            p = g0 + np.array([_half(rng, -4, 4) for _ in range(4)])
                        else:
                            p = g0 + np.array([1.0, 0.0, 1.0, 0.0]) * (np.round(rng.uniform(0.38, 0.5) * (g0[2] - g0[0]) * 2) / 2)
                            p = p + np.array([0.0, 1.0, 0.0, 1.0]) * _half(rng, -3, 3)
                        p = np.clip(p, 0.0, [w - 1, h - 1, w - 1, h - 1])
                    cov["rows"] += 1 if attempt == 0 else 0
                    ok = p[2] - p[0] >= 4 and p[3] - p[1] >= 4 and all(_lossless(float(p[i]), (w, h)[i % 2]) for i in range(4))
                    if ok and len(gsel):
                        iou = _iou64(p + offset, gb)
                        best = int(np.argmax(iou))
                        ok = float(np.abs(iou - ovthresh).min()) >= M_IOU
                        if ok and iou[best] > ovthresh:
                            others = [iou[i] for i in range(len(iou)) if i != best and not (dup_gt and np.array_equal(gb[i], gb[best]))]
                            ok = not others or iou[best] - max(others) >= M_IOU
                            if ok and others:
                                m_gap = min(m_gap, float(iou[best] - max(others)))
                        if ok:
                            m_thr = min(m_thr, float(np.abs(iou - ovthresh).min()))
                            if iou[best] > ovthresh:
                                hits.setdefault(best, []).append(r)
                                if dup_gt and any(i != best and np.array_equal(gb[i], gb[best]) for i in range(len(iou))):
                                    cov["twin_last" if difficult[n, gsel[best]] else "twin_first"] += 1          # matches of a doubled box whose non-difficult copy is the first / the last
                            elif kind == "near":
                                cov["near"] += 1
                    if ok:
                        break
                    cov["redrawn"] += 1
                else:
                    raise RuntimeError("voc_scenes: no admissible row in 200 draws")
                det[n, c, r] = (np.float32(pool[c].pop() / 1000.0), np.float32(p[0]) / np.float32(w), np.float32(p[1]) / np.float32(h), np.float32(p[2]) / np.float32(w),
                                np.float32(p[3]) / np.float32(h))
            if c == det_only:
                cov["det_only"] += len(plan)
            for j, rs in hits.items():
                if difficult[n, gsel[j]]:
                    cov["difficult_twice"] += 1 if len(rs) >= 2 else 0
                else:
                    cov["tp"] += 1
                    cov["dup"] += len(rs) - 1
    # scores distinct within a class
    for c in fg:
        s = det[:, c, :, 0][det[:, c, :, 0] > 0]
        assert len(np.unique(s)) == len(s)
    info = dict(seed=seed, m_thresh=m_thr, m_gap=m_gap, **cov)
    return det, gt, difficult, valid, sizes, info


def covered(info):
    """Every situation the golden scenes must contain."""
    return all(info[k] > 0 for k in ("tp", "dup", "near", "difficult_twice", "partial_class", "gt_only", "det_only", "image_without_gt")) and info["sizes"] >= 2


def find(seed0, tries=64, require=covered, **kw):
    for seed in range(seed0, seed0 + tries):
        out = build(seed, **kw)
        if require is None or require(out[5]):
            return out
    raise RuntimeError(f"voc_scenes: no scene with the required coverage in seeds {seed0} .. {seed0 + tries - 1}")

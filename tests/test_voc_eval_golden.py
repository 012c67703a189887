"""The VOC mean-AP evaluator's CPU definition (frostnet_amd.voc_eval.VOCEvaluator on CPU tensors) against the reference's voc_eval / voc_ap
(Object_Detection/qeval_convert.py:177-345, recorded by tools/gen_golden.py g16 on scenes with decision margins, tests/voc_scenes.py), and the parts of the
contract the reference leaves open: the tie rule, det_offset, the refusals, and that the state does not depend on how the images are split into updates.
AP under the 07 metric is compared for bit equality (every step is a correctly rounded fp64 operation on the same integers in the same order); under the area
metric within 1e-9 (at most 10^6 terms, each at most 1, summed in another order than numpy's pairwise sum); rec / prec for equality; mean_ap within 1e-12."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voc_scenes as V  # noqa: E402

from frostnet_amd import VOCEvaluator  # noqa: E402
from frostnet_amd import voc_eval as VE  # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def golden_scene(g, case):
    k = f"s{case}_"
    return tuple(T(g[k + name]) for name in ("det", "gt", "difficult", "valid", "sizes"))


def same_or_both_nan(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def assert_same_state(a, b, what=""):
    """Two evaluators (any devices) hold the same evaluation: sorted records word for word, and every count."""
    ra, rb = a.sorted_records().cpu(), b.sorted_records().cpu()
    assert ra.shape == rb.shape, (what, ra.shape, rb.shape)
    assert torch.equal(ra, rb), (what, "records differ", (ra != rb).nonzero()[:8].tolist())
    ca, cb = a.compute(), b.compute()
    for name in ("npos", "ndet", "tp", "fp", "ignored"):
        assert ca[name].dtype == torch.int64 and torch.equal(ca[name].cpu(), cb[name].cpu()), (what, name, ca[name].tolist(), cb[name].tolist())
    return ca, cb


def assert_same_ap(ca, cb, use_07_metric, what=""):
    apa, apb = ca["ap"].cpu().numpy(), cb["ap"].cpu().numpy()
    assert apa.dtype == np.float64 and apb.dtype == np.float64
    print(f"[voc {what}] ap {apa.tolist()} vs {apb.tolist()}")
    for c in range(len(apa)):
        if use_07_metric or np.isnan(apb[c]) or apb[c] == -1.0:
            assert same_or_both_nan(apa[c], apb[c]), (what, c, apa[c], apb[c])
        else:
            assert abs(apa[c] - apb[c]) <= 1e-9, (what, c, apa[c], apb[c])
    ma, mb = float(ca["mean_ap"]), float(cb["mean_ap"])
    assert (np.isnan(ma) and np.isnan(mb)) or abs(ma - mb) <= (1e-12 if use_07_metric else 1e-9), (what, ma, mb)


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("metric", [1, 0])
def test_cpu_definition_vs_reference_golden(golden, case, metric):
    g = golden("g16_voc_eval")
    k = f"s{case}_"
    assert g[k + "margins"][0] >= V.M_IOU and g[k + "margins"][1] >= V.M_IOU
    assert (g[k + "coverage"][:8] > 0).all() and g[k + "coverage"][8] >= 2, g[k + "coverage"]
    det, gt, difficult, valid, sizes = golden_scene(g, case)
    C = det.shape[1]
    ev = VOCEvaluator(num_classes=C, use_07_metric=bool(metric), det_offset=1.0, max_images=16, top_k=det.shape[2])
    ev.update(det, gt, difficult, valid, sizes)
    out = ev.compute()
    assert sorted(out) == ["ap", "fp", "ignored", "mean_ap", "ndet", "npos", "tp"]
    ap, ref = out["ap"].numpy(), g[k + f"ap_m{metric}"]
    print(f"[g16 scene {case} metric {'07' if metric else 'area'}] ap {ap.tolist()}  reference {ref.tolist()}")
    assert np.isnan(ap[0]) and np.isnan(ref[0])
    for c in range(1, C):
        if metric or np.isnan(ref[c]) or ref[c] == -1.0:
            assert same_or_both_nan(ap[c], ref[c]), (c, ap[c], ref[c])          # bit-equal; the sentinels -1 / 0.0 / NaN where the reference has them
        else:
            assert abs(ap[c] - ref[c]) <= 1e-9, (c, ap[c], ref[c])
    assert (ref[1:] == -1.0).any() and ((ref[1:] == 0.0).any() if metric else np.isnan(ref[1:]).any())
    want_mean = np.mean(ref[1:])
    got_mean = float(out["mean_ap"])
    assert (np.isnan(want_mean) and np.isnan(got_mean)) or abs(got_mean - want_mean) <= 1e-12, (got_mean, want_mean)
    offs = g[k + "curve_offsets"]
    for c in range(1, C):
        rec, prec = g[k + f"rec_m{metric}"][offs[c - 1]:offs[c]], g[k + f"prec_m{metric}"][offs[c - 1]:offs[c]]
        if ref[c] == -1.0:
            assert rec.size == 0 and int(out["ndet"][c]) == 0
            continue
        mine_rec, mine_prec = ev.pr_curve(c)
        assert np.array_equal(mine_rec, rec, equal_nan=True) and np.array_equal(mine_prec, prec), c
        assert int(out["ndet"][c]) == rec.size
    assert int(out["tp"].sum()) > 0 and int(out["ignored"].sum()) > 0 and int(out["fp"].sum()) > 0


def _one_class(rows, gt_rows, **kw):
    """Evaluator over images given as lists of (score, x1, y1, x2, y2) rows of class 1 and (x1, y1, x2, y2) ground truth."""
    ev = VOCEvaluator(num_classes=2, max_images=8, top_k=4, **kw)
    return ev, [(T(np.stack([np.zeros((len(r), 5), dtype=np.float32), np.array(r, dtype=np.float32)])[None]), T(np.array([g + [0.0] for g in gts], dtype=np.float32).reshape(1, -1, 5)))
                for r, gts in zip(rows, gt_rows)]


def test_tie_rule_resolves_by_ordinal():
    """Equal scores within one image and across images: the lower image ordinal * top_k + row ranks first -- it takes the TP, and it comes first in the records."""
    box = [10.0, 10.0, 50.0, 50.0]
    far = [200.0, 200.0, 240.0, 240.0]
    # image 0: rows 0 and 1 tie on the same box (row 0 is the TP); image 1: the same score again on its own box, and a miss with that score
    ev, batches = _one_class([[[0.5] + far, [0.5] + box, [0.5] + box], [[0.5] + box, [0.5] + far]], [[box], [box]])
    for det, gt in batches:
        ev.update(det, gt, torch.zeros(1, 1, dtype=torch.bool), torch.ones(1, 1, dtype=torch.bool))
    rec = ev.sorted_records()[1].numpy().view(np.uint64)
    rec = rec[rec != 0]
    assert rec.size == 5 and len(set((rec >> np.uint64(32)).tolist())) == 1
    ordinal = (~(rec >> np.uint64(2))) & np.uint64(VE.ORD_MASK)
    assert ordinal.tolist() == [0, 1, 2, 4, 5]
    assert (rec & np.uint64(3)).tolist() == [VE.FLAG_FP, VE.FLAG_TP, VE.FLAG_FP, VE.FLAG_TP, VE.FLAG_FP]
    out = ev.compute()
    assert out["tp"].tolist() == [0, 2] and out["fp"].tolist() == [0, 3] and out["npos"].tolist() == [0, 2]


def walk_counts(parts, num_classes, bkg_label=0, last_index=False, ovthresh=0.5):
    """(tp, fp, ignored) per class by the reference's own procedure, written out a second time: one sequential walk over a class's detections in rank order with
    a `taken` flag per ground-truth box (det_offset 0).  last_index=True takes the last of several equal largest IoUs instead of the first: the rule a scene with
    doubled ground truth has to tell apart from the definition's."""
    det, gt, difficult, valid, sizes = [None if p is None else p.numpy() for p in parts]
    N, C, K = det.shape[:3]
    out = np.zeros((3, num_classes), dtype=np.int64)
    for c in range(num_classes):
        if c == bkg_label:
            continue
        label = c if c < bkg_label else c - 1
        taken = {}
        for s, n, r in sorted((-float(det[n, c, r, 0]), n, r) for n in range(N) for r in range(K) if det[n, c, r, 0] > 0):
            w, h = (sizes[n] if sizes is not None else np.ones(2, dtype=np.float32)).astype(np.float32)
            b = det[n, c, r, 1:] * np.array([w, h, w, h], dtype=np.float32)
            best, jmax = np.float32(-np.inf), -1
            for j in np.nonzero(valid[n] & (gt[n, :, 4].astype(np.int64) == label))[0]:
                g = gt[n, j, :4]
                iw, ih = max(min(g[2], b[2]) - max(g[0], b[0]), np.float32(0)), max(min(g[3], b[3]) - max(g[1], b[1]), np.float32(0))
                inter = iw * ih
                iou = inter / ((b[2] - b[0]) * (b[3] - b[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter)
                assert iou.dtype == np.float32
                if iou > best or (last_index and iou == best):
                    best, jmax = iou, int(j)
            if jmax < 0 or not best > np.float32(ovthresh):
                out[1, c] += 1
            elif difficult[n, jmax]:
                out[2, c] += 1
            else:
                out[1 if taken.get((n, jmax)) else 0, c] += 1
                taken[(n, jmax)] = True
    return out


def twin_case():
    """Two images, each with the same box at ground-truth rows 0 and 2 and exactly one of the two difficult (row 2 in image 0, row 0 in image 1), with two
    detections of that box in image 0 and one in image 1.  The lowest index wins the tie of the two equal IoUs: image 0 gives TP + FP, image 1 an ignored one; a
    last-index rule would give two ignored and a TP."""
    box, other = [10.0, 10.0, 50.0, 50.0], [200.0, 200.0, 240.0, 240.0]
    det = torch.zeros(2, 2, 4, 5)
    det[0, 1, 1:3] = torch.tensor([[0.9] + box, [0.8, 11.0, 10.0, 50.0, 50.0]])
    det[1, 1, 3] = torch.tensor([0.7] + box)
    gt = torch.tensor([box + [0.0], other + [0.0], box + [0.0]]).repeat(2, 1, 1)
    difficult = torch.tensor([[False, False, True], [True, False, False]])
    return [det, gt, difficult, torch.ones(2, 3, dtype=torch.bool), None], dict(flags=[VE.FLAG_TP, VE.FLAG_FP, VE.FLAG_IGNORED], npos=4)


TWIN_SCENE = dict(K=200, G=65, C=2, N=5, bkg=1, dup_gt=True)          # the doubled box sits at rows 0 and 64: its copies are in different waves of boxes


def twin_scene(seed0=500):
    """A scene from voc_scenes with doubled ground truth in which detections match the doubled box both where its first copy is the non-difficult one and where
    its last copy is, and in which all 65 rows of an image are valid boxes of one class."""
    out = V.find(seed0, tries=32, require=lambda i: i["tp"] > 0 and i["twin_first"] > 0 and i["twin_last"] > 0, offset=0.0, fill=0.6, **TWIN_SCENE)
    return [T(a) for a in out[:5]], out[5]


def test_equal_ious_resolve_to_the_lowest_index():
    """Two identical ground-truth boxes: jmax is the first of them, and the tests' scenes can tell -- a last-index rule gives other counts on both."""
    parts, want = twin_case()
    ev = VOCEvaluator(num_classes=2, max_images=2, top_k=4)
    ev.update(*parts)
    rec = ev.sorted_records()[1].numpy().view(np.uint64)
    assert (rec[rec != 0] & np.uint64(3)).tolist() == want["flags"]
    out = ev.compute()
    assert (out["tp"][1], out["fp"][1], out["ignored"][1], out["npos"][1]) == (1, 1, 1, want["npos"])
    assert walk_counts(parts, 2).T[1].tolist() == [1, 1, 1] and walk_counts(parts, 2, last_index=True).T[1].tolist() == [1, 0, 2]
    parts, info = twin_scene()
    assert bool(parts[3][:4].all()) and info["twin_first"] > 0 and info["twin_last"] > 0, info
    ev = VOCEvaluator(num_classes=2, bkg_label=1, max_images=8, top_k=200)
    ev.update(*parts)
    out = ev.compute()
    got = np.stack([out[k].numpy() for k in ("tp", "fp", "ignored")])
    first, last = walk_counts(parts, 2, bkg_label=1), walk_counts(parts, 2, bkg_label=1, last_index=True)
    print(f"[twin scene seed {info['seed']}] tp / fp / ignored {got[:, 0].tolist()}, first index {first[:, 0].tolist()}, last index {last[:, 0].tolist()}")
    assert np.array_equal(got, first)
    assert first[0, 0] != last[0, 0] and first[2, 0] != last[2, 0], "the scene does not depend on which of two identical boxes is taken"


def test_det_offset_changes_the_match():
    """A detection whose IoU with its box is above 0.5 as drawn and below it when shifted by one pixel: det_offset = 1 reproduces the reference's shift."""
    gt_box = [10.0, 10.0, 14.0, 14.0]
    row = [[0.9, 11.0, 10.0, 15.0, 14.0]]                                  # IoU 12 / 20 = 0.6; shifted by (1, 1): 2 * 3 / (32 - 6) = 0.23
    tps = []
    for off in (0.0, 1.0):
        ev, batches = _one_class([row], [[gt_box]], det_offset=off)
        ev.update(*batches[0], torch.zeros(1, 1, dtype=torch.bool), torch.ones(1, 1, dtype=torch.bool))
        out = ev.compute()
        tps.append((int(out["tp"][1]), int(out["fp"][1]), float(out["ap"][1]) > 0.99))
    assert tps == [(1, 0, True), (0, 1, False)]


def test_sizes_scale_the_detection_only():
    ev = VOCEvaluator(num_classes=2, max_images=2, top_k=1)
    det = T(np.array([[0.0] * 5, [0.9, 0.1, 0.2, 0.5, 0.6]], dtype=np.float32).reshape(1, 2, 1, 5))
    gt = T(np.array([30.0, 40.0, 150.0, 120.0, 0.0], dtype=np.float32).reshape(1, 1, 5))
    ev.update(det, gt, torch.zeros(1, 1, dtype=torch.bool), torch.ones(1, 1, dtype=torch.bool), T(np.array([[300.0, 200.0]], dtype=np.float32)))
    assert ev.compute()["tp"].tolist() == [0, 1]


def test_refusals():
    with pytest.raises(ValueError):
        VOCEvaluator(max_images=1 << 23, top_k=200)                        # max_images * top_k > 2^30
    with pytest.raises(ValueError):
        VOCEvaluator(max_images=4, top_k=8, capacity=(1 << 30) + 1)        # the device's class cursor is an int32 that stops at 2^30
    ev = VOCEvaluator(num_classes=3, max_images=4, top_k=8)
    det, gt = torch.zeros(2, 3, 8, 5), torch.zeros(2, 4, 5)
    dif, val = torch.zeros(2, 4, dtype=torch.bool), torch.ones(2, 4, dtype=torch.bool)
    ev.update(det, gt, dif, val)
    for bad in ((torch.zeros(2, 3, 9, 5), gt, dif, val),                   # K > top_k
                (torch.zeros(2, 4, 8, 5), gt, dif, val),                   # classes
                (det.double(), gt, dif, val), (det, gt.double(), dif, val),
                (det, torch.zeros(3, 4, 5), dif, val), (det, torch.zeros(2, 4, 4), dif, val),
                (det, gt, dif.float(), val), (det, gt, dif, val[:, :3]), (det, gt, dif, val.to(torch.uint8))):
        with pytest.raises(ValueError):
            ev.update(*bad)
    with pytest.raises(ValueError):
        ev.update(det, gt, dif, val, torch.ones(2, 3))
    with pytest.raises(ValueError):
        ev.update(det, gt, dif, val, torch.ones(2, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        ev.update(det.to("meta"), gt, dif, val)                            # tensors on different devices
    small = VOCEvaluator(num_classes=2, max_images=4, top_k=2, capacity=1)
    d = torch.tensor([[[[0.9, 0.0, 0.0, 1.0, 1.0], [0.8, 0.0, 0.0, 1.0, 1.0]]] * 2])
    small.update(d, torch.zeros(1, 1, 5), torch.zeros(1, 1, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="overflow"):
        small.compute()
    small.reset()
    assert small.compute()["ndet"].tolist() == [0, 0]


def test_one_update_equals_three():
    det, gt, difficult, valid, sizes, info = V.build(7, N=6, C=5, K=40, G=8, offset=0.0)
    parts = [T(a) for a in (det, gt, difficult, valid, sizes)]
    for metric in (True, False):
        one = VOCEvaluator(num_classes=5, use_07_metric=metric, max_images=6, top_k=40)
        one.update(*parts)
        three = VOCEvaluator(num_classes=5, use_07_metric=metric, max_images=6, top_k=40)
        for lo, hi in ((0, 1), (1, 4), (4, 6)):
            three.update(*[p[lo:hi] for p in parts])
        ca, cb = assert_same_state(one, three, "1 update vs 3")
        assert_same_ap(ca, cb, True, "1 update vs 3")                      # the same records in the same order: bit-equal under either metric
        assert int(ca["tp"].sum()) > 0
    one.reset()
    assert int(one.compute()["ndet"].sum()) == 0 and one.compute()["ap"][1:].tolist() == [-1.0] * 4


def test_val_detector_loop_on_cpu_tensors():
    """harness.val_detector: eval mode, the evaluator reset first, every batch of the loader through model.detect into update, (mean AP, per-class AP) out;
    an overflow of the record storage raises there as well."""
    from frostnet_amd import harness
    det, gt, difficult, valid, sizes, _ = V.build(3, N=4, C=5, K=40, G=8, offset=0.0)
    parts = [T(a) for a in (gt, difficult, valid, sizes)]

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def detect(self, x, top_k, conf_thresh, nms_thresh):
            assert not self.training and (top_k, conf_thresh, nms_thresh) == (40, 0.01, 0.45)
            return T(det)[x.long()]

    loader = [(torch.tensor([0.0, 1.0]), *[p[:2] for p in parts]), (torch.tensor([2.0, 3.0]), *[p[2:] for p in parts])]
    ev = VOCEvaluator(num_classes=5, max_images=4, top_k=40)
    ev.update(T(det)[:1], *[p[:1] for p in parts])                        # stale state: val_detector must reset it
    mean_ap, aps = harness.val_detector(loader, Stub().train(), ev, top_k=40)
    want = VOCEvaluator(num_classes=5, max_images=4, top_k=40)
    want.update(T(det), *parts)
    out = want.compute()
    assert np.isnan(aps[0]) and aps[1:] == out["ap"][1:].tolist() and mean_ap == float(out["mean_ap"]) and int(out["tp"].sum()) > 0
    with pytest.raises(RuntimeError, match="overflow"):
        harness.val_detector(loader, Stub(), VOCEvaluator(num_classes=5, max_images=3, top_k=40), top_k=40)
    with pytest.raises(ValueError):
        harness.val_detector([], Stub(), ev)

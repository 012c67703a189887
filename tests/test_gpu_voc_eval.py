"""The VOC mean-AP evaluator on the device (csrc/frost_voceval.hip: per-batch matching + packed records, per-evaluation AP) against
  1. the reference's voc_eval recorded in g16 (tools/gen_golden.py),
  2. the CPU definition (VOCEvaluator on CPU tensors) over a grid of shapes, on scenes whose every decision has a margin (tests/voc_scenes.py),
and the plumbing: exact score ties, capture into a HIP graph, determinism, overflow without an out-of-bounds write, harness.val_detector end to end.
Criteria, without exceptions: equal tp / fp / ignored / ndet / npos, sorted record rows equal word for word, AP bit-equal under the 07 metric and within 1e-9
under the area metric (test_voc_eval_golden.assert_same_state / assert_same_ap); only frost_voc_* entries run during update."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voc_scenes as V  # noqa: E402
from test_voc_eval_golden import TWIN_SCENE, T, assert_same_ap, assert_same_state, golden_scene, same_or_both_nan, twin_case, twin_scene  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib, voc_eval
    return voc_eval, _lib


def _update(L, ev, parts):
    """ev.update on the device with the proof that only the evaluator's HIP entries ran."""
    L.CALL_LOG = []
    try:
        ev.update(*[None if p is None else p.cuda() for p in parts])
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    assert log and all(name.startswith("frost_voc_") for name in log), log


def _pair(E, L, parts, splits, **kw):
    """The same images through a CPU evaluator and a device evaluator, in the same updates."""
    cpu, dev = E.VOCEvaluator(**kw), E.VOCEvaluator(device="cuda", **kw)
    for lo, hi in splits:
        cut = [None if p is None else p[lo:hi] for p in parts]
        cpu.update(*cut)
        _update(L, dev, cut)
    return cpu, dev


def _scene(seed, require=None, **kw):
    det, gt, difficult, valid, sizes, info = V.find(seed, tries=32, require=require, **kw)
    return [T(a) for a in (det, gt, difficult, valid, sizes)], info


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("metric", [1, 0])
def test_hip_voc_eval_vs_reference_golden(mods, golden, case, metric):
    E, L = mods
    g = golden("g16_voc_eval")
    parts = list(golden_scene(g, case))
    C, K = parts[0].shape[1], parts[0].shape[2]
    cpu, dev = _pair(E, L, parts, [(0, parts[0].shape[0])], num_classes=C, use_07_metric=bool(metric), det_offset=1.0, max_images=16, top_k=K)
    ca, cb = assert_same_state(dev, cpu, f"HIP vs CPU on g16 scene {case}")
    assert cb["ap"].is_cpu and ca["ap"].is_cuda and ca["mean_ap"].is_cuda and ca["tp"].is_cuda
    assert_same_ap(ca, cb, bool(metric), f"g16 scene {case} metric {metric}")
    ap, ref = ca["ap"].cpu().numpy(), g[f"s{case}_ap_m{metric}"]
    for c in range(1, C):
        if metric or np.isnan(ref[c]) or ref[c] == -1.0:
            assert same_or_both_nan(ap[c], ref[c]), (c, ap[c], ref[c])
        else:
            assert abs(ap[c] - ref[c]) <= 1e-9, (c, ap[c], ref[c])


# every listed value of K, G, C, N and one non-zero bkg_label occurs once.  G = 65: all 65 rows are valid boxes of the one class (two waves of boxes in LDS), rows 0
# and 64 are the same box and one of the two is difficult, so the records depend on the lowest index winning (test_voc_eval_golden.twin_scene, which
# test_equal_ious_resolve_to_the_lowest_index shows to tell the first index from the last)
GRID = [dict(K=1, G=1, C=2, N=1, bkg=0, no_gt=True), dict(K=40, G=1, C=21, N=5, bkg=0), TWIN_SCENE]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: f"K{s['K']}-G{s['G']}-C{s['C']}-N{s['N']}-bkg{s['bkg']}")
def test_hip_voc_eval_vs_cpu_definition_grid(mods, shape):
    E, L = mods
    if shape.get("dup_gt"):
        parts, info = twin_scene()
        assert bool(parts[3][:4].all()) and info["twin_first"] > 0 and info["twin_last"] > 0, info
    else:
        parts, info = _scene(seed=300 + shape["K"], require=lambda i: shape.get("no_gt") or i["tp"] > 0, offset=0.0, fill=0.6, **shape)
    print(f"[scene {shape}] seed {info['seed']}, margins {info['m_thresh']:.2e} / {info['m_gap']:.2e}, tp {info['tp']} dup {info['dup']} near {info['near']} redrawn {info['redrawn']} of {info['rows']}")
    assert not (shape.get("no_gt") and bool(parts[3].any()))
    for metric in (True, False):
        cpu, dev = _pair(E, L, parts, [(0, shape["N"])], num_classes=shape["C"], bkg_label=shape["bkg"], use_07_metric=metric, max_images=8, top_k=shape["K"])
        ca, cb = assert_same_state(dev, cpu, f"{shape} metric {metric}")
        assert_same_ap(ca, cb, metric, f"{shape} metric {metric}")
        assert int(cb["ndet"].sum()) > 0 and int(cb["ndet"][shape["bkg"]]) == 0
        assert shape.get("no_gt") or int(cb["tp"].sum()) > 0


def test_three_updates_across_scan_chunks(mods):
    """Three consecutive updates; one class ends with more than two 256-record scan chunks of frost_voc_ap, with TPs on both sides of each chunk boundary."""
    E, L = mods
    for seed in range(400, 416):
        parts, info = _scene(seed=seed, N=6, C=3, K=200, G=24, offset=0.0, fill=0.8)
        cpu = E.VOCEvaluator(num_classes=3, max_images=6, top_k=200)
        cpu.update(*parts)
        rec = cpu.sorted_records().numpy().view(np.uint64)
        rows = [r[r != 0] for r in rec]
        c = int(np.argmax([r.size for r in rows]))
        tp_rank = np.nonzero((rows[c] & np.uint64(3)) == E.FLAG_TP)[0]
        if rows[c].size > 512 and all(((tp_rank >= lo) & (tp_rank < hi)).any() for lo, hi in ((0, 256), (256, 512), (512, 1 << 20))):
            break
    else:
        pytest.fail("no scene with a TP in each of three scan chunks")
    print(f"[chunks] seed {seed}: class {c} has {rows[c].size} records, TP ranks {tp_rank.tolist()}")
    for metric in (True, False):
        cpu, dev = _pair(E, L, parts, [(0, 2), (2, 4), (4, 6)], num_classes=3, use_07_metric=metric, max_images=6, top_k=200)
        ca, cb = assert_same_state(dev, cpu, f"three updates metric {metric}")
        assert_same_ap(ca, cb, metric, f"three updates metric {metric}")


def test_exact_score_ties_on_the_device(mods):
    """Equal scores within an image, across images of one update and across updates resolve by the ordinal, and equal IoUs by the lower ground-truth index, on
    the device as on the CPU."""
    E, L = mods
    box, far = [10.0, 10.0, 50.0, 50.0], [200.0, 200.0, 240.0, 240.0]
    det = torch.zeros(3, 2, 4, 5)
    det[0, 1, :3] = torch.tensor([[0.5] + far, [0.5] + box, [0.5] + box])
    det[1, 1, 1:3] = torch.tensor([[0.5] + box, [0.5] + box])
    det[2, 1, :2] = torch.tensor([[0.5] + box, [0.5] + far])
    gt = torch.tensor([box + [0.0]]).repeat(3, 1, 1)
    parts = [det, gt, torch.zeros(3, 1, dtype=torch.bool), torch.ones(3, 1, dtype=torch.bool), None]
    cpu, dev = _pair(E, L, parts, [(0, 2), (2, 3)], num_classes=2, max_images=4, top_k=4)
    ca, cb = assert_same_state(dev, cpu, "ties")
    assert_same_ap(ca, cb, True, "ties")
    rec = dev.sorted_records()[1].cpu().numpy().view(np.uint64)
    rec = rec[rec != 0]
    assert ((~(rec >> np.uint64(2))) & np.uint64(E.ORD_MASK)).tolist() == [0, 1, 2, 5, 6, 8, 9]
    assert (rec & np.uint64(3)).tolist() == [2, 1, 2, 1, 2, 1, 2]
    # two identical ground-truth boxes tie on the IoU itself: the lowest index is taken, whichever of the two is the difficult one
    parts, want = twin_case()
    cpu, dev = _pair(E, L, parts, [(0, 2)], num_classes=2, max_images=2, top_k=4)
    ca, cb = assert_same_state(dev, cpu, "identical boxes")
    assert_same_ap(ca, cb, True, "identical boxes")
    rec = dev.sorted_records()[1].cpu().numpy().view(np.uint64)
    assert (rec[rec != 0] & np.uint64(3)).tolist() == want["flags"] and int(ca["npos"][1]) == want["npos"]


def test_update_captures_into_a_graph(mods):
    """One update recorded into a HIP graph and replayed on three batches written into the captured buffers equals three eager updates: the count of images seen
    lives in device memory and advances there."""
    E, L = mods
    parts, _ = _scene(seed=500, N=6, C=5, K=40, G=8, offset=0.0)
    kw = dict(num_classes=5, max_images=8, top_k=40)
    eager = E.VOCEvaluator(device="cuda", **kw)
    for lo in (0, 2, 4):
        _update(L, eager, [p[lo:lo + 2] for p in parts])
    ev = E.VOCEvaluator(device="cuda", **kw)
    static = [p[:2].clone().cuda() for p in parts]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture
        ev.update(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    L.CALL_LOG = []
    try:
        with torch.cuda.graph(graph):
            ev.update(*static)
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    assert log == ["frost_voc_update"], log
    assert int(ev.compute()["ndet"].sum()) == 0, "capture must not execute"
    for lo in (0, 2, 4):
        for s, p in zip(static, parts):
            s.copy_(p[lo:lo + 2])
        graph.replay()
    torch.cuda.synchronize()
    ca, cb = assert_same_state(ev, eager, "graph replay vs eager")
    assert_same_ap(ca, cb, True, "graph replay vs eager")
    assert int(ca["tp"].sum()) > 0 and int(ev._ctr[2 * 5]) == 6


def test_evaluation_is_deterministic(mods):
    E, L = mods
    parts, _ = _scene(seed=600, N=5, C=21, K=40, G=8, offset=0.0)
    outs = []
    for _ in range(2):
        ev = E.VOCEvaluator(device="cuda", num_classes=21, use_07_metric=False, max_images=8, top_k=40)
        _update(L, ev, [p[:3] for p in parts])
        _update(L, ev, [p[3:] for p in parts])
        out = ev.compute()
        outs.append((ev.sorted_records().cpu(), out["ap"].cpu().numpy().tobytes(), out["mean_ap"].cpu().numpy().tobytes()))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert int((outs[0][0] != 0).sum()) > 0


def test_overflow_is_flagged_and_stays_in_bounds(mods):
    """capacity below the records of one class: compute() raises, the guard region behind the record rows is untouched, the other classes' state is right."""
    E, L = mods
    parts, _ = _scene(seed=700, N=4, C=4, K=40, G=8, offset=0.0, fill=0.5)
    per_class = (parts[0][..., 0] > 0).sum((0, 2))
    big = int(per_class.argmax())
    cap = int(per_class[big]) - 5
    assert cap >= int(per_class[[c for c in range(4) if c != big]].max()), per_class
    kw = dict(num_classes=4, max_images=4, top_k=40, capacity=cap)
    cpu = E.VOCEvaluator(**kw)
    cpu.update(*parts)
    dev = E.VOCEvaluator(device="cuda", **kw)
    guard = 4096
    arena = torch.full((4 * cap + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    dev._records = arena[:4 * cap].view(4, cap)
    dev.reset()
    _update(L, dev, parts)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="overflow"):
        dev.compute()
    with pytest.raises(RuntimeError, match="overflow"):
        cpu.compute()
    assert bool((arena[4 * cap:] == 0x5A5A5A5A5A5A5A5A).all()), "a record was written behind the rows"
    want, got = cpu.sorted_records(), dev.sorted_records().cpu()
    ctr = dev._ctr.cpu()
    assert int((got[big] != 0).sum()) == cap and int(ctr[big]) == int(per_class[big]) and int(ctr[2 * 4 + 1]) == 1
    for c in range(4):
        if c != big:
            assert torch.equal(got[c], want[c]), c
            assert int(ctr[c]) == int(per_class[c]) and int(ctr[4 + c]) == int(cpu._npos[c])
    # more images than max_images: flagged as well, nothing written for them
    dev2 = E.VOCEvaluator(device="cuda", num_classes=4, max_images=3, top_k=40)
    _update(L, dev2, parts)
    with pytest.raises(RuntimeError, match="overflow"):
        dev2.compute()


def _explain(c, rec_dev, rec_cpu, fed, gt, valid, sizes, top_k):
    """One differing record of class c (bkg_label 0, det_offset 0) with the fp32 IoUs its flag was decided on, in the definition's operation order."""
    f32 = np.float32
    rec = rec_dev or rec_cpu
    ordinal = ~(rec >> 2) & 0x3FFFFFFF
    img, row = divmod(ordinal, top_k)
    b, n = divmod(img, fed[0].shape[0])
    d = fed[b][n, c, row].numpy()
    box = d[1:] * np.tile(sizes[n].numpy(), 2)
    ious = []
    for j in np.nonzero(valid[n].numpy() & (gt[n, :, 4].numpy().astype(np.int64) == c - 1))[0]:
        g = gt[n, j, :4].numpy()
        inter = max(min(g[2], box[2]) - max(g[0], box[0]), f32(0)) * max(min(g[3], box[3]) - max(g[1], box[1]), f32(0))
        ious.append((int(j), float(inter / ((box[2] - box[0]) * (box[3] - box[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter))))
    return (f"class {c} batch {b} image {n} row {row} score {float(d[0])!r}: device record {rec_dev:#018x} (flag {rec_dev & 3}), CPU {rec_cpu:#018x} "
            f"(flag {rec_cpu & 3}); fp32 IoU per ground-truth row {[(j, repr(v)) for j, v in ious]}")


def test_val_detector_end_to_end(mods):
    """SSDLite-FrostNet-Small at 128 x 128, B = 3, randomised BatchNorm: harness.val_detector on the device equals the CPU definition fed the same device
    detections copied to the host.  Flags may depend on fp32 IoU here; both sides compute it in the same fp32 order, so the counts must be equal."""
    E, L = mods
    from frostnet_amd import harness
    from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for
    torch.manual_seed(19)
    model = SSDLiteFrostNet(mode="small", cfg=ssd_cfg_for(128))
    g = torch.Generator().manual_seed(21)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=g) * 0.8 + 0.6
            m.bias.data = torch.rand(m.num_features, generator=g) * 0.2 - 0.1
            m.running_mean.data = torch.randn(m.num_features, generator=g) * 0.1
            m.running_var.data = torch.rand(m.num_features, generator=g) * 0.5 + 0.5
    model.eval().cuda()
    x = torch.randn(2, 3, 3, 128, 128, generator=torch.Generator().manual_seed(3))
    probe = model.hip_detect_bf16(x[0].cuda(), 200, 0.01, 0.45).cpu()
    assert int((probe[..., 0] > 0).sum()) > 50, "conf_thresh 0.01 leaves no detections to score"
    # ground truth: a few detected boxes (so matches exist), one of them difficult, plus boxes that match nothing; image 2 of every batch has none
    gt = torch.zeros(3, 6, 5)
    difficult, valid = torch.zeros(3, 6, dtype=torch.bool), torch.zeros(3, 6, dtype=torch.bool)
    for n in range(2):
        g = 0
        for c in (1 + n, 7, 15):
            rows = probe[n, c][probe[n, c, :, 0] > 0]
            if rows.shape[0]:
                gt[n, g, :4], gt[n, g, 4] = rows[rows.shape[0] // 2, 1:] * 128.0, c - 1
                difficult[n, g], valid[n, g] = c == 7, True
                g += 1
        gt[n, 5] = torch.tensor([3.0, 5.0, 20.0, 30.0, 4.0])
        valid[n, 5] = True
    sizes = torch.full((3, 2), 128.0)
    loader = [(x[0], gt, difficult, valid, sizes), (x[1], gt, difficult, valid, sizes)]

    class Spy(E.VOCEvaluator):
        def update(self, detections, *rest):
            self.fed.append(detections.cpu())
            super().update(detections, *rest)

    dev = Spy(device="cuda", max_images=6, top_k=200)
    dev.fed = []
    mean_ap, aps = harness.val_detector(loader, model, dev, top_k=200, conf_thresh=0.01, nms_thresh=0.45)
    assert len(dev.fed) == 2 and dev.fed[0].shape == (3, 21, 200, 5) and torch.equal(dev.fed[0], probe)
    cpu = E.VOCEvaluator(max_images=6, top_k=200)
    for det in dev.fed:
        cpu.update(det, gt, difficult, valid, sizes)
    ca, cb = dev.compute(), cpu.compute()
    for name in ("npos", "ndet", "tp", "fp", "ignored"):
        if not torch.equal(ca[name].cpu(), cb[name]):
            ra, rb = dev.sorted_records().cpu(), cpu.sorted_records()
            bad = (ra != rb).nonzero()[:4].tolist()
            pytest.fail(f"{name}: device {ca[name].tolist()} vs CPU {cb[name].tolist()}; first differing records: "
                        + "; ".join(_explain(c, int(ra[c, r]), int(rb[c, r]), dev.fed, gt, valid, sizes, 200) for c, r in bad))
    assert_same_state(dev, cpu, "val_detector")
    assert_same_ap(ca, cb, True, "val_detector")
    assert len(aps) == 21 and np.isnan(aps[0]) and aps[1:] == cb["ap"][1:].tolist()
    assert same_or_both_nan(mean_ap, float(cb["mean_ap"])) or abs(mean_ap - float(cb["mean_ap"])) <= 1e-12
    assert int(cb["tp"].sum()) > 0 and int(cb["ignored"].sum()) > 0 and int(cb["fp"].sum()) > 0

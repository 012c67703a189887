"""The SSD Detect layer on the device (csrc/frost_detect.hip: softmax + decode, radix-select top-k, ballot-word NMS) against
  1. the reference's test phase recorded in g15 (tools/gen_golden.py: torch.softmax + Detect of Object_Detection/layers/functions/detection.py),
  2. Detect.forward_torch on the CPU over a grid of shapes, on scenes with decision margins built at test time (tests/detect_scenes.py),
and the plumbing: SSDLiteFrostNet.detect on the four model variants, capture into a HIP graph, run-to-run determinism.
Criteria of 1 and 2: identical kept rows in identical order, equal counts, values within 1e-5 + 1e-5 |ref| (test_detect_golden.assert_same_detections)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_scenes as D  # noqa: E402
from test_detect_golden import T, assert_same_detections, golden_case  # noqa: E402

pytestmark = pytest.mark.gpu

RES_OF_P = {1536: 128, 24528: 512, 878: 96}          # priors of ssd_cfg_for(res); 878 = 13 * 64 + 46


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib, frostnet, ssdlite
    assert ssdlite._DETECT_HIP, "FROST_DETECT_HIP=0 selects the torch stages: these tests are about the HIP kernels"
    return frostnet, ssdlite, _lib


def _hip(S, L, det, loc, conf, pri):
    """det on the device, with the proof that the HIP entry ran."""
    L.CALL_LOG = []
    try:
        out = det(loc.cuda(), conf.cuda(), pri.cuda())
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    torch.cuda.synchronize()
    assert log == ["frost_detect_forward"], log
    assert out.is_cuda and det.last_counts.is_cuda and det.last_counts.dtype == torch.int32
    return out, det.last_counts


@pytest.mark.parametrize("case", [0, 1])
def test_hip_detect_vs_reference_golden(mods, golden, case):
    F, S, L = mods
    loc, conf, pri, cfg, top_k, ref, ref_counts = golden_case(golden("g15_detect"), case)
    det = S.Detect(21, 0, top_k, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    out, counts = _hip(S, L, det, loc, conf, pri)
    assert_same_detections(out, counts, ref, ref_counts, f"HIP vs g15 case {case}")


# (C, P, N, top_k): every listed value of each axis occurs; 24 528 priors only where listed
GRID = [(21, 1536, 1, 40), (21, 24528, 5, 200), (2, 878, 5, 512), (81, 1536, 5, 1), (81, 24528, 1, 512), (2, 24528, 1, 200), (21, 878, 1, 200),
        (81, 878, 5, 40), (2, 1536, 5, 40)]


@pytest.mark.parametrize("c,p,n,top_k", GRID)
def test_hip_detect_vs_forward_torch_grid(mods, c, p, n, top_k):
    F, S, L = mods
    torch.set_num_threads(16)
    cfg = S.ssd_cfg_for(RES_OF_P[p])
    pri = S.prior_boxes(cfg)
    assert pri.shape[0] == p
    few = (c, p, top_k) == (2, 878, 512)                    # the case whose top_k exceeds the number of candidates of every (image, class)
    loc, conf, info = D.find_scene(pri.numpy(), n, c, top_k, cfg["min_dim"], seed0=100 + 37 * GRID.index((c, p, n, top_k)), tries=32,
                                   require=(lambda m: 0 < m["ncand"].max() < top_k) if few else None)
    print(f"[scene C={c} P={p} N={n} top_k={top_k}] seed {info['seed']}, margins {info['m_thresh']:.2e} / {info['m_gap']:.2e} / {info['m_iou']:.2e}, "
          f"most candidates {int(info['ncand'].max())}, pairs over top_k {info['pairs_over_top_k']}, empty {info['pairs_empty']} of {info['pairs']}")
    loc, conf = T(loc), T(conf)
    det = S.Detect(c, 0, top_k, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    ref = det.forward_torch(loc, conf, pri)
    ref_counts = det.last_counts
    assert int(ref_counts.sum()) > 0
    out, counts = _hip(S, L, det, loc, conf, pri)
    assert_same_detections(out, counts, ref, ref_counts, f"HIP vs forward_torch C={c} P={p} N={n} top_k={top_k}")


def test_hip_detect_ties_and_top_k_cap(mods):
    """Exact ties (duplicated rows, as quantised models produce them) across the top_k boundary: lower prior index first, on the device as on the CPU;
    top_k above the kernel's cap is refused with the cap in the message."""
    F, S, L = mods
    cfg = S.ssd_cfg_for(128)
    pri = S.prior_boxes(cfg)
    g = torch.Generator().manual_seed(9)
    levels = torch.tensor([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0])
    conf = levels[torch.randint(0, 6, (3, pri.shape[0], 3), generator=g)]          # six logit levels only: identical rows, scores tie in their hundreds
    conf[..., 0] = 2.0
    loc = torch.zeros(3, pri.shape[0], 4)                                           # boxes = priors exactly on both sides, so the IoUs are the same bits on both sides
    for top_k in (1, 64, 200):
        det = S.Detect(3, 0, top_k, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
        ref = det.forward_torch(loc, conf, pri)
        ref_counts = det.last_counts
        out, counts = _hip(S, L, det, loc, conf, pri)
        assert torch.equal(counts.cpu(), ref_counts)
        assert torch.equal(out.cpu()[..., 1:], ref[..., 1:]), "ties resolved differently from the CPU definition"        # boxes: exact (loc = 0)
        assert float((out.cpu()[..., 0] - ref[..., 0]).abs().max()) <= 1e-5
    cap = L.load_library().frost_detect_max_top_k()
    assert cap >= 512
    with pytest.raises(ValueError, match=str(cap)):
        S.Detect(3, 0, cap + 1, 0.01, 0.45, cfg["variance"], cfg["min_dim"])(loc.cuda(), conf.cuda(), pri.cuda())


def _variants(F, S):
    """The four ways model(x) returns (loc, conf, priors) on the device, Small at 128 x 128."""
    def base(seed):
        torch.manual_seed(seed)
        return S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128))

    def calibrated(seed):
        m = base(seed)
        F.qat_prepare(m, version=0)
        m.cuda().train()
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for _ in range(2):
                m(torch.randn(4, 3, 128, 128, generator=g).cuda())
        return m

    yield "float bf16", base(21).cuda().eval()
    m = base(22)
    m.float_precision = "fp32"
    yield "float fp32", m.cuda().eval()
    m = calibrated(23)
    m.apply(torch.quantization.disable_observer)             # as the reference evaluates a QAT model: enabled observers keep moving in eval forwards, call after call
    yield "qat", m.eval()
    m = calibrated(24)
    m.hip_convert()
    yield "converted", m.eval()


def test_model_detect_is_detect_of_model_outputs(mods):
    F, S, L = mods
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    seen = []
    for name, model in _variants(F, S):
        keys = list(model.state_dict().keys())
        with torch.no_grad():
            loc, conf, pri = model(x)
        assert loc.is_cuda and loc.shape == (2, 1536, 4) and conf.shape == (2, 1536, 21)
        det = S.Detect(21, 0, 200, 0.01, 0.45, model.cfg["variance"], model.cfg["min_dim"])
        want = det(loc, conf, pri)
        got = model.detect(x)
        assert got.shape == (2, 21, 200, 5) and not got.requires_grad
        assert torch.equal(got, want), name
        got50 = model.detect(x, top_k=50, conf_thresh=0.05, nms_thresh=0.3)
        want50 = S.Detect(21, 0, 50, 0.05, 0.3, model.cfg["variance"], model.cfg["min_dim"])(loc, conf, pri)
        assert got50.shape == (2, 21, 50, 5) and torch.equal(got50, want50), name
        assert list(model.state_dict().keys()) == keys and not any(isinstance(m, S.Detect) for m in model.modules()), name
        seen.append(name)
    assert seen == ["float bf16", "float fp32", "qat", "converted"]
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128)).cuda().train()
    with pytest.raises(RuntimeError, match="eval"):
        model.detect(x)


def _scene(S, seed0):
    cfg = S.ssd_cfg_for(128)
    pri = S.prior_boxes(cfg)
    loc, conf, _ = D.find_scene(pri.numpy(), 3, 21, 200, cfg["min_dim"], seed0=seed0, tries=32)
    return cfg, pri, T(loc), T(conf)


def test_detect_captures_into_a_graph(mods):
    """Fixed launch shapes, no host synchronisation: the layer records on a single stream and replays on fresh inputs bit for bit; only frost_detect_* ran."""
    F, S, L = mods
    cfg, pri, loc_a, conf_a = _scene(S, 500)
    _, _, loc_b, conf_b = _scene(S, 600)
    det = S.Detect(21, 0, 200, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    pri_d, loc_s, conf_s = pri.cuda(), loc_a.cuda(), conf_a.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture (library load, function attributes, allocator pool)
        det(loc_s, conf_s, pri_d)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    L.CALL_LOG = []
    try:
        with torch.cuda.graph(graph):
            out_s = det(loc_s, conf_s, pri_d)
            counts_s = det.last_counts
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    assert log and all(name.startswith("frost_detect_") for name in log), log
    for loc, conf in ((loc_b, conf_b), (loc_a, conf_a)):
        loc_s.copy_(loc)
        conf_s.copy_(conf)
        graph.replay()
        torch.cuda.synchronize()
        got, got_counts = out_s.clone(), counts_s.clone()
        want = det(loc.cuda(), conf.cuda(), pri_d)
        assert torch.equal(got, want) and torch.equal(got_counts, det.last_counts)
        assert int(got_counts.sum()) > 0


def test_detect_is_deterministic(mods):
    F, S, L = mods
    cfg, pri, loc, conf = _scene(S, 700)
    det = S.Detect(21, 0, 200, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    a, ca = _hip(S, L, det, loc, conf, pri)
    b, cb = _hip(S, L, det, loc, conf, pri)
    assert torch.equal(a, b) and torch.equal(ca, cb) and int(ca.sum()) > 0

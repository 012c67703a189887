"""The converted int8 detector's inference path: the fused prediction-head kernel (csrc/frost_iheadq.hip, frost_cvt_head) and the placement pass (frost_cvt_place)
against the layer launches they replace, SSDLiteFrostNet.hip_infer_int8 / hip_detect_int8 against model(x) / model.detect(x) and against stock torch's converted CPU
model, hipGraph capture, harness.val_detector and the guards.

Everything is integer arithmetic plus identical fp32 expressions: EVERY comparison is bit equality (torch.equal), there are no tolerances."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_BUILT = []


def _build():
    if not _BUILT:
        import __graft_entry__ as ge
        ge.build()
        _BUILT.append(1)


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=g) * 0.8 + 0.6
            m.bias.data = torch.rand(m.num_features, generator=g) * 0.2 - 0.1
            m.running_mean.data = torch.randn(m.num_features, generator=g) * 0.1
            m.running_var.data = torch.rand(m.num_features, generator=g) * 0.5 + 0.5


# ------------------------------------------------------------------------------------------------ head kernel / placement against the layer launches
class _HeadPair(torch.nn.Module):
    """The two SepHeads of one SSD source, QAT-preparable like the detector (fuse_model of frostnet._FrostBase)."""

    def __init__(self, cin, cout_loc, cout_conf):
        super().__init__()
        from frostnet_amd.ssdlite import SepHead
        self.loc, self.conf = SepHead(cin, cout_loc), SepHead(cin, cout_conf)

    def fuse_model(self):
        from frostnet_amd.frostnet import ConvBN, ConvBNReLU
        for m in self.modules():
            if type(m) in (ConvBNReLU, ConvBN):
                m.fuse_model()


def _bound_heads(cin, A, C, backend):
    """QAT-prepared SepHeads with randomised BatchNorm, bound the way SSDRunner binds them (`_conv_layer`: qrecord rows aliased by the modules' observer buffers)
    and converted (Engine.prepare_converted, as FrostRunner.convert); the 'fbgemm' records stay 7-bit (reduce_range: quant_max 127), so the `lowq` cap is live."""
    from frostnet_amd import frostnet as F
    from frostnet_amd.engine import Engine, QArena
    from frostnet_amd.runner import SSDRunner
    dev = torch.device("cuda")
    torch.manual_seed(2000 + cin + A)
    conf_pad = (A * C + 7) // 8 * 8
    pair = _HeadPair(cin, 4 * A, conf_pad)
    for m in pair.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, mode="fan_out")
    _randomize_bn(pair, 91 + cin)
    F.qat_prepare(pair, version=0, backend=backend)
    pair.to(dev).eval()
    r = SSDRunner.__new__(SSDRunner)
    r.model = types.SimpleNamespace(ANCHORS=[A], num_classes=C, training=False)
    r.device, r.E, r.qa, r.rule127 = dev, Engine(dev), QArena(32, dev), False
    layers = (r._conv_layer("loc.dw", pair.loc.dw, "dw"), r._conv_layer("loc.pw", pair.loc.pw, "pw"),
              r._conv_layer("conf.dw", pair.conf.dw, "dw"), r._conv_layer("conf.pw", pair.conf.pw, "pw"))
    r.E.rule127 = 1 if r.rule127 else 0
    fb = backend == "fbgemm"
    assert all(l.per_channel == fb for l in layers)
    r.E.prepare_converted(observe=True)
    r.converted, r.converted_fb = True, fb
    r.q_x = r.qa.alloc()
    return r, pair, layers


def _float_stage(seq, x):
    """fp32 value of a fused QAT ConvBn(ReLU)2d on x with its running statistics (only used to CHOOSE records; nothing is compared against it)."""
    m = seq.conv[0]
    y = torch.nn.functional.conv2d(x, m.weight, None, m.stride, m.padding, 1, m.groups)
    y = (y - m.bn.running_mean[None, :, None, None]) * torch.rsqrt(m.bn.running_var + m.bn.eps)[None, :, None, None] * m.bn.weight[None, :, None, None] \
        + m.bn.bias[None, :, None, None]
    return torch.relu(y) if type(m).__name__ == "ConvBnReLU2d" else y


def _set_records(r, pair, layers, xr, qmax):
    """Records narrow enough that outputs saturate at both ends: the depthwise (ReLU) records reach their top index at the 85 % quantile of the layer's fp32 output
    (the bottom is the ReLU floor), the linear 1x1 records span the 15 % .. 85 % quantiles.  Written in place into the qrecord rows (the coefficient cache is keyed
    on their version counter)."""
    from frostnet_amd.engine import QArena
    for hd, dw, pw in ((pair.loc, layers[0], layers[1]), (pair.conf, layers[2], layers[3])):
        yd = _float_stage(hd.dw, xr)
        top = float(torch.quantile(yd.flatten()[:200000], 0.85))
        sd = max(top, 1e-3) / qmax
        QArena.set_qparams(dw.qy, sd, 0)
        yp = _float_stage(hd.pw, yd.clamp(max=sd * qmax))
        lo, hi = (float(v) for v in torch.quantile(yp.flatten()[:200000], torch.tensor([0.15, 0.85], device=yp.device)))
        sp = max(hi - lo, 1e-3) / qmax
        QArena.set_qparams(pw.qy, sp, min(max(int(round(-lo / sp)), 0), qmax))


CASES = [(40, 5, 3, 4, 21, 4, 4, 2), (96, 1, 1, 6, 21, 5, 3, 3), (512, 2, 2, 6, 21, 5, 3, 2), (320, 16, 16, 6, 21, 4, 4, 2), (72, 7, 9, 4, 3, 4, 4, 3)]


# cin, h, w, anchors, classes, priors in front of / behind this source in the image row (a second source's region), batch
@pytest.mark.parametrize("backend", ["qnnpack", "fbgemm"])
@pytest.mark.parametrize("cin,h,w,A,C,front,back,n", CASES)
def test_head_kernel_and_placement_equal_layer_launches(cin, h, w, A, C, front, back, n, backend):
    """frost_cvt_head, and conv_converted x 4 + frost_cvt_place x 2, against conv_converted x 4 + frost_dequant_act + SSDLiteFrostNet._assemble (its permute, reshape and
    slice of the padded class channels): partial K blocks of 64 (40, 72, 96, 320), 5 and 8 K blocks, 84 of 88 / 126 of 128 / 12 of 16 stored channels, 1 x 1 and 2 x 2
    maps where almost every tap is padding, ragged pixel tiles across image borders, aligned (16-byte) and unaligned (scalar) stores; input zero points 0, mid-range
    and 255 (zero-point padding and the weight-sum correction), records narrow enough to saturate at both ends, both requantisation forms (the FBGEMM one on 7-bit
    records).  The rows carry sentinel-filled `front` / `back` regions that must survive."""
    _build()
    from frostnet_amd import _lib as L, runner as R
    from frostnet_amd.engine import QArena
    from frostnet_amd.ssdlite import SSDLiteFrostNet
    dev = torch.device("cuda")
    fb = backend == "fbgemm"
    r, pair, layers = _bound_heads(cin, A, C, backend)
    E = r.E
    qmax = 127 if fb else 255
    assert all(int(l.qy[L.Q_QMAX]) == qmax for l in layers)
    assert L.load_library().frost_cvt_head_ok(h, w, cin, layers[1].cout, layers[3].cout) == 1
    g = torch.Generator().manual_seed(cin * 7 + h)
    idx = torch.randint(0, 256, (n, cin, h, w), generator=g, dtype=torch.int32).to(torch.uint8)
    P = front + h * w * A + back
    SENT = -12345.0
    stub = types.SimpleNamespace(ANCHORS=[A], num_classes=C, priors=None)
    old = R._CVT_HEAD
    try:
        for zp in (0, 117, 255):
            sx = 0.02
            QArena.set_qparams(r.q_x, sx, zp)
            xa = E.act_from_indices(idx, r.q_x)
            xr = (idx.to(dev).float() - zp) * sx
            _set_records(r, pair, layers, xr, qmax)
            # the yardstick: the layer launches model(x) runs, Act.dequant and _assemble
            maps = [E.conv_converted(layers[1], E.conv_converted(layers[0], xa, fb), fb), E.conv_converted(layers[3], E.conv_converted(layers[2], xa, fb), fb)]
            for m in maps:                                      # saturation at both ends of the records, in the reference itself
                used = m.indices()
                assert int(used.min()) == 0 and int(used.max()) == qmax, (zp, int(used.min()), int(used.max()))
            want_loc, want_conf, _ = SSDLiteFrostNet._assemble(stub, [m.dequant() for m in maps])
            for mode, entry in (("1", "frost_cvt_head"), ("0", "frost_cvt_place")):
                R._CVT_HEAD = mode
                loc = torch.full((n, P * 4), SENT, device=dev)
                conf = torch.full((n, P * C), SENT, device=dev)
                L.CALL_LOG = []
                try:
                    r._head_converted(0, xa, layers, loc, conf, front, P)
                    log = list(L.CALL_LOG)
                finally:
                    L.CALL_LOG = None
                torch.cuda.synchronize()
                assert log.count(entry) == (1 if mode == "1" else 2) and (mode == "0" or "frost_pw_conv_fwd" not in log), log
                for out, unit, ref in ((loc, 4, want_loc), (conf, C, want_conf)):
                    width, lo = A * unit, front * unit
                    hi = lo + h * w * width
                    assert bool((out[:, :lo] == SENT).all()) and bool((out[:, hi:] == SENT).all()), (entry, zp, "stored outside the source's region")
                    got = out[:, lo:hi].reshape(n, h * w * A, unit)
                    bad = got != ref
                    assert torch.equal(got, ref), (entry, zp, unit, int(bad.sum()), bad.nonzero()[:4].tolist())
                    assert float(got.abs().max()) > 0
    finally:
        R._CVT_HEAD = old
    E.tape = []


def test_head_geometry_predicate():
    _build()
    from frostnet_amd import _lib as L
    ok = L.load_library().frost_cvt_head_ok
    assert ok(64, 64, 40, 16, 88) == 1 and ok(2, 2, 256, 24, 128) == 1
    assert ok(4, 4, 36, 16, 88) == 0                    # Cin no multiple of 8
    assert ok(4, 4, 64, 24, 168) == 0                   # more than ten channel tiles over the two heads
    assert ok(0, 4, 64, 16, 88) == 0


# ------------------------------------------------------------------------------------------------ whole model
_DET = {}


def _make(backend, res=128):
    from frostnet_amd import frostnet as F, ssdlite as S

    def make():
        m = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(res))
        F.qat_prepare(m, version=0, **({"backend": "fbgemm"} if backend == "fbgemm" else {}))
        return m
    return make


def _detector(backend):
    """SSDLite-FrostNet-Small at 128 x 128, calibrated by three train-mode forwards and hip_convert()-ed (tests/test_gpu_convert.py's recipe), B = 2; the yardstick
    model(x) is computed once per backend."""
    if backend not in _DET:
        _build()
        torch.manual_seed(3)
        make = _make(backend)
        model = make().cuda().train()
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for _ in range(3):
                model(torch.randn(4, 3, 128, 128, generator=g).cuda())
        x = torch.randn(2, 3, 128, 128, generator=g)
        keys = list(model.state_dict().keys())
        model.hip_convert()
        with torch.no_grad():
            loc, conf, _ = model(x.cuda())
        _DET[backend] = dict(model=model, make=make, x=x, loc=loc.clone(), conf=conf.clone(), keys=keys)
    return _DET[backend]


@pytest.mark.parametrize("backend", ["qnnpack", "fbgemm"])
def test_infer_int8_equals_model_and_stock_torch(backend):
    d = _detector(backend)
    from frostnet_amd import _lib as L, runner as R
    from test_gpu_convert import _stock_converted_cpu
    model, xd = d["model"], d["x"].cuda()
    old = R._CVT_HEAD
    res = {}
    try:
        for mode in ("1", "0", "auto"):
            R._CVT_HEAD = mode
            L.CALL_LOG = []
            try:
                loc, conf, priors = model.hip_infer_int8(xd)
                log = list(L.CALL_LOG)
            finally:
                L.CALL_LOG = None
            assert priors is model.priors and loc.dtype == torch.float32 and conf.dtype == torch.float32
            assert torch.equal(loc, d["loc"]) and torch.equal(conf, d["conf"]), mode
            assert "frost_dequant_act" not in log
            if mode == "1":
                assert log.count("frost_cvt_head") == 6 and "frost_cvt_place" not in log
            if mode == "0":
                assert log.count("frost_cvt_place") == 12 and "frost_cvt_head" not in log
            res[mode] = (loc, conf)
    finally:
        R._CVT_HEAD = old
    with torch.no_grad():
        loc2, conf2, _ = model(xd)                           # model(x) itself is unchanged by the new path
    assert torch.equal(loc2, d["loc"]) and torch.equal(conf2, d["conf"])
    mc = _stock_converted_cpu(d["make"], model.hip_export_converted(), backend)
    with torch.no_grad():
        loc_c, conf_c, _ = mc(d["x"])
    loc, conf = res["auto"]
    dl, dc = (loc.cpu() - loc_c).abs(), (conf.cpu() - conf_c).abs()
    print(f"[hip_infer_int8 vs stock torch {backend}] loc max |d| {float(dl.max()):.3e} ({float((dl > 0).float().mean()):.2e} differ), "
          f"conf max |d| {float(dc.max()):.3e} ({float((dc > 0).float().mean()):.2e})")
    assert torch.equal(loc.cpu(), loc_c) and torch.equal(conf.cpu(), conf_c)


@pytest.mark.parametrize("backend", ["qnnpack", "fbgemm"])
def test_detect_int8_equals_detect(backend):
    d = _detector(backend)
    model, xd = d["model"], d["x"].cuda()
    for args in ((), (50, 0.05, 0.3)):
        want = model.detect(xd, *args).clone()
        wc = model.__dict__["_detect"][1].last_counts.clone()
        layer = model.__dict__["_detect"][1]
        got = model.hip_detect_int8(xd, *args)
        assert model.__dict__["_detect"][1] is layer             # the Detect object detect() caches
        assert got.shape == (2, 21, args[0] if args else 200, 5)
        assert torch.equal(got, want) and torch.equal(layer.last_counts, wc)
    assert int(wc.sum()) >= 0


def test_graph_capture():
    """One eager call fills the coefficient cache; then hip_detect_int8 records on one stream (no finalize launch, no host synchronisation) and replays on new input
    contents."""
    d = _detector("qnnpack")
    from frostnet_amd import _lib as L
    model, x = d["model"], d["x"].cuda()
    torch.manual_seed(5)
    xs = [torch.randn_like(x), torch.randn_like(x) * 0.5 + 0.2]
    eager = [model.hip_detect_int8(v).clone() for v in [x] + xs][1:]
    assert not torch.equal(eager[0], eager[1])
    static = x.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    L.CALL_LOG = []
    try:
        with torch.cuda.stream(s):
            model.hip_detect_int8(static)                       # warm-up on the capture stream
            del L.CALL_LOG[:]
            with torch.cuda.graph(g, stream=s):
                out = model.hip_detect_int8(static)
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    torch.cuda.current_stream().wait_stream(s)
    assert log.count("frost_cvt_head") + log.count("frost_cvt_place") // 2 == 6 and "frost_detect_forward" in log, log
    assert not [e for e in log if e.startswith("frost_conv_finalize") or e == "frost_dequant_act" or e == "frost_weight_prep"], log
    for v, want in zip(xs, eager):
        static.copy_(v)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    first = out.clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)                              # two replays are identical


def test_val_detector_routes_through_int8_path():
    """harness.val_detector on a converted model: the detections fed to the evaluator come from hip_detect_int8 and equal model.detect's, so the AP values are those
    of feeding model.detect outputs to the same evaluator."""
    d = _detector("qnnpack")
    from frostnet_amd import _lib as L, harness
    from frostnet_amd.voc_eval import VOCEvaluator
    model = d["model"]
    x = torch.randn(2, 2, 3, 128, 128, generator=torch.Generator().manual_seed(8))
    thr = 0.02
    probe = [model.detect(x[b].cuda(), 200, thr, 0.45).clone() for b in range(2)]
    gt = torch.zeros(2, 4, 5)
    difficult, valid = torch.zeros(2, 4, dtype=torch.bool), torch.zeros(2, 4, dtype=torch.bool)
    for n in range(2):
        gi = 0
        for c in range(1, 21):
            rows = probe[0][n, c][probe[0][n, c, :, 0] > 0].cpu()
            if rows.shape[0] and gi < 3:
                gt[n, gi, :4], gt[n, gi, 4] = rows[0, 1:] * 128.0, c - 1
                valid[n, gi] = True
                gi += 1
        gt[n, 3] = torch.tensor([3.0, 5.0, 20.0, 30.0, 4.0])
        valid[n, 3] = True
    sizes = torch.full((2, 2), 128.0)
    loader = [(x[0], gt, difficult, valid, sizes), (x[1], gt, difficult, valid, sizes)]
    want_ev = VOCEvaluator(device="cuda", max_images=4, top_k=200)
    for det in probe:
        want_ev.update(det, gt.cuda(), difficult.cuda(), valid.cuda(), sizes.cuda())
    want = want_ev.compute()
    ev = VOCEvaluator(device="cuda", max_images=4, top_k=200)
    L.CALL_LOG = []
    try:
        mean_ap, aps = harness.val_detector(loader, model, ev, top_k=200, conf_thresh=thr, nms_thresh=0.45)
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    assert "frost_dequant_act" not in log and log.count("frost_cvt_head") + log.count("frost_cvt_place") // 2 == 12, "val_detector did not take hip_detect_int8"
    wa = want["ap"].tolist()
    assert len(aps) == 21 and all((a == b) or (a != a and b != b) for a, b in zip(aps, wa)), (aps, wa)
    wm = float(want["mean_ap"])
    assert mean_ap == wm or (mean_ap != mean_ap and wm != wm)


def test_guards():
    d = _detector("qnnpack")
    from frostnet_amd import frostnet as F
    from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for
    model, x = d["model"], d["x"].cuda()
    model.hip_infer_int8(x)
    assert list(model.state_dict().keys()) == d["keys"]          # state_dict() keys unchanged by convert + the new path
    model.train()
    try:
        with pytest.raises(RuntimeError):
            model.hip_infer_int8(x)
        with pytest.raises(RuntimeError):
            model.hip_detect_int8(x)
    finally:
        model.eval()
    with pytest.raises(RuntimeError):
        model.hip_infer_int8(d["x"])                            # input on the host
    q = F.qat_prepare(SSDLiteFrostNet(mode="small", cfg=ssd_cfg_for(128))).cuda().eval()
    flt = SSDLiteFrostNet(mode="small", cfg=ssd_cfg_for(128)).cuda().eval()
    for m in (q, flt):
        with pytest.raises(RuntimeError, match="hip_convert"):
            m.hip_infer_int8(x)
        with pytest.raises(RuntimeError, match="hip_convert"):
            m.hip_detect_int8(x)
    loc, conf, _ = model.hip_infer_int8(x)                      # still serving after the refused calls
    assert torch.equal(loc, d["loc"]) and torch.equal(conf, d["conf"])

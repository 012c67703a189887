"""bf16 inference of the SSDLite detector: the fused prediction-head kernel (csrc/frost_ihead.hip) against the layer launches it replaces, the whole detector
against the fp32 definition of the same module (CPU, stock torch modules), independence of the measured kernel choice, Detect behind it, hipGraph capture, the
feature backbone's taps and the guards.

Tolerances: bf16(fp32 head output) == layer-by-layer bf16 output bit for bit (same tap order, same K order, same rounding points: the contract of the fused
bottleneck kernels, tests/test_gpu_infer.py); whole model <= 3e-2 norm-wise against the fp32 definition and fused-everywhere <= 1e-2 against layer-by-layer
(the bounds of tests/test_gpu_infer.py for bf16 inference)."""
import pytest
import torch

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


def _rel(a, b):
    return float((a - b).norm() / b.norm())


_DET = {}


def _detector():
    """SSDLite-FrostNet-Small @128, B = 3, randomised BN: the model on the GPU, its input and the CPU fp32 forward, made once for the module."""
    if not _DET:
        _build()
        from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for
        torch.manual_seed(19)
        model = SSDLiteFrostNet(mode="small", cfg=ssd_cfg_for(128))
        _randomize_bn(model, 21)
        model.eval()
        x = torch.randn(3, 3, 128, 128)
        with torch.no_grad():
            loc, conf, _ = model(x)
        model.cuda()
        _DET.update(model=model, x=x.cuda(), loc=loc, conf=conf)
    return _DET["model"], _DET["x"], _DET["loc"], _DET["conf"]


# cin, h, w, anchors, classes, priors in front of / behind this source in the image row (a second source's region)
@pytest.mark.parametrize("cin,h,w,A,C,front,back,n", [(40, 5, 3, 4, 21, 4, 4, 2), (96, 1, 1, 6, 21, 5, 3, 3), (512, 2, 2, 6, 21, 5, 3, 2),
                                                      (320, 16, 16, 6, 21, 4, 4, 2), (72, 7, 9, 4, 3, 4, 4, 3)])
def test_head_kernel_equals_layer_launches(cin, h, w, A, C, front, back, n):
    """frost_infer_head against frost_infer_dw + frost_infer_pw of both heads on the same packs: conf 84 of 88 / 126 of 128 stored channels, a 1 x 1 map, K chunking
    (512 = 8 chunks, 320 = 5, 72 / 40: a partial chunk, 72 and 40 no multiple of 32), several pixel tiles with a ragged last one across image borders (16 x 16 x 2,
    7 x 9 x 3 = 189 pixels), aligned (16-byte store) and unaligned (scalar store) offsets.  The row also holds `front` + `back` priors of other sources, filled with a
    sentinel that must survive."""
    _build()
    from frostnet_amd import _lib as L, infer as I
    from frostnet_amd.ssdlite import SepHead
    dev = torch.device("cuda")
    torch.manual_seed(1000 + cin + h)
    conf_pad = (A * C + 7) // 8 * 8
    heads = torch.nn.ModuleList([SepHead(cin, 4 * A), SepHead(cin, conf_pad)])
    for m in heads.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, mode="fan_out")
    _randomize_bn(heads, 77 + cin)
    heads.to(dev).eval()
    lay = [I._ILayer(seq, relu, dev) for hd in heads for seq, relu in ((hd.dw.conv, 1), (hd.pw.conv, 0))]
    arr = (L.FrostIDesc * len(lay))()
    for i, l in enumerate(lay):
        arr[i] = l.desc()
    table = L.struct_to_tensor(arr, dev)
    L.call("frost_infer_weight_prep", L.ptr(table), len(lay), L.stream())
    npix = n * h * w
    x = torch.randn(npix * cin).to(torch.bfloat16)
    xb = torch.zeros(npix * cin + 64, dtype=torch.int16, device=dev)
    xb[: npix * cin] = x.view(torch.int16).to(dev)
    want = []
    for dw, pw in ((lay[0], lay[1]), (lay[2], lay[3])):
        t = torch.empty(npix * cin + 64, dtype=torch.int16, device=dev)
        L.call("frost_infer_dw", L.ptr(xb), L.ptr(dw.pack), L.ptr(dw.biasf), n, h, w, cin, 3, 1, 1, L.ptr(t), L.stream())
        y = torch.empty(npix * pw.cout + 64, dtype=torch.int16, device=dev)
        L.call("frost_infer_pw", L.ptr(t), L.ptr(pw.pack), L.ptr(pw.biasf), npix, cin, pw.cout, 0, L.ptr(y), L.stream())
        want.append(y[: npix * pw.cout].view(torch.bfloat16).view(n, h * w, pw.cout))
    assert L.load_library().frost_infer_head_ok(h, w, cin, 4 * A, C * A) == 1
    P = front + h * w * A + back
    SENT = -12345.0
    loc = torch.full((n, P * 4), SENT, device=dev)
    conf = torch.full((n, P * C), SENT, device=dev)
    L.call("frost_infer_head", L.ptr(xb), L.ptr(lay[0].pack), L.ptr(lay[0].biasf), L.ptr(lay[1].pack), L.ptr(lay[1].biasf), L.ptr(lay[2].pack), L.ptr(lay[2].biasf),
           L.ptr(lay[3].pack), L.ptr(lay[3].biasf), n, h, w, cin, 4 * A, C * A, L.ptr(loc), P * 4, front * 4, L.ptr(conf), P * C, front * C, L.stream())
    torch.cuda.synchronize()
    for out, unit, ref in ((loc, 4, want[0]), (conf, C, want[1])):
        width, lo = A * unit, front * unit
        hi = lo + h * w * width
        assert bool((out[:, :lo] == SENT).all()) and bool((out[:, hi:] == SENT).all()), "stored outside the source's region"
        got = out[:, lo:hi].reshape(n, h * w, width)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0 and not bool((got == SENT).any())
        bad = got.bfloat16() != ref[:, :, :width]
        assert torch.equal(got.bfloat16(), ref[:, :, :width]), (unit, int(bad.sum()), bad.nonzero()[:4].tolist())


def test_detector_vs_fp32_definition():
    """hip_infer_bf16 of the detector against the CPU forward of the same module; the same two errors of the parent's bf16 eval path (model(x): FloatSSDRunner)
    are printed next to them.  Measured on MI355X: see DESIGN.md, "bf16 inference of the detector"."""
    model, x, rloc, rconf = _detector()
    loc, conf, priors = model.hip_infer_bf16(x)
    assert priors is model.priors
    assert loc.shape == rloc.shape and conf.shape == rconf.shape and loc.dtype == torch.float32 and conf.dtype == torch.float32
    e_loc, e_conf = _rel(loc.cpu(), rloc), _rel(conf.cpu(), rconf)
    with torch.no_grad():
        ploc, pconf, _ = model(x)
    print(f"hip_infer_bf16 vs fp32 definition: loc {e_loc:.3e} conf {e_conf:.3e}; model(x) bf16 eval path: loc {_rel(ploc.cpu(), rloc):.3e} conf {_rel(pconf.cpu(), rconf):.3e}")
    assert e_loc <= 3e-2 and e_conf <= 3e-2, (e_loc, e_conf)
    loc2, conf2, _ = model.hip_infer_bf16(x.contiguous(memory_format=torch.channels_last))
    assert torch.equal(loc2, loc) and torch.equal(conf2, conf)


def test_choice_independence_and_head_fallback():
    model, x, _, _ = _detector()
    from frostnet_amd import _lib as L, infer as I
    old, old_head = I._FUSED, I._HEAD_FUSED
    res = {}
    try:
        for mode in (False, True, "auto"):
            I._FUSED = mode
            model.__dict__.pop("_bf16_infer", None)
            loc, conf, _ = model.hip_infer_bf16(x)
            res[mode] = (loc.clone(), conf.clone())
        loc, conf, _ = model.hip_infer_bf16(x)                  # the cached choices
        assert torch.equal(loc, res["auto"][0]) and torch.equal(conf, res["auto"][1])
        I._HEAD_FUSED = False
        L.CALL_LOG = []
        floc, fconf, _ = model.hip_infer_bf16(x)
        log = list(L.CALL_LOG)
    finally:
        I._FUSED, I._HEAD_FUSED = old, old_head
        L.CALL_LOG = None
        model.__dict__.pop("_bf16_infer", None)
    assert torch.equal(res["auto"][0], res[False][0]) and torch.equal(res["auto"][1], res[False][1])
    r_loc, r_conf = _rel(res[True][0], res[False][0]), _rel(res[True][1], res[False][1])
    print(f"fused everywhere vs layer-by-layer: loc {r_loc:.3e} conf {r_conf:.3e}")
    assert r_loc <= 1e-2 and r_conf <= 1e-2, (r_loc, r_conf)
    assert "frost_infer_head" not in log
    assert torch.equal(floc.bfloat16(), res["auto"][0].bfloat16()) and torch.equal(fconf.bfloat16(), res["auto"][1].bfloat16())
    assert torch.equal(floc, floc.bfloat16().float())           # (the fallback's values are the layers' bf16 outputs)


def test_detections():
    model, x, _, _ = _detector()
    from frostnet_amd.ssdlite import Detect
    out = model.hip_detect_bf16(x, top_k=50, conf_thresh=0.02, nms_thresh=0.4)
    counts = model.__dict__["_detect"][1].last_counts
    assert out.shape == (3, model.num_classes, 50, 5) and counts is not None and counts.shape == (3, model.num_classes)
    d = Detect(model.num_classes, 0, 50, 0.02, 0.4, tuple(model.cfg["variance"]), model.cfg["min_dim"])
    want = d(*model.hip_infer_bf16(x))
    assert torch.equal(out, want) and torch.equal(counts, d.last_counts)
    assert int(counts.sum()) > 0 and float(out.abs().max()) > 0
    none = model.hip_detect_bf16(x, conf_thresh=0.9)
    assert none.shape == (3, model.num_classes, 200, 5) and not bool(none.any())
    assert int(model.__dict__["_detect"][1].last_counts.sum()) == 0


def test_graph_capture(monkeypatch):
    """One eager call (measures the bottleneck choices, folds the weights), then the whole hip_detect_bf16 records on one stream and replays on new inputs."""
    model, x, _, _ = _detector()
    from frostnet_amd import _lib as L
    # a training step captured by an earlier test of the same process switches the prep cache off for good (its writes are invisible to the version counters,
    # _lib.RAW_WRITES_CAPTURED); this test is about the cache with no such writer around
    monkeypatch.setattr(L, "RAW_WRITES_CAPTURED", False)
    torch.manual_seed(5)
    xs = [torch.randn_like(x), torch.randn_like(x) * 0.5 + 0.2]
    eager = [model.hip_detect_bf16(v).clone() for v in [x] + xs][1:]
    static = x.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    L.CALL_LOG = []
    try:
        with torch.cuda.stream(s):
            model.hip_detect_bf16(static)                       # warm-up on the capture stream
            del L.CALL_LOG[:]
            with torch.cuda.graph(g, stream=s):
                out = model.hip_detect_bf16(static)
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    torch.cuda.current_stream().wait_stream(s)
    assert log.count("frost_infer_head") == 6 and "frost_infer_weight_prep" not in log and not [e for e in log if e.startswith("frost_float_")], log
    assert "frost_detect_forward" in log
    for v, want in zip(xs, eager):
        static.copy_(v)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_features_backbone():
    _build()
    from frostnet_amd import frostnet_features as FF
    torch.manual_seed(23)
    model = FF.FrostNet(mode="small")
    model._init_weights()
    _randomize_bn(model, 25)
    model.eval()
    x = torch.randn(2, 3, 96, 96)
    with torch.no_grad():
        ref = model(x)
    model.cuda()
    feats = model.hip_infer_bf16(x.cuda())
    assert [f.shape[1] for f in feats] == [24, 40, 96, 320] and len(feats) == 4
    for f, r in zip(feats, ref):
        assert f.shape == r.shape and f.dtype == torch.float32 and f.is_contiguous()
        e = _rel(f.cpu(), r)
        print(f"feature map {tuple(f.shape)}: {e:.3e}")
        assert e <= 3e-2, e


def test_guards_and_classifier_unchanged():
    model, x, _, _ = _detector()
    from frostnet_amd import frostnet as F
    from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for
    torch.manual_seed(31)
    clf = F.MODEL_REGISTRY["frostnet_small_1_0"]()
    _randomize_bn(clf, 33)
    clf.eval().cuda()
    xc = torch.randn(2, 3, 64, 64, device="cuda")
    before = clf.hip_infer_bf16(xc).clone()
    model.__dict__.pop("_bf16_infer", None)
    model.hip_infer_bf16(x)                                     # constructs a detector runner in the same process
    assert torch.equal(clf.hip_infer_bf16(xc), before)
    with pytest.raises(ValueError):
        model.hip_infer_bf16(x.cpu())
    model.train()
    try:
        with pytest.raises(RuntimeError):
            model.hip_infer_bf16(x)
        with pytest.raises(RuntimeError):
            model.hip_detect_bf16(x)
    finally:
        model.eval()
    q = F.qat_prepare(SSDLiteFrostNet(mode="small", cfg=ssd_cfg_for(128))).cuda().eval()
    with pytest.raises(RuntimeError):
        q.hip_infer_bf16(x)
    with pytest.raises(RuntimeError):
        q.hip_detect_bf16(x)

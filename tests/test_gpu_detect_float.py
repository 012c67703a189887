"""The float SSDLite detector on the device (frostnet_amd.float_train.FloatSSDRunner): the StatAssist warm-up phase of the detection recipe
(Object_Detection/qtrainval.py:187-238) and float training in general.  Yardstick: the detector's own stock-module CPU forward (the definition of the
float model), in fp64 for the gates and in fp32 for comparison; MultiBoxLoss.forward_torch on the CPU where a loss is needed.  Gradient parity is driven by
a fixed dense upstream gradient on (loc, conf), so that hard-negative mining cannot change which priors count.  Small @128, B = 4 keeps the 1x1 tail
maps at a BatchNorm count of 4."""
import copy
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import frostnet, ssdlite
    return frostnet, ssdlite


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=g) * 0.8 + 0.6
            m.bias.data = torch.rand(m.num_features, generator=g) * 0.2 - 0.1
            m.running_mean.data = torch.randn(m.num_features, generator=g) * 0.1
            m.running_var.data = torch.rand(m.num_features, generator=g) * 0.5 + 0.5


def _grad_errors(dev_model, ref_model):
    ref = {n: p.grad.double() for n, p in ref_model.named_parameters()}
    out = {}
    for n, p in dev_model.named_parameters():
        a, b = p.grad.detach().cpu().double(), ref[n]
        den = float(b.norm())
        if n.endswith(".conv.1.weight") or n.endswith(".conv.1.bias"):          # BN gamma / beta: against the conv's gradient norm when that is larger
            den = max(den, float(ref[n.rsplit(".conv.1.", 1)[0] + ".conv.0.weight"].norm()))
        out[n] = float((a - b).norm()) / max(den, 1e-30)
    return out


def _flip_budget(ref, run_ref):
    """ReLU-mask flip candidates of the fp64 run (|z| < 3e-6 rms) -> 3 * sqrt(fraction), as tests/test_gpu_float.py counts them."""
    cnt = [0, 0]

    def hook(m, i, o):
        z = i[0].detach()
        cnt[0] += int((z.abs() < 3e-6 * z.pow(2).mean().sqrt()).sum()); cnt[1] += z.numel()
    hs = [m.register_forward_hook(hook) for m in ref.modules() if isinstance(m, torch.nn.ReLU)]
    out = run_ref()
    for h in hs:
        h.remove()
    return out, cnt[0], 3.0 * (cnt[0] / max(cnt[1], 1)) ** 0.5


def _targets(n):
    rng = np.random.Generator(np.random.PCG64(77))
    out = []
    for i in range(n):
        k = 1 + i % 3
        c = rng.random((k, 2)) * 0.5 + 0.25
        wh = rng.random((k, 2)) * 0.3 + 0.1
        boxes = np.concatenate([c - wh / 2, c + wh / 2, rng.integers(0, 20, (k, 1)).astype(np.float64)], 1)
        if i == 0:      # one image-filling object: the coarse maps receive positives as well
            boxes = np.concatenate([boxes, [[0.04, 0.06, 0.97, 0.93, 5.0]]], 0)
        out.append(torch.from_numpy(boxes.astype(np.float32)))
    return out


def _small128(S, seed):
    torch.manual_seed(seed)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128))
    _randomize_bn(model, seed + 1)
    return model


def _dense(loc, conf, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(loc.shape, generator=g), torch.randn(conf.shape, generator=g)


# ------------------------------------------------------------------------------------------------------------------- 1. gather / scatter kernels
@pytest.mark.parametrize("shape", ["small128", "large512"])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ssd_gather_scatter_kernels(mods, shape, prec):
    """frost_float_ssd_gather / _scatter (and _f32) on synthetic NHWC maps shaped like the detector's, read as emitted outputs (the eval form): the gather
    is SSDLiteFrostNet._assemble bit for bit; the scatter is autograd through _assemble, rounded once to the storage type, with exact zeros in the padded conf
    channels; a NULL dloc / dconf gives zero gradients."""
    from frostnet_amd import _lib as L
    F, S = mods
    fmaps = [16, 8, 4, 2, 1, 1] if shape == "small128" else [64, 32, 16, 8, 4, 2]
    n, C = 2, 21
    A = S.SSDLiteFrostNet.ANCHORS
    conf_pad = [(a * C + 7) // 8 * 8 for a in A]
    fake = types.SimpleNamespace(ANCHORS=A, num_classes=C, priors=None)
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    sfx = "" if prec == "bf16" else "_f32"
    g = torch.Generator().manual_seed(31 + len(fmaps) + fmaps[0])
    maps, chans = [], []
    for k, f in enumerate(fmaps):
        for c in (A[k] * 4, conf_pad[k]):
            maps.append((torch.randn(n, f, f, c, generator=g) * 3).to(dt).cuda())       # NHWC in the storage type
            chans.append(c)
    P = sum(f * f * a for f, a in zip(fmaps, A))

    def table(bufs):
        tab = (L.FrostSSDMap * 12)()
        off = 0
        for k, f in enumerate(fmaps):
            for which in (0, 1):
                m, width = tab[2 * k + which], (4 if which == 0 else C)
                m.buf, m.coef, m.hw, m.doff = bufs[2 * k + which].data_ptr(), None, f * f, off * width
                m.stored, m.used, m.cpad, m.which = chans[2 * k + which], A[k] * width, chans[2 * k + which], which
            off += f * f * A[k]
        return tab

    nchw = [m.float().permute(0, 3, 1, 2) for m in maps]
    loc_r, conf_r, _ = S.SSDLiteFrostNet._assemble(fake, [m.cpu() for m in nchw])
    loc = torch.full((n, P, 4), float("nan"), device="cuda")
    conf = torch.full((n, P, C), float("nan"), device="cuda")
    L.call("frost_float_ssd_gather" + sfx, table(maps), 12, n, P * 4, P * C, L.ptr(loc), L.ptr(conf), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(loc.cpu(), loc_r) and torch.equal(conf.cpu(), conf_r)

    dloc, dconf = torch.randn(n, P, 4, generator=g), torch.randn(n, P, C, generator=g)
    leaves = [m.cpu().clone().requires_grad_(True) for m in nchw]
    lr, cr, _ = S.SSDLiteFrostNet._assemble(fake, leaves)
    ((lr * dloc).sum() + (cr * dconf).sum()).backward()
    want = [lf.grad.permute(0, 2, 3, 1).contiguous().to(dt) for lf in leaves]
    dloc_d, dconf_d = dloc.cuda(), dconf.cuda()
    for dl, dc in ((dloc_d, dconf_d), (None, dconf_d), (dloc_d, None)):
        outs = [torch.full_like(m, float("nan")) for m in maps]
        L.call("frost_float_ssd_scatter" + sfx, table(outs), 12, n, P * 4, P * C, L.ptr(dl), L.ptr(dc), L.stream())
        torch.cuda.synchronize()
        for i, (o, w) in enumerate(zip(outs, want)):
            k, which = divmod(i, 2)
            o = o.cpu()
            if (dl if which == 0 else dc) is None:
                assert torch.equal(o, torch.zeros_like(o)), i
            else:
                assert torch.equal(o, w), (i, _rel(o.float(), w.float()))
            if which == 1:
                assert torch.equal(o[..., A[k] * C:], torch.zeros_like(o[..., A[k] * C:]))


# ------------------------------------------------------------------------------------------------------------------- 2. fp32-mode gate
def test_fp32_mode_detector_train_step_vs_fp64(mods):
    """One training step of the float detector in fp32 mode against the fp64 stock-module definition: loc / conf 3e-5 and within 2x of the CPU fp32 run's
    own error (measured 2.1e-5 / 2.0e-5, CPU fp32 1.6e-5 / 1.2e-5); MultiBoxLoss (HIP kernels on the device outputs vs forward_torch on the fp64 outputs)
    1e-5 per term; the gradient of all parameters concatenated 1e-4 + 10x the ReLU-flip budget (measured 2.4e-3 with 14 flip candidates, CPU fp32 3.7e-3);
    eval-mode loc / conf 3e-5.  Running statistics rtol 6e-4 (the classifier's 2e-4 widened): the heads of the 1x1 tail maps take their variance from 4
    values of activations that carry the whole network's round-off, measured 2.7e-4 on loc.5.pw."""
    F, S = mods
    torch.set_num_threads(16)
    model = _small128(S, 21)
    ref, ref32 = copy.deepcopy(model).double().train(), copy.deepcopy(model).train()
    x = torch.randn(4, 3, 128, 128, generator=torch.Generator().manual_seed(3))
    (loc_r, conf_r, pri_r), cands, budget = _flip_budget(ref, lambda: ref(x.double()))
    gl, gc = _dense(loc_r, conf_r)
    ((loc_r * gl.double()).sum() + (conf_r * gc.double()).sum()).backward()
    loc32, conf32, _ = ref32(x)
    ((loc32 * gl).sum() + (conf32 * gc).sum()).backward()
    model.float_precision = "fp32"
    model.cuda().train()
    run = model.hip_runner()
    assert type(run).__name__ == "FloatSSDRunner" and run.precision == "fp32"
    loc, conf, pri = model(x.cuda())
    assert loc.shape == (4, 1536, 4) and conf.shape == (4, 1536, 21) and loc.dtype == torch.float32
    crit = S.MultiBoxLoss(21)
    tg = _targets(4)
    ll, lc = crit((loc.detach(), conf.detach(), pri), tg)
    boxes, valid = S.pad_targets(tg, "cpu")
    ll_r, lc_r = crit.forward_torch(loc_r.detach(), conf_r.detach(), pri_r.double(), boxes.double(), valid)
    ((loc * gl.cuda()).sum() + (conf * gc.cuda()).sum()).backward()
    torch.cuda.synchronize()
    el, ec = _rel(loc.detach().cpu(), loc_r.detach()), _rel(conf.detach().cpu(), conf_r.detach())
    el32, ec32 = _rel(loc32.detach(), loc_r.detach()), _rel(conf32.detach(), conf_r.detach())
    cat = lambda mod: torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in mod.parameters()])
    eg, eg32 = _rel(cat(model), cat(ref)), _rel(cat(ref32), cat(ref))
    print(f"[fp32 detector] loc {el:.1e} conf {ec:.1e} (CPU fp32 {el32:.1e} / {ec32:.1e}); loss_l {float(ll):.6f} vs {float(ll_r):.6f}, loss_c {float(lc):.6f} vs "
          f"{float(lc_r):.6f}; gradient {eg:.1e} (CPU fp32 {eg32:.1e}); {cands} flip candidates, budget {budget:.1e}")
    assert el <= 3e-5 and el <= 2 * el32 + 1e-6, (el, el32)
    assert ec <= 3e-5 and ec <= 2 * ec32 + 1e-6, (ec, ec32)
    assert abs(float(ll) - float(ll_r)) <= 1e-5 * abs(float(ll_r)), (float(ll), float(ll_r))
    assert abs(float(lc) - float(lc_r)) <= 1e-5 * abs(float(lc_r)), (float(lc), float(lc_r))
    assert eg <= 1e-4 + 10 * budget, (eg, budget)
    sd, sr = model.state_dict(), ref.state_dict()
    worst = max(float(((sd[k].cpu().double() - sr[k]).abs() / (sr[k].abs() + 1e-30)).max()) for k in sr if k.endswith("running_var"))
    print(f"[fp32 detector] worst running_var relative deviation {worst:.1e}")
    for k in sr:
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd[k].cpu().numpy(), sr[k].float().numpy(), rtol=6e-4, atol=1e-5, err_msg=k)
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    model.eval(); ref.eval()
    with torch.no_grad():
        le, ce, _ = model(x.cuda())
        lr_, cr_, _ = ref(x.double())
    assert _rel(le.cpu(), lr_) <= 3e-5 and _rel(ce.cpu(), cr_) <= 3e-5, (_rel(le.cpu(), lr_), _rel(ce.cpu(), cr_))


# ------------------------------------------------------------------------------------------------------------------- 3. bf16 sanity
def test_bf16_detector_train_step_vs_fp32_definition(mods):
    """Default (bf16 storage) mode, one training step against the fp32 definition, with the classifier's bounds (test_float_train_step_vs_fp32_definition):
    stem output 4e-3, conv-weight gradient-norm ratios (median in [0.8, 1.25], min >= 0.33, max <= 3), the loc.0 / conf.0 head parameters -- the tail of the
    backward, not yet amplified -- 6e-2, every gradient finite.
    Held at 512x512, B = 2 (tail BatchNorm count 8): at 128x128, B = 4 the freshly initialised detector is chaotic at bf16 precision whatever computes it --
    on the CPU, rounding only the 1x1 weights and the input to bf16 moves loc by 1e-1 and the median gradient-norm ratio to 1.93 (the device measures 1.91
    there), while the same CPU experiment at 512x512, B = 2 gives a median of 1.00 (min 0.73, max 1.21); the device measures 1.14 (0.92, 1.63).  The two
    head depthwise weights of source 0 are the one exception to 6e-2 (measured 0.12, bound 0.25): their gradient is the product of the head's dc with the
    source activation itself, which has been through five bf16 bottlenecks; the head's other ten parameters measure <= 2.6e-2."""
    F, S = mods
    torch.manual_seed(41)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small")
    _randomize_bn(model, 42)
    ref = copy.deepcopy(model).train()
    x = torch.randn(2, 3, 512, 512, generator=torch.Generator().manual_seed(4))
    caps = {}
    ref.conv1.register_forward_hook(lambda m, i, o: caps.__setitem__("stem", o.detach()))
    loc_r, conf_r, _ = ref(x)
    gl, gc = _dense(loc_r, conf_r, 6)
    ((loc_r * gl).sum() + (conf_r * gc).sum()).backward()
    model.cuda().train()
    run = model.hip_runner()
    assert type(run).__name__ == "FloatSSDRunner" and run.precision == "bf16"
    dev_caps, orig_conv = {}, run._conv

    def conv(l, a, training, record, out=None, ldy=None, **kw):
        o = orig_conv(l, a, training, record, out, ldy, **kw)
        if l.name == "conv1":
            dev_caps["stem"] = o
        return o
    run._conv = conv
    loc, conf, _ = model(x.cuda())
    ((loc * gl.cuda()).sum() + (conf * gc.cuda()).sum()).backward()
    torch.cuda.synchronize()
    run._conv = orig_conv
    assert _rel(dev_caps["stem"].float().cpu(), caps["stem"]) <= 4e-3
    print(f"[bf16 detector] loc {_rel(loc.detach().cpu(), loc_r.detach()):.2e} conf {_rel(conf.detach().cpu(), conf_r.detach()):.2e}")
    gn = np.array([float(p.grad.double().norm()) for p in model.parameters()])
    gr = np.array([float(p.grad.double().norm()) for p in ref.parameters()])
    assert np.isfinite(gn).all()
    cv = np.array([p.dim() == 4 for p in model.parameters()])
    ratio = gn[cv] / gr[cv]
    assert 0.8 <= np.median(ratio) <= 1.25 and ratio.min() >= 0.33 and ratio.max() <= 3.0, (np.median(ratio), ratio.min(), ratio.max())
    errs = _grad_errors(model, ref)
    tail = {n: e for n, e in errs.items() if n.startswith("loc.0.") or n.startswith("conf.0.")}
    print(f"[bf16 detector] gradient-norm ratio median {np.median(ratio):.3f} min {ratio.min():.3f} max {ratio.max():.3f}; worst loc.0 / conf.0 "
          f"parameter {max(tail.values()):.1e}")
    dww = {n: e for n, e in tail.items() if n.endswith(".dw.conv.0.weight")}
    assert len(tail) == 12 and all(e <= 6e-2 for n, e in tail.items() if n not in dww), tail
    assert all(e <= 0.25 for e in dww.values()), dww


# ------------------------------------------------------------------------------------------------------------------- 4. tiny maps
@pytest.mark.parametrize("h,s", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_float_dw_passes_on_tail_maps(h, s, prec):
    """The detector's 2x2 and 1x1 tail maps: frost_float_dw(_f32) modes 0 / 1, frost_float_dw_dgrad(_f32) and frost_float_dw_wgrad(_f32) at h = w in {1, 2},
    stride 1 and 2, against fp64 conv2d on the same (bf16-rounded for the bf16 mode) operands.  bf16 stores round once (3e-3); fp32: summation order."""
    from frostnet_amd import _lib as L
    k, c, n = 3, 256, 4
    sfx = "" if prec == "bf16" else "_f32"
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    g = torch.Generator().manual_seed(900 + 10 * h + s)
    pad, cpad = 1, c
    ho = (h + 2 * pad - k) // s + 1
    wgt = torch.randn(c, 1, k, k, generator=g) * 0.3
    x = torch.randn(n, c, h, h, generator=g)
    dc = torch.randn(n, c, ho, ho, generator=g)
    if prec == "bf16":
        x, dc = x.bfloat16().float(), dc.bfloat16().float()
    xw = x.double().requires_grad_(True)
    wd = wgt.double().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xw, wd, stride=s, padding=pad, groups=c)
    ref.backward(dc.double())
    refo = ref.detach().permute(0, 2, 3, 1).contiguous()
    pack = torch.zeros(k * k, cpad)
    pack[:, :c] = wgt.reshape(c, k * k).t()
    pack = pack.cuda()
    coef = torch.zeros(8, cpad)
    coef[0] = torch.rand(c, generator=g) + 0.5
    coef[1] = torch.randn(c, generator=g) * 0.3
    coef = coef.cuda()
    stat = torch.zeros(8 * 4 * cpad, dtype=torch.float64, device="cuda")
    d = L.FrostFDesc()
    d.pack, d.coef, d.stat, d.cout, d.cin_g, d.kk, d.kind, d.cpad, d.fp32 = pack.data_ptr(), coef.data_ptr(), stat.data_ptr(), c, 1, k * k, 1, cpad, int(prec == "fp32")
    tab = L.struct_to_tensor(d, "cuda")
    xd = x.permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    dd = dc.permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    cv = torch.full((n, ho, ho, c), float("nan"), dtype=dt, device="cuda")
    y = torch.full((n, ho, ho, c), float("nan"), dtype=dt, device="cuda")
    dx = torch.full((n, h, h, c), float("nan"), dtype=dt, device="cuda")
    dw = torch.zeros(c, k * k, device="cuda")
    L.call("frost_float_dw" + sfx, L.ptr(tab), L.ptr(xd), n, h, h, c, k, s, 1, 0, None, L.ptr(cv), L.stream())
    L.call("frost_float_dw" + sfx, L.ptr(tab), L.ptr(xd), n, h, h, c, k, s, 1, 1, None, L.ptr(y), L.stream())
    L.call("frost_float_dw_dgrad" + sfx, L.ptr(tab), L.ptr(dd), n, h, h, c, k, s, L.ptr(dx), L.stream())
    L.call("frost_float_dw_wgrad" + sfx, L.ptr(dd), L.ptr(xd), n, h, h, c, k, s, L.ptr(dw), L.stream())
    torch.cuda.synchronize()
    tol = 3e-3 if prec == "bf16" else 2e-6
    assert _rel(cv.float().cpu(), refo) <= tol, _rel(cv.float().cpu(), refo)
    yref = torch.relu(refo * coef[0].cpu().double() + coef[1].cpu().double())
    assert _rel(y.float().cpu(), yref) <= tol, _rel(y.float().cpu(), yref)
    sums = stat.view(8, 4, cpad).sum(0).cpu()
    flat = refo.reshape(-1, c)
    assert _rel(sums[0], flat.sum(0)) <= 1e-4 and _rel(sums[1], (flat * flat).sum(0)) <= 1e-4
    assert torch.isfinite(dx.float()).all() and _rel(dx.float().cpu(), xw.grad.permute(0, 2, 3, 1)) <= tol, _rel(dx.float().cpu(), xw.grad.permute(0, 2, 3, 1))
    assert _rel(dw.cpu(), wd.grad.reshape(c, k * k)) <= 2e-5, _rel(dw.cpu(), wd.grad.reshape(c, k * k))


@pytest.mark.parametrize("h,s", [(1, 1), (2, 2)])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_float_pointwise_passes_on_a_few_pixels(mods, h, s, prec):
    """The pointwise statistics / emit / reduce / dc passes (and the depthwise ones) on N*1*1 pixels: a bottleneck teacher-forced at N = 4 with a 1x1 output
    map, against the fp64 stock module.  fp32 mode: fp32 round-off (y 5e-6, dx and parameter gradients 2e-5 + the flip budget; measured 4e-7 .. 1e-6);
    bf16 mode: the well-conditioned block bounds (y 1e-2, dx and parameter gradients 1e-1; measured 9e-3 / 9e-2 / 9e-2 on 16 input pixels) -- on 4 pixels,
    where every BatchNorm of the block averages over 4 values and amplifies the bf16 storage error, twice the measured 1.2e-2 / 2.2e-1 / 1.9e-1."""
    F, S = mods
    from frostnet_amd.float_train import FloatRunner
    torch.manual_seed(12)
    m = F.CascadePreExBottleneck(64, 64 if s == 1 else 96, quantized=False, kernel_size=3, stride=s, expand_ratio=3, reduce_factor=4)
    _randomize_bn(m, 7)
    ref = copy.deepcopy(m).double().train()
    x = torch.randn(4, 64, h, h)
    xr = x.double().requires_grad_(True)
    yr, cands, budget = _flip_budget(ref, lambda: ref(xr))
    gy = torch.randn(yr.shape)
    yr.backward(gy.double())
    m.cuda().train()
    run = FloatRunner.for_block(m, precision=prec)
    y, dx = run.block_step(x.cuda(), gy.cuda())
    torch.cuda.synchronize()
    ey, edx = _rel(y.cpu(), yr.detach()), _rel(dx.cpu(), xr.grad)
    worst = max(_grad_errors(m, ref).values())
    print(f"[{prec} block on {4 * h * h} pixels] y {ey:.1e} dx {edx:.1e} worst grad {worst:.1e}; {cands} flip candidates")
    if prec == "fp32":
        assert ey <= 5e-6 and edx <= 2e-5 + budget and worst <= 2e-5 + budget, (ey, edx, worst, budget)
    elif h == 1:
        assert ey <= 2.5e-2 and edx <= 0.45 and worst <= 0.4, (ey, edx, worst)
    else:
        assert ey <= 1e-2 and edx <= 0.1 and worst <= 0.1, (ey, edx, worst)
    sd, sr = m.state_dict(), ref.state_dict()
    for key in sr:
        if key.endswith("running_mean") or key.endswith("running_var"):
            tol = (1e-5, 1e-6) if prec == "fp32" else (5e-3, 2e-3)
            np.testing.assert_allclose(sd[key].cpu().numpy(), sr[key].float().numpy(), rtol=tol[0], atol=tol[1], err_msg=key)


# ------------------------------------------------------------------------------------------------------------------- 5. StatAssist on the detector
def test_statassist_switch_detector_on_device(mods):
    """Object_Detection/qtrainval.py:187-251 on the GPU: float warm-up steps of the detector with QSGD (is_warmup=True) through MultiBoxLoss, then
    statassist_qat_switch (fuse + prepare_qat with the same Parameter objects and optimizer state) and one fake-quant step on SSDRunner."""
    F, S = mods
    from frostnet_amd import harness as H
    from frostnet_amd.optimizer import QSGD
    torch.manual_seed(2)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128)).cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
    mbox = S.MultiBoxLoss(21)
    crit = lambda out, t: sum(mbox(out, t))
    x = torch.randn(4, 3, 128, 128, device="cuda")
    t = S.pad_targets(_targets(4), "cuda")
    assert opt.is_warmup
    w0 = model.conv1.conv[0].weight.detach().clone()
    losses = []
    for _ in range(3):
        loss, _ = H.train_one_iter(model, crit, opt, x, t)
        losses.append(float(loss))
    assert type(model.hip_runner()).__name__ == "FloatSSDRunner"
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert not torch.equal(w0, model.conv1.conv[0].weight)
    ids = [id(p) for p in model.parameters()]
    steps = [int(opt.state[p]["step"]) for p in model.parameters()]
    H.statassist_qat_switch(model, opt)
    assert not opt.is_warmup and ids == [id(p) for p in model.parameters()]
    loss, _ = H.train_one_iter(model, crit, opt, x, t)
    assert type(model.hip_runner()).__name__ == "SSDRunner"
    assert np.isfinite(float(loss))
    assert [int(opt.state[p]["step"]) for p in model.parameters()] == [s + 1 for s in steps]
    print(f"[statassist detector] float losses {losses}, QAT loss {float(loss):.4f}")


# ------------------------------------------------------------------------------------------------------------------- 6. c5 size
def test_float_detector_c5_size(mods):
    """Config c5's size: Large at 512x512, B = 2, one float training step through MultiBoxLoss; then a dense synthetic loss once -- every parameter tensor
    gets a finite, non-zero gradient."""
    F, S = mods
    torch.manual_seed(0)
    model = S.SSDLiteFrostNet(num_classes=21, mode="large").cuda().train()
    crit = S.MultiBoxLoss(21)
    x = torch.randn(2, 3, 512, 512, device="cuda")
    loc, conf, pri = model(x)
    assert loc.shape == (2, 24528, 4) and conf.shape == (2, 24528, 21)
    ll, lc = crit((loc, conf, pri), _targets(2))
    (ll + lc).backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(ll)) and np.isfinite(float(lc))
    model.zero_grad(set_to_none=True)
    loc, conf, pri = model(x)
    g = torch.Generator(device="cuda").manual_seed(5)
    ((loc * torch.randn(loc.shape, device="cuda", generator=g)).sum() + (conf * torch.randn(conf.shape, device="cuda", generator=g)).sum()).backward()
    torch.cuda.synchronize()
    dead = [n for n, p in model.named_parameters() if p.grad is None or not (np.isfinite(float(p.grad.norm())) and float(p.grad.norm()) > 0)]
    assert not dead, dead


# ------------------------------------------------------------------------------------------------------------------- 7. guards
def test_float_detector_guards(mods):
    """Refusals match stock torch / the float classifier: an eval-mode BatchNorm in a training forward (NotImplementedError), one value per channel in a
    training forward (ValueError: B = 1 at 128 leaves 1x1 tail maps), a CPU tensor handed to the runner.  B = 1 works in eval mode; eval-mode
    forward_maps assembles to forward's (loc, conf); setting float_precision rebinds the runner."""
    F, S = mods
    model = _small128(S, 61).cuda().train()
    x2 = torch.randn(2, 3, 128, 128, device="cuda")
    model.extras[1].dw.conv[1].eval()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        model(x2)
    model.train()
    x1 = torch.randn(1, 3, 128, 128, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model(x1)
    with pytest.raises(ValueError):
        model.hip_runner().forward(x1.cpu())
    loc, conf, _ = model(x2)                                  # B = 2 trains
    assert torch.isfinite(loc).all() and torch.isfinite(conf).all()
    model.eval()
    with torch.no_grad():
        loc, conf, pri = model(x1)
        assert loc.shape == (1, 1536, 4) and torch.isfinite(loc).all() and torch.isfinite(conf).all()
        maps = model.hip_runner().forward_maps(x1)
        la, ca, _ = S.SSDLiteFrostNet._assemble(model, maps)
    assert torch.equal(la, loc) and torch.equal(ca, conf)
    r0 = model.hip_runner()
    model.float_precision = "fp32"
    r1 = model.hip_runner()
    assert r1 is not r0 and type(r1).__name__ == "FloatSSDRunner" and r1.precision == "fp32"

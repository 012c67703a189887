"""The float FrostNet + Lite R-ASPP segmentation network on the device (frostnet_amd.seg_model.FrostNetSeg on frostnet_amd.float_train.FloatSegRunner).  Yardstick:
the model's own stock-module CPU forward (its definition), in fp64 for the gates and in fp32 for comparison, as tests/test_gpu_detect_float.py holds the float
detector; the head alone is held to the reference's own head code through tests/golden/g20_seg_head.npz.  Gradient parity is driven by a seeded dense upstream
gradient on the stride-8 logits."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_kernel_refs as FR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import seg, seg_model
    return seg_model, seg


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
    """Mask flip candidates of the fp64 run -- ReLU inputs with |z| < 3e-6 rms, hard-sigmoid inputs that close to either kink (-3, +3) -> 3 * sqrt(fraction)."""
    cnt = [0, 0]

    def hook(kinks):
        def f(m, i, o):
            z = i[0].detach()
            thr = 3e-6 * z.pow(2).mean().sqrt()
            cnt[0] += sum(int(((z - k).abs() < thr).sum()) for k in kinks); cnt[1] += z.numel()
        return f
    hs = [m.register_forward_hook(hook((0.0,))) for m in ref.modules() if isinstance(m, torch.nn.ReLU)]
    hs += [m.register_forward_hook(hook((-3.0, 3.0))) for m in ref.modules() if type(m).__name__ == "Hsigmoid"]
    assert len(hs) > 10 and any(type(m).__name__ == "Hsigmoid" for m in ref.modules())
    out = run_ref()
    for h in hs:
        h.remove()
    return out, cnt[0], 3.0 * (cnt[0] / max(cnt[1], 1)) ** 0.5


def _small(M, seed, **kw):
    torch.manual_seed(seed)
    model = M.FrostNetSeg(21, "small", **kw)
    _randomize_bn(model, seed + 1)
    return model


X_SHAPE = (4, 3, 129, 161)


def _targets(n, h, w, c=21, seed=8):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, c, (n, h, w), generator=g)
    return torch.where(torch.rand(n, h, w, generator=g) < 0.03, torch.full_like(t, 255), t)          # 3 % ignore


# ------------------------------------------------------------------------------------------------------------------- 1. fp32-mode gate
def test_fp32_mode_train_step_vs_fp64(mods):
    """One training step in fp32 mode against the fp64 stock-module definition: logits 3e-5 and within 2x of the CPU fp32 run's own error + 1e-6; the gradient
    of all parameters concatenated 1e-4 + 10x the flip budget (ReLU and both hard-sigmoid kinks); running statistics rtol max(6e-4, 4x the CPU fp32 run's own worst
    deviation from fp64), atol 1e-5; num_batches_tracked == 1; eval-mode logits 3e-5.  b1's BatchNorm count is 4 * 2 * 2 = 16."""
    M, _ = mods
    torch.set_num_threads(16)
    model = _small(M, 21, pool_kernel=3, pool_stride=2)
    ref, ref32 = copy.deepcopy(model).double().train(), copy.deepcopy(model).train()
    x = torch.randn(*X_SHAPE, generator=torch.Generator().manual_seed(3))
    out_r, cands, budget = _flip_budget(ref, lambda: ref(x.double()))
    assert tuple(out_r.shape) == (4, 21, 17, 21)
    gout = torch.randn(out_r.shape, generator=torch.Generator().manual_seed(5))
    out_r.backward(gout.double())
    out32 = ref32(x)
    out32.backward(gout)
    model.float_precision = "fp32"
    model.cuda().train()
    run = model.hip_runner()
    assert type(run).__name__ == "FloatSegRunner" and run.precision == "fp32"
    out = model(x.cuda())
    assert tuple(out.shape) == (4, 21, 17, 21) and out.dtype == torch.float32 and out.is_contiguous(memory_format=torch.channels_last)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    eo, eo32 = _rel(out.detach().cpu(), out_r.detach()), _rel(out32.detach(), out_r.detach())
    cat = lambda mod: torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in mod.parameters()])
    eg, eg32 = _rel(cat(model), cat(ref)), _rel(cat(ref32), cat(ref))
    print(f"[fp32 seg] logits {eo:.1e} (CPU fp32 {eo32:.1e}); gradient {eg:.1e} (CPU fp32 {eg32:.1e}); {cands} flip candidates, budget {budget:.1e}")
    assert eo <= 3e-5 and eo <= 2 * eo32 + 1e-6, (eo, eo32)
    assert eg <= 1e-4 + 10 * budget, (eg, budget)
    sd, sr, s32 = model.state_dict(), ref.state_dict(), ref32.state_dict()
    stat = [k for k in sr if k.endswith("running_mean") or k.endswith("running_var")]
    dev32 = max(float(((s32[k].double() - sr[k]).abs() / (sr[k].abs() + 1e-30)).max()) for k in stat if k.endswith("running_var"))
    worst = max(float(((sd[k].cpu().double() - sr[k]).abs() / (sr[k].abs() + 1e-30)).max()) for k in stat if k.endswith("running_var"))
    rtol = max(6e-4, 4 * dev32)
    print(f"[fp32 seg] worst running_var relative deviation {worst:.1e} (CPU fp32 {dev32:.1e}, rtol {rtol:.1e})")
    for k in stat:
        np.testing.assert_allclose(sd[k].cpu().numpy(), sr[k].float().numpy(), rtol=rtol, atol=1e-5, err_msg=k)
    nbt = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert len(nbt) == len(stat) // 2 and all(v == 1 for v in nbt)
    model.eval(); ref.eval()
    with torch.no_grad():
        oe, oe_r = model(x.cuda()), ref(x.double())
    assert _rel(oe.cpu(), oe_r) <= 3e-5, _rel(oe.cpu(), oe_r)


# ------------------------------------------------------------------------------------------------------------------- 2. the head against the reference's head
def _hold(what, prec, dev, gold, ref64, storage):
    """dev against the golden value with the kernel tests' rule; E32 = the golden (reference fp32) run's own error against the fp64 CPU head."""
    dev, gold, ref64 = (t.double() if t.dim() < 4 else t.double().permute(0, 2, 3, 1) for t in (dev, gold, ref64))
    if dev.dim() == 1:
        dev, gold, ref64 = dev[:, None], gold[:, None], ref64[:, None]          # a vector is one channel: an entry is a sum that may cancel to nothing
    assert bool(torch.isfinite(dev).all()), (what, "not finite")
    whole, chan, e32 = FR.rel(dev, gold), FR.rel_per_channel(dev, gold), FR.rel(gold, ref64)
    if storage == "bf16":
        bw, bc = 3e-3, FR.BF16_U + 8 * e32
    else:
        bw = max(2e-5 if storage == "dw_bf16" else 2e-6, 8 * e32)
        bc = 2 * bw
    print(f"[seg head vs golden] {what} {prec}: observed {whole:.2e} / {chan:.2e} (worst channel) bound {bw:.2e} / {bc:.2e} E32 {e32:.2e}")
    return [] if whole <= bw and chan <= bc else [(what, prec, whole, bw, chan, bc, e32)]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_head_step_vs_reference_head(mods, golden, prec):
    """FloatSegRunner.for_head(head).head_step on g20_seg_head's inputs: out, dc1, dc4, every parameter gradient, the running statistics and the eval-mode out,
    with the kernel tests' rule (tests/test_gpu_seg_head_kernels.py) against the golden values; running statistics rtol 1e-5 (fp32), 2^-8 (bf16: one rounding of
    the pooled map in front of b1).
    Worst observed, fp32 mode: 6.1e-7 (project.weight) against max(2e-6, 8 E32).  bf16 mode: out 1.0e-7, out_eval 9.4e-8, dc1 and dc4 1.7e-3 (one rounding to
    bf16 each) against 3e-3; parameter gradients <= 6.3e-7 against 2e-5.  The head's c4-resolution part runs in fp32 storage in both modes (FloatSegRunner._c4_scope):
    in bf16 storage b0's ReLU mask came from a rounded conv output and dc4 measured 2.8e-2, b0's conv weight 3.1e-2."""
    M, _ = mods
    from frostnet_amd.float_train import FloatSegRunner
    g = golden("g20_seg_head")
    T = lambda k: torch.from_numpy(g[k])
    head = M.LRASPPHead(6, 16, 8, dataset="pascal", c4_stride=16)
    head.load_state_dict({k[2:]: T(k) for k in g.files if k.startswith("w/")})
    ref = copy.deepcopy(head).double().train()
    c1r, c4r = T("c1").double().requires_grad_(True), T("c4").double().requires_grad_(True)
    out_r = ref(c1r, c4r)
    out_r.backward(T("gout").double())
    head.cuda().train()
    run = FloatSegRunner.for_head(head, precision=prec)
    out, dc1, dc4 = run.head_step(T("c1").cuda(), T("c4").cuda(), T("gout").cuda())
    torch.cuda.synchronize()
    bad = _hold("out", prec, out.cpu(), T("out"), out_r.detach(), "fp32" if prec == "fp32" else "bf16")
    bad += _hold("dc1", prec, dc1.cpu(), T("dc1"), c1r.grad, prec)
    bad += _hold("dc4", prec, dc4.cpu(), T("dc4"), c4r.grad, prec)
    refg = dict(ref.named_parameters())
    for n, p in head.named_parameters():
        gr = p.grad.detach().cpu()
        if gr.dim() == 4:
            gr, gg, g64 = gr.flatten(1).t(), T("grad/" + n).flatten(1).t(), refg[n].grad.flatten(1).t()          # (channel = the output channel: a row of the weight)
        else:
            gg, g64 = T("grad/" + n), refg[n].grad
        bad += _hold("grad " + n, prec, gr, gg, g64, "dw_bf16" if prec == "bf16" else "fp32")
    sd = head.state_dict()
    for k in g.files:
        if k.startswith("stat/") and "num_batches" in k:
            assert int(sd[k[5:]]) == 1
        elif k.startswith("stat/"):
            np.testing.assert_allclose(sd[k[5:]].cpu().numpy(), g[k], rtol=1e-5 if prec == "fp32" else 2.0 ** -8, atol=1e-6 if prec == "fp32" else 1e-4, err_msg=k)
    head.eval(); ref.eval()
    with torch.no_grad():
        bad += _hold("out_eval", prec, run.head_eval(T("c1").cuda(), T("c4").cuda()).cpu(), T("out_eval"), ref(c1r, c4r), "fp32" if prec == "fp32" else "bf16")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------- 3. through the criterion
def test_through_the_criterion(mods):
    """SegmentationLoss(21, class_wts) with a SegMeter on the model's logits: the loss within 1e-5 relative of the fp64 CPU loss; loss.backward() fills every
    p.grad, finite; a second backward without zero_grad() doubles the arena (the _carry path)."""
    M, S = mods
    torch.set_num_threads(16)
    model = _small(M, 23, pool_kernel=3, pool_stride=2)
    ref = copy.deepcopy(model).double().train()
    x = torch.randn(*X_SHAPE, generator=torch.Generator().manual_seed(4))
    t = _targets(4, 129, 161)
    wts = torch.rand(21, generator=torch.Generator().manual_seed(6)) + 0.5
    loss_r = S.SegmentationLoss(21, class_wts=wts.double())(ref(x.double()), t)
    model.float_precision = "fp32"
    model.cuda().train()
    meter = S.SegMeter(21, "cuda")
    crit = S.SegmentationLoss(21, class_wts=wts, meter=meter)
    loss = crit(model(x.cuda()), t.cuda())
    print(f"[seg criterion] loss {float(loss):.7f} vs fp64 CPU {float(loss_r):.7f}")
    assert abs(float(loss) - float(loss_r)) <= 1e-5 * abs(float(loss_r)), (float(loss), float(loss_r))
    loss.backward()
    torch.cuda.synchronize()
    run = model.hip_runner()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(run._params, run._grad_views))
    assert 0.0 <= meter.compute() <= 100.0
    first = run.grad_arena.clone()
    assert float(first.abs().sum()) > 0
    crit(model(x.cuda()), t.cuda()).backward()          # no zero_grad(): the second backward accumulates
    torch.cuda.synchronize()
    assert _rel(run.grad_arena.cpu(), 2 * first.cpu()) <= 1e-5, _rel(run.grad_arena.cpu(), 2 * first.cpu())


# ------------------------------------------------------------------------------------------------------------------- 4. bf16 sanity
def test_bf16_train_step_vs_fp32_definition(mods):
    """Default (bf16 storage) mode, one training step against the CPU fp32 definition with the detector's bf16 bounds: stem output 4e-3, conv-weight gradient-norm
    ratios (median in [0.8, 1.25], min >= 0.33, max <= 3), the head's ten parameters 6e-2, every gradient finite.  Held at 513 x 513, B = 2, the default pool
    (17^2 -> 2 x 2, BatchNorm count 8): a freshly initialised small net is chaotic at bf16 precision at 128^2 (tests/test_gpu_detect_float.py).
    Three head parameters exceed 6e-2 on the device: b0's and b1's 1x1 weights and project's (measured 4.8e-1, 3.7e-1, 2.2e-1; the other seven <= 5.8e-2).  Rounding
    alone explains them: on the CPU, rounding ONLY the 1x1 weights and the input to bf16 moves the same three by 3.3e-1, 2.0e-1 and 1.2e-1 (the other seven <= 3.5e-2,
    the logits by 5.6e-2) -- their gradients are products with x5, which has been through every stage, and b1's BatchNorm normalises over 8 values.  That experiment
    runs here, and a parameter's bound is max(6e-2, 2x its error in the experiment): the device rounds every activation and activation gradient as well as the
    weights, at least twice as many rounding sites as the experiment has."""
    M, _ = mods
    torch.set_num_threads(16)
    model = _small(M, 41)
    ref = copy.deepcopy(model).train()
    x = torch.randn(2, 3, 513, 513, generator=torch.Generator().manual_seed(4))
    caps = {}
    ref.conv1.register_forward_hook(lambda m, i, o: caps.__setitem__("stem", o.detach()))
    out_r = ref(x)
    assert tuple(out_r.shape) == (2, 21, 65, 65)
    gout = torch.randn(out_r.shape, generator=torch.Generator().manual_seed(6))
    out_r.backward(gout)
    exp = copy.deepcopy(model).train()                        # the CPU experiment: only the 1x1 weights and the input rounded to bf16
    for m in exp.modules():
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1):
            m.weight.data = m.weight.data.bfloat16().float()
    exp(x.bfloat16().float()).backward(gout)
    exp_errs = _grad_errors(exp, ref)
    model.cuda().train()
    run = model.hip_runner()
    assert type(run).__name__ == "FloatSegRunner" and run.precision == "bf16"
    dev_caps, orig_conv = {}, run._conv

    def conv(l, a, training, record, out=None, ldy=None, **kw):
        o = orig_conv(l, a, training, record, out, ldy, **kw)
        if l.name == "conv1":
            dev_caps["stem"] = o
        return o
    run._conv = conv
    out = model(x.cuda())
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    run._conv = orig_conv
    assert _rel(dev_caps["stem"].float().cpu(), caps["stem"]) <= 4e-3
    print(f"[bf16 seg] logits {_rel(out.detach().cpu(), out_r.detach()):.2e}")
    gn = np.array([float(p.grad.double().norm()) for p in model.parameters()])
    gr = np.array([float(p.grad.double().norm()) for p in ref.parameters()])
    assert np.isfinite(gn).all()
    cv = np.array([p.dim() == 4 for p in model.parameters()])
    ratio = gn[cv] / gr[cv]
    errs = _grad_errors(model, ref)
    tail = {n: e for n, e in errs.items() if n.startswith("head.")}
    print(f"[bf16 seg] gradient-norm ratio median {np.median(ratio):.3f} min {ratio.min():.3f} max {ratio.max():.3f}; head parameters "
          + ", ".join(f"{n[5:]} {e:.1e} (CPU experiment {exp_errs[n]:.1e})" for n, e in tail.items()))
    assert 0.8 <= np.median(ratio) <= 1.25 and ratio.min() >= 0.33 and ratio.max() <= 3.0, (np.median(ratio), ratio.min(), ratio.max())
    assert len(tail) == 10 and all(e <= max(6e-2, 2 * exp_errs[n]) for n, e in tail.items()), (tail, {n: exp_errs[n] for n in tail})


# ------------------------------------------------------------------------------------------------------------------- 5. the loops
def test_train_seg_and_val_seg_loops(mods):
    """SegmentationAugmentation -> FrostNetSeg('small') -> SegmentationLoss through one harness.train_seg epoch of two batches with QSGD at a small lr, then
    harness.val_seg: finite loss, mean IoU in [0, 100], parameters and running statistics changed by training, running statistics unchanged by validation."""
    M, S = mods
    from frostnet_amd import harness, seg_augment
    from frostnet_amd.optimizer import QSGD
    rng = np.random.default_rng(14)
    loader = []
    for _ in range(2):
        pics = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((120, 150), (100, 170), (140, 130))]
        labs = [np.where(rng.random(p.shape[:2]) < 0.1, 255, rng.integers(0, 21, p.shape[:2])).astype(np.uint8) for p in pics]
        loader.append(seg_augment.pad_pairs(pics, labs))
    torch.manual_seed(9)
    model = M.FrostNetSeg(21, "small", pool_kernel=3, pool_stride=2).cuda()
    opt = QSGD(harness.make_param_groups(model, 1e-5), lr=1e-3, momentum=0.9)
    crit = S.SegmentationLoss(n_classes=21, device="cuda")
    aug, ev = seg_augment.SegmentationAugmentation(crop_size=(129, 161), seed=3), seg_augment.SegmentationEvalTransform(size=(129, 161))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    miou, loss = harness.train_seg(model, loader, opt, crit, 21, transform=aug)
    torch.cuda.synchronize()
    assert type(model.hip_runner()).__name__ == "FloatSegRunner"
    assert np.isfinite(loss) and 0.0 <= miou <= 100.0, (miou, loss)
    after = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k in ("conv1.conv.0.weight", "head.project.weight", "head.auxlayer.bias", "head.lr_aspp.b1.1.conv.0.weight", "head.lr_aspp.b0.conv.1.running_var",
              "head.lr_aspp.b1.1.conv.1.running_mean", "layer3.0.conv2.conv.1.running_var"):
        assert not torch.equal(before[k], after[k]), k
    assert int(after["head.lr_aspp.b1.1.conv.1.num_batches_tracked"]) == 2
    vmiou, vloss = harness.val_seg(model, loader, criterion=crit, num_classes=21, transform=ev)
    torch.cuda.synchronize()
    assert np.isfinite(vloss) and 0.0 <= vmiou <= 100.0, (vmiou, vloss)
    final = model.state_dict()
    assert all(torch.equal(final[k], after[k]) for k in after)
    print(f"[seg loops] train mIoU {miou:.3f} loss {loss:.4f}; val mIoU {vmiou:.3f} loss {vloss:.4f}")


# ------------------------------------------------------------------------------------------------------------------- 6. guards
def test_guards(mods):
    M, _ = mods
    from frostnet_amd import _lib as L
    model = M.FrostNetSeg(21, "small").cuda().train()                       # default window 13 x 13
    model(torch.randn(2, 3, 513, 513, device="cuda"))                       # (binds the runner)
    L.CALL_LOG = []
    try:
        with pytest.raises(ValueError, match=r"5 x 6.*13 x 13"):            # the window is larger than the map
            model(torch.randn(2, 3, 129, 161, device="cuda"))
        one = M.FrostNetSeg(21, "small", pool_kernel=5, pool_stride=1).cuda().train()
        one.hip_runner()
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):          # 1 x 5 x 5 map -> one pooled value per channel
            one(torch.randn(1, 3, 129, 129, device="cuda"))
        one.head.lr_aspp.b0.conv[1].eval()
        with pytest.raises(NotImplementedError, match="BatchNorm in eval mode"):
            one(torch.randn(2, 3, 129, 129, device="cuda"))
        assert L.CALL_LOG == []
    finally:
        L.CALL_LOG = None
    fused = M.FrostNetSeg(21, "small").eval()
    fused.fuse_model()
    with pytest.raises(NotImplementedError, match="segmentation QAT is not built"):
        fused.cuda()(torch.randn(1, 3, 513, 513, device="cuda"))
    prepared = M.FrostNetSeg(21, "small").train()
    prepared.fuse_model()
    prepared.qconfig = torch.quantization.get_default_qat_qconfig("qnnpack")
    torch.quantization.prepare_qat(prepared, inplace=True)
    with pytest.raises(NotImplementedError, match="segmentation QAT is not built"):
        prepared.cuda()(torch.randn(2, 3, 513, 513, device="cuda"))
    with pytest.raises(ValueError, match="nclass"):
        M.FrostNetSeg(1, "small")

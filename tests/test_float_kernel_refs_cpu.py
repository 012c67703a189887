"""The references of tests/float_kernel_refs.py, checked without a device: against torch's own fp64 Conv2d(1x1) -> BatchNorm2d(train) ->
activation under autograd (1e-12), the pack index formulas against their inverse, and the share of band-marked elements of every case the
GPU file runs (tests/test_gpu_float_kernels.py asserts the same condition before it launches anything)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_kernel_refs as R  # noqa: E402


def _module(cin, cout, act, p):
    layers = [torch.nn.Conv2d(cin, cout, 1, bias=False), torch.nn.BatchNorm2d(cout)]
    if act == R.ACT_RELU:
        layers.append(torch.nn.ReLU())
    elif act == R.ACT_HSWISH:
        layers.append(torch.nn.Hardswish())
    m = torch.nn.Sequential(*layers).double().train()
    with torch.no_grad():
        m[0].weight.copy_(p["w"].double().reshape(cout, cin, 1, 1))
        m[1].weight.copy_(p["gamma"]); m[1].bias.copy_(p["beta"])
        m[1].running_mean.copy_(p["rmean"]); m[1].running_var.copy_(p["rvar"])
    return m


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_HSWISH], ids=lambda a: R.ACT_NAMES[a])
@pytest.mark.parametrize("shape", [(2, 5, 3, 8, 24), (1, 1, 1, 8, 8), (3, 4, 4, 24, 40)], ids=lambda s: "n%d_%dx%d_%dto%d" % s)
def test_layer_reference_matches_torch_autograd(shape, act):
    """y, running statistics, dx, dW, dgamma, dbeta of two steps (the second accumulates the parameter gradients and moves the running
    statistics again) against the stock modules in fp64: 1e-12 norm-wise.  (1, 1, 1): a single sample -- torch refuses to train BatchNorm on
    it, so that shape checks the count-1 rule on the reference alone: biased variance into the running variance, y = act(beta)."""
    n, h, wd, cin, cout = shape
    npix = n * h * wd
    p = R.layer_inputs(npix, cin, cout, "fp32", 77 + cin + act)
    g2 = torch.randn(npix, cout, generator=torch.Generator().manual_seed(5)) * 0.1
    rmean, rvar, nbt = p["rmean"].double(), p["rvar"].double(), 0
    dgamma, dbeta, dW = torch.zeros(cout, dtype=R.F64), torch.zeros(cout, dtype=R.F64), torch.zeros(cout, cin, dtype=R.F64)
    if npix == 1:
        f = R.conv_bn_forward(p["x"], p["w"], p["gamma"], p["beta"], rmean, rvar, nbt, act)
        assert float(f["var"].abs().max()) == 0.0 and f["nbt"] == 1
        assert R.rel(f["rvar"], 0.9 * rvar) <= 1e-15 and R.rel(f["y"][0], R.act_fwd(p["beta"].double(), act)) <= 1e-12
        return
    m = _module(cin, cout, act, p)
    xt = p["x"].double().reshape(n, h, wd, cin).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    for step, gy in enumerate((p["gy"], g2)):
        f = R.conv_bn_forward(p["x"], p["w"], p["gamma"], p["beta"], rmean, rvar, nbt, act)
        b = R.conv_bn_backward(f, p["x"], p["w"], gy, p["gamma"], act, dgamma, dbeta)
        rmean, rvar, nbt, dgamma, dbeta, dW = f["rmean"], f["rvar"], f["nbt"], b["dgamma"], b["dbeta"], dW + b["dW"]
        xt.grad = None
        yt = m(xt)
        yt.backward(gy.double().reshape(n, h, wd, cout).permute(0, 3, 1, 2))
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(npix, -1)
        for name, mine, theirs in (("y", f["y"], nhwc(yt.detach())), ("rmean", rmean, m[1].running_mean), ("rvar", rvar, m[1].running_var),
                                   ("dx", b["dx"], nhwc(xt.grad)), ("dW", dW, m[0].weight.grad.reshape(cout, cin)),
                                   ("dgamma", dgamma, m[1].weight.grad), ("dbeta", dbeta, m[1].bias.grad)):
            assert R.rel(mine, theirs) <= 1e-12, (step, name, R.rel(mine, theirs))
        assert nbt == int(m[1].num_batches_tracked) == step + 1
        # the folded form the bf16 mode evaluates is the same function
        folded = R.dc_folded(f["conv"], gy, f["scale"], f["bias"], b["K1"], b["E"], b["F"], act)
        assert R.rel(folded, b["dc"]) <= 1e-12


def test_band_mask_marks_the_kinks_and_nothing_else():
    conv = torch.tensor([[-3.0, -3.0 + 1e-4, 0.0, 2e-5, 3.0 - 2e-5, 3.0, 1.0, -1.0]], dtype=R.F64)
    one, zero = torch.ones(8, dtype=R.F64), torch.zeros(8, dtype=R.F64)
    assert R.band_mask(conv, one, zero, R.ACT_NONE).sum() == 0
    assert R.band_mask(conv, one, zero, R.ACT_RELU)[0].tolist() == [False, False, True, False, False, False, False, False]
    assert R.band_mask(conv, one, zero, R.ACT_HSWISH)[0].tolist() == [True, False, True, False, True, True, False, False]
    # tau follows the size of the terms, not of their sum: conv*scale = 1000, bias = -1000 + 1e-3 is inside the band of 0
    assert bool(R.band_mask(torch.tensor([[1000.0]], dtype=R.F64), one[:1], torch.tensor([-1000.0 + 1e-3], dtype=R.F64), R.ACT_RELU)[0, 0])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_band_share_of_every_gpu_case(prec):
    """At most 1e-3 of a case's elements may be marked (expected with unit-variance pre-activations: ~1e-5); same seeds as the GPU file."""
    for npix, cin, cout, act, _ in R.PW_CASES[prec]:
        p = R.layer_inputs(npix, cin, cout, prec, R.pw_seed(npix, cin, cout, act))
        f = R.conv_bn_forward(p["x"], p["w_seen"], p["gamma"], p["beta"], p["rmean"], p["rvar"], 0, act)
        _, share = R.zero_band(p["gy"], f["conv"], f["scale"], f["bias"], act)
        assert share <= R.BAND_SHARE, ("pw", npix, cin, cout, R.ACT_NAMES[act], share)
        assert float((f["mean"] * f["inv"]).abs().max()) <= 2.0 or npix == 1          # conv means within +-2 sigma
    for npix, c, act, _ in R.EW_CASES[prec]:
        p = R.kept_inputs(npix, c, prec, R.ew_seed(npix, c, act))
        _, share = R.zero_band(p["gy"], p["conv"], p["scale"], p["bias"], act)
        assert share <= R.BAND_SHARE, ("ew", npix, c, R.ACT_NAMES[act], share)


@pytest.mark.parametrize("prec,kq", [("bf16", 32), ("fp32", 16)])
@pytest.mark.parametrize("cin,cout", [(8, 8), (24, 40), (40, 24), (360, 592)])
def test_pack_formulas_invert(cin, cout, prec, kq):
    """pack, then unpack, returns the weight matrix with zeros in the padding; every pack slot is written exactly once."""
    w = torch.randn(cout, cin, generator=torch.Generator().manual_seed(cin + cout))
    fwd, tr, kpad, kpad_t = R.layer_packs(w, 0, prec)
    cpad, cipad = R.round_up(cout, 16), R.round_up(cin, 16)
    assert kpad == R.round_up(cin, kq) and kpad_t == R.round_up(cout, kq)
    assert fwd.numel() == cpad * kpad and tr.numel() == cipad * kpad_t
    ws = R.seen(w, prec)
    for flat, m, rp, kp in ((fwd, ws, cpad, kpad), (tr, ws.t(), cipad, kpad_t)):
        back = R.unpack_matrix(flat, rp, kp, kq)
        assert not torch.isnan(back).any()                                   # the index map is onto
        assert torch.equal(back[: m.shape[0], : m.shape[1]], m)
        assert float(back[m.shape[0]:].abs().sum()) == 0.0 and float(back[:, m.shape[1]:].abs().sum()) == 0.0
    row, k = R.pack_index(cpad, kpad, kq)
    assert len(set((row * kpad + k).tolist())) == cpad * kpad                # and one-to-one
    # the documented element: lane 37 = (row 5, group 2) of tile (ct 1, kb 0), element 3
    ne = kq // 4
    i = ((1 * (kpad // kq) + 0) * 64 + 37) * ne + 3
    if cout > 21 and cin > 2 * ne + 3:
        assert float(fwd[i]) == float(ws[16 + 5, 2 * ne + 3])


@pytest.mark.parametrize("prec,kq", [("bf16", 32), ("fp32", 16)])
def test_stem_pack_formula(prec, kq):
    w = torch.randn(32, 3, 3, 3, generator=torch.Generator().manual_seed(3))
    flat, tr, kpad, _ = R.layer_packs(w, 2, prec)
    assert tr is None and kpad == 64
    m = R.unpack_matrix(flat, 32, 64, kq)
    ws = R.seen(w, prec)
    for tap in range(16):
        for c in range(4):
            exp = ws[:, c, tap // 3, tap % 3] if (tap < 9 and c < 3) else torch.zeros(32)
            assert torch.equal(m[:, tap * 4 + c], exp)
    assert torch.equal(R.stem_unscatter(m, 32), ws.reshape(32, 27))          # the scatter's permutation is the inverse

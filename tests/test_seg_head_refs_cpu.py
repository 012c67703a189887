"""tests/seg_head_refs.py held to torch: the fp64 forms of the five kernel pairs against autograd over stock AvgPool2d / F.interpolate(align_corners=True) /
Conv2d (<= 1e-12), the commuted form up(project(z)) against the reference's project(up(z)) (<= 1e-12 in fp64), and the seeds of the device tests: no element of
their g lies in the band around a kink of the hard sigmoid (the share allowed is BAND_SHARE; the seeds chosen leave it empty)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_head_refs as R  # noqa: E402

TOL = 1e-12


def rel(a, ref):
    err = float((a.double() - ref.double()).norm())
    return 0.0 if err == 0.0 else err / max(float(ref.double().norm()), 1e-300)


def interp(x, size):
    return F.interpolate(x, tuple(size), mode="bilinear", align_corners=True)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_pool_pair_is_avgpool2d_and_its_autograd(case):
    n, h, w, c, k, s = case
    x, dy, addend = (t.double() for t in R.pool_inputs(case))
    xr = x.clone().requires_grad_(True)
    y = torch.nn.AvgPool2d(R.pair(k), R.pair(s))(xr)
    assert y.shape == R.pool(x, k, s).shape
    assert rel(R.pool(x, k, s), y.detach()) <= TOL
    y.backward(dy)
    assert rel(R.pool_bwd(dy, (h, w), k, s), xr.grad) <= TOL
    assert rel(R.pool_bwd(dy, (h, w), k, s, addend), xr.grad + addend) <= TOL


@pytest.mark.parametrize("case", R.GATE_CASES, ids=str)
def test_gate_project_pair_is_the_stock_ops_and_their_autograd(case):
    feat1, g, w, b, dp = (t.double() for t in R.gate_inputs(case))
    f, gr, wr, br = (t.clone().requires_grad_(True) for t in (feat1, g, w, b))
    gt = interp(F.relu6(gr + 3.0) * (1 / 6), feat1.shape[2:])
    p = F.conv2d(f * gt, wr[:, :, None, None], br)
    assert rel(R.gate_project(feat1, g, w, b), p.detach()) <= TOL
    p.backward(dp)
    dW, db, df, dg = R.gate_project_bwd(feat1, g, dp, w)
    for name, mine, ref in (("dW", dW, wr.grad), ("db", db, br.grad), ("dfeat1", df, f.grad), ("dg", dg, gr.grad)):
        assert rel(mine, ref) <= TOL, (name, rel(mine, ref))


@pytest.mark.parametrize("case", R.GATE_CASES, ids=str)
def test_device_seeds_keep_g_out_of_the_band(case):
    _, g, _, _, _ = R.gate_inputs(case)
    for t in (g, g.bfloat16().float()):            # what the device sees in either precision
        assert R.band_count(t) <= R.BAND_SHARE * t.numel()
        assert R.band_count(t) == 0


@pytest.mark.parametrize("case", R.LOGITS_CASES, ids=str)
def test_logits_pair_is_the_stock_ops_and_their_autograd(case):
    p, c1, w, b, dout = (t.double() for t in R.logits_inputs(case))
    pr, cr, wr, br = (t.clone().requires_grad_(True) for t in (p, c1, w, b))
    out = interp(pr, c1.shape[2:]) + F.conv2d(cr, wr[:, :, None, None], br)
    assert rel(R.logits(p, c1, w, b), out.detach()) <= TOL
    out.backward(dout)
    dc1, dW, db, dp = R.logits_bwd(dout, c1, w, p.shape[2:])
    for name, mine, ref in (("dc1", dc1, cr.grad), ("dW", dW, wr.grad), ("db", db, br.grad), ("dp", dp, pr.grad)):
        assert rel(mine, ref) <= TOL, (name, rel(mine, ref))


@pytest.mark.parametrize("shape", [((2, 2), (5, 6), (17, 21)), ((2, 3), (17, 17), (65, 65)), ((3, 3), (3, 3), (9, 9)), ((1, 3), (5, 6), (5, 6))], ids=str)
def test_commuted_form_is_the_reference_order(shape):
    (ph, pw), (h4, w4), (h1, w1) = shape
    gen = torch.Generator().manual_seed(5)
    k, ch = 21, 24
    feat1 = torch.randn(2, R.CF, h4, w4, generator=gen, dtype=torch.float64).clamp_min(0)
    g = torch.randn(2, R.CF, ph, pw, generator=gen, dtype=torch.float64) * 3
    c1 = torch.randn(2, ch, h1, w1, generator=gen, dtype=torch.float64)
    wp, bp = torch.randn(k, R.CF, generator=gen, dtype=torch.float64), torch.randn(k, generator=gen, dtype=torch.float64)
    wa, ba = torch.randn(k, ch, generator=gen, dtype=torch.float64), torch.randn(k, generator=gen, dtype=torch.float64)
    ref = head_stock = F.conv2d(interp(feat1 * interp(F.relu6(g + 3.0) * (1 / 6), (h4, w4)), (h1, w1)), wp[:, :, None, None], bp) + F.conv2d(c1, wa[:, :, None, None], ba)
    assert rel(R.head_reference_order(feat1, g, c1, wp, bp, wa, ba), head_stock) <= TOL
    assert rel(R.logits(R.gate_project(feat1, g, wp, bp), c1, wa, ba), ref) <= TOL

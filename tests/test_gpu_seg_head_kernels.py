"""The segmentation head's kernels (csrc/frost_seghead.hip), entry by entry through the C ABI and in both precisions, against fp64 references of the operands the
device sees (tests/seg_head_refs.py; held to torch's autograd by tests/test_seg_head_refs_cpu.py).

Tolerances: the one rule of tests/test_gpu_float_kernels.py, nothing taken from the device.  E32 = the error against fp64 of the same quantity in plain fp32 torch ops.
  fp32 storage (fp32 mode, and p / logits / dp in either mode)   max(2e-6, 8 E32) norm-wise over the tensor, twice that for the worst channel
  bf16 storage                                                   3e-3 over the tensor, 2^-8 + 8 E32 for the worst channel
  weight and bias gradients in bf16 mode                         max(2e-5, 8 E32)
The seeded g holds no element within 1e-5 of a kink of the hard sigmoid (checked on the CPU), so no gradient has to be masked.  Every buffer carries a sentinel in
the 64 elements of slack behind it; each test asserts they are untouched.  Every check prints `[seghead-kernels] what precision: observed / bound / E32`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_kernel_refs as FR  # noqa: E402
import seg_head_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
PRECS = ["bf16", "fp32"]
SLACK, SENT, NAN = 64, 7.0, float("nan")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib
    return _lib


def _dt(prec):
    return torch.bfloat16 if prec == "bf16" else torch.float32


def _fn(name, prec):
    return "frost_seghead_" + name + ("_f32" if prec == "fp32" else "")


def seen(t, prec):
    """The operand as the device stores it, in fp32."""
    return t.bfloat16().float() if prec == "bf16" else t.float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Buf:
    """`numel` elements (data, or NaN for a result) and a sentinel in the slack behind them."""

    def __init__(self, dtype, numel=None, data=None, fill=NAN):
        numel = data.numel() if data is not None else numel
        self.numel = numel
        self.t = torch.full((numel + SLACK,), SENT, dtype=dtype, device="cuda")
        self.t[:numel] = data.reshape(-1).to(dtype).cuda() if data is not None else fill

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self, *shape):
        assert bool((self.t[self.numel:].float() == SENT).all()), "the slack behind the tensor was written"
        return self.t[: self.numel].float().cpu().view(*shape)


def act(t_nchw, prec):
    return Buf(_dt(prec), data=nhwc(t_nchw))


def f32(t):
    return Buf(torch.float32, data=t)


def _hold(what, prec, dev, ref, ref32, storage):
    """dev against ref (fp64) with the yardstick ref32; channel = the last dimension."""
    assert bool(torch.isfinite(dev).all()), (what, "not finite")
    whole, chan, e32 = FR.rel(dev, ref), FR.rel_per_channel(dev, ref), FR.rel(ref32, ref)
    if storage == "bf16":
        bw, bc = 3e-3, FR.BF16_U + 8 * e32
    else:
        bw = max(2e-5 if storage == "dw_bf16" else 2e-6, 8 * e32)
        bc = 2 * bw
    print(f"[seghead-kernels] {what} {prec}: observed {whole:.2e} / {chan:.2e} (worst channel) bound {bw:.2e} / {bc:.2e} E32 {e32:.2e}")
    assert whole <= bw, (what, prec, "whole tensor", whole, bw, e32)
    assert chan <= bc, (what, prec, "worst channel", chan, bc, e32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ pool
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_pool_forward_and_backward(L, case, prec):
    n, h, w, c, k, s = case
    (kh, kw), (sh, sw) = R.pair(k), R.pair(s)
    x, dy, addend = (seen(t, prec) for t in R.pool_inputs(case))
    ph, pw = dy.shape[2:]
    y, bx, bdy = Buf(_dt(prec), n * ph * pw * c), act(x, prec), act(dy, prec)          # (every buffer stays referenced until its result is read)
    L.call(_fn("pool", prec), bx.p, n, h, w, c, kh, kw, sh, sw, y.p, _stream())
    _hold("pool y", prec, y.get(n, ph, pw, c), nhwc(R.pool(x.double(), k, s)), nhwc(R.pool(x, k, s)), prec)
    for add in (None, addend):
        dx, badd = Buf(_dt(prec), n * h * w * c), act(add, prec) if add is not None else None
        L.call(_fn("pool_bwd", prec), bdy.p, badd.p if badd is not None else None, n, h, w, c, kh, kw, sh, sw, dx.p, _stream())
        ref = R.pool_bwd(dy.double(), (h, w), k, s, add.double() if add is not None else None)
        _hold("pool dx" + (" + addend" if add is not None else ""), prec, dx.get(n, h, w, c), nhwc(ref), nhwc(R.pool_bwd(dy, (h, w), k, s, add)), prec)
        if add is None and ((h - kh) % sh or (w - kw) % sw):          # rows / columns past the last window receive nothing
            got = dx.get(n, h, w, c)
            assert bool((got[:, (ph - 1) * sh + kh:] == 0).all()) and bool((got[:, :, (pw - 1) * sw + kw:] == 0).all())


# ================================================================================================ gate + project
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.GATE_CASES, ids=str)
def test_gate_project_forward_and_backward(L, case, prec):
    (ph, pw), (h4, w4), k = case
    n, cf = R.N_GATE, R.CF
    feat1, g, w, b, dp = R.gate_inputs(case)
    feat1, g = seen(feat1, prec), seen(g, prec)
    assert R.band_count(g) == 0
    bf, bg, bw_ = act(feat1, prec), act(g, prec), f32(w)
    p, bb, bdp = Buf(torch.float32, n * h4 * w4 * k), f32(b), f32(nhwc(dp))
    L.call(_fn("gate_project", prec), bf.p, bg.p, bw_.p, bb.p, n, h4, w4, ph, pw, cf, k, p.p, _stream())
    _hold("gate_project p", prec, p.get(n, h4, w4, k), nhwc(R.gate_project(feat1.double(), g.double(), w.double(), b.double())), nhwc(R.gate_project(feat1, g, w, b)), "fp32")
    dW, db = Buf(torch.float32, k * cf, fill=0.0), Buf(torch.float32, k, fill=0.0)
    df, dg, scratch = Buf(_dt(prec), n * h4 * w4 * cf), Buf(_dt(prec), n * ph * pw * cf), Buf(torch.float32, n * h4 * w4 * cf)
    L.call(_fn("gate_project_bwd", prec), bf.p, bg.p, bdp.p, bw_.p, n, h4, w4, ph, pw, cf, k, dW.p, db.p, df.p, dg.p, scratch.p, _stream())
    ref = R.gate_project_bwd(feat1.double(), g.double(), dp.double(), w.double())
    r32 = R.gate_project_bwd(feat1, g, dp, w)
    wst = "dw_bf16" if prec == "bf16" else "fp32"
    _hold("gate_project dW", prec, dW.get(k, cf).t(), ref[0].t(), r32[0].t(), wst)          # (channel = the output channel of the product: a row of dW)
    _hold("gate_project db", prec, db.get(k, 1), ref[1][:, None], r32[1][:, None], wst)          # (a vector: one channel -- an entry is a sum that may cancel to nothing)
    _hold("gate_project dfeat1", prec, df.get(n, h4, w4, cf), nhwc(ref[2]), nhwc(r32[2]), prec)
    _hold("gate_project dg", prec, dg.get(n, ph, pw, cf), nhwc(ref[3]), nhwc(r32[3]), prec)
    scratch.get(n * h4 * w4 * cf)


# ================================================================================================ logits
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.LOGITS_CASES, ids=str)
def test_logits_forward_and_backward(L, case, prec):
    (h4, w4), (h1, w1), ch, k = case
    n = R.N_LOGITS
    p, c1, w, b, dout = R.logits_inputs(case)
    c1 = seen(c1, prec)
    bc1, bw_ = act(c1, prec), f32(w)
    out, bp, bb = Buf(torch.float32, n * h1 * w1 * k), f32(nhwc(p)), f32(b)
    L.call(_fn("logits", prec), bp.p, bc1.p, bw_.p, bb.p, n, h1, w1, h4, w4, ch, k, out.p, _stream())
    _hold("logits out", prec, out.get(n, h1, w1, k), nhwc(R.logits(p.double(), c1.double(), w.double(), b.double())), nhwc(R.logits(p, c1, w, b)), "fp32")
    ref = R.logits_bwd(dout.double(), c1.double(), w.double(), (h4, w4))
    r32 = R.logits_bwd(dout, c1, w, (h4, w4))
    wst = "dw_bf16" if prec == "bf16" else "fp32"
    for layout, data, strides in (("NCHW", dout, (k * h1 * w1, h1 * w1, w1, 1)), ("channels-last", nhwc(dout), (h1 * w1 * k, 1, w1 * k, k))):
        dc1, dW, db, dp = Buf(_dt(prec), n * h1 * w1 * ch), Buf(torch.float32, k * ch, fill=0.0), Buf(torch.float32, k, fill=0.0), Buf(torch.float32, n * h4 * w4 * k)
        bd = f32(data)
        L.call(_fn("logits_bwd", prec), bd.p, *strides, bc1.p, bw_.p, n, h1, w1, h4, w4, ch, k, dc1.p, dW.p, db.p, dp.p, _stream())
        _hold(f"logits dc1 ({layout})", prec, dc1.get(n, h1, w1, ch), nhwc(ref[0]), nhwc(r32[0]), prec)
        _hold(f"logits dW ({layout})", prec, dW.get(k, ch).t(), ref[1].t(), r32[1].t(), wst)
        _hold(f"logits db ({layout})", prec, db.get(k, 1), ref[2][:, None], r32[2][:, None], wst)
        _hold(f"logits dp ({layout})", prec, dp.get(n, h4, w4, k), nhwc(ref[3]), nhwc(r32[3]), "fp32")

"""Plain definitions of the segmentation head's kernels (csrc/frost_seghead.hip) in the dtype of their arguments: fp64 is the reference, fp32 the yardstick.
NCHW tensors, torch ops only, no autograd: tests/test_seg_head_refs_cpu.py holds the fp64 forms to torch's autograd over the stock modules, and the commuted form
project-then-upsample to the reference's order.  The case lists and the seeded inputs are shared with tests/test_gpu_seg_head_kernels.py."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from float_kernel_refs import BAND_RTOL, BAND_SHARE  # noqa: E402,F401

from frostnet_amd.seg import _axis, upsample_reference  # noqa: E402

CF = 128                                  # the head's width (LRASPP.py: 256 // 2)
HSIG_KINKS = (-3.0, 3.0)


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# ------------------------------------------------------------------------------------------------ the pieces
def pool(x, k, s):
    """Windowed mean, no padding, floor mode."""
    (kh, kw), (sh, sw) = pair(k), pair(s)
    ph, pw = (x.shape[2] - kh) // sh + 1, (x.shape[3] - kw) // sw + 1
    rows = [torch.stack([x[:, :, py * sh: py * sh + kh, px * sw: px * sw + kw].sum((2, 3)) for px in range(pw)], 2) for py in range(ph)]
    return torch.stack(rows, 2) / (kh * kw)


def pool_bwd(dy, hw, k, s, addend=None):
    (kh, kw), (sh, sw) = pair(k), pair(s)
    dx = torch.zeros(dy.shape[0], dy.shape[1], hw[0], hw[1], dtype=dy.dtype)
    for py in range(dy.shape[2]):
        for px in range(dy.shape[3]):
            dx[:, :, py * sh: py * sh + kh, px * sw: px * sw + kw] += dy[:, :, py, px][:, :, None, None]
    dx = dx / (kh * kw)
    return dx if addend is None else dx + addend


def up_matrix(n_in, n_out, dtype):
    """[n_out, n_in]: row d holds (1 - f) at i0 and f at i1 (seg._axis)."""
    i0, i1, f = _axis(n_in, n_out, dtype, torch.device("cpu"))
    m = torch.zeros(n_out, n_in, dtype=dtype)
    r = torch.arange(n_out)
    m.index_put_((r, i0), 1 - f, accumulate=True)
    m.index_put_((r, i1), f, accumulate=True)
    return m


def up(x, size):
    return upsample_reference(x, tuple(size))


def up_adjoint(g, size):
    """Transpose of up(. -> g's size) applied to g: [.., size]."""
    my, mx = up_matrix(size[0], g.shape[2], g.dtype), up_matrix(size[1], g.shape[3], g.dtype)
    return torch.einsum("Yy,ncYX,Xx->ncyx", my, g, mx)


def hsig(v):
    return torch.clamp(v + 3.0, 0.0, 6.0) * (1 / 6)


def dhsig(v):
    t = v + 3.0
    return ((t > 0) & (t < 6)).to(v.dtype) * (1 / 6)


def gate(g, size):
    return up(hsig(g), size)


def gate_project(feat1, g, w, b):
    z = feat1 * gate(g, feat1.shape[2:])
    return torch.einsum("kc,nchw->nkhw", w, z) + b[None, :, None, None]


def gate_project_bwd(feat1, g, dp, w):
    """-> (dW, db, dfeat1, dg)"""
    gt = gate(g, feat1.shape[2:])
    dz = torch.einsum("kc,nkhw->nchw", w, dp)
    return (torch.einsum("nkhw,nchw->kc", dp, feat1 * gt), dp.sum((0, 2, 3)), dz * gt, up_adjoint(dz * feat1, g.shape[2:]) * dhsig(g))


def logits(p, c1, w, b):
    return up(p, c1.shape[2:]) + (torch.einsum("kc,nchw->nkhw", w, c1) + b[None, :, None, None])


def logits_bwd(dout, c1, w, p_hw):
    """-> (dc1, dW, db, dp)"""
    return (torch.einsum("kc,nkhw->nchw", w, dout), torch.einsum("nkhw,nchw->kc", dout, c1), dout.sum((0, 2, 3)), up_adjoint(dout, p_hw))


def head_reference_order(feat1, g, c1, wp, bp, wa, ba):
    """The reference's order: project AFTER the upsampling of the 128-channel map."""
    z = up(feat1 * gate(g, feat1.shape[2:]), c1.shape[2:])
    return (torch.einsum("kc,nchw->nkhw", wp, z) + bp[None, :, None, None]) + (torch.einsum("kc,nchw->nkhw", wa, c1) + ba[None, :, None, None])


def band_count(g, rtol=BAND_RTOL):
    """Elements of g within rtol (relative to the size of the terms of g + 3) of a kink of the hard sigmoid."""
    gd = g.double()
    m = torch.zeros_like(gd, dtype=torch.bool)
    for k in HSIG_KINKS:
        m |= (gd - k).abs() <= rtol * (gd.abs() + 3.0)
    return int(m.sum())


# ------------------------------------------------------------------------------------------------ cases and seeded inputs (fp32, NCHW)
# (n, h, w, c, kernel, stride): uncovered last row / column at 6 x 6; one window = the global pool at 13 x 13; a rectangular window; a single channel
POOL_CASES = [(2, 17, 21, 40, 13, 4), (1, 33, 41, 24, 25, 8), (3, 6, 6, 72, 3, 2), (2, 13, 13, 8, 13, 4), (1, 7, 9, 20, (3, 5), (2, 3)), (2, 9, 8, 1, 3, 2)]
# (pooled hw, c4 hw, nclass): a constant axis (in == 1), the identity (3 x 3 -> 3 x 3), above the 32-class register path
GATE_CASES = [(p, c, k) for p, c in [((2, 2), (5, 6)), ((1, 3), (5, 6)), ((3, 1), (5, 6)), ((2, 3), (5, 6)), ((2, 2), (17, 17)), ((1, 3), (17, 17)),
                                     ((3, 1), (17, 17)), ((2, 3), (17, 17)), ((3, 3), (3, 3))] for k in (2, 21, 33)]
# (p hw, c1 hw, c1 channels, nclass)
LOGITS_CASES = [(p, c, ch, k) for p, c in [((5, 6), (17, 21)), ((17, 17), (65, 65)), ((1, 1), (4, 4))] for ch in (24, 40) for k in (2, 21, 33)]
N_GATE, N_LOGITS = 2, 2


def _flat(v):
    if isinstance(v, int):
        yield v
    else:
        for e in v:
            yield from _flat(e)


def case_seed(case):
    return 11 + sum((i + 1) * v for i, v in enumerate(_flat(case)))


def pool_inputs(case):
    n, h, w, c, k, s = case
    gen = torch.Generator().manual_seed(case_seed(case))
    (kh, kw), (sh, sw) = pair(k), pair(s)
    x = torch.randn(n, c, h, w, generator=gen)
    dy = torch.randn(n, c, (h - kh) // sh + 1, (w - kw) // sw + 1, generator=gen)
    return x, dy, torch.randn(n, c, h, w, generator=gen)


def gate_inputs(case):
    """feat1 >= 0 (a ReLU output), g spread over both kinks of the hard sigmoid."""
    (ph, pw), (h4, w4), k = case
    gen = torch.Generator().manual_seed(case_seed(case))
    feat1 = torch.randn(N_GATE, CF, h4, w4, generator=gen).clamp_min(0)
    g = (torch.randn(N_GATE, CF, ph, pw, generator=gen) * 3).bfloat16().float()          # the same values in either precision ...
    for kink in HSIG_KINKS:                                                              # ... and none in the band around a kink (bf16 rounding lands ON them otherwise)
        g = torch.where((g - kink).abs() <= 1e-3, g + 0.25, g)
    w = torch.randn(k, CF, generator=gen) * CF ** -0.5
    return feat1, g, w, torch.randn(k, generator=gen), torch.randn(N_GATE, k, h4, w4, generator=gen)


def logits_inputs(case):
    (h4, w4), (h1, w1), ch, k = case
    gen = torch.Generator().manual_seed(case_seed(case))
    p = torch.randn(N_LOGITS, k, h4, w4, generator=gen)
    c1 = torch.randn(N_LOGITS, ch, h1, w1, generator=gen)
    w = torch.randn(k, ch, generator=gen) * ch ** -0.5
    return p, c1, w, torch.randn(k, generator=gen), torch.randn(N_LOGITS, k, h1, w1, generator=gen)

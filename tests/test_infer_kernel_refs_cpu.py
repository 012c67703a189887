"""tests/infer_kernel_refs.py against torch's own modules in double, its pack formulas against their inverses, and the conditions under which
class X of tests/test_gpu_infer_kernels.py is exact, for every case of the tables.  No device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_kernel_refs as R  # noqa: E402

F64 = torch.float64
ACT_MODULES = {R.ACT_NONE: torch.nn.Identity, R.ACT_RELU: torch.nn.ReLU, R.ACT_HSWISH: torch.nn.Hardswish}


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


@pytest.mark.parametrize("cin,cout,k,stride,groups,act", [(24, 40, 1, 1, 1, R.ACT_RELU), (40, 40, 5, 2, 40, R.ACT_HSWISH), (24, 24, 3, 1, 24, R.ACT_NONE),
                                                          (3, 32, 3, 2, 1, R.ACT_RELU), (8, 8, 1, 1, 1, R.ACT_HSWISH)])
def test_fold_and_layer_are_conv_batchnorm_activation(cin, cout, k, stride, groups, act):
    g = torch.Generator().manual_seed(5 + cin + cout)
    conv = torch.nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False).double()
    bn = torch.nn.BatchNorm2d(cout).double().eval()
    p = R.bn_params(cout, g)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        bn.weight.copy_(p["gamma"]); bn.bias.copy_(p["beta"]); bn.running_mean.copy_(p["rmean"]); bn.running_var.copy_(p["rvar"])
        x = torch.randn(2, cin, 7, 9, generator=g).double()
        want = ACT_MODULES[act]()(bn(conv(x)))
    wf, bf = R.fold(conv.weight.detach(), p["gamma"], p["beta"], p["rmean"], p["rvar"], eps=bn.eps)
    _close(R.layer(x, wf, bf, k, stride, groups, act), want)
    # the device's eps is the float 1e-5f: 2.5e-13 below the double 1e-5, far inside any bound used here
    wd, _ = R.fold(conv.weight.detach(), p["gamma"], p["beta"], p["rmean"], p["rvar"])
    assert float((wd - wf).abs().max()) <= 1e-9 * float(wf.abs().max())


def test_fold_without_batchnorm_is_the_identity():
    w, beta = torch.randn(8, 8), torch.randn(8)
    wf, bf = R.fold(w, None, beta, None, None)
    assert torch.equal(wf, w.double()) and torch.equal(bf, beta.double())
    wf, bf = R.fold(w, None, None, None, None)
    assert torch.equal(wf, w.double()) and float(bf.abs().sum()) == 0.0


def test_wiring_references_are_torch():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 8, 3, 5, generator=g).double(), torch.randn(2, 24, 3, 5, generator=g).double()
    assert torch.equal(R.cat(a, b), torch.cat([a, b], 1))
    _close(R.avgpool(b), torch.nn.functional.adaptive_avg_pool2d(b, 1).flatten(1))
    lin = torch.nn.Linear(24, 21).double()
    x = torch.randn(3, 24, generator=g).double()
    _close(R.linear(x, lin.weight.detach(), lin.bias.detach()), lin(x).detach())
    x8 = torch.randn(2, 3, 7, 9, generator=g)
    conv = torch.nn.Conv2d(3, 8, 3, 2, 1).double()
    _close(R.stem(x8, conv.weight.detach(), conv.bias.detach(), R.ACT_RELU), torch.relu(conv(x8.bfloat16().double())).detach())
    u, v = torch.randn(64, generator=g).bfloat16(), (torch.randn(64, generator=g) * 2.0 ** 20).bfloat16()
    assert torch.equal(R.add(u, v), (u.double() + v.double()).float().bfloat16())      # exact in double, rounded once to fp32, once to bf16


def test_pack_formulas_invert():
    g = torch.Generator().manual_seed(9)
    for cout, cin in ((24, 40), (8, 8), (144, 320)):
        m = torch.randn(cout, cin, generator=g)
        flat = R.pack0(m)
        assert flat.numel() == R.round_up(cout, 16) * R.round_up(cin, 32)
        assert torch.equal(R.unpack0(flat, cout, cin), m)
        assert int((flat != 0).sum()) == int((m != 0).sum())                         # the padding is zero
        # the formula itself, at one element: (ct, kb, lane, e) -> (co, k)
        ct, kb, lane, e = (cout - 1) // 16, (cin - 1) // 32, 37, 5
        co, k = ct * 16 + (lane & 15), kb * 32 + (lane >> 4) * 8 + e
        want = m[co, k] if co < cout and k < cin else 0.0
        assert float(flat[((ct * (R.round_up(cin, 32) // 32) + kb) * 64 + lane) * 8 + e]) == float(want)
    for cout in (24, 32):
        w = torch.randn(cout, 3, 3, 3, generator=g)
        flat = R.pack2(w)
        assert flat.numel() == R.round_up(cout, 16) * 64 and torch.equal(R.unpack2(flat, cout), w)
        assert int((flat != 0).sum()) == w.numel()
    for k in (3, 5):
        w = torch.randn(24, 1, k, k, generator=g)
        flat = R.pack1(w)
        assert flat.numel() == k * k * 32 and torch.equal(R.unpack1(flat, 24, k), w)
        assert float(flat.reshape(k * k, 32)[4, 7]) == float(w[7, 0, 4 // k, 4 % k])


def _conditions(stats, numel_of, compared=None):
    """sum|term| < 2^24 at every layer; at least 25 % of every ReLU output nonzero; at least 64 distinct values in every output that is compared (the
    last layer of a composition; a single layer in either form).  Two caps that follow from the case's size alone.  A quarter of the elements, where a
    map has fewer than 256 of them (a 1 x 1 head map of three images holds 48 numbers).  And the spread the operands allow: with x in [-4, 4] (variance
    20/3), weights in {-1, 0, 1} (2/3) and sum|term| averaging 1.5 per product, an output of max sum|term| = m is a sum of about m / 1.5 products and
    has a standard deviation of about 1.7 sqrt(m); a linear output is asked for 2 sqrt(m) distinct integers (those within +-0.6 sigma, where every
    integer is hit once a few hundred elements are drawn), a ReLU output, which keeps the positive half, for sqrt(m).  An 8-channel layer (m about 25)
    is thus asked for 10 and 5 values, a 1 x 1 depthwise map under a 5 x 5 window (one tap inside the image, m = 7) for 5 and 2."""
    compared = compared or [not st[4] for st in stats]          # compositions: the last layer of a bottleneck, the 1x1 layers of the heads
    for (name, mx, nz, distinct, relu), numel, cmp in zip(stats, numel_of, compared):
        assert mx < R.EXACT_LIMIT, (name, mx)
        if relu:
            assert nz >= 0.25, (name, nz)
        if cmp:
            assert distinct >= min(64, numel // 4, int((1 if relu else 2) * mx ** 0.5)), (name, distinct, numel, mx)


def _block_geom(c):
    return {k: c[k] for k in ("cin", "r", "cexp", "cout", "k", "stride", "h", "w", "residual")}


ALL_BLOCKS = R.BLOCK_CASES + R.BLOCKW_CASES + R.EXTRA_CPU_BLOCKS


@pytest.mark.parametrize("c", ALL_BLOCKS, ids=lambda c: c["name"])
def test_block_cases_meet_the_conditions_of_the_exact_class(c):
    """... and the fp32 emulation (torch fp32 convolutions, bf16 roundings) equals the fp64 path bit for bit: summation order is immaterial."""
    tr = []
    ops, y, stats = R.int_case(R.block_seed(c), "block", n=2, **_block_geom(c))
    R.bottleneck(ops["x"], ops["sq"], ops["c1"], ops["dw"], ops["red"], c["k"], c["stride"], c["residual"], trace=tr)
    _conditions(stats, [t[2].numel() for t in tr])
    print("[infer-refs] %s: largest sum|term| %d" % (c["name"], max(s[1] for s in stats)))
    y32 = R.bottleneck(ops["x"], ops["sq"], ops["c1"], ops["dw"], ops["red"], c["k"], c["stride"], c["residual"], dtype=torch.float32)
    assert y32.dtype == torch.float32 and torch.equal(R.bits(y32), R.bits(y))
    # a flaw must show: without the last 8 K columns of the reduce conv most outputs change
    red = (ops["red"][0].clone(), ops["red"][1])
    red[0][:, -8:] = 0
    y0 = R.bottleneck(ops["x"], ops["sq"], ops["c1"], ops["dw"], red, c["k"], c["stride"], c["residual"])
    assert float((y0 != y).double().mean()) >= 0.5


def test_the_four_emulated_bottlenecks_are_in_the_tables():
    assert set(R.EMULATED) <= {c["name"] for c in ALL_BLOCKS}


@pytest.mark.parametrize("c", R.HEAD_CASES, ids=lambda c: "c%d_%dx%d_a%d" % c[:4])
def test_head_cases_meet_the_conditions_of_the_exact_class(c):
    cin, h, w, a, _ = c
    tr = []
    ops, (loc, conf), stats = R.int_case(R.head_seed(c), "heads", n=3, cin=cin, h=h, w=w, cl=R.round_up(4 * a, 8), cc=R.round_up(R.HEAD_CLASSES * a, 8))
    R.sep_heads(ops["x"], ops["dw_loc"], ops["pw_loc"], ops["dw_conf"], ops["pw_conf"], trace=tr)
    _conditions(stats, [t[2].numel() for t in tr])
    l32, c32 = R.sep_heads(ops["x"], ops["dw_loc"], ops["pw_loc"], ops["dw_conf"], ops["pw_conf"], dtype=torch.float32)
    assert torch.equal(l32.double(), loc) and torch.equal(c32.double(), conf)          # fp32 stores: the integers themselves


SINGLE = ([("pw", c) for c in R.PW_CASES] + [("dw", c) for c in R.DW_CASES] + [("stem", c) for c in R.STEM_CASES] + [("linear", c) for c in R.LIN_CASES]
          + [("avgpool", c) for c in R.POOL_CASES])


@pytest.mark.parametrize("group,c", SINGLE, ids=lambda v: str(v).replace(" ", ""))
def test_single_layer_cases_meet_the_conditions_of_the_exact_class(group, c):
    """Every entry of the single-layer tables, on the operands the GPU file uploads, in the linear and (where the kernel has one) the ReLU form: sum|term| <
    2^24, >= 25 % of a ReLU output nonzero, the distinct-value condition on the compared output of either form, and the fp32 evaluation bit-equal to fp64."""
    draw = dict(pw=R.pw_ints, dw=R.dw_ints, stem=R.stem_ints)
    forms = [(R.ACT_NONE,), (R.ACT_RELU,)] if group in draw else [()]
    for form in forms:
        ops, y, stats = (draw[group](c, *form) if group in draw else dict(linear=R.lin_ints, avgpool=R.pool_ints)[group](c))
        _conditions(stats, [y.numel()], compared=[True])
        if group == "linear":
            y32 = R.linear(ops["x"], ops["w"], ops["b"], torch.float32)
        elif group == "avgpool":
            y32 = ops["x"].float().sum((2, 3)) / torch.tensor(float(c[1]))
        else:
            k, st, gr = dict(pw=(1, 1, 1), dw=(c[0], c[1], c[2]) if group == "dw" else None, stem=(3, 2, 1))[group]
            y32 = R.layer(ops["x"], ops["w"], ops["b"], k, st, gr, form[0], torch.float32)
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), y.double())


def test_tie_slack_marks_only_weights_at_a_rounding_tie():
    w = torch.tensor([1.0, 1.00390625, 1.0 + 2.0 ** -8 + 1e-9, 0.3], dtype=F64)      # 1 + 2^-8 is the tie between 1 and 1 + 2^-7
    q, slack = R.bf16_weights(w)
    assert slack[0] == 0 and slack[3] == 0 and slack[1] == 2.0 ** -7 and slack[2] == 2.0 ** -7
    assert float((q - w).abs().max()) <= 2.0 ** -8 * (1 + R.TIE_RTOL)      # (the way through float rounds 1 + 2^-8 + 1e-9 onto the tie: what the slack is for)

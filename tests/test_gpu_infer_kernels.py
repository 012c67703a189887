"""The bf16 inference kernels (csrc/frost_infer.hip, frost_iblock.hip, frost_iblockw.hip, frost_ihead.hip, frost_infer_pw with its wide GEMM,
frost_linear_f32), one by one and by C-ABI entry name, against references of their own operation (tests/infer_kernel_refs.py; held to torch's
modules by tests/test_infer_kernel_refs_cpu.py).

Class X (exact): integer operands and gamma = NULL descriptors prepared by frost_infer_weight_prep.  Every partial sum is an integer below 2^24
(checked per case on the CPU), so the device must give the bits of the fp64 reference: torch.equal, no tolerance, no element left out.
Class T (tolerance): random operands as the device sees them (bf16 x, real BatchNorm parameters, the packs the prep kernel made) against fp64 of
the operation; the reference folds for itself.  E32 = the error against fp64 of the same quantity in plain fp32 torch ops.  The rule of
tests/test_gpu_float_kernels.py:
  bf16 results   3e-3 norm-wise over the tensor, 2^-8 + 8 E32 for the worst channel
  fp32 results   max(2e-6, 8 E32), twice that for the worst channel
  (E32 is the whole tensor's.  Where a tensor has ONE row -- one pixel, one image -- a channel is a single element that may cancel: the norms are
  then measured against the norms of sum|term|, device and yardstick alike, as that file's `den` does for its single-pixel batches.)
and element-wise, every element:  |dev - ref| <= 2^-8 |ref| + tau sum|term| + tie   (fp32 results: no 2^-8 term)
  2^-8        one round-to-nearest bf16 rounding
  tau         max(2e-6, 8 E32t), E32t = the largest |ref32 - ref| / sum|term| of the tensor; sum|term| includes the terms of the folded bias
  tie         sum |x| |bf16 neighbours' distance| over the weights whose fp64 fold lies within 3e-7 of a bf16 rounding tie: the device rounds its own
              fp32 fold, and either neighbour is correct there (about one weight in 10^4; zero for all others)
Buffers carry 64 elements of slack holding 7.0, results start as NaN (bit buffers as a fixed pattern); the slack is asserted untouched after every launch.
Every check prints `[infer-kernels] group what: observed / bound / E32`; DESIGN.md ("Inference kernels, one by one") lists the worst."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_kernel_refs as R  # noqa: E402
from float_kernel_refs import rel  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK, SENT, NAN = 64, 7.0, float("nan")
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NONE, RELU, HSWISH = R.ACT_NONE, R.ACT_RELU, R.ACT_HSWISH
ACTN = {NONE: "none", RELU: "relu", HSWISH: "hswish"}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib
    return _lib


# ================================================================================================ buffers
class _Buf:
    """numel elements (NaN, or `data`) and SLACK elements of sentinel behind them."""

    def __init__(self, numel, dtype, data=None, fill=NAN):
        self.n = int(numel)
        self.t = torch.full((self.n + SLACK,), SENT, dtype=dtype, device="cuda")
        self.t[: self.n] = fill if data is None else data.reshape(-1).to(dtype).cuda()

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr())

    def get(self, *shape):
        v = self.t[: self.n].cpu()
        return v.view(*shape) if shape else v

    def check(self):
        assert bool((self.t[self.n:].float() == SENT).all()), "the slack behind the tensor was written"


def _act(t_nchw):
    """NCHW reference-side activation -> NHWC bf16 device buffer"""
    return _Buf(t_nchw.numel(), BF, R.nhwc(t_nchw))


def _back(buf, n, h, w, c):
    """NHWC device result -> NCHW double"""
    return R.nchw(buf.get(n, h, w, c).double())


class _Lay:
    """Device state of one layer: parameters, FrostIDesc, pack and folded bias (both start as a pattern)."""

    def __init__(self, L, w, kind, bn=None, beta=None):
        w = w.float()
        self.kind, self.cout, self.cin_g, self.k = kind, w.shape[0], w.shape[1], w.shape[2]
        self.kk, self.cpad = self.k * self.k, R.round_up(self.cout, 16)
        self.kpad = 64 if kind == 2 else (R.round_up(self.cin_g, 32) if kind == 0 else 0)
        dev = lambda t: None if t is None else t.float().contiguous().cuda()
        self.w = dev(w)
        self.bn = {k: dev(v) for k, v in bn.items()} if bn is not None else None
        self.beta = dev(bn["beta"] if bn is not None else beta)
        if kind == 1:
            self.pack = _Buf(self.kk * self.cpad, F32, fill=-123.0)
        else:
            self.pack = _Buf(self.cpad * self.kpad, torch.int16, fill=0x5A5A)
        self.biasf = _Buf(self.cpad, F32, fill=-123.0)
        pt = lambda t: None if t is None else t.data_ptr()
        b = self.bn or {}
        self.desc = L.FrostIDesc(self.w.data_ptr(), pt(b.get("gamma")), pt(self.beta), pt(b.get("rmean")), pt(b.get("rvar")), self.pack.t.data_ptr(),
                                 self.biasf.t.data_ptr(), self.cout, self.cin_g, self.kk, kind, self.cpad, self.kpad, 0, 0)

    def check(self):
        self.pack.check()
        self.biasf.check()


def _prep(L, lays):
    table = (L.FrostIDesc * len(lays))(*[l.desc for l in lays])
    tab = L.struct_to_tensor(table, "cuda")
    L.call("frost_infer_weight_prep", L.ptr(tab), len(lays), L.stream())
    torch.cuda.synchronize()
    for l in lays:
        l.check()
    return lays


def _xlay(L, wb, kind):
    """class X layer: gamma = NULL, beta = the bias"""
    return _Lay(L, wb[0], kind, beta=wb[1])


# ================================================================================================ comparisons
def _note(group, what, obs, bound, e32=0.0):
    print(f"[infer-kernels] {group} {what}: observed {obs:.2e} bound {bound:.2e} E32 {e32:.2e}")


def _same_bits(group, what, dev, ref, dtype=BF):
    """class X: the bit patterns, every element"""
    a, b = dev.to(dtype), ref.to(dtype)
    it = torch.int16 if dtype == BF else torch.int32
    bad = int((a.contiguous().view(it) != b.contiguous().view(it)).sum())
    _note(group, what + " (differing elements)", bad, 0)
    assert a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it)), (group, what, bad, "of", a.numel())


def _hold(group, what, dev, ref, ref32, terms, storage, tie=None):
    """class T; all tensors with the channel as the LAST dimension.  A tensor of ONE row (one pixel, one image) has channels of a single element, which
    may be a sum that cancels: there the norms are measured against the norms of sum|term| (the `den` of tests/test_gpu_float_kernels.py), for the
    device and for the yardstick alike; the bounds are the rule's, with the whole tensor's E32."""
    assert bool(torch.isfinite(dev).all()), (group, what, "not finite")
    c = ref.shape[-1]
    d, d32 = (dev.double() - ref.double()).reshape(-1, c), (ref32.double() - ref.double()).reshape(-1, c)
    den = (terms if d.shape[0] == 1 else ref).double().reshape(-1, c)
    dn, dc = max(float(den.norm()), 1e-300), den.norm(dim=0).clamp_min(1e-300)
    whole, e32 = float(d.norm()) / dn, float(d32.norm()) / dn
    chan = float(torch.where(d.norm(dim=0) == 0, torch.zeros_like(dc), d.norm(dim=0) / dc).max())
    if storage == "bf16":
        bw, bc, u = 3e-3, R.BF16_U + 8 * e32, R.BF16_U
    else:
        bw = max(2e-6, 8 * e32)
        bc, u = 2 * bw, 0.0
    _note(group, what, whole, bw, e32)
    _note(group, what + " (worst channel)", chan, bc, e32)
    assert whole <= bw, (group, what, "whole tensor", whole, bw, e32)
    assert chan <= bc, (group, what, "worst channel", chan, bc, e32)
    t = terms.double().clamp_min(1e-300)
    e32t = float(((ref32.double() - ref.double()).abs() / t).max())
    tau = max(2e-6, 8 * e32t)
    err = (dev.double() - ref.double()).abs() - u * ref.double().abs()
    if tie is not None:
        err = err - tie.double()
    obs = float((err / t).max())
    _note(group, what + " (element-wise, in sum|term|)", max(obs, 0.0), tau, e32t)
    assert obs <= tau, (group, what, "element-wise", obs, tau, e32t)


class _TLayer:
    """class T operands of one conv + BatchNorm layer and its reference, folded from the parameters in fp64."""

    def __init__(self, L, g, cout, cin_g, k, kind, wscale=None):
        self.w = torch.randn(cout, cin_g, k, k, generator=g) * (wscale if wscale else (cin_g * k * k) ** -0.5)
        self.bnp = R.bn_params(cout, g)
        self.lay = _Lay(L, self.w, kind, bn=self.bnp)
        wf, self.b = R.fold(self.w, self.bnp["gamma"], self.bnp["beta"], self.bnp["rmean"], self.bnp["rvar"])
        self.wq, self.wtie = (wf, None) if kind == 1 else R.bf16_weights(wf)          # depthwise taps stay fp32
        self.bterms = R.fold_terms(self.bnp["gamma"], self.bnp["beta"], self.bnp["rmean"], self.bnp["rvar"])

    def refs(self, x, k=1, stride=1, groups=1):
        """pre-activation: (fp64, fp32 yardstick, sum|term|, tie slack), NCHW"""
        z = R.layer(x, self.wq, self.b, k, stride, groups)
        z32 = R.layer(x, self.wq, self.b, k, stride, groups, dtype=F32)
        terms = R.layer_terms(x, self.wq, None, k, stride, groups, bterms=self.bterms)
        tie = None if self.wtie is None else R.layer(x.abs(), self.wtie, None, k, stride, groups)
        return z, z32, terms, tie


def _t_input(draw, refs_of, acts=(NONE, RELU, HSWISH)):
    """(x, refs) of a class T case.  3e-3 norm-wise is what correctly rounded bf16 results of many elements keep (their rounding errors average about
    2^-8 / 3); a tensor of eight numbers can miss it by its own rounding alone, whose worst case is 2^-8 = 3.9e-3.  So x is drawn again from the same
    generator until the correctly rounded REFERENCE keeps 2.5e-3 for every activation: decided by the reference, nothing taken from the device."""
    for n in range(64):
        x = draw()
        refs = refs_of(x)
        if all(rel(R.rb(R.act_fwd(refs[0], a)), R.act_fwd(refs[0], a)) <= 2.5e-3 for a in acts):
            print(f"[infer-kernels] redraws {n} (outputs {refs[0].numel()})")
            return x, refs
    raise AssertionError("no input whose rounded reference keeps 2.5e-3")


def _hold_layer(group, what, dev_nchw, refs, act):
    z, z32, terms, tie = refs
    _hold(group, f"{what} {ACTN[act]}", R.nhwc(dev_nchw), R.nhwc(R.act_fwd(z, act)), R.nhwc(R.act_fwd(z32, act)), R.nhwc(terms), "bf16",
          None if tie is None else R.nhwc(tie))


# ================================================================================================ frost_infer_weight_prep
def _half_ulp_bf16(w):
    _, e = torch.frexp(w.double().abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(w, dtype=F64), e - 9)


def test_weight_prep_folds_and_packs(L):
    """One table, eleven descriptors in one launch (blockIdx.y): kind 0 (24, 40), (8, 8), (144, 320) -- the last has 46,080 pack elements, more than the
    64 x 256 threads, so the grid-stride loop runs -- kind 1 with 24 channels and 9 / 25 taps, kind 2 with 24 / 32 channels, and two gamma = NULL
    descriptors (with and without beta).  Channel 3 of the first descriptor has rvar = 0: eps alone carries the division."""
    g = torch.Generator().manual_seed(21)
    specs = [(0, 24, 40, 1), (0, 8, 8, 1), (0, 144, 320, 1), (1, 24, 1, 3), (1, 24, 1, 5), (2, 24, 3, 3), (2, 32, 3, 3)]
    items = []
    for i, (kind, cout, cin_g, k) in enumerate(specs):
        w = torch.randn(cout, cin_g, k, k, generator=g) * (cin_g * k * k) ** -0.5
        bn = R.bn_params(cout, g)
        if i == 0:
            bn["rvar"][3] = 0.0
        items.append((_Lay(L, w, kind, bn=bn), w, bn, None))
    wn = torch.randn(24, 40, 1, 1, generator=g)
    beta = torch.randn(24, generator=g)
    items.append((_Lay(L, wn, 0, beta=beta), wn, None, beta))
    wd = torch.randn(24, 1, 3, 3, generator=g)
    items.append((_Lay(L, wd, 1), wd, None, None))
    _prep(L, [it[0] for it in items])
    for lay, w, bn, beta in items:
        tag = f"kind{lay.kind} {lay.cout}x{lay.cin_g}x{lay.kk}" + ("" if bn else " no-bn")
        wf, bf = R.fold(w, *(bn[k] for k in ("gamma", "beta", "rmean", "rvar"))) if bn else R.fold(w, None, beta, None, None)
        bias = lay.biasf.get()
        assert torch.equal(bias[lay.cout:].view(torch.int32), torch.zeros(lay.cpad - lay.cout, dtype=torch.int32)), (tag, "bias padding")
        if bn:
            bt = R.fold_terms(*(bn[k] for k in ("gamma", "beta", "rmean", "rvar")))
            obs = float(((bias[: lay.cout].double() - bf).abs() / bt).max())
            _note("prep", tag + " bias (in the size of its terms)", obs, 2e-6)
            assert obs <= 2e-6, (tag, obs)
        else:
            assert torch.equal(bias[: lay.cout], bf.float()), (tag, "bias without BatchNorm is beta (or zero) itself")
        if lay.kind == 1:
            dev = lay.pack.get(lay.kk, lay.cpad)
            assert torch.equal(dev[:, lay.cout:].contiguous().view(torch.int32), torch.zeros(lay.kk, lay.cpad - lay.cout, dtype=torch.int32)), (tag, "tap padding")
            want = R.pack1(wf).reshape(lay.kk, lay.cpad)[:, : lay.cout]
            obs = float(((dev[:, : lay.cout].double() - want).abs() / want.abs().clamp_min(1e-300)).max())
            _note("prep", tag + " taps", obs, 0.0 if not bn else 2e-6)
            assert obs <= (2e-6 if bn else 0.0), (tag, obs)
            continue
        pk = lay.pack.get()
        wm = R.FR.stem_matrix(wf) if lay.kind == 2 else wf.reshape(lay.cout, lay.cin_g)
        want = torch.zeros(lay.cpad, lay.kpad, dtype=F64)
        want[: lay.cout, : wm.shape[1]] = wm
        devm = R.FR.unpack_matrix(pk.float(), lay.cpad, lay.kpad, 32)                # int16 bit patterns as numbers: exact below 2^24
        devbits = devm.to(torch.int32).to(torch.int16)
        pad = want == 0                                                               # rows co >= cout, columns k >= cin_g, stem slots c == 3 / tap >= 9
        if lay.kind == 2:
            slot = torch.zeros(16, 4, dtype=torch.bool)
            slot[9:, :] = True
            slot[:, 3] = True
            assert bool(pad[: lay.cout][:, slot.reshape(-1)].all())
        assert int(pad.sum()) == lay.cpad * lay.kpad - w.numel() and bool((devbits[pad] == 0).all()), (tag, "pack padding is not zero bits")
        devw = devbits.view(BF).double()
        if bn:
            exc = (devw - want).abs() - _half_ulp_bf16(want) - 2e-6 * want.abs()
            obs = float(exc[~pad].max())
            _note("prep", tag + " weights (beyond half a bf16 ulp + 2e-6 |W'|)", max(obs, 0.0), 0.0)
            assert obs <= 0.0, (tag, obs)
        else:
            assert torch.equal(devbits, R.bits(want)), (tag, "pack without BatchNorm is bf16(W)")


# ================================================================================================ frost_infer_pw
def _pw(L, lay, xbuf, npix, cin, act):
    y = _Buf(npix * lay.cout, BF)
    L.call("frost_infer_pw", xbuf.p, lay.pack.p, lay.biasf.p, npix, cin, lay.cout, act, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), xbuf.check(), lay.check()
    return y


@pytest.mark.parametrize("npix,cin,cout", R.PW_CASES, ids=lambda v: str(v))
def test_pointwise(L, npix, cin, cout):
    """frost_infer_pw on every branch of its dispatch (the case table of tests/infer_kernel_refs.py names the threshold each shape crosses): class X
    with act 0 / 1 bit-equal to the reference, class T with act 0 / 1 / 2 within the rule."""
    ops, z, _ = R.pw_ints((npix, cin, cout))
    g = torch.Generator().manual_seed(R.pw_seed((npix, cin, cout)))
    tl = _TLayer(L, g, cout, cin, 1, 0)
    xl = _xlay(L, (ops["w"], ops["b"]), 0)
    _prep(L, [xl, tl.lay])
    xb = _act(ops["x"])
    for act in (NONE, RELU):
        y = _pw(L, xl, xb, npix, cin, act)
        _same_bits("pw", f"X {npix}x{cin}x{cout} {ACTN[act]}", _back(y, 1, 1, npix, cout), R.act_fwd(z, act))
    xt, refs = _t_input(lambda: R.rb(torch.randn(1, cin, 1, npix, generator=g).double()), tl.refs)
    xb = _act(xt)
    for act in (NONE, RELU, HSWISH):
        y = _pw(L, tl.lay, xb, npix, cin, act)
        _hold_layer("pw", f"T {npix}x{cin}x{cout}", _back(y, 1, 1, npix, cout), refs, act)


# ================================================================================================ frost_infer_dw
def _out_hw(h, w, k, s):
    p = (k - 1) // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _dw(L, lay, xbuf, n, h, w, c, k, s, act):
    ho, wo = _out_hw(h, w, k, s)
    y = _Buf(n * ho * wo * c, BF)
    L.call("frost_infer_dw", xbuf.p, lay.pack.p, lay.biasf.p, n, h, w, c, k, s, act, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), xbuf.check(), lay.check()
    return y, ho, wo


@pytest.mark.parametrize("k,s,c,h,w", R.DW_CASES, ids=lambda v: str(v))
def test_depthwise(L, k, s, c, h, w):
    """frost_infer_dw, batch 2: class X with dense taps in {-1, 0, 1} (every tap position matters) bit-equal, class T within the rule."""
    n = 2
    ops, z, _ = R.dw_ints((k, s, c, h, w), n=n)
    g = torch.Generator().manual_seed(R.dw_seed((k, s, c, h, w)))
    tl = _TLayer(L, g, c, 1, k, 1, wscale=0.5)
    xl = _xlay(L, (ops["w"], ops["b"]), 1)
    _prep(L, [xl, tl.lay])
    xb = _act(ops["x"])
    for act in (NONE, RELU):
        y, ho, wo = _dw(L, xl, xb, n, h, w, c, k, s, act)
        _same_bits("dw", f"X k{k}s{s} c{c} {h}x{w} {ACTN[act]}", _back(y, n, ho, wo, c), R.act_fwd(z, act))
    xt, refs = _t_input(lambda: R.rb(torch.randn(n, c, h, w, generator=g).double()), lambda x: tl.refs(x, k, s, c))
    xb = _act(xt)
    for act in (NONE, RELU, HSWISH):
        y, ho, wo = _dw(L, tl.lay, xb, n, h, w, c, k, s, act)
        _hold_layer("dw", f"T k{k}s{s} c{c} {h}x{w}", _back(y, n, ho, wo, c), refs, act)


# ================================================================================================ the stem, both ways
def _image(x, layout):
    """the logical (N, 3, H, W) fp32 image on the device in one of three memory layouts -> (tensor view, keep-alive)"""
    n, _, h, w = x.shape
    if layout == "nchw":
        t = x.float().contiguous().cuda()
    elif layout == "nhwc":
        t = x.float().cuda().contiguous(memory_format=torch.channels_last)
    else:                                                                             # a crop of a larger image: sh != w * sw
        big = torch.full((n, 3, h + 3, w + 5), 99.0, dtype=F32, device="cuda")
        t = big[:, :, 1: 1 + h, 2: 2 + w]
        t.copy_(x.float())
    assert tuple(t.shape) == tuple(x.shape) and torch.equal(t.cpu(), x.float())
    return t


def _stem_both(L, lay, img, act):
    n, _, h, w = img.shape
    ho, wo = _out_hw(h, w, 3, 2)
    npix = n * ho * wo
    st = [img.stride(i) for i in range(4)]
    y = _Buf(npix * lay.cout, BF)
    L.call("frost_infer_stem", C.c_void_p(img.data_ptr()), n, h, w, *st, lay.pack.p, lay.biasf.p, lay.cout, act, y.p, L.stream())
    col = _Buf(npix * 64, BF)
    L.call("frost_infer_stem_im2col", C.c_void_p(img.data_ptr()), n, h, w, *st, col.p, L.stream())
    torch.cuda.synchronize()
    y.check(), col.check(), lay.check()
    y2 = _pw(L, lay, col, npix, 64, act)
    return _back(y, n, ho, wo, lay.cout), _back(y2, n, ho, wo, lay.cout)


@pytest.mark.parametrize("h,w,cout,layout", R.STEM_CASES, ids=lambda v: str(v))
def test_stem_direct_and_im2col(L, h, w, cout, layout):
    """frost_infer_stem and frost_infer_stem_im2col + frost_infer_pw, batch 2, three memory layouts of the image: each against the reference (X: bits;
    T: the rule) and the two bit-equal to each other in both classes."""
    n = 2
    ops, z, _ = R.stem_ints((h, w, cout, layout), n=n)
    xi, wx, bx = ops["x"], ops["w"], ops["b"]
    g = torch.Generator().manual_seed(R.stem_seed((h, w, cout, layout)))
    tl = _TLayer(L, g, cout, 3, 3, 2)
    xl = _xlay(L, (wx, bx), 2)
    _prep(L, [xl, tl.lay])
    img = _image(xi, layout)
    assert torch.equal(z, R.stem(xi, wx, bx, NONE))
    for act in (NONE, RELU):
        a, b = _stem_both(L, xl, img, act)
        _same_bits("stem", f"X direct {h}x{w} c{cout} {layout} {ACTN[act]}", a, R.act_fwd(z, act))
        _same_bits("stem", f"X im2col {h}x{w} c{cout} {layout} {ACTN[act]}", b, R.act_fwd(z, act))
    xt, refs = _t_input(lambda: torch.randn(n, 3, h, w, generator=g), lambda x: tl.refs(R.rb(x.double()), 3, 2, 1))
    img = _image(xt, layout)
    for act in (NONE, RELU, HSWISH):
        a, b = _stem_both(L, tl.lay, img, act)
        _hold_layer("stem", f"T direct {h}x{w} c{cout} {layout}", a, refs, act)
        _same_bits("stem", f"T direct == im2col {h}x{w} c{cout} {layout} {ACTN[act]}", a, b)


# ================================================================================================ cat / add / pool / linear
def _wild_bf16(g, *shape):
    """random bf16 values whose exponents spread over 2^-20 .. 2^20, some zeros"""
    v = torch.randn(*shape, generator=g) * torch.pow(2.0, torch.randint(-20, 21, shape, generator=g).float())
    return torch.where(torch.rand(*shape, generator=g) < 0.05, torch.zeros(()), v).bfloat16()


@pytest.mark.parametrize("ca,cb,npix", R.CAT_CASES, ids=lambda v: str(v))
def test_cat(L, ca, cb, npix):
    g = torch.Generator().manual_seed(ca + cb + npix)
    a, b = _wild_bf16(g, npix, ca), _wild_bf16(g, npix, cb)
    ab, bb, y = _Buf(a.numel(), BF, a), _Buf(b.numel(), BF, b), _Buf(npix * (ca + cb), BF)
    L.call("frost_infer_cat", ab.p, ca, bb.p, cb, npix, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), ab.check(), bb.check()
    _same_bits("cat", f"{ca}+{cb} x {npix}", y.get(npix, ca + cb), torch.cat([a, b], 1))


@pytest.mark.parametrize("n", R.ADD_CASES)
def test_add(L, n):
    """bit-equal to (a.float() + b.float()).bfloat16(); the pairs include exponents more than 16 apart (the smaller operand only decides a tie)."""
    g = torch.Generator().manual_seed(n)
    a, b = _wild_bf16(g, n), _wild_bf16(g, n)
    assert n < 64 or bool(((torch.frexp(a.float())[1] - torch.frexp(b.float())[1]).abs() > 16).any())
    ab, bb, y = _Buf(n, BF, a), _Buf(n, BF, b), _Buf(n, BF)
    L.call("frost_infer_add", ab.p, bb.p, n, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), ab.check(), bb.check()
    _same_bits("add", f"n {n}", y.get(), R.add(a, b))


@pytest.mark.parametrize("n,hw,c", R.POOL_CASES, ids=lambda v: str(v))
def test_avgpool(L, n, hw, c):
    g = torch.Generator().manual_seed(n + hw + c)
    xi = R.pool_ints((n, hw, c))[0]["x"]
    xt = R.rb(torch.randn(n, c, 1, hw, generator=g).double() + 0.5)
    for cls, x in (("X", xi), ("T", xt)):
        xb, y = _act(x), _Buf(n * c, F32)
        L.call("frost_infer_avgpool", xb.p, n, hw, c, y.p, L.stream())
        torch.cuda.synchronize()
        y.check(), xb.check()
        if cls == "X":
            _same_bits("avgpool", f"X {n}x{hw}x{c}", y.get(n, c), R.avgpool_exact(x), F32)
        else:
            _hold("avgpool", f"T {n}x{hw}x{c}", y.get(n, c), R.avgpool(x), R.avgpool(x, F32), R.avgpool(x.abs()), "fp32")


@pytest.mark.parametrize("n,k,o", R.LIN_CASES, ids=lambda v: str(v))
def test_linear(L, n, k, o):
    """frost_linear_f32 across launch_sgemm's rules (K split in two from K = 128, 64-deep stages from K / ks = 256); class X twice with equal bits: the
    split adds its halves through atomics."""
    g = torch.Generator().manual_seed(n + k + o)
    xi, wi, bi = (R.lin_ints((n, k, o))[0][key] for key in ("x", "w", "b"))
    xt, wt, bt = torch.randn(n, k, generator=g), torch.randn(o, k, generator=g) * k ** -0.5, torch.randn(o, generator=g) * 0.1
    for cls, (x, w, b) in (("X", (xi, wi, bi)), ("X again", (xi, wi, bi)), ("T", (xt, wt, bt))):
        xb, wb, bb, y = _Buf(n * k, F32, x), _Buf(o * k, F32, w), _Buf(o, F32, b), _Buf(n * o, F32)
        L.call("frost_linear_f32", xb.p, wb.p, bb.p, n, k, o, y.p, L.stream())
        torch.cuda.synchronize()
        y.check(), xb.check(), wb.check(), bb.check()
        if cls != "T":
            _same_bits("linear", f"{cls} {n}x{k}x{o}", y.get(n, o), R.linear(x, w, b), F32)
        else:
            _hold("linear", f"T {n}x{k}x{o}", y.get(n, o), R.linear(x, w, b), R.linear(x, w, b, F32), R.linear(x.abs(), w.abs(), b.abs()), "fp32")


# ================================================================================================ the bottleneck kernels
def _geom(c):
    return {k: c[k] for k in ("cin", "r", "cexp", "cout", "k", "stride", "h", "w", "residual")}


def _has_conv1(c):
    return c["cexp"] != c["cin"] or c["r"] > 0


def _block_lays_x(L, ops):
    lays = dict(sq=_xlay(L, ops["sq"], 0) if ops["sq"] else None, c1=_xlay(L, ops["c1"], 0) if ops["c1"] else None, dw=_xlay(L, ops["dw"], 1),
                red=_xlay(L, ops["red"], 0))
    _prep(L, [l for l in lays.values() if l is not None])
    return lays


def _block_lays_t(L, g, c):
    mk = lambda cout, cin_g, k, kind: _TLayer(L, g, cout, cin_g, k, kind, wscale=0.5 if kind == 1 else None).lay
    lays = dict(sq=mk(c["r"], c["cin"], 1, 0) if c["r"] else None, c1=mk(c["cexp"], c["r"] + c["cin"], 1, 0) if _has_conv1(c) else None,
                dw=mk(c["cexp"], 1, c["k"], 1), red=mk(c["cout"], c["cexp"], 1, 0))
    _prep(L, [l for l in lays.values() if l is not None])
    return lays


def _layers_block(L, lays, xb, n, c):
    """the bottleneck as layer launches, as Bf16Inference._block_plain chains them"""
    h, w, cin, npix = c["h"], c["w"], c["cin"], n * c["h"] * c["w"]
    a, ch = xb, cin
    if lays["c1"] is not None:
        if lays["sq"] is not None:
            s = _pw(L, lays["sq"], a, npix, cin, RELU)
            cat = _Buf(npix * (c["r"] + cin), BF)
            L.call("frost_infer_cat", s.p, c["r"], a.p, cin, npix, cat.p, L.stream())
            a, ch = cat, c["r"] + cin
        a, ch = _pw(L, lays["c1"], a, npix, ch, RELU), c["cexp"]
    a, ho, wo = _dw(L, lays["dw"], a, n, h, w, ch, c["k"], c["stride"], RELU)
    a = _pw(L, lays["red"], a, n * ho * wo, ch, NONE)
    if c["residual"]:
        out = _Buf(n * ho * wo * c["cout"], BF)
        L.call("frost_infer_add", xb.p, a.p, n * ho * wo * c["cout"], out.p, L.stream())
        torch.cuda.synchronize()
        out.check()
        a = out
    return _back(a, n, ho, wo, c["cout"])


def _pp(l):
    return (None, None) if l is None else (l.pack.p, l.biasf.p)


def _fused_block(L, lays, xb, n, c, th, tw, waves, chunk, out=None):
    ho, wo = _out_hw(c["h"], c["w"], c["k"], c["stride"])
    y = out or _Buf(n * ho * wo * c["cout"], BF)
    L.call("frost_infer_block", xb.p, *_pp(lays["sq"]), *_pp(lays["c1"]), *_pp(lays["dw"]), *_pp(lays["red"]), n, c["h"], c["w"], c["cin"], c["r"],
           c["cexp"], c["cout"], c["k"], c["stride"], c["residual"], th, tw, waves, chunk, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), xb.check()
    for l in lays.values():
        if l is not None:
            l.check()
    return _back(y, n, ho, wo, c["cout"])


def _wave_block(L, lays, xb, n, c, th, tw, out=None):
    ho, wo = _out_hw(c["h"], c["w"], c["k"], c["stride"])
    y = out or _Buf(n * ho * wo * c["cout"], BF)
    L.call("frost_infer_block_w", xb.p, *_pp(lays["c1"]), *_pp(lays["dw"]), *_pp(lays["red"]), n, c["h"], c["w"], c["cin"], c["cexp"], c["cout"], c["k"],
           c["stride"], c["residual"], th, tw, y.p, L.stream())
    torch.cuda.synchronize()
    y.check(), xb.check()
    return _back(y, n, ho, wo, c["cout"])


def _tile(c, th, tw):
    ho, wo = _out_hw(c["h"], c["w"], c["k"], c["stride"])
    return (ho, wo) if th == 0 else (th, tw)


def _pixel_norm(group, what, dev, lay):
    """class T of the fused kernels, against the layer launches: per output pixel, norm over the channels <= 2^-7 (an element is at most one bf16 ulp off)"""
    d, r = R.nhwc(dev - lay).norm(dim=-1), R.nhwc(lay).norm(dim=-1).clamp_min(1e-300)
    obs = float((d / r).max())
    _note(group, what + " (worst pixel, against the layer launches)", obs, 2.0 ** -7)
    assert bool(torch.isfinite(dev).all()) and obs <= 2.0 ** -7, (group, what, obs)


@pytest.mark.parametrize("c", R.BLOCK_CASES, ids=lambda c: c["name"])
def test_block(L, c):
    """frost_infer_block, batch 2, tile / waves / chunk given explicitly; class X against the fp64 reference and the layer launches (bits), class T against
    the layer launches.  The instance k_iblock<K, S, MAXT, KB1M, NW, CH> each variant engages (MAXT from ceil(ct3 tpt / waves), KB1M 2 for conv1 K <= 64):
      sq24_72_k5      24+8 -> 72 -> 24, k5 s1, 7x9, residual: whole map <5,1,4,2,4,64> (72 = 64 + 8: a partial chunk; cout % 16 == 8);
                      tile 4x4 <5,1,4,2,4,32> (ragged on both axes, 72 = 32 + 32 + 8)
      nosq16_96_k3s2  16 -> 96 -> 24, k3 s2, 9x11, tile 4x8: <3,2,4,2,4,32> and <3,2,4,2,4,64>
      noconv1_32      32 -> 32 -> 16 without conv1, k3 s1, 6x6: <3,1,4,2,4,64>
      sq40_240_k5s2   40+16 -> 240 -> 40, k5 s2, 8x8: the row stride r + round_up(cin, 32) = 80; tiles 4x4 and 3x3 (9 < 16 pixels): <5,2,4,2,4,64>
      sq104_624_k5    104+24 -> 624 -> 104, k5 s1, 7x7 whole map, kb1 = 4: <5,1,8,10,4,64>, <5,1,4,10,8,64>, <5,1,4,10,16,64> (7, 4, 2 accumulators)
      kb1_10          256+64 -> 96 -> 24: r + cin = 320, kb1 = 10, the most the kernel holds: <3,1,4,10,4,64>
      acc_cout320     40+8 -> 64 -> 320, k3 s1, 7x7: 4x4 at 8 / 4 waves = 3 / 5 accumulators (MAXT 4, 8), 7x7 at 8 / 4 waves = 10 / 20 (MAXT 12, 20),
                      4x7 at 4 waves = 10 (MAXT 12 in the 4-wave instance)"""
    n = 2
    ops, y, _ = R.int_case(R.block_seed(c), "block", n=n, **_geom(c))
    lays = _block_lays_x(L, ops)
    xb = _act(ops["x"])
    lay_out = _layers_block(L, lays, xb, n, c)
    _same_bits("block", f"X {c['name']} layer launches", lay_out, y)
    g = torch.Generator().manual_seed(R.block_seed(c) + 1)
    tlays = _block_lays_t(L, g, c)
    xtb = _act(R.rb(torch.randn(n, c["cin"], c["h"], c["w"], generator=g).double()))
    tlay_out = _layers_block(L, tlays, xtb, n, c)
    for th, tw, waves, chunk in c["variants"]:
        th, tw = _tile(c, th, tw)
        assert L.load_library().frost_infer_block_ok(c["h"], c["w"], c["cin"], c["r"], c["cexp"], c["cout"], c["k"], c["stride"], th, tw) > 0
        tag = f"{c['name']} tile {th}x{tw} waves {waves} chunk {chunk}"
        out = _fused_block(L, lays, xb, n, c, th, tw, waves, chunk)
        _same_bits("block", f"X {tag} against the reference", out, y)
        _same_bits("block", f"X {tag} against the layer launches", out, lay_out)
        _pixel_norm("block", f"T {tag}", _fused_block(L, tlays, xtb, n, c, th, tw, waves, chunk), tlay_out)


def test_block_refusals(L):
    """r + cin = 352 (kb1 = 11), more than 20 accumulators per wave, 16 waves with more than 4, chunk 32 with conv1 K > 64, a residual with stride 2:
    each returns an error and writes nothing."""
    base = dict(cin=40, r=8, cexp=64, cout=320, k=3, stride=1, h=7, w=7, residual=0)
    bad = [("r + cin = 352", dict(base, cin=288, r=64, cout=24), (4, 4, 4, 64), True),
           ("25 accumulators per wave", dict(base, h=8, w=9), (8, 9, 4, 64), True),
           ("16 waves, 5 accumulators", base, (7, 7, 16, 64), False),
           ("chunk 32 with K = 128", dict(base, cin=104, r=24, cout=24), (4, 4, 4, 32), False),
           ("residual with stride 2", dict(base, cin=24, cout=24, stride=2, residual=1), (4, 4, 4, 64), False)]
    lib = L.load_library()
    for what, c, (th, tw, waves, chunk), not_ok in bad:
        assert (lib.frost_infer_block_ok(c["h"], c["w"], c["cin"], c["r"], c["cexp"], c["cout"], c["k"], c["stride"], th, tw) <= 0) == not_ok, what
        ops, _, _ = R.int_case(5, "block", n=1, **dict(c, residual=0))
        lays = _block_lays_x(L, ops)
        xb = _act(ops["x"])
        ho, wo = _out_hw(c["h"], c["w"], c["k"], c["stride"])
        out = _Buf(ho * wo * c["cout"], BF, fill=3.0)
        with pytest.raises(RuntimeError):
            _fused_block(L, lays, xb, 1, c, th, tw, waves, chunk, out=out)
        torch.cuda.synchronize()
        out.check()
        assert bool((out.get().float() == 3.0).all()), (what, "a refused launch wrote")


@pytest.mark.parametrize("c", R.BLOCKW_CASES, ids=lambda c: c["name"])
def test_block_wave(L, c):
    """frost_infer_block_w, batch 2, wave tiles 4x4 and 4x8 on ragged maps: class X against the reference, the layer launches and frost_infer_block
    (chunk 32 where conv1's K allows it, else 64), all bit-equal."""
    n = 2
    ops, y, _ = R.int_case(R.block_seed(c), "block", n=n, **_geom(c))
    lays = _block_lays_x(L, ops)
    xb = _act(ops["x"])
    lay_out = _layers_block(L, lays, xb, n, c)
    _same_bits("block_w", f"X {c['name']} layer launches", lay_out, y)
    chunk = 32 if R.round_up(c["cin"], 32) <= 64 else 64
    for th, tw in c["variants"]:
        assert L.load_library().frost_infer_block_w_ok(c["cin"], 0, c["cexp"], c["cout"], c["k"], c["stride"], int(_has_conv1(c)), th, tw) == 1
        out = _wave_block(L, lays, xb, n, c, th, tw)
        _same_bits("block_w", f"X {c['name']} tile {th}x{tw} against the reference", out, y)
        _same_bits("block_w", f"X {c['name']} tile {th}x{tw} against the layer launches", out, lay_out)
        _same_bits("block_w", f"X {c['name']} tile {th}x{tw} against frost_infer_block chunk {chunk}", out, _fused_block(L, lays, xb, n, c, th, tw, 4, chunk))


def test_block_wave_refusals(L):
    """cout = 56, cin = 40 with conv1, k5 s1: frost_infer_block_w_ok says no, the launch returns an error and writes nothing."""
    lib = L.load_library()
    base = dict(cin=24, r=0, cexp=72, cout=24, k=3, stride=1, h=5, w=7, residual=0)
    for what, c in (("cout = 56", dict(base, cout=56)), ("cin = 40 with conv1", dict(base, cin=40)), ("k5 s1", dict(base, k=5))):
        assert lib.frost_infer_block_w_ok(c["cin"], 0, c["cexp"], c["cout"], c["k"], c["stride"], 1, 4, 4) == 0, what
        ops, _, _ = R.int_case(6, "block", n=1, **c)
        lays = _block_lays_x(L, ops)
        ho, wo = _out_hw(c["h"], c["w"], c["k"], c["stride"])
        out = _Buf(ho * wo * c["cout"], BF, fill=3.0)
        with pytest.raises(RuntimeError):
            _wave_block(L, lays, _act(ops["x"]), 1, c, 4, 4, out=out)
        torch.cuda.synchronize()
        out.check()
        assert bool((out.get().float() == 3.0).all()), (what, "a refused launch wrote")


# ================================================================================================ frost_infer_head
PATTERN = -55.5


@pytest.mark.parametrize("c", R.HEAD_CASES, ids=lambda c: "c%d_%dx%d_a%d_off%d" % (c[0], c[1], c[2], c[3], c[4][0]))
def test_head(L, c):
    """frost_infer_head, batch 3, class X: fp32 loc / conf equal to the reference (the integers themselves), bf16(loc / conf) bit-equal to frost_infer_dw +
    frost_infer_pw, and every element of loc / conf outside the source's slot untouched.  A = 4 with zero offsets and rows that are multiples of 4 floats
    takes the vector store (conf: 84 of 96 computed channels stored); A = 6 (conf 126) and the offsets (6, 21) take the scalar store."""
    cin, h, w, a, (loff, coff) = c
    n, wl, wc = 3, 4 * a, R.HEAD_CLASSES * a
    cl, cc = R.round_up(wl, 8), R.round_up(wc, 8)
    ops, (loc, conf), _ = R.int_case(R.head_seed(c), "heads", n=n, cin=cin, h=h, w=w, cl=cl, cc=cc)
    lays = [_xlay(L, ops["dw_loc"], 1), _xlay(L, ops["pw_loc"], 0), _xlay(L, ops["dw_conf"], 1), _xlay(L, ops["pw_conf"], 0)]
    _prep(L, lays)
    xb = _act(ops["x"])
    assert L.load_library().frost_infer_head_ok(h, w, cin, wl, wc) == 1
    ls, cs = R.round_up(loff + h * w * wl + 5, 4), R.round_up(coff + h * w * wc + 5, 4)
    lb, cb = _Buf(n * ls, F32, fill=PATTERN), _Buf(n * cs, F32, fill=PATTERN)
    L.call("frost_infer_head", xb.p, lays[0].pack.p, lays[0].biasf.p, lays[1].pack.p, lays[1].biasf.p, lays[2].pack.p, lays[2].biasf.p, lays[3].pack.p,
           lays[3].biasf.p, n, h, w, cin, wl, wc, lb.p, ls, loff, cb.p, cs, coff, L.stream())
    torch.cuda.synchronize()
    lb.check(), cb.check(), xb.check()
    for l in lays:
        l.check()
    for name, buf, stride, off, width, ref, dwl, pwl in (("loc", lb, ls, loff, wl, loc, lays[0], lays[1]), ("conf", cb, cs, coff, wc, conf, lays[2], lays[3])):
        rows = buf.get(n, stride)
        slot = rows[:, off: off + h * w * width]
        rest = torch.cat([rows[:, :off], rows[:, off + h * w * width:]], 1)
        assert bool((rest == PATTERN).all()), (name, "written outside the source's slot")
        want = R.nhwc(ref)[..., :width].reshape(n, -1)
        tag = f"X c{cin} {h}x{w} A{a} off {off} {name}"
        _same_bits("head", tag + " against the reference (fp32)", slot, want, F32)
        t, _, _ = _dw(L, dwl, xb, n, h, w, cin, 3, 1, RELU)
        y = _pw(L, pwl, t, n * h * w, cin, NONE).get(n, h * w, pwl.cout)[:, :, :width].reshape(n, -1)
        _same_bits("head", tag + " against frost_infer_dw + frost_infer_pw (bf16)", slot, y)


def test_head_refuses_eleven_channel_tiles(L):
    lib = L.load_library()
    assert lib.frost_infer_head_ok(2, 3, 8, 16, 160) == 0 and lib.frost_infer_head_ok(2, 3, 8, 16, 144) == 1
    ops, _, _ = R.int_case(7, "heads", n=1, cin=8, h=2, w=3, cl=16, cc=160)
    lays = [_xlay(L, ops["dw_loc"], 1), _xlay(L, ops["pw_loc"], 0), _xlay(L, ops["dw_conf"], 1), _xlay(L, ops["pw_conf"], 0)]
    _prep(L, lays)
    xb = _act(ops["x"])
    lb, cb = _Buf(6 * 16, F32, fill=PATTERN), _Buf(6 * 160, F32, fill=PATTERN)
    with pytest.raises(RuntimeError):
        L.call("frost_infer_head", xb.p, lays[0].pack.p, lays[0].biasf.p, lays[1].pack.p, lays[1].biasf.p, lays[2].pack.p, lays[2].biasf.p, lays[3].pack.p,
               lays[3].biasf.p, 1, 2, 3, 8, 16, 160, lb.p, 96, 0, cb.p, 960, 0, L.stream())
    torch.cuda.synchronize()
    assert bool((lb.get() == PATTERN).all()) and bool((cb.get() == PATTERN).all())

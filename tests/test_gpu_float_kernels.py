"""The float trainer's pointwise, BatchNorm and wiring kernels (csrc/frost_float.hip, frost_float_head_bwd of frost_head.hip), one by one,
against fp64 references of the operands the device sees (tests/float_kernel_refs.py; held to torch's autograd by
tests/test_float_kernel_refs_cpu.py).  Shapes follow the launch code's own thresholds: pixel tails around the 16- and 64-row tiles, K tails
below one 64-byte step, cout % 16 != 0, pixel-split / channel-split waves, coefficient rows in LDS or not, channel tiles dealt over
gridDim.y, several tiles per statistics workgroup, the pixel split of the weight gradient.

Tolerances (one rule, nothing taken from the device): E32 = the error against fp64 of the same quantity in plain fp32 torch ops.
  fp32 storage (outputs, dW, dx)   max(2e-6, 8 E32) norm-wise over the tensor, twice that for the worst output channel
  bf16 storage                     3e-3 over the tensor, 2^-8 + 8 E32 for the worst channel
  dW in bf16 mode                  max(2e-5, 8 E32)
  sums (sum, sum of squares, S1, S2)  per channel |delta| <= tau * sum|term|, tau = max(1e-6, 8 E32) (fp32 mode), max(4e-6, 8 E32) (bf16 mode)
  coefficient rows                 element-wise, 2e-6 of the size of their terms; 1e-12 for what is computed in double before the cast
The incoming gradient is zeroed where the pre-activation lies within 1e-5 of a kink of the activation's derivative (band_mask): either
outcome of the device's fp32 comparison then gives the same sums and dc, and no element is left out of a comparison.
Every check prints `[float-kernels] group what precision: observed / bound / E32`; DESIGN.md ("Float kernels, one by one") lists the worst."""
import ctypes as C
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
PRECS = ["bf16", "fp32"]
SLACK = 64                  # elements behind every activation buffer, as the trainer allocates them (FAct)
NAN = float("nan")
SENT = 7.0                  # exactly representable in bf16: columns and slack a kernel must not touch
E = {  # the C-ABI entry of either precision, by name
    "pw": {"bf16": "frost_float_pw", "fp32": "frost_float_pw_f32"},
    "ew": {"bf16": "frost_float_ew", "fp32": "frost_float_ew_f32"},
    "wgrad": {"bf16": "frost_float_pw_wgrad", "fp32": "frost_float_pw_wgrad_f32"},
    "merge": {"bf16": "frost_float_grad_merge", "fp32": "frost_float_grad_merge_f32"},
    "avgpool": {"bf16": "frost_float_avgpool", "fp32": "frost_float_avgpool_f32"},
    "head_bwd": {"bf16": "frost_float_head_bwd", "fp32": "frost_float_head_bwd_f32"},
}
STATS, EMIT, BRED, BDC, PLAIN = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib
    return _lib


def _dt(prec):
    return torch.bfloat16 if prec == "bf16" else torch.float32


def _up(t, prec):
    buf = torch.zeros(t.numel() + SLACK, dtype=_dt(prec), device="cuda")
    buf[: t.numel()] = t.reshape(-1).to(_dt(prec))
    return buf


def _at(buf, off):
    return C.c_void_p(buf.data_ptr() + off * buf.element_size())


class _Slice:
    """A [rows][cols] operand or result inside rows of `ld` elements at column `off`; everything else holds a sentinel."""

    def __init__(self, rows, cols, prec, ld=None, off=0, fill=NAN, data=None, sentinel=SENT):
        self.rows, self.cols, self.ld, self.off, self.sent = rows, cols, ld or cols, off, sentinel
        self.buf = torch.full((rows * self.ld + SLACK,), sentinel, dtype=_dt(prec), device="cuda")
        v = self.buf[: rows * self.ld].view(rows, self.ld)
        v[:, off: off + cols] = fill if data is None else data.to(_dt(prec)).cuda()

    @property
    def p(self):
        return _at(self.buf, self.off)

    def get(self):
        return self.buf[: self.rows * self.ld].view(self.rows, self.ld)[:, self.off: self.off + self.cols].float().cpu()

    def check_untouched(self):
        v = self.buf[: self.rows * self.ld].view(self.rows, self.ld).float()
        assert bool((v[:, : self.off] == self.sent).all()) and bool((v[:, self.off + self.cols:] == self.sent).all()), "columns outside the slice were written"
        assert bool((self.buf[self.rows * self.ld:].float() == self.sent).all()), "the slack behind the tensor was written"


class _Layer:
    """Device state of one conv + BatchNorm layer and its FrostFDesc, statistics and packs starting from garbage."""

    def __init__(self, L, p, cin_g, cout, prec, kind=0, kk=1):
        kq, es = (32, 2) if prec == "bf16" else (16, 4)
        self.prec, self.cout, self.cpad, self.kq = prec, cout, R.round_up(cout, 16), kq
        self.kpad = 64 if kind == 2 else R.round_up(cin_g, kq)
        self.kpad_t = R.round_up(cout, kq) if kind == 0 else 0
        dev = lambda t: t.float().contiguous().cuda()
        self.w, self.gamma, self.beta, self.rmean, self.rvar = dev(p["w"]), dev(p["gamma"]), dev(p["beta"]), dev(p["rmean"]), dev(p["rvar"])
        self.nbt = torch.tensor([p.get("nbt0", 0)], dtype=torch.int64, device="cuda")
        self.pack = torch.full((self.cpad * self.kpad * es,), 0xA5, dtype=torch.uint8, device="cuda")
        self.pack_t = torch.full((R.round_up(cin_g, 16) * self.kpad_t * es,), 0xA5, dtype=torch.uint8, device="cuda") if kind == 0 else None
        self.stat = torch.full((8 * 4 * self.cpad,), 3.25, dtype=torch.float64, device="cuda")
        self.coef = torch.zeros(8 * self.cpad, dtype=torch.float32, device="cuda")
        self.dgamma, self.dbeta = dev(p.get("dgamma0", torch.zeros(cout))), dev(p.get("dbeta0", torch.zeros(cout)))
        self.desc = L.FrostFDesc(w=self.w.data_ptr(), gamma=self.gamma.data_ptr(), beta=self.beta.data_ptr(), rmean=self.rmean.data_ptr(), rvar=self.rvar.data_ptr(),
                                 nbt=self.nbt.data_ptr(), pack=self.pack.data_ptr(), pack_t=self.pack_t.data_ptr() if self.pack_t is not None else None,
                                 stat=self.stat.data_ptr(), coef=self.coef.data_ptr(), dgamma=self.dgamma.data_ptr(), dbeta=self.dbeta.data_ptr(), cout=cout,
                                 cin_g=cin_g, kk=kk, kind=kind, cpad=self.cpad, kpad=self.kpad, kpad_t=self.kpad_t, fp32=int(prec == "fp32"))
        self.tab = L.struct_to_tensor(self.desc, "cuda")

    def pack_bits(self, which="pack"):
        t = getattr(self, which)
        return t.view(torch.int16 if self.prec == "bf16" else torch.int32).cpu()

    def rows(self):
        """statistics [slot][row][cpad] as doubles, and the four rows added up over the slots in the kernels' order (slot 0 first)"""
        st = self.stat.view(8, 4, self.cpad).cpu()
        tot = torch.zeros(4, self.cpad, dtype=torch.float64)
        for k in range(8):
            tot = tot + st[k]
        return st, tot

    def coefs(self):
        return self.coef.view(8, self.cpad).cpu()

    def set_coef(self, **rows):
        idx = dict(scale=0, bias=1, mean=2, inv=3, K1=4, E=5, F=6, var=7)
        c = self.coef.view(8, self.cpad)
        for k, v in rows.items():
            c[idx[k], : self.cout] = v.float().cuda()


def _bits(ref, prec):
    return ref.bfloat16().view(torch.int16) if prec == "bf16" else ref.float().view(torch.int32)


def _note(group, what, prec, obs, bound, e32=0.0):
    print(f"[float-kernels] {group} {what} {prec}: observed {obs:.2e} bound {bound:.2e} E32 {e32:.2e}")


def _hold(group, what, prec, dev, ref, ref32, storage=None, den=None):
    """dev against ref (fp64) with the yardstick ref32 (the same quantity in fp32 torch ops).  storage: 'fp32' / 'bf16' (what the result is
    rounded to) / 'dw_bf16'.  den: the tensor whose norms the errors are measured against when ref is a total cancellation (a single-pixel batch)."""
    storage = storage or prec
    assert bool(torch.isfinite(dev).all()), (group, what, "not finite")
    if den is None:
        whole, chan, e32 = R.rel(dev, ref), R.rel_per_channel(dev, ref), R.rel(ref32, ref)
    else:
        dn, dc = max(float(den.double().norm()), 1e-300), den.double().reshape(-1, den.shape[-1]).norm(dim=0).clamp_min(1e-300)
        d, d32 = (dev.double() - ref.double()).reshape(-1, ref.shape[-1]), (ref32.double() - ref.double()).reshape(-1, ref.shape[-1])
        whole, chan, e32 = float(d.norm()) / dn, float((d.norm(dim=0) / dc).max()), float(d32.norm()) / dn
    if storage == "bf16":
        bw, bc = 3e-3, R.BF16_U + 8 * e32
    else:
        bw = max(2e-5 if storage == "dw_bf16" else 2e-6, 8 * e32)
        bc = 2 * bw
    _note(group, what, prec, whole, bw, e32)
    _note(group, what + " (worst channel)", prec, chan, bc, e32)
    assert whole <= bw, (group, what, prec, "whole tensor", whole, bw, e32)
    assert chan <= bc, (group, what, prec, "worst channel", chan, bc, e32)


def _hold_sums(group, what, prec, dev, ref, ref32, terms):
    """per channel |dev - ref| <= tau * sum|term|"""
    t = terms.double().clamp_min(1e-300)
    e32 = float(((ref32.double() - ref.double()).abs() / t).max())
    tau = max(1e-6 if prec == "fp32" else 4e-6, 8 * e32)
    obs = float(((dev.double() - ref.double()).abs() / t).max())
    _note(group, what, prec, obs, tau, e32)
    assert bool(torch.isfinite(dev).all()) and obs <= tau, (group, what, prec, obs, tau, e32)


def _hold_rows(group, what, prec, dev, ref, mag=None, rtol=2e-6):
    """element-wise: |dev - ref| <= rtol * (the size of the terms ref is made of; |ref| itself where it is a product)"""
    m = (ref.double().abs() if mag is None else mag.double()).clamp_min(1e-300)
    obs = float(((dev.double() - ref.double()).abs() / m).max())
    _note(group, what, prec, obs, rtol)
    assert bool(torch.isfinite(dev).all()) and obs <= rtol, (group, what, prec, obs, rtol)


def _cast_exact(group, what, prec, dev, ref64):
    """computed in double, then cast: the device's float against the cast of the fp64 value, 1e-12"""
    _hold_rows(group, what, prec, dev, ref64.double().float(), rtol=1e-12)


# ================================================================================================ a. weight preparation
PREP_CASES = [(8, 8), (24, 40), (40, 24), (360, 592)]


@pytest.mark.parametrize("prec", PRECS)
def test_weight_prep_packs_are_the_layout_formulas(L, prec):
    """frost_float_weight_prep over a table of five descriptors in ONE launch (four pointwise layers and the 3 -> 32 stem, k = 3, kpad 64): forward,
    transposed and stem packs bit-equal to the Python index formulas (weights rounded to bf16 by torch in bf16 mode), every pack byte written
    (they start as 0xA5), all 8 x 4 x cpad statistics words zeroed from a non-zero state.  Observed: bit-equal."""
    g = torch.Generator().manual_seed(11)
    layers, ws = [], []
    for cin, cout in PREP_CASES:
        w = torch.randn(cout, cin, generator=g) * cin ** -0.5
        p = dict(w=w, **R.bn_params(cout, g))
        layers.append(_Layer(L, p, cin, cout, prec))
        ws.append((w, 0))
    wstem = torch.randn(32, 3, 3, 3, generator=g) * 0.2
    layers.append(_Layer(L, dict(w=wstem, **R.bn_params(32, g)), 3, 32, prec, kind=2, kk=9))
    ws.append((wstem, 2))
    table = (L.FrostFDesc * len(layers))(*[l.desc for l in layers])
    tab = L.struct_to_tensor(table, "cuda")
    L.call("frost_float_weight_prep", L.ptr(tab), len(layers), L.stream())
    torch.cuda.synchronize()
    for l, (w, kind) in zip(layers, ws):
        fwd, tr, kpad, kpad_t = R.layer_packs(w, kind, prec)
        assert (kpad, kpad_t) == (l.kpad, l.kpad_t)
        assert torch.equal(l.pack_bits("pack"), _bits(fwd, prec)), ("forward pack", tuple(w.shape))
        if kind == 0:
            assert torch.equal(l.pack_bits("pack_t"), _bits(tr, prec)), ("transposed pack", tuple(w.shape))
        assert float(l.stat.abs().sum()) == 0.0


# ================================================================================================ b / c(fp32) / f. the pointwise chain
def _pw_id(c):
    return "p%d_k%d_c%d_%s%s" % (c[0], c[1], c[2], R.ACT_NAMES[c[3]], "_strided" if c[4] else "")


_PW_PARAMS = [pytest.param(prec, c, id=prec + "-" + _pw_id(c)) for prec in PRECS for c in R.PW_CASES[prec]]


@pytest.mark.parametrize("prec,case", _PW_PARAMS)
def test_pw_chain(L, prec, case):
    """One layer through every pass: weight_prep -> mode 0 (conv kept, then again with out = NULL) -> bn_finalize -> mode 1 -> mode 2 -> bwd_finalize
    (twice: dgamma / dbeta accumulate) -> mode 3 -> data gradient (fp32: mode 4 on the transposed pack; bf16: frost_infer_pw on the transposed pack
    frost_float_weight_prep wrote), each stage against fp64 of the operands that stage reads (the device's own statistics and coefficient rows).
    fp32 mode also runs frost_float_ew_f32 modes 1 / 3 over the kept conv output: bit-equal to the recomputing GEMM (the backward's mask is the
    forward's), mode 2's sums to 1e-12.
    Cases: (1, 8, 8) .. (65, 32, 16) pixel tails around the 16- / 64-row tiles, K tails below one 64-byte step, cout % 16 != 0, all with csplit > 1;
    row lengths 704 / 720 bytes = the last pixel-split and the first channel-split (WPX = 1) form, (98, 1728, 288) the widest layer; cout 576 / 592 =
    coefficient rows in LDS or not; (70000, 16, 80) statistics workgroups that walk several tiles, csplit 1 with two channel groups.  `strided`: gy is
    a 16-column-offset slice of rows of cout + 24 elements, out a slice of the same rows (sentinels around it must survive).
    A single-pixel batch has zero variance: y = act(beta) and dc = 0 are total cancellations of terms ~ 1/sqrt(eps) larger, and a "channel" is one
    element, so there every error is measured against the norm of the terms the element is made of (|x|.|W|, |conv*scale| + |bias|, K1*gm, |dc|.|W|)
    instead of the (vanishing, or single) result.
    Observed worst (MI355X), fp32 mode: conv 7.3e-7, y 8.1e-7 (worst channel 1.5e-6), dc 1.2e-7, dx 4.4e-7, sums 6.9e-7 of sum|term| (tau 2.9e-6), E32 up to 2.9e-7;
    bf16 mode: conv / y / dc / dx 1.7e-3 .. 1.9e-3 (worst channel 3.1e-3 of 3.9e-3), sums 2.6e-7.  The bf16 figures are within a factor two of 3e-3: they are the one
    rounding of the stored element (half an ulp, 2^-8 / sqrt(3) over an rms mantissa of 1.5), not the arithmetic.  Coefficient rows: 2.0e-7; the double-then-cast rows and
    the ew / GEMM comparison: bit-equal."""
    npix, cin, cout, act, strided = case
    sfx32 = prec == "fp32"
    p = R.layer_inputs(npix, cin, cout, prec, R.pw_seed(npix, cin, cout, act))
    full = R.conv_bn_forward(p["x"], p["w_seen"], p["gamma"], p["beta"], p["rmean"], p["rvar"], 0, act)
    gy, share = R.zero_band(p["gy"], full["conv"], full["scale"], full["bias"], act)
    assert share <= R.BAND_SHARE, share                                  # before anything is launched
    conv64, conv32 = full["conv"], R.conv1x1(p["x"], p["w_seen"], R.F32)
    ld, off = (cout + 24, 16) if strided else (cout, 0)
    single = npix == 1
    G = "b.pw"

    lay = _Layer(L, p, cin, cout, prec)
    x = _up(p["x"], prec)
    gyd = _Slice(npix, cout, prec, ld, off, data=gy, sentinel=1000.0)
    pw = lambda mode, g, ldg, out, ldy: L.call(E["pw"][prec], L.ptr(lay.tab), L.ptr(x), L.ptr(lay.pack), npix, cin, cout, act, mode, g, ldg, out, ldy, L.stream())
    L.call("frost_float_weight_prep", L.ptr(lay.tab), 1, L.stream())

    # ---- mode 0: conv output + statistics
    kept = _Slice(npix, cout, prec)
    pw(STATS, None, 0, kept.p, cout)
    torch.cuda.synchronize()
    st_a, tot_a = lay.rows()
    lay.stat.zero_()
    pw(STATS, None, 0, None, 0)
    torch.cuda.synchronize()
    st_b, tot_b = lay.rows()
    kept.check_untouched()
    xw = p["x"].double().abs() @ p["w_seen"].double().abs().t()          # the size of a conv element's terms
    _hold(G, "mode 0 conv", prec, kept.get(), conv64, conv32, den=xw if single else None)
    s64, q64, a64 = R.channel_sums(conv64)
    s32, q32, _ = R.channel_sums(conv32)
    for tot, tag in ((tot_a, "kept"), (tot_b, "out=NULL")):
        _hold_sums(G, f"mode 0 sum ({tag})", prec, tot[0, :cout], s64, s32, a64)
        _hold_sums(G, f"mode 0 sum of squares ({tag})", prec, tot[1, :cout], q64, q32, q64)
    if sfx32:      # the same values in the same partial sums: equal up to the order of the double additions
        assert R.rel(tot_a[:2], tot_b[:2]) <= 1e-12
    assert float(st_a[:, 2:].abs().sum()) == 0.0 and float(st_b[:, 2:].abs().sum()) == 0.0          # rows mode 0 does not own
    assert float(tot_b[:, cout:].abs().sum()) == 0.0                                                  # channels past cout

    # ---- bn_finalize: from the device's own sums
    L.call("frost_float_bn_finalize", L.ptr(lay.tab), cout, npix, L.stream())
    torch.cuda.synchronize()
    co = R.bn_coefficients(tot_b[0, :cout], tot_b[1, :cout], npix, p["gamma"], p["beta"], p["rmean"], p["rvar"], eps=R.DEV_BN_EPS)
    cf = lay.coefs()
    for row, key in ((2, "mean"), (3, "inv"), (7, "var")):
        _cast_exact("d.fin", "chain " + key, prec, cf[row, :cout], co[key])
    _hold_rows("d.fin", "chain scale", prec, cf[0, :cout], co["scale"])
    _hold_rows("d.fin", "chain bias", prec, cf[1, :cout], co["bias"], co["bias_mag"])
    _hold_rows("d.fin", "chain running mean", prec, lay.rmean.cpu(), co["rmean"], co["rmean_mag"])
    _hold_rows("d.fin", "chain running var", prec, lay.rvar.cpu(), co["rvar"])
    assert int(lay.nbt) == p["nbt0"] + 1 and float(cf[:, cout:].abs().sum()) == 0.0
    sc, bi, mu, iv = (cf[r, :cout].clone() for r in range(4))
    zterms = (conv64 * sc.double()).abs() + bi.double().abs()

    # ---- mode 1
    y = _Slice(npix, cout, prec, ld, off)
    pw(EMIT, None, 0, y.p, ld)
    torch.cuda.synchronize()
    y.check_untouched()
    _hold(G, "mode 1 y", prec, y.get(), R.emit(conv64, sc, bi, act), R.emit(conv32, sc, bi, act, R.F32), den=zterms if single else None)

    # ---- mode 2
    st0, _ = lay.rows()
    pw(BRED, gyd.p, ld, None, 0)
    torch.cuda.synchronize()
    st1, tot1 = lay.rows()
    S1r, S2r, T1, T2 = R.bwd_sums(conv64, gy, sc, bi, mu, iv, act)
    S1y, S2y, _, _ = R.bwd_sums(conv32, gy, sc, bi, mu, iv, act, R.F32)
    _hold_sums(G, "mode 2 S1", prec, tot1[2, :cout], S1r, S1y, T1)
    _hold_sums(G, "mode 2 S2", prec, tot1[3, :cout], S2r, S2y, T2)
    assert torch.equal(st1[:, :2], st0[:, :2]) and float(tot1[:, cout:].abs().sum()) == 0.0
    if sfx32:
        L.call(E["ew"][prec], L.ptr(lay.tab), kept.p, npix, cout, act, BRED, gyd.p, ld, None, 0, L.stream())
        torch.cuda.synchronize()
        _, tot2 = lay.rows()
        ew_s = tot2[2:, :cout] - tot1[2:, :cout]
        assert float((ew_s - tot1[2:, :cout]).abs().max()) <= 1e-12 * float(torch.stack([T1, T2]).max()), "ew mode 2 over the kept conv output"
        lay.stat.copy_(st1.reshape(-1).cuda())

    # ---- bwd_finalize, twice
    S1d, S2d = tot1[2, :cout], tot1[3, :cout]
    bc = R.bwd_coefficients(S1d, S2d, npix, p["gamma"], iv, mu)
    for call in (1, 2):
        L.call("frost_float_bwd_finalize", L.ptr(lay.tab), cout, npix, L.stream())
        torch.cuda.synchronize()
        _hold_rows("d.fin", f"chain dgamma after call {call}", prec, lay.dgamma.cpu(), p["dgamma0"].double() + call * S2d.float().double(), p["dgamma0"].abs() + call * S2d.abs())
        _hold_rows("d.fin", f"chain dbeta after call {call}", prec, lay.dbeta.cpu(), p["dbeta0"].double() + call * S1d.float().double(), p["dbeta0"].abs() + call * S1d.abs())
    cf = lay.coefs()
    _hold_rows("d.fin", "chain K1", prec, cf[4, :cout], bc["K1"])
    if sfx32:      # rows E / F carry (b, a)
        _cast_exact("d.fin", "chain E = S2/N", prec, cf[5, :cout], bc["b"])
        _cast_exact("d.fin", "chain F = S1/N", prec, cf[6, :cout], bc["a"])
    else:          # the folded form
        _hold_rows("d.fin", "chain E folded", prec, cf[5, :cout], bc["E"])
        _hold_rows("d.fin", "chain F folded", prec, cf[6, :cout], bc["F"], bc["F_mag"])
    assert torch.equal(cf[:4, :cout], torch.stack([sc, bi, mu, iv])) and float(cf[:, cout:].abs().sum()) == 0.0
    K1, Er, Fr = cf[4, :cout].clone(), cf[5, :cout].clone(), cf[6, :cout].clone()

    # ---- mode 3
    dc = _Slice(npix, cout, prec, ld, off)
    pw(BDC, gyd.p, ld, dc.p, ld)
    torch.cuda.synchronize()
    dc.check_untouched()
    if sfx32:
        dref, dyard = (R.dc_direct(c, gy, sc, bi, mu, iv, K1, Fr, Er, act, dt) for c, dt in ((conv64, R.F64), (conv32, R.F32)))
    else:
        dref, dyard = (R.dc_folded(c, gy, sc, bi, K1, Er, Fr, act, dt) for c, dt in ((conv64, R.F64), (conv32, R.F32)))
    gmk = R.masked_grad(conv64, gy, sc, bi, act) * K1.double()
    _hold(G, "mode 3 dc", prec, dc.get(), dref, dyard, den=gmk if single else None)
    if sfx32:      # element-wise passes over the kept conv output reproduce the recomputing GEMM bit for bit
        y2, dc2 = _Slice(npix, cout, prec, ld, off), _Slice(npix, cout, prec, ld, off)
        L.call(E["ew"][prec], L.ptr(lay.tab), kept.p, npix, cout, act, EMIT, None, 0, y2.p, ld, L.stream())
        L.call(E["ew"][prec], L.ptr(lay.tab), kept.p, npix, cout, act, BDC, gyd.p, ld, dc2.p, ld, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(y2.buf.view(torch.int32), y.buf.view(torch.int32)), "ew mode 1 != pw mode 1"
        assert torch.equal(dc2.buf.view(torch.int32), dc.buf.view(torch.int32)), "ew mode 3 != pw mode 3"

    # ---- data gradient dx = dc . W on the transposed pack
    dcd = dc.get()
    dcb = _up(dcd, prec)
    dx = _Slice(npix, cin, prec)
    if sfx32:
        L.call("frost_float_pw_f32", None, L.ptr(dcb), L.ptr(lay.pack_t), npix, cout, cin, 0, PLAIN, None, 0, dx.p, cin, L.stream())
    else:
        L.call("frost_infer_pw", L.ptr(dcb), L.ptr(lay.pack_t), None, npix, cout, cin, 0, dx.p, L.stream())
    torch.cuda.synchronize()
    dx.check_untouched()
    _hold("f.dgrad", "dx", prec, dx.get(), dcd.double() @ p["w_seen"].double(), dcd @ p["w_seen"], den=dcd.double().abs() @ p["w_seen"].double().abs() if single else None)


def test_pw_dgrad_wide_on_the_float_transposed_pack(L):
    """frost_pw_dgrad_wide with qrec_w = NULL and accumulate = 0 (the float trainer's call) on the transposed pack written by
    frost_float_weight_prep, at the two smallest shapes frost_pw_dgrad_wide_ok takes (256 pixels, 8 / 16 channels), against dc . W in fp64 of the
    bf16-rounded operands.  Observed: 1.7e-3 (one bf16 rounding), worst channel 1.9e-3."""
    lib = L.load_library()
    assert lib.frost_pw_dgrad_wide_ok(255, 8, 8) == 0
    for npix, cin, cout in ((256, 8, 8), (256, 16, 8)):
        assert lib.frost_pw_dgrad_wide_ok(npix, cin, cout) == 1
        p = R.layer_inputs(npix, cin, cout, "bf16", 4242 + cin)
        lay = _Layer(L, p, cin, cout, "bf16")
        L.call("frost_float_weight_prep", L.ptr(lay.tab), 1, L.stream())
        dcd = p["gy"]
        dcb, dx = _up(dcd, "bf16"), _Slice(npix, cin, "bf16")
        L.call("frost_pw_dgrad_wide", L.ptr(dcb), L.ptr(lay.pack_t), None, npix, cin, cout, dx.p, 0, L.stream())
        torch.cuda.synchronize()
        dx.check_untouched()
        _hold("f.dgrad", "wide dx", "bf16", dx.get(), dcd.double() @ p["w_seen"].double(), dcd @ p["w_seen"])


# ================================================================================================ c. element-wise passes over a kept conv output
_EW_PARAMS = [pytest.param(prec, c, id="%s-p%d_c%d_%s%s" % (prec, c[0], c[1], R.ACT_NAMES[c[2]], "_strided" if c[3] else "")) for prec in PRECS for c in R.EW_CASES[prec]]


@pytest.mark.parametrize("prec,case", _EW_PARAMS)
def test_ew_passes(L, prec, case):
    """frost_float_ew(_f32) modes 1 / 2 / 3 fed a kept conv output and coefficient rows made on the CPU (fp32 values of the fp64 batch statistics of that
    very tensor), against the same references as the GEMM passes.  (1, 8); (5, 24) cpad 32 with 24 used; (50, 1728) the widest row; (9000, 64) more
    threads than the reduce cap of 256 workgroups; (131100, 128), bf16, modes 1 and 3: past the 8192-workgroup cap.
    Observed worst (MI355X): fp32 y 7.0e-8, dc 9.8e-8 (worst channel 5.8e-7), S1 / S2 1.1e-7 of sum|term|; bf16 y / dc 1.8e-3 (worst channel 3.4e-3 of 3.9e-3: a channel of
    five elements near the worst single rounding), S1 / S2 1.1e-7."""
    npix, c, act, strided = case
    big = npix > 100000
    p = R.kept_inputs(npix, c, prec, R.ew_seed(npix, c, act))
    gy, share = R.zero_band(p["gy"], p["conv"], p["scale"], p["bias"], act)
    assert share <= R.BAND_SHARE, share
    ld, off = (c + 24, 16) if strided else (c, 0)
    conv, sc, bi, mu, iv = p["conv"], p["scale"], p["bias"], p["mean"], p["inv"]
    lay = _Layer(L, dict(w=torch.zeros(1), **{k: p[k] for k in ("gamma", "beta", "rmean", "rvar")}), 8, c, prec)
    lay.stat.zero_()
    lay.set_coef(scale=sc, bias=bi, mean=mu, inv=iv)
    S1, S2, T1, T2 = R.bwd_sums(conv, gy, sc, bi, mu, iv, act)
    bc = R.bwd_coefficients(S1, S2, npix, p["gamma"], iv, mu)
    K1 = bc["K1"].float()
    Er, Fr = (bc["b"].float(), bc["a"].float()) if prec == "fp32" else (bc["E"].float(), bc["F"].float())
    lay.set_coef(K1=K1, E=Er, F=Fr)
    cv = _up(conv, prec)
    gyd = _Slice(npix, c, prec, ld, off, data=gy, sentinel=1000.0)
    ew = lambda mode, g, ldg, out, ldy: L.call(E["ew"][prec], L.ptr(lay.tab), L.ptr(cv), npix, c, act, mode, g, ldg, out, ldy, L.stream())
    single = npix == 1
    G = "c.ew"
    y = _Slice(npix, c, prec, ld, off)
    ew(EMIT, None, 0, y.p, ld)
    torch.cuda.synchronize()
    y.check_untouched()
    zterms = (conv.double() * sc.double()).abs() + bi.double().abs()
    _hold(G, "mode 1 y", prec, y.get(), R.emit(conv, sc, bi, act), R.emit(conv, sc, bi, act, R.F32), den=zterms if single else None)
    if not big:
        ew(BRED, gyd.p, ld, None, 0)
        torch.cuda.synchronize()
        st, tot = lay.rows()
        S1y, S2y, _, _ = R.bwd_sums(conv, gy, sc, bi, mu, iv, act, R.F32)
        _hold_sums(G, "mode 2 S1", prec, tot[2, :c], S1, S1y, T1)
        _hold_sums(G, "mode 2 S2", prec, tot[3, :c], S2, S2y, T2)
        assert float(st[:, :2].abs().sum()) == 0.0 and float(tot[:, c:].abs().sum()) == 0.0
    dc = _Slice(npix, c, prec, ld, off)
    ew(BDC, gyd.p, ld, dc.p, ld)
    torch.cuda.synchronize()
    dc.check_untouched()
    if prec == "fp32":
        dref, dyard = (R.dc_direct(conv, gy, sc, bi, mu, iv, K1, Fr, Er, act, dt) for dt in (R.F64, R.F32))
    else:
        dref, dyard = (R.dc_folded(conv, gy, sc, bi, K1, Er, Fr, act, dt) for dt in (R.F64, R.F32))
    gmk = R.masked_grad(conv, gy, sc, bi, act) * K1.double()
    _hold(G, "mode 3 dc", prec, dc.get(), dref, dyard, den=gmk if single else None)


# ================================================================================================ d. the coefficient kernels, directly
def _spread(total, g):
    """[8][n] partials with very uneven (also negative) weights that add up to `total` in double"""
    wgt = torch.randn(8, total.numel(), generator=g, dtype=torch.float64) * torch.tensor([5.0, 0.0, 1.0, 0.01, 3.0, 0.0, 0.5, 2.0], dtype=torch.float64)[:, None]
    part = wgt * total.double()
    part[7] += total.double() - part.sum(0)
    return part


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout", [8, 264])
@pytest.mark.parametrize("kind", ["plain", "count1", "clamp"])
def test_bn_finalize_direct(L, prec, cout, kind):
    """frost_float_bn_finalize from hand-filled statistics spread unevenly over the 8 slots (cout 264: more than one workgroup).  count1: the running
    variance takes the biased value.  clamp: the sum of squares lies just below mean^2 * count, the variance clamps to 0 and everything stays finite.
    num_batches_tracked rises by exactly one per call; running statistics start from non-trivial values.  The epsilon is the device's (the float literal 1e-5f).
    Observed: mean / var / inv bit-equal to the cast fp64 value; scale, bias, running statistics within 2.0e-7 of their terms."""
    g = torch.Generator().manual_seed(cout + len(kind))
    count = 1 if kind == "count1" else 37
    mean = torch.randn(cout, generator=g, dtype=torch.float64)
    var = torch.rand(cout, generator=g, dtype=torch.float64) + 0.3
    s = mean * count
    q = (mean * mean) * count * (1.0 - 1e-12) if kind == "clamp" else (var + mean * mean) * count
    p = dict(w=torch.zeros(1), nbt0=41, **R.bn_params(cout, g))
    lay = _Layer(L, p, 8, cout, prec)
    st = torch.zeros(8, 4, lay.cpad, dtype=torch.float64)
    st[:, 0, :cout], st[:, 1, :cout] = _spread(s, g), _spread(q, g)
    st[:, 2:] = 9.0                                                      # the backward's rows are not this kernel's
    lay.stat.copy_(st.reshape(-1).cuda())
    for call in (1, 2):
        L.call("frost_float_bn_finalize", L.ptr(lay.tab), cout, count, L.stream())
        torch.cuda.synchronize()
        assert int(lay.nbt) == 41 + call
    _, tot = lay.rows()
    co = R.bn_coefficients(tot[0, :cout], tot[1, :cout], count, p["gamma"], p["beta"], p["rmean"], p["rvar"], eps=R.DEV_BN_EPS)
    co2 = R.bn_coefficients(tot[0, :cout], tot[1, :cout], count, p["gamma"], p["beta"], co["rmean"], co["rvar"], eps=R.DEV_BN_EPS)          # the second call moves them again
    cf = lay.coefs()
    if kind == "clamp":
        assert float((tot[1, :cout] / count - (tot[0, :cout] / count) ** 2).min()) < 0.0 and float(co["var"].max()) <= 1e-9 and float(cf[7].abs().max()) <= 1e-9
    if kind == "count1":
        assert float(co["var"].min()) > 0.2                               # a wrong unbiased factor (count / (count - 1)) would not be finite
    for row, key in ((2, "mean"), (3, "inv"), (7, "var")):
        _cast_exact("d.fin", f"{kind} {key}", prec, cf[row, :cout], co[key])
    _hold_rows("d.fin", f"{kind} scale", prec, cf[0, :cout], co["scale"])
    _hold_rows("d.fin", f"{kind} bias", prec, cf[1, :cout], co["bias"], co["bias_mag"])
    _hold_rows("d.fin", f"{kind} running mean (two calls)", prec, lay.rmean.cpu(), co2["rmean"], co2["rmean_mag"])
    _hold_rows("d.fin", f"{kind} running var (two calls)", prec, lay.rvar.cpu(), co2["rvar"])
    assert float(cf[:, cout:].abs().sum()) == 0.0 and float(cf[4:7].abs().sum()) == 0.0
    assert torch.equal(lay.stat.cpu(), st.reshape(-1))                    # read, not consumed


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout", [8, 264])
def test_bwd_finalize_direct(L, prec, cout):
    """frost_float_bwd_finalize from hand-filled S1 / S2 spread unevenly over the 8 slots: K1 = gamma * inv; rows E / F carry the folded form in bf16 mode
    and (b, a) = (S2/N, S1/N) in fp32 mode; dgamma / dbeta accumulate onto non-zero values over two calls.  Observed: (b, a) bit-equal, the rest within 1.8e-7."""
    g = torch.Generator().manual_seed(5 * cout)
    count = 53
    S1, S2 = torch.randn(cout, generator=g, dtype=torch.float64) * 3, torch.randn(cout, generator=g, dtype=torch.float64) * 3
    p = dict(w=torch.zeros(1), dgamma0=torch.randn(cout, generator=g), dbeta0=torch.randn(cout, generator=g), **R.bn_params(cout, g))
    inv, mean = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    lay = _Layer(L, p, 8, cout, prec)
    lay.set_coef(inv=inv, mean=mean)
    st = torch.zeros(8, 4, lay.cpad, dtype=torch.float64)
    st[:, 2, :cout], st[:, 3, :cout] = _spread(S1, g), _spread(S2, g)
    st[:, :2] = 9.0
    lay.stat.copy_(st.reshape(-1).cuda())
    _, tot = lay.rows()
    S1d, S2d = tot[2, :cout], tot[3, :cout]
    bc = R.bwd_coefficients(S1d, S2d, count, p["gamma"], inv, mean)
    for call in (1, 2):
        L.call("frost_float_bwd_finalize", L.ptr(lay.tab), cout, count, L.stream())
        torch.cuda.synchronize()
        _hold_rows("d.fin", f"direct dgamma after call {call}", prec, lay.dgamma.cpu(), p["dgamma0"].double() + call * S2d.float().double(), p["dgamma0"].abs() + call * S2d.abs())
        _hold_rows("d.fin", f"direct dbeta after call {call}", prec, lay.dbeta.cpu(), p["dbeta0"].double() + call * S1d.float().double(), p["dbeta0"].abs() + call * S1d.abs())
    cf = lay.coefs()
    _hold_rows("d.fin", "direct K1", prec, cf[4, :cout], bc["K1"])
    if prec == "fp32":
        _cast_exact("d.fin", "direct E = S2/N", prec, cf[5, :cout], bc["b"])
        _cast_exact("d.fin", "direct F = S1/N", prec, cf[6, :cout], bc["a"])
    else:
        _hold_rows("d.fin", "direct E folded", prec, cf[5, :cout], bc["E"])
        _hold_rows("d.fin", "direct F folded", prec, cf[6, :cout], bc["F"], bc["F_mag"])
    assert float(cf[:, cout:].abs().sum()) == 0.0 and float(cf[:2].abs().sum()) == 0.0 and float(cf[7].abs().sum()) == 0.0


def test_bn_eval_table(L):
    """frost_float_bn_eval over a table of three descriptors in one launch: scale / bias / mean / inv from the running statistics."""
    g = torch.Generator().manual_seed(3)
    ps = [dict(w=torch.zeros(1), **R.bn_params(c, g)) for c in (8, 24, 264)]
    lays = [_Layer(L, p, 8, p["gamma"].numel(), "bf16") for p in ps]
    tab = L.struct_to_tensor((L.FrostFDesc * 3)(*[l.desc for l in lays]), "cuda")
    L.call("frost_float_bn_eval", L.ptr(tab), 3, L.stream())
    torch.cuda.synchronize()
    for p, l in zip(ps, lays):
        c = l.cout
        inv = 1.0 / torch.sqrt(p["rvar"].double() + R.DEV_BN_EPS)
        scale = p["gamma"].double() * inv
        cf = l.coefs()
        _hold_rows("d.fin", "eval inv", "bf16", cf[3, :c], inv)
        _hold_rows("d.fin", "eval scale", "bf16", cf[0, :c], scale)
        _hold_rows("d.fin", "eval bias", "bf16", cf[1, :c], p["beta"].double() - p["rmean"].double() * scale, p["beta"].abs().double() + (p["rmean"].double() * scale).abs())
        assert torch.equal(cf[2, :c], p["rmean"]) and float(cf[:, c:].abs().sum()) == 0.0 and float(cf[4:].abs().sum()) == 0.0
        assert int(l.nbt) == 0 and torch.equal(l.rvar.cpu(), p["rvar"])


# ================================================================================================ e. pointwise weight gradient, stem scatter
# (npix, cin, cout, ldx, ldw).  The pixel range splits when a split owns >= 32 (bf16, 128-pixel blocks) / >= 4 (fp32, 64-pixel blocks) blocks:
# from 8065 / 449 pixels on.  8229 / 8100 (bf16) and 530 / 500 (fp32) all split in two; 8064 and 448 are the last that do not.
WG_BOTH = [(1, 8, 8, 16, 16), (127, 24, 40, 32, 28), (129, 72, 136, 80, 76), (300, 64, 32, 64, 64)]
WG_CASES = {"bf16": WG_BOTH + [(8229, 64, 64, 64, 64), (8100, 64, 64, 64, 64), (8065, 64, 64, 64, 64), (8064, 64, 64, 64, 64)],
            "fp32": WG_BOTH + [(530, 64, 64, 64, 64), (500, 64, 64, 64, 64), (449, 64, 64, 64, 64), (448, 64, 64, 64, 64)]}
_WG_PARAMS = [pytest.param(prec, c, id="%s-p%d_k%d_c%d_ldx%d_ldw%d" % ((prec,) + c)) for prec in PRECS for c in WG_CASES[prec]]


@pytest.mark.parametrize("prec,case", _WG_PARAMS)
def test_pw_wgrad(L, prec, case):
    """frost_float_pw_wgrad(_f32): dW[co][ci] += sum_p dc[p][co] * x[p][ci] onto a non-zero dW; x rows of ldx > cin elements (the rest holds large values),
    dW rows of ldw > cin (the rest holds a sentinel that must survive); (300, 64, 32) is the stem's form, ldx = ldw = 64.  (129, 72, 136): two 64-wide
    tiles each way with partial 16-blocks.  Observed worst (MI355X): fp32 1.9e-7 (E32 2.4e-7), bf16 mode 2.8e-7 (E32 1.6e-7)."""
    npix, cin, cout, ldx, ldw = case
    g = torch.Generator().manual_seed(900 + npix + cin)
    x = R.seen(torch.randn(npix, cin, generator=g) + 0.5, prec)
    dc = R.seen(torch.randn(npix, cout, generator=g) * 0.1, prec)
    dw0 = torch.randn(cout, cin, generator=g) * 0.5
    xd = _Slice(npix, cin, prec, ldx, 0, data=x, sentinel=1000.0)
    dcd = _up(dc, prec)
    dw = _Slice(cout, cin, "fp32", ldw, 0, data=dw0)
    L.call(E["wgrad"][prec], L.ptr(dcd), xd.p, npix, cin, ldx, cout, dw.p, ldw, L.stream())
    torch.cuda.synchronize()
    dw.check_untouched()
    _hold("e.wgrad", "dW", prec, dw.get(), dw0.double() + dc.double().t() @ x.double(), dw0 + dc.t() @ x, storage="dw_bf16" if prec == "bf16" else "fp32")


@pytest.mark.parametrize("cout", [32, 40])
def test_stem_wscatter(L, cout):
    """frost_float_stem_wscatter: dw[co][c][tap] += tmp[co][tap*4 + c], bit-equal to the index permutation added onto a non-zero dw."""
    g = torch.Generator().manual_seed(cout)
    tmp, dw0 = torch.randn(cout, 64, generator=g), torch.randn(cout, 27, generator=g)
    tmpd, dw = tmp.cuda(), _Slice(cout, 27, "fp32", data=dw0)
    L.call("frost_float_stem_wscatter", L.ptr(tmpd), cout, dw.p, L.stream())
    torch.cuda.synchronize()
    dw.check_untouched()
    assert torch.equal(dw.get(), dw0 + R.stem_unscatter(tmp, cout))


# ================================================================================================ g. wiring and head
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("npix", [1, 333])
def test_grad_merge(L, prec, npix):
    """frost_float_grad_merge(_f32): every non-empty subset of {residual, cat slice at column cs of rows of c + cs, squeeze}, (c, cs) = (8, 8), (40, 24).
    fp32: bit-equal to ((0 + res) + cat) + sq, the kernel's order; bf16: within one rounding of the exact sum."""
    g = torch.Generator().manual_seed(npix)
    for (c, cs), subset in itertools.product(((8, 8), (40, 24)), [s for s in itertools.product((0, 1), repeat=3) if any(s)]):
        ccat = c + cs
        res, sq = (R.seen(torch.randn(npix, c, generator=g), prec) for _ in range(2))
        cat = R.seen(torch.randn(npix, ccat, generator=g), prec)
        ops = [res if subset[0] else None, cat[:, cs:] if subset[1] else None, sq if subset[2] else None]
        resd, catd, sqd = _up(res, prec), _up(cat, prec), _up(sq, prec)
        out = _Slice(npix, c, prec)
        L.call(E["merge"][prec], L.ptr(resd) if subset[0] else None, L.ptr(catd) if subset[1] else None, cs, ccat, L.ptr(sqd) if subset[2] else None, npix, c,
               out.p, L.stream())
        torch.cuda.synchronize()
        out.check_untouched()
        acc, exact, mag = torch.zeros(npix, c), torch.zeros(npix, c, dtype=R.F64), torch.zeros(npix, c, dtype=R.F64)
        for o in ops:
            if o is not None:
                acc, exact, mag = acc + o, exact + o.double(), mag + o.double().abs()
        got = out.get()
        if prec == "fp32":
            assert torch.equal(got, acc), (c, cs, subset)
        else:
            assert bool(((got.double() - exact).abs() <= R.BF16_U * exact.abs() + 2.0 ** -22 * mag).all()), (c, cs, subset)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("c", [8, 1280])
@pytest.mark.parametrize("hw", [1, 49, 196])
def test_avgpool(L, prec, hw, c, masked):
    """frost_float_avgpool(_f32): y[n][c] = mean over hw of x, times the dropout mask (0 or 1/keep) when there is one; n = 3, fp32 result.
    Yardstick: the same sequential fp32 sum in torch.  Observed: equal to the yardstick's own error (2.4e-7 at most)."""
    n = 3
    g = torch.Generator().manual_seed(hw + c)
    x = R.seen(torch.randn(n, hw, c, generator=g) + 0.3, prec)
    mask = ((torch.rand(n, c, generator=g) < 0.8).float() / 0.8) if masked else None
    xd, md = _up(x, prec), mask.cuda() if masked else None
    y = _Slice(n, c, "fp32")
    L.call(E["avgpool"][prec], L.ptr(xd), n, hw, c, L.ptr(md), y.p, L.stream())
    torch.cuda.synchronize()
    y.check_untouched()
    ref = x.double().mean(1)
    s32 = torch.zeros(n, c)
    for i in range(hw):
        s32 = s32 + x[:, i]
    y32 = s32 / float(hw)
    if masked:
        ref, y32 = ref * mask.double(), y32 * mask
    _hold("g.wiring", "avgpool", prec, y.get(), ref, y32, storage="fp32")


def test_cat_and_add_f32(L):
    """frost_float_cat_f32 / frost_float_add_f32: bit-equal to torch.cat / +, element counts that are no multiple of 1024."""
    g = torch.Generator().manual_seed(8)
    npix, ca, cb = 333, 24, 40
    a, b = torch.randn(npix, ca, generator=g), torch.randn(npix, cb, generator=g)
    ad, bd = _up(a, "fp32"), _up(b, "fp32")
    y = _Slice(npix, ca + cb, "fp32")
    L.call("frost_float_cat_f32", L.ptr(ad), ca, L.ptr(bd), cb, npix, y.p, L.stream())
    u, v = torch.randn(npix * cb, generator=g), torch.randn(npix * cb, generator=g)
    ud, vd = _up(u, "fp32"), _up(v, "fp32")
    s = _Slice(1, npix * cb, "fp32")
    L.call("frost_float_add_f32", L.ptr(ud), L.ptr(vd), npix * cb, s.p, L.stream())
    torch.cuda.synchronize()
    y.check_untouched(); s.check_untouched()
    assert torch.equal(y.get(), torch.cat([a, b], 1)) and torch.equal(s.get()[0], u + v)


@pytest.mark.parametrize("h,w", [(7, 9), (8, 8)])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_stem_im2col_f32(L, h, w, layout):
    """frost_float_stem_im2col_f32: 3x3 stride-2 pad-1 patches of a strided (N, 3, H, W) image -> [npix][16 taps][4], bit-equal to an unfold-built tensor with
    zeros in taps 9..15 and channel 3."""
    n = 2
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(h * w))
    xd = x.cuda()
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = _Slice(n * ho * wo, 64, "fp32")
    sn, sc, sh, sw = xd.stride()
    L.call("frost_float_stem_im2col_f32", L.ptr(xd), n, h, w, sn, sc, sh, sw, out.p, L.stream())
    torch.cuda.synchronize()
    out.check_untouched()
    cols = torch.nn.functional.unfold(x, 3, padding=1, stride=2).reshape(n, 3, 9, ho * wo).permute(0, 3, 2, 1)          # [n][pixel][tap][c]
    exp = torch.zeros(n, ho * wo, 16, 4)
    exp[:, :, :9, :3] = cols
    assert torch.equal(out.get(), exp.reshape(n * ho * wo, 64))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,cin,nclass,hw,masked", [(3, 40, 10, 1, 0), (9, 1280, 1000, 49, 1), (3, 1280, 10, 49, 1), (9, 40, 1000, 1, 0), (9, 40, 10, 49, 1)])
def test_head_bwd(L, prec, n, cin, nclass, hw, masked):
    """frost_float_head_bwd(_f32): dW = dlogits^T . pooled, dbias = column sums of dlogits, gx[n][hw][c] = (dlogits . Wfc)[n][c] * mask[n][c] / hw, against fp64.
    launch_sgemm stores its result (accumulate = 0; a split-K launch zeroes the tensor first) and k_colsum assigns: dW and dbias are WRITTEN, not
    accumulated.  The trainer zeroes its gradient arena before every backward and adds carried gradients afterwards, so it relies on nothing more than
    that; asserted here from non-zero tensors.  dbias is a sum and is held by the sum rule (1.2e-7 of sum|term| observed).  Observed: dW 6.2e-8, gx fp32 2.1e-7 (worst
    channel 2.3e-6 of 5.4e-6: three rows, each a 1000-term sum with cancellation), gx bf16 1.8e-3 (worst channel 3.5e-3 of 3.9e-3)."""
    g = torch.Generator().manual_seed(n + cin + nclass)
    dl = torch.randn(n, nclass, generator=g) * 0.1
    pooled = torch.randn(n, cin, generator=g)
    wfc = torch.randn(nclass, cin, generator=g) * cin ** -0.5
    mask = ((torch.rand(n, cin, generator=g) < 0.8).float() / 0.8) if masked else None
    dld, pd, wd, md = dl.cuda(), pooled.cuda(), wfc.cuda(), mask.cuda() if masked else None
    dw = _Slice(nclass, cin, "fp32", data=torch.randn(nclass, cin, generator=g))
    db = _Slice(1, nclass, "fp32", data=torch.randn(1, nclass, generator=g))
    gx = _Slice(n * hw, cin, prec)
    scratch = torch.full((n * cin,), NAN, device="cuda")
    L.call(E["head_bwd"][prec], L.ptr(dld), L.ptr(pd), L.ptr(wd), n, cin, nclass, hw, L.ptr(md), dw.p, db.p, gx.p, L.ptr(scratch), L.stream())
    torch.cuda.synchronize()
    for t in (dw, db, gx):
        t.check_untouched()
    _hold("g.head", "dW", prec, dw.get(), dl.double().t() @ pooled.double(), dl.t() @ pooled, storage="fp32")
    _hold_sums("g.head", "dbias", "fp32", db.get()[0], dl.double().sum(0), dl.sum(0), dl.double().abs().sum(0))
    dp64, dp32 = dl.double() @ wfc.double(), dl @ wfc
    if masked:
        dp64, dp32 = dp64 * mask.double(), dp32 * mask
    rep = lambda t: (t / hw)[:, None, :].expand(n, hw, cin).reshape(n * hw, cin)
    _hold("g.head", "gx", prec, gx.get(), rep(dp64), rep(dp32))

"""Per-channel ('fbgemm' qconfig) QAT TRAINING at the shapes where the fast kernels run, teacher-forced against the CPU oracle.

tests/test_gpu_fbgemm.py holds this mode to the reference goldens at N = 2 on 6x6 .. 16x16 maps, where none of the size-selected kernels engage; every
path-equivalence test is per-tensor with index range 255.  Here one ConvBN(ReLU) layer per kernel family runs in per-channel + reduce_range mode
(per-channel symmetric weights with a per-channel moving-average observer, activation indices 0..127) at the smallest batch that selects the family's
fast kernel -- asserted from the C-ABI call log -- against oracle.convbn_qat under QState(qconfig="fbgemm") (pinned to the reference by the g12 goldens):
fp32 evaluation = the reference's arithmetic (indices, observers, statistics), fp64 evaluation = the yardstick of the gradients.

Stated bounds (those of tests/test_gpu_fbgemm.py for this mode, and the gradient rule of test_gpu_prod.run_layer_case):
  indices |delta| <= 1 on <= FLIP_RATE of the elements; activation scale 2e-5, zero point equal; per-channel wscale / wmin / wmax 1e-6; running statistics 1e-3;
  gradients norm-wise within max(GRAD, 1.5 x the fp32 oracle's own distance from the fp64 oracle).

Weight ties.  With the version-0 symmetric rule scale_c = max|w_c| / 127.5 EVERY channel's largest weight sits on a rounding tie of its own quantiser
(w / scale = +-127.5 up to the last bits of three fp32 roundings): a negative one quantises to -128 or -127 (an INDEX tie: the channel's outputs move by
a fraction of a step), a positive one to 127 either way but with q = 128 (outside the STE mask) or q = 127 (inside): a CLIP tie, which switches that
weight's gradient and its share of the channel's dgamma on or off.  Which side is taken depends on the last bit of sqrt / divide (torch's vectorised CPU
forms are not bit-identical to IEEE, the device's are), so
  * a device / oracle weight-index difference is accepted only where it is verified to be a tie (|frac - 0.5| <= 2e-4, |delta| = 1); a channel holding one is
    compared with |delta index| <= 2 and the relaxed statistics bound of run_layer_case; at most TIE_CHANNEL_CAP of the channels may hold one;
  * dW / dgamma are ALSO compared off the verified clip ties (those elements / their channels set aside on all three sides), where the fp32 oracle is close to the
    fp64 one and the bound is therefore tight; the full vectors are held to the same rule, which the clip ties of the two oracle evaluations widen.

The cap: a channel's extreme weight is negative with probability 1/2, and two independent roundings of 127.5 (1 + eps) land on different sides of the tie with
probability <= 1/2, i.e. an expected share <= 1/4; TIE_CHANNEL_CAP = 0.4 leaves room for the spread at 24 .. 96 channels.  The seeds are chosen so that the
oracle's own fp32-vs-fp64 weight indices stay inside it (asserted on every case: `amb_w`)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":          # run as a script (see the end of the file): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import frost_oracle as O
from test_gpu_prod import GRAD, T, _layer_state, device_int_weights, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIP_RATE = 5e-4
TIE_CHANNEL_CAP = 0.4
TIE = 2e-4
A = "L.conv.0.activation_post_process"
WFQ = "L.conv.0.weight_fake_quant"

#  name               kind  cin   cout  k  s  H    N  relu  input zp != 0   entries the case is named for
LAYERS = [
    ("pw16_96_112",     "pw",   16,   96, 1, 1, 112, 2, 1, 0, ("frost_pw_conv_bwd_fused",)),
    ("pw96_24_56_lin",  "pw",   96,   24, 1, 1, 56,  2, 0, 1, ("frost_pw_conv_bwd_fused",)),
    ("dw3s1_40_30",     "dw",   40,   40, 3, 1, 30,  5, 1, 0, ("frost_dw_bwd_fused",)),
    ("dw3s1_168_28",    "dw",  168,  168, 3, 1, 28,  3, 1, 0, ("frost_dw_bwd_fused",)),
    ("dw5s2_144_56",    "dw",  144,  144, 5, 2, 56,  2, 1, 0, ("frost_dw_bwd_fused",)),
    ("dw3s1_360_14",    "dw",  360,  360, 3, 1, 14,  7, 1, 0, ("frost_block_dw_bwd", "frost_block_dw_bwd_reduce")),
    ("dw5s1_1440_7",    "dw", 1440, 1440, 5, 1, 7,   5, 1, 0, ("frost_block_dw_bwd", "frost_block_dw_bwd_reduce")),
    ("pw104_624_14",    "pw",  104,  624, 1, 1, 14,  6, 1, 1, ("frost_pwc_conv_fwd_emit", "frost_pwc_conv_bwd", "frost_pw_dgrad_wide", "frost_pw_wgrad")),
    ("pw312_80_14_lin", "pw",  312,   80, 1, 1, 14,  3, 0, 0, ("frost_pw_conv_fwd_keep", "frost_pw_ew", "frost_pw_dgrad_wide", "frost_pw_wgrad")),
    ("pw1440_192_7_lin", "pw", 1440, 192, 1, 1, 7,   6, 0, 0, ("frost_pw_conv_fwd_keep", "frost_pw_ew", "frost_pw_dgrad_wide", "frost_pw_wgrad")),
    ("stem_64",         "stem",   3,  32, 3, 2, 64,  2, 1, 1, ("frost_stem_im2col", "frost_pw_conv_bwd_fused", "frost_stem_wgrad_remap")),
]
BY_NAME = {c[0]: c for c in LAYERS}
SEED = {c[0]: 7300 + 13 * i for i, c in enumerate(LAYERS)}
# per-tensor clipping (part 3) needs the layer's largest folded weight in an ODD channel (the ones scaled up): a property of the seed, found on the CPU
SEED_FOR = {("pw16_96_112", "qnnpack", "clip"): 7302}


def _seed(name, qconfig, variant):
    return SEED_FOR.get((name, qconfig, variant), SEED[name])


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import engine
    assert torch.cuda.is_available()
    return engine


def _inputs(case, qconfig, seed):
    name, kind, cin, cout, k, s, H, N, relu, zpnz = case[:10]
    hi = 127 if qconfig == "fbgemm" else 255
    in_zp = (58 if hi == 127 else 117) if zpnz else 0
    in_scale = 0.0231 * 255 / hi
    xi = np.clip(np.round(O.synth((N, cin, H, H), seed + 1) * (hi / 6.4) + (hi + 1) / 2 - (0 if zpnz else 0.235 * hi)), 0, hi).astype(np.uint8)
    return hi, in_scale, in_zp, xi


def _weight_side(P, qs, rv_before, cout):
    """The weight quantiser of this step as the oracle evaluated it: BN-folded weights, t = w / scale, unclamped and clamped indices, the STE mask."""
    with torch.no_grad():
        sf = P["L.conv.0.bn.weight"] / torch.sqrt(rv_before + O.BN_EPS)
        wsc = (P["L.conv.0.weight"] * sf.reshape(-1, 1, 1, 1)).reshape(cout, -1)
        sc = qs.sd[WFQ + ".scale"]
        if sc.numel() == cout and "ch_axis" in qs.wgt:
            inv = (1.0 / sc).reshape(-1, 1)                                   # _FQPC: x * (1 / scale_c)
        else:
            inv = float(np.float32(1.0) / np.float32(float(sc[0])))           # _FQ: x * float(1.0f / scale)
        q = torch.round(wsc * inv)
        t = wsc.double() / sc.double().reshape(-1, 1)
    return dict(wsc=wsc, sf=sf, scale=sc.clone(), t=t.numpy(), q_un=q.numpy().astype(np.int64), q=torch.clamp(q, -128, 127).numpy().astype(np.int32),
                mask=((q >= -128) & (q <= 127)).numpy())


def _capture_pre(qs):
    """The output site's FakeQuantize input (the layer's output before the index clamp) is kept on `qs.pre`."""
    orig = qs.fq_site

    def fq_site(prefix, x, kind, observe=True):
        if prefix == A:
            qs.pre = x.detach()
        return orig(prefix, x, kind, observe)
    qs.fq_site = fq_site


def _run_oracle(case, qconfig, seed, steps, record=None, clip=False):
    """`steps` training steps of the layer on the oracle, fp32 and fp64 side by side.  record = (scale, zero_point): the output site's observer is DISABLED and the
    site keeps this record.  clip: after step 0 the odd output channels' weights are scaled by 1.25, the even ones by 0.8."""
    name, kind, cin, cout, k, s, H, N, relu, zpnz = case[:10]
    groups = cout if kind == "dw" else 1
    torch.set_num_threads(16)
    hi, in_scale, in_zp, xi = _inputs(case, qconfig, seed)
    sd = _layer_state(cin, cout, k, groups, seed)
    sides = []
    for dt in (torch.float32, torch.float64):
        P, B = O.split_state({O.float_to_qat_key(k_): (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k_, v in sd.items()})
        qs = O.QState(B, qconfig=qconfig)
        if record is not None:
            qs.sd[A + ".activation_post_process.min_val"], qs.sd[A + ".activation_post_process.max_val"] = torch.tensor(float("inf")), torch.tensor(float("-inf"))
            qs.sd[A + ".scale"], qs.sd[A + ".zero_point"] = torch.tensor([record[0]], dtype=torch.float32), torch.tensor([record[1]], dtype=torch.int32)
            qs.sd[A + ".observer_enabled"] = torch.tensor([0], dtype=torch.uint8)
            _capture_pre(qs)
        x = ((T(xi.astype(np.float64)).to(dt) - in_zp) * in_scale).requires_grad_(True)
        sides.append((P, qs, x, dt))
    out = []
    for step in range(steps):
        rec = {}
        for P, qs, x, dt in sides:
            x.grad = None
            for p in P.values():
                p.grad = None
            rv_before = qs.sd["L.conv.0.bn.running_var"].clone()          # the BN fold uses the running variance BEFORE this step's update
            yo = O.convbn_qat(P, qs, "L", x, s, (k - 1) // 2, groups, bool(relu), True)
            gr = T(O.synth(tuple(yo.shape), seed + 2 + 50 * step))
            yo.backward(gr if dt == torch.float32 else gr.bfloat16().double())                # the device receives bf16 gradients
            tag = "32" if dt == torch.float32 else "64"
            sc, zp = float(qs.sd[A + ".scale"][0]), int(qs.sd[A + ".zero_point"][0])
            rec["idx" + tag] = O.fq_index(yo.detach(), sc, zp).to(torch.uint8)
            rec["w" + tag] = _weight_side(P, qs, rv_before, cout)
            rec["g" + tag] = dict(dx=x.grad.clone(), dw=P["L.conv.0.weight"].grad.clone(), dgamma=P["L.conv.0.bn.weight"].grad.clone(), dbeta=P["L.conv.0.bn.bias"].grad.clone())
            rec["rm" + tag], rec["rv" + tag] = qs.sd["L.conv.0.bn.running_mean"].numpy().copy(), qs.sd["L.conv.0.bn.running_var"].numpy().copy()
            if dt == torch.float32:
                rec.update(gr=gr, scale=sc, zp=zp, min_val=float(qs.sd[A + ".activation_post_process.min_val"]), max_val=float(qs.sd[A + ".activation_post_process.max_val"]),
                           yq=yo.detach().clone() if record is None and steps == 1 else None)
            if "ch_axis" in qs.wgt:
                rec["wmin" + tag], rec["wmax" + tag] = qs.sd[WFQ + ".activation_post_process.min_val"].numpy().copy(), qs.sd[WFQ + ".activation_post_process.max_val"].numpy().copy()
            if record is not None:          # membership of the activation STE window (and of the ReLU's), element by element
                qu = torch.round(qs.pre * float(np.float32(1.0) / np.float32(record[0]))) + record[1]
                rec["win" + tag] = (qu >= 0) & (qu <= hi) & ((qs.pre > 0) if relu else torch.ones_like(qu, dtype=torch.bool))
            if clip and step == 0:
                with torch.no_grad():
                    P["L.conv.0.weight"][1::2] *= 1.25
                    P["L.conv.0.weight"][0::2] *= 0.8
        if record is not None:
            # where the oracle's own two evaluations disagree about an element's membership the device may take either side: per channel, the sum of |g| over those
            amb = rec.pop("win32") != rec.pop("win64")
            rec["db_slack"], rec["db_amb"] = (rec["gr"].bfloat16().double().abs() * amb).sum((0, 2, 3)), int(amb.sum())
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, qconfig, variant):
    """The oracle's side of one case, computed once and shared by the tests that need it (never modified).  variant 'live': two steps, live observers; 'sat': two
    steps under a fixed, deliberately narrow output record chosen from the oracle's own outputs under a live observer (whose first-step range covers every value):
    for a ReLU layer the top index sits at their 85th percentile, for a linear one index 0 at the 15th as well; 'clip': two steps, weights rescaled after step 0."""
    case, seed = BY_NAME[name], _seed(name, qconfig, variant)
    if variant == "sat":
        hi = 127 if qconfig == "fbgemm" else 255
        y = _run_oracle(case, qconfig, seed, 1)[0]["yq"].flatten()
        top = float(torch.quantile(y[:: max(1, y.numel() // 1000000)], 0.85))
        low = float(torch.quantile(y[:: max(1, y.numel() // 1000000)], 0.15)) if not case[8] else 0.0
        assert top > 0.0 and low <= 0.0, (name, low, top)
        scale = float(np.float32((top - low) / hi))
        zp = int(min(max(round(-low / scale), 0), hi))
        return (scale, zp), _run_oracle(case, qconfig, seed, 2, record=(scale, zp))
    return None, _run_oracle(case, qconfig, seed, 2, clip=(variant == "clip"))


def _rel(a, b, keep=None):
    a, b = a.double(), b.double()
    if keep is not None:
        a, b = a * keep, b * keep
    return float((a - b).norm() / (b.norm() + 1e-30))


def run_case(engine, name, qconfig="fbgemm", variant="live", expect=None, g32=False):
    """The device's side of one case (through the C ABI) against oracle(name, qconfig, variant); asserts the bounds stated in the module docstring and that every entry in
    `expect` (default: the case's own list) was launched.  g32: the fp32-gradient mode (csrc/frost_g32.hip), held to test_fp32_gradient_mode_layer_vs_oracle's bound."""
    from frostnet_amd import _lib as L
    case = BY_NAME[name]
    _, kind, cin, cout, k, s, H, N, relu, zpnz, entries = case
    expect = entries if expect is None else expect
    pc = qconfig == "fbgemm"
    groups = cout if kind == "dw" else 1
    record, ref = oracle(name, qconfig, variant)
    seed = _seed(name, qconfig, variant)
    hi, in_scale, in_zp, xi = _inputs(case, qconfig, seed)
    dev = "cuda"
    sd = _layer_state(cin, cout, k, groups, seed)
    E, qa = engine.Engine(dev), engine.QArena(4, dev)
    E.grad_fp32 = bool(g32)
    if pc:
        qa.t[:, L.Q_QMAX] = 127.0                                   # reduce_range activations
        E.act_qmax = 127
    w = sd["L.conv.0.weight"].to(dev).contiguous().requires_grad_(True)
    gamma, beta = sd["L.conv.1.weight"].to(dev).requires_grad_(True), sd["L.conv.1.bias"].to(dev).requires_grad_(True)
    l = engine.ConvLayer("L", kind, w, gamma, beta, sd["L.conv.1.running_mean"].to(dev), sd["L.conv.1.running_var"].to(dev),
                         torch.zeros((), dtype=torch.int64, device=dev), None, k, s, bool(relu), qa.alloc(), qa.alloc())
    if pc:
        l.per_channel = True
        l.wmin = torch.full((cout,), float("inf"), device=dev)
        l.wmax = torch.full((cout,), float("-inf"), device=dev)
    E.add_layer(l)
    qx = qa.alloc()
    qa.set_qparams(qx, in_scale, in_zp)
    if record is not None:                 # the output site: observer disabled, a fixed record
        qa.set_qparams(l.qy, record[0], record[1])
        l.qy.view(torch.int32)[L.Q_OBS_EN] = 0
    xi_t = T(xi)
    if kind == "stem":
        xi_t = torch.cat([xi_t, torch.full_like(xi_t[:, :1], in_zp)], 1)
    results = []
    for step, r in enumerate(ref):
        L.CALL_LOG = []
        try:
            E.begin_step()
            x = E.act_from_indices(xi_t, qx)
            y = E.conv(l, x, training=True, observe=record is None)
            # (fp32-gradient mode: the bf16-representable gradient the fp64 evaluation received, stored in fp32)
            y.grad = engine.float_to_grad((r["gr"].bfloat16().float() if g32 else r["gr"]).to(dev), fp32=bool(g32))
            yidx = y.indices().cpu()
            E.backward()
            torch.cuda.synchronize()
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        print(f"[{name} {qconfig} {variant}{' g32' if g32 else ''} step {step}] entries: {' '.join(sorted(set(log)))}")
        missing = [e for e in expect if e not in log]
        assert not missing, (name, "entries expected but not launched", missing, sorted(set(log)))
        qy = qa.get(l.qy)
        # ---- weights: indices as the kernels hold them against the oracle's clamped indices; differences only at verified ties
        w32, w64 = r["w32"], r["w64"]
        q_dev = device_int_weights(l)
        wdiff = np.argwhere(w32["q"] != q_dev)
        for a_, b_ in wdiff:
            if w64["q"][a_, b_] == q_dev[a_, b_] and abs(int(w32["q"][a_, b_]) - int(q_dev[a_, b_])) == 1:
                continue          # the oracle's own fp32 and fp64 evaluations land on different indices here (its fp32 BN fold is the noisy one): either side is accepted
            t = float(w32["t"][a_, b_])
            assert abs(int(w32["q"][a_, b_]) - int(q_dev[a_, b_])) == 1 and abs(abs(t - np.floor(t)) - 0.5) <= TIE, (name, step, "weight quantised differently away from a tie", int(a_), int(b_), t)
        tie_ch = sorted(set(int(a_) for a_, _ in wdiff))
        amb_w = float((w32["q"] != w64["q"]).any(1).mean())
        if pc:
            assert len(tie_ch) <= TIE_CHANNEL_CAP * cout and amb_w <= TIE_CHANNEL_CAP, (name, step, "too many tie channels", len(tie_ch), cout, amb_w)
        else:
            assert len(wdiff) <= 4, (name, step, "too many weight ties", len(wdiff))
        keep = torch.ones(cout, dtype=torch.bool)
        keep[tie_ch] = False
        # ---- output indices
        d = (yidx.to(torch.int16) - r["idx32"].to(torch.int16)).abs()
        if tie_ch:
            assert int(d[:, ~keep].max()) <= 2, (name, step, "tie channel", int(d[:, ~keep].max()))
        dk = d[:, keep]
        mx, rate = int(dk.max()), float((dk > 0).float().mean())
        assert int(yidx.max()) <= hi, (name, step, int(yidx.max()))
        # ---- gradients against the fp64 evaluation; `off`: off the verified clip ties (weights within TIE of +127.5 / -128.5 on the fp64 side)
        clip_tie = (np.abs(w64["t"] - 127.5) <= TIE) | (np.abs(w64["t"] + 128.5) <= TIE)
        offw = T(~clip_tie).reshape(l.w.shape)
        offc = T(~clip_tie.any(1))
        g32_, g64 = r["g32"], r["g64"]
        mine = dict(dw=l.w.grad.detach().cpu(), dgamma=l.gamma.grad.detach().cpu(), dbeta=l.beta.grad.detach().cpu())
        if kind != "stem":
            mine["dx"] = engine.grad_to_float(x.grad, x.n, x.h, x.w, x.c).cpu()
        e = {k_: _rel(v, g64[k_]) for k_, v in mine.items()}
        rr = {k_: _rel(g32_[k_], g64[k_]) for k_ in mine}
        e_off = dict(dw=_rel(mine["dw"], g64["dw"], offw), dgamma=_rel(mine["dgamma"], g64["dgamma"], offc))
        r_off = dict(dw=_rel(g32_["dw"], g64["dw"], offw), dgamma=_rel(g32_["dgamma"], g64["dgamma"], offc))
        print(f"[{name} {qconfig} {variant} step {step}] weight-tie channels {len(tie_ch)} of {cout} (oracle fp32 vs fp64: {amb_w:.3f}); clip-tie channels {int(clip_tie.any(1).sum())}; "
              f"idx max {mx} flip {rate:.2e}, top index {int(yidx.max())}, share on it {float((yidx == hi).float().mean()):.3f}, on 0 {float((yidx == 0).float().mean()):.3f} | vs fp64: "
              + " ".join(f"{k_} {v:.2e}" for k_, v in e.items()) + " | off clip ties: " + " ".join(f"{k_} {v:.2e}" for k_, v in e_off.items())
              + " | ref32 vs fp64: " + " ".join(f"{k_} {v:.2e}" for k_, v in rr.items()) + " | off clip ties: " + " ".join(f"{k_} {v:.2e}" for k_, v in r_off.items()))
        results.append(dict(log=log, mine=mine, e=e, rr=rr, q_dev=q_dev, keep=keep, yidx=yidx, tie_ch=tie_ch, clip_tie=clip_tie))
        assert mx <= 1 and rate <= FLIP_RATE, (name, step, mx, rate)
        # ---- observer scalars, per-channel weight observer, running statistics
        np.testing.assert_allclose(qy["scale"], r["scale"], rtol=2e-5)
        assert qy["zero_point"] == r["zp"]
        if record is None:
            np.testing.assert_allclose(qy["min_val"], r["min_val"], rtol=2e-5, atol=1e-6)
            np.testing.assert_allclose(qy["max_val"], r["max_val"], rtol=2e-5, atol=1e-6)
        if pc:
            # against the oracle's per-channel buffers at 1e-6 -- of its fp32 evaluation or, channel by channel, of its fp64 one: from step 1 on the folded weights carry the
            # running variance, and where the fp32 evaluation's own variance sum is noisy (measured: 3.1e-4 relative on one channel of 16 -> 96 @112, which moves ITS scale
            # by 1.5e-6 from the fp64 evaluation's) the device, whose statistics are exact integers, sits with the fp64 evaluation -- the rule of the running statistics below
            for what, v, r32, r64 in (("wscale", l.wscale[:cout], w32["scale"].numpy(), w64["scale"].numpy()), ("wmin", l.wmin, r["wmin32"], r["wmin64"]), ("wmax", l.wmax, r["wmax32"], r["wmax64"])):
                v = v.cpu().numpy()
                ok = np.isclose(v, r32, rtol=1e-6, atol=1e-9) | np.isclose(v, r64, rtol=1e-6, atol=1e-9)
                assert ok.all(), (name, step, what, np.nonzero(~ok)[0][:8], v[~ok][:8], r32[~ok][:8], r64[~ok][:8])
        else:
            np.testing.assert_allclose(qa.get(l.qw)["scale"], float(w32["scale"][0]), rtol=1e-6)
        for key, dev_v in (("rm", l.rmean), ("rv", l.rvar)):
            v, r32, r64 = dev_v.cpu().numpy(), r[key + "32"], r[key + "64"]
            ok = np.isclose(v, r32, rtol=1e-3, atol=2e-4) | np.isclose(v, r64, rtol=1e-3, atol=2e-4)
            ok[tie_ch] |= np.isclose(v[tie_ch], r32[tie_ch], rtol=2e-2, atol=2e-3)          # a channel with one weight a level apart: its statistics move with it
            assert ok.all(), (name, step, key, np.nonzero(~ok)[0][:8], v[~ok][:8], r32[~ok][:8], r64[~ok][:8])
        # ---- gradients
        if g32:
            # test_fp32_gradient_mode_layer_vs_oracle's bound (either evaluation, 1e-3 + 3 sqrt(flip fraction)); dW / dgamma off the clip ties, whose mask is the last bit's decision
            flips = min(float((yidx != r["idx32"]).float().mean()), float((yidx != r["idx64"]).float().mean()))
            tol = 1e-3 + 3.0 * flips ** 0.5
            e2 = {k_: min(_rel(v, g64[k_], {"dw": offw, "dgamma": offc}.get(k_)), _rel(v, g32_[k_], {"dw": offw, "dgamma": offc}.get(k_))) for k_, v in mine.items()}
            print(f"    fp32-gradient mode: forward flips {flips:.1e}; " + " ".join(f"{k_} {v:.2e}" for k_, v in e2.items()))
            assert all(v <= tol for v in e2.values()), (name, step, e2, tol)
        else:
            for k_ in mine:
                assert e[k_] <= max(GRAD, 1.5 * rr[k_]), (name, step, k_, e[k_], rr[k_])
            for k_ in e_off:
                assert e_off[k_] <= max(GRAD, 1.5 * r_off[k_]), (name, step, k_, "off the clip ties", e_off[k_], r_off[k_])
        if variant == "clip" and step == 0:
            with torch.no_grad():          # the same fp32 products as on the oracle's side
                l.w[1::2] *= 1.25
                l.w[0::2] *= 0.8
    return ref, results


# ------------------------------------------------------------------------------------------ 1. teacher-forced layers, per-channel + reduce_range
@pytest.mark.parametrize("name", [c[0] for c in LAYERS])
def test_fbgemm_layer_on_the_fast_path_vs_oracle(engine, name):
    run_case(engine, name)


def test_fbgemm_classifier_head_vs_oracle(engine):
    """frost_classifier_fwd / frost_head_bwd with per-channel weight scales: N = 4 on a 7 x 7 map with 1280 inputs, two steps, against oracle.classifier_forward under the
    fbgemm QState (driving code of test_gpu_prod.test_classifier_head_vs_reference_golden; its bounds, with the logits' index range 0..127 asserted)."""
    from frostnet_amd import _lib as L
    N, H, C, NC, seed = 4, 7, 1280, 1000, 7700
    dev = "cuda"
    torch.set_num_threads(16)
    wts = O.synth_state(["classifier.2.weight", "classifier.2.bias"], [(NC, C, 1, 1), (NC,)], seed)
    in_scale, in_zp = 0.0462, 0
    xi = np.clip(np.round(O.synth((N, C, H, H), seed + 1) * 20 + 34), 0, 127).astype(np.uint8)
    sides = []
    for dt in (torch.float32, torch.float64):
        P = {k_: v.clone().to(dt).requires_grad_(True) for k_, v in wts.items()}
        sides.append((P, O.QState(qconfig="fbgemm"), ((T(xi.astype(np.float64)).to(dt) - in_zp) * in_scale).requires_grad_(True), dt))
    E, qa = engine.Engine(dev), engine.QArena(4, dev)
    qa.t[:, L.Q_QMAX] = 127.0
    E.act_qmax = 127
    W = wts["classifier.2.weight"].to(dev).requires_grad_(True)
    b = wts["classifier.2.bias"].to(dev).requires_grad_(True)
    l = engine.ConvLayer("classifier.2", "cls", W, None, None, None, None, None, b, 1, 1, False, qa.alloc(), qa.alloc())
    l.per_channel = True
    l.wmin, l.wmax = torch.full((NC,), float("inf"), device=dev), torch.full((NC,), float("-inf"), device=dev)
    E.add_layer(l)
    qx = qa.alloc()
    qa.set_qparams(qx, in_scale, in_zp)
    a = "classifier.2.activation_post_process"
    for step in range(2):
        gr = T(O.synth((N, NC, 1, 1), seed + 2 + 50 * step))
        ev = {}
        for P, qs, xo, dt in sides:
            xo.grad = None
            for p in P.values():
                p.grad = None
            yo = O.classifier_forward(P, qs, xo, True)
            yo.backward(gr.to(dt))
            ev[dt] = (yo.detach().reshape(N, NC), qs, P, xo)
        y32, qs, P32, _ = ev[torch.float32]
        _, _, P64, x64 = ev[torch.float64]
        L.CALL_LOG = []
        try:
            E.begin_step()
            act = E.act_from_indices(T(xi), qx)
            logits = E.head(l, act, None, True)
            E.backward(gr.reshape(N, NC).to(dev))
            torch.cuda.synchronize()
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        print(f"[fbgemm classifier step {step}] entries: {' '.join(sorted(set(log)))}")
        assert "frost_classifier_fwd" in log and "frost_head_bwd" in log, log
        qy = qa.get(l.qy)
        np.testing.assert_allclose(qy["scale"], float(qs.sd[a + ".scale"][0]), rtol=2e-5)
        assert qy["zero_point"] == int(qs.sd[a + ".zero_point"][0])
        wq = "classifier.2.weight_fake_quant"
        np.testing.assert_allclose(l.wscale[:NC].cpu().numpy(), qs.sd[wq + ".scale"].numpy(), rtol=1e-6)
        np.testing.assert_allclose(l.wmin.cpu().numpy(), qs.sd[wq + ".activation_post_process.min_val"].numpy(), rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(l.wmax.cpu().numpy(), qs.sd[wq + ".activation_post_process.max_val"].numpy(), rtol=1e-6, atol=1e-9)
        idx = torch.round(logits.cpu() / qy["scale"] + qy["zero_point"]).to(torch.int16)
        ref_idx = O.fq_index(y32, qs.sd[a + ".scale"][0], qs.sd[a + ".zero_point"][0]).to(torch.int16)
        d = (idx - ref_idx).abs()
        dx = engine.grad_to_float(act.grad, act.n, act.h, act.w, act.c).cpu()
        # the weight STE mask at each class's largest positive weight is a clip tie (module docstring): those elements are set aside
        with torch.no_grad():
            t64 = (P64["classifier.2.weight"].reshape(NC, -1) / ev[torch.float64][1].sd[wq + ".scale"].double().reshape(-1, 1)).numpy()
        off = T(~(np.abs(t64 - 127.5) <= TIE)).reshape(W.shape)
        e_y = relerr(logits.cpu(), y32)
        e_dx = relerr(dx, x64.grad)
        e_dw = _rel(l.w.grad.detach().cpu(), P64["classifier.2.weight"].grad, off)
        e_db = relerr(l.bias.grad.cpu(), P64["classifier.2.bias"].grad)
        print(f"[fbgemm classifier step {step}] idx max {int(d.max())} (top {int(idx.max())}) flip {float((d > 0).float().mean()):.2e} y {e_y:.2e} dx {e_dx:.2e} dW {e_dw:.2e} ({int((~off).sum())} clip ties set aside) db {e_db:.2e}")
        assert int(idx.max()) <= 127 and int(d.max()) <= 1 and float((d > 0).float().mean()) <= 2e-3
        assert float((dx - dx[:, :, :1, :1]).abs().max()) == 0.0
        assert e_dx <= GRAD and e_dw <= 1e-3 and e_db <= 1e-4          # the head's GEMMs are exact fp32 (v_mfma_f32_16x16x4_f32)


# ------------------------------------------------------------------------------------------ 2. saturated outputs: both clamps of the activation STE window
SAT = ["pw16_96_112", "dw3s1_168_28", "pw96_24_56_lin"]
PLAIN_EXPECT = {"pw16_96_112": ("frost_pw_conv_bwd",), "dw3s1_168_28": ("frost_dw_dgrad",), "pw96_24_56_lin": ("frost_pw_conv_bwd",)}


def _saturated(engine, name, qconfig, plain):
    hi = 127 if qconfig == "fbgemm" else 255
    record, ref = oracle(name, qconfig, "sat")
    for step, r in enumerate(ref):          # the input condition, on the oracle's own indices
        top, zero = float((r["idx32"] == hi).float().mean()), float((r["idx32"] == 0).float().mean())
        print(f"[{name} {qconfig} saturated step {step}] record scale {record[0]:.5f} zp {record[1]}: oracle share on index {hi}: {top:.3f}, on index 0: {zero:.3f}")
        assert top >= 0.10 and int(r["idx32"].max()) == hi, (name, step, top)
        if not BY_NAME[name][8]:
            assert zero >= 0.10 and 0 < record[1] < hi, (name, step, zero, record)
    _, res = run_case(engine, name, qconfig, "sat", expect=PLAIN_EXPECT[name] if plain else None)
    for step, (r, o) in enumerate(zip(ref, res)):
        if plain:
            assert not any(e in o["log"] for e in BY_NAME[name][10] if e.endswith("fused")), o["log"]
        assert int(o["yidx"].max()) <= hi
        # dbeta = the plain sum of the in-window gradient, no cancellation: a wrong window shows directly.  (A channel holding a weight-index tie sees other outputs,
        # and so does the fp64 yardstick where ITS weight indices differ from the fp32 evaluation's: both kinds of channel are set aside here, and held by part 1's bound.)
        keep = o["keep"] & T(~(r["w32"]["q"] != r["w64"]["q"]).any(1))
        # One element on the wrong side of the window moves dbeta by |g|: 1e-3 of the norm at these sizes.  Where the oracle's fp32 and fp64 evaluations THEMSELVES
        # disagree about an element (db_amb of them; measured on 16 -> 96 @112, range 255: 50 / 2 elements in steps 0 / 1, which put the fp32 evaluation 1.0e-3 / 1.1e-3
        # from the fp64 one) the device may take either side: per channel, a deviation up to the sum of |g| over those elements is set aside, the rest is held to 1e-3.
        delta = (o["mine"]["dbeta"].double() - r["g64"]["dbeta"]).abs()
        e_raw = float((delta * keep).norm() / ((r["g64"]["dbeta"] * keep).norm() + 1e-30))
        e_db = float((torch.clamp(delta - r["db_slack"], min=0.0) * keep).norm() / ((r["g64"]["dbeta"] * keep).norm() + 1e-30))
        print(f"[{name} {qconfig} saturated step {step}{' plain' if plain else ''}] dbeta vs fp64 ({int(keep.sum())} of {keep.numel()} channels without a weight-index tie): {e_raw:.2e}; "
              f"beyond the {r['db_amb']} elements the oracle's two evaluations disagree on: {e_db:.2e}")
        assert int(keep.sum()) >= 0.5 * keep.numel()
        assert e_db <= 1e-3, (name, step, e_db)


@pytest.mark.parametrize("qconfig", ["fbgemm", "qnnpack"])
@pytest.mark.parametrize("name", SAT)
def test_saturated_outputs_ste_window(engine, name, qconfig):
    _saturated(engine, name, qconfig, False)


@pytest.mark.parametrize("qconfig", ["fbgemm", "qnnpack"])
@pytest.mark.parametrize("name", SAT)
def test_saturated_outputs_ste_window_plain_paths(name, qconfig):
    """The same case with every size-selected path switched off (the PLAIN environment of tests/test_gpu_paths.py; the switches are read when the library loads,
    hence a process of its own)."""
    from test_gpu_paths import PLAIN
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "saturated", name, qconfig], env=dict(os.environ, **PLAIN), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(p.stdout[-6000:])
    assert p.returncode == 0, p.stdout[-6000:]


# ------------------------------------------------------------------------------------------ 3. clipped weights: the weight STE mask per channel
CLIP = ["pw16_96_112", "dw3s1_168_28"]


@pytest.mark.parametrize("qconfig", ["fbgemm", "qnnpack"])
@pytest.mark.parametrize("name", CLIP)
def test_clipped_weights_ste_mask(engine, name, qconfig):
    _, ref = oracle(name, qconfig, "clip")
    w32 = ref[1]["w32"]
    off_mask = ~w32["mask"]
    share, ch_share = float(off_mask.mean()), float(off_mask.any(1).mean())
    print(f"[{name} {qconfig} clipped] oracle, step 1: {share:.4f} of the weights outside the quantiser's range, {ch_share:.3f} of the channels hold one; "
          f"largest |unclamped index| {int(np.abs(w32['q_un']).max())}")
    if qconfig == "fbgemm":
        assert share >= 0.01 and ch_share >= 0.40, (name, share, ch_share)
    else:
        # one scale for the layer: a weight is clipped only where its (odd) channel's largest folded weight x 1.25 exceeds the LAYER's largest x 1.0025, and the channels'
        # gamma / sigma scatter keeps that to a handful -- required: at least 5 such weights in at least 4 channels, the largest robustly outside (index beyond +-140)
        assert int(off_mask.sum()) >= 5 and int(off_mask.any(1).sum()) >= 4 and int(np.abs(w32["q_un"]).max()) > 140, (name, int(off_mask.sum()), int(off_mask.any(1).sum()))
    _, res = run_case(engine, name, qconfig, "clip")
    o = res[1]
    robust = ~o["clip_tie"]          # away from the mask's own rounding boundaries (+127.5 / -128.5)
    dw = o["mine"]["dw"].reshape(w32["mask"].shape).numpy()
    masked, live = off_mask & robust, w32["mask"] & robust
    assert masked.sum() >= 0.9 * off_mask.sum()
    nz = float((dw[live] != 0).mean())
    print(f"[{name} {qconfig} clipped] device dW: max |dW| where the oracle's mask is off {float(np.abs(dw[masked]).max()) if masked.any() else 0.0:.1e}, non-zero share where it is on {nz:.4f}")
    assert (dw[masked] == 0).all(), (name, int((dw[masked] != 0).sum()))
    assert nz >= 0.99, (name, nz)
    differ = np.argwhere(o["q_dev"] != w32["q"])          # (each one verified to be a tie by run_case)
    # per-channel: after the moving-average update no weight sits on its channel's 127.5 tie any more -- the indices are EQUAL; per-tensor: run_layer_case's allowance
    assert len(differ) <= (0 if qconfig == "fbgemm" else 4), (name, differ[:8])


# ------------------------------------------------------------------------------------------ 5. one bottleneck at its true shape through the module surface
#          name        cin  cout k  e  r  H   N
BLOCKS = [("cas_res_14", 104, 104, 5, 6, 4, 14, 4),          # squeeze + cat + residual at 14 x 14 (r as in FrostNet-Large's layer3): 128 -> 768 -> 104
          ("cas_res_7",  192, 192, 3, 6, 4, 7,  6)]          # 7 x 7: 240 -> 1440 -> 192
G4T_GRAD = 2e-2          # tests/test_gpu_model.py::test_g4_block_true_shapes


@pytest.mark.parametrize("case", BLOCKS, ids=[c[0] for c in BLOCKS])
def test_fbgemm_block_true_shape_through_the_module_surface(engine, case, monkeypatch):
    """test_g4_block_true_shapes without a golden, in per-channel + reduce_range mode: a CascadePreExBottleneck prepared with get_default_qat_qconfig('fbgemm', version=0),
    wrapped by FrostRunner.for_block, two teacher-forced steps with the block kernels engaged (asserted) against oracle.block_forward under QState(qconfig='fbgemm') --
    the fp32 evaluation for indices and state, fp32 or fp64 (that test's either-yardstick rule, its bounds and stated exceptions) for the gradients.  Weight gradients are
    compared off the verified clip ties and dgamma off their channels (module docstring).  The engine's guards are held too: no frost_block_dw_bwd_c1 behind a per-channel
    conv1, and -- with the FROST_SQ_BWD_CAT form switched ON for this test -- no frost_sq_bwd_cat behind a per-channel squeeze_conv."""
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat
    from frostnet_amd import _lib as L, frostnet as F, runner as R
    name, cin, cout, k, e, r, H, N = case
    torch.set_num_threads(16)
    seed = 7900 + 31 * BLOCKS.index(case)
    m = F.CascadePreExBottleneck(cin, cout, quantized=True, kernel_size=k, stride=1, expand_ratio=e, reduce_factor=r)
    keys, shapes = list(m.state_dict().keys()), [tuple(v.shape) for v in m.state_dict().values()]
    sd0 = O.synth_state(keys, shapes, seed)
    m.load_state_dict(sd0)
    bc = O.block_cfg(cin, cout, k, e, r, 1)
    assert bc["squeeze"] and bc["residual"]
    in_scale, in_zp = 0.0462, 58
    xi = T(np.clip(np.round(O.synth((N, cin, H, H), seed + 500) * 20 + 64), 0, 127).astype(np.uint8))
    sides = {}
    for dt in (torch.float32, torch.float64):
        P, B = O.split_state({O.float_to_qat_key(k_): (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k_, v in sd0.items()})
        sides[dt] = ({"B." + k_: v for k_, v in P.items()}, O.QState({"B." + k_: v for k_, v in B.items()}, qconfig="fbgemm"),
                     ((xi.to(dt) - in_zp) * in_scale).requires_grad_(True))
    m.train()
    for mod in m.modules():
        if type(mod) in (F.ConvBNReLU, F.ConvBN):
            mod.fuse_model()
    m.qconfig = get_default_qat_qconfig("fbgemm", version=0)
    prepare_qat(m, inplace=True)
    m.cuda()
    monkeypatch.setattr(engine, "_SQ_BWD_CAT", True)
    run = R.FrostRunner.for_block(m)
    assert run.E.act_qmax == 127 and all(l.per_channel for l in run.E.layers)
    qx = run.qa.alloc()
    run.qa.set_qparams(qx, in_scale, in_zp)
    xf = (xi.float() - in_zp) * in_scale
    qx[L.Q_FQMIN], qx[L.Q_FQMAX], qx[L.Q_QMAX] = float(xf.min()), float(xf.max()), 127.0
    site = "B.skip_add.activation_post_process"
    convs = [n_ for n_ in ("squeeze_conv", "conv1", "conv2", "reduce_conv")]
    tie_chs = {}
    for step in range(2):
        gr = T(O.synth((N, cout, H, H), seed + 600 + 50 * step))
        ties, q32, t32, q64 = {}, {}, {}, {}
        for dt, (P, qs, x_) in sides.items():
            x_.grad = None
            for p in P.values():
                p.grad = None
            rv = {c_: qs.sd[f"B.{c_}.conv.0.bn.running_var"].clone() for c_ in convs}
            y_ = O.block_forward(P, qs, "B", x_, bc, True, True)
            y_.backward(gr if dt == torch.float32 else gr.bfloat16().double())                      # the device receives bf16 gradients
            if dt == torch.float32:
                idx32 = O.fq_index(y_.detach(), qs.sd[site + ".scale"][0], qs.sd[site + ".zero_point"][0])
            else:
                idx64 = O.fq_index(y_.detach(), qs.sd[site + ".scale"][0], qs.sd[site + ".zero_point"][0])
            with torch.no_grad():
                for c_ in convs:
                    b_ = f"B.{c_}.conv.0"
                    wsc = (P[b_ + ".weight"] * (P[b_ + ".bn.weight"] / torch.sqrt(rv[c_] + O.BN_EPS)).reshape(-1, 1, 1, 1)).double()
                    t = wsc / qs.sd[b_ + ".weight_fake_quant.scale"].double().reshape(-1, 1, 1, 1)
                    ties[c_] = ties.get(c_, False) | ((t - 127.5).abs() <= TIE)
                    if dt == torch.float64:
                        q64[c_] = torch.clamp(torch.round(wsc * (1.0 / qs.sd[b_ + ".weight_fake_quant.scale"].double()).reshape(-1, 1, 1, 1)), -128, 127).reshape(wsc.shape[0], -1).numpy().astype(np.int32)
                    if dt == torch.float32:
                        q32[c_], t32[c_] = torch.clamp(torch.round((wsc.float() * (1.0 / qs.sd[b_ + ".weight_fake_quant.scale"]).reshape(-1, 1, 1, 1))), -128, 127).reshape(wsc.shape[0], -1).numpy().astype(np.int32), \
                            t.reshape(wsc.shape[0], -1).numpy()
        (P32, qs32, x32), (P64, qs64, x64) = sides[torch.float32], sides[torch.float64]
        rv_dev = {l.name.split(".")[-1]: l.rvar.detach().clone() for l in run.E.layers}
        L.CALL_LOG = []
        try:
            run.E.begin_step()
            x = run.E.act_from_indices(xi, qx)
            y = run.block_forward(run.block, x, True, True)
            yidx = y.indices().cpu()
            y.grad = engine.float_to_grad(gr.cuda())
            run.bind_grads()
            run.E.backward()
            torch.cuda.synchronize()
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        print(f"[fbgemm block {name} step {step}] entries: {' '.join(sorted(set(log)))}")
        assert ("frost_block_expand_dw_stats" in log) or ("frost_block_dw_stats" in log), log
        assert "frost_block_dw_reduce" in log and "frost_block_dw_bwd" in log and "frost_block_dw_bwd_reduce" in log, log
        assert "frost_dw_conv_fwd" not in log and "frost_dw_dgrad" not in log, log
        assert log.count("frost_pw_ew_add_bwd") == 2 and "frost_add_bwd" not in log, log
        assert "frost_block_dw_bwd_c1" not in log and "frost_sq_bwd_cat" not in log and "frost_cat_bwd" in log, log          # the per-channel guards of engine.py
        d = (yidx.to(torch.int16) - idx32.to(torch.int16)).abs()
        flips = float((d > 0).float().mean())
        ref_flips = float((idx32 != idx64).float().mean())
        dx = engine.grad_to_float(x.grad, x.n, x.h, x.w, x.c).cpu()
        e_32, e_64, r_ = relerr(dx, x32.grad), relerr(dx, x64.grad), relerr(x32.grad, x64.grad)
        print(f"[fbgemm block {name} step {step}] index flips {flips:.2e} (max {int(d.max())}, top index {int(yidx.max())}; the oracle's fp32 vs fp64 evaluations: {ref_flips:.2e}); "
              f"dx vs fp32 oracle {e_32:.2e}, vs fp64 {e_64:.2e} (fp32 oracle vs fp64: {r_:.2e})")
        # Bounds: test_g4_block_true_shapes' own (|delta| <= 2, G4T_GRAD against either evaluation; the share of flipped indices is bounded below, behind the weight comparison),
        # the gradient bounds widened to 1.5 x the distance between the oracle's OWN fp32 and fp64 evaluations where that is larger.  It is, in this mode: every channel's largest weight sits on a rounding tie of its per-channel quantiser
        # (module docstring), ~2.5 % of a layer's channels quantise one weight a level apart between device and fp32 oracle (measured by part 1: 13 of 624, 8 of 360, 36 of
        # 1440) and ~20 % between the oracle's two evaluations; reduce_conv mixes all of them into every output.  Measured at step 0: device vs fp32 oracle 6.1e-2 / 3.6e-2
        # of the output indices one step apart (14 x 14 / 7 x 7 block), every layer of the chain being within 6e-6 of the oracle when teacher-forced alone (part 1).
        bad = []
        if int(yidx.max()) > 127 or int(d.max()) > 2:
            bad.append(("indices", int(yidx.max()), int(d.max())))
        if min(e_64, e_32) > max(G4T_GRAD, 1.5 * r_):
            bad.append(("dx", e_32, e_64, r_))
        for pn, p in m.named_parameters():
            mine = p.grad.detach().double().cpu()
            g32_, g64 = P32["B." + pn].grad.double(), P64["B." + pn].grad
            tie = ties[pn.split(".")[0]]
            keep = ~tie if pn.endswith("conv.0.weight") else (~tie.reshape(tie.shape[0], -1).any(1) if pn.endswith("bn.weight") else None)
            e_32, e_64, r_ = _rel(mine, g32_, keep), _rel(mine, g64, keep), _rel(g32_, g64, keep)
            tol = G4T_GRAD
            if pn.endswith("bn.bias") and "reduce_conv" not in pn:
                # dbeta of a layer followed by another BatchNorm is mathematically ~0 (all rounding noise): bounded against the scale of dgamma instead (test_g4_block_true_shapes)
                gam = P64["B." + pn.replace("bn.bias", "bn.weight")].grad
                e_64 = float((mine - g64).norm() / (max(float(g64.norm()), float(gam.norm())) + 1e-30))
                e_32 = float((mine - g32_).norm() / (max(float(g32_.norm()), float(gam.norm())) + 1e-30))
                r_ = float((g32_ - g64).norm() / (max(float(g64.norm()), float(gam.norm())) + 1e-30))
            if pn.startswith("conv1.") and ".bn." in pn:
                tol = 5e-2          # conv1 feeds a depthwise conv + train-mode BatchNorm: its dgamma / dbeta are residuals of cancelling sums (test_g4_block_true_shapes)
            print(f"    {pn:40s} vs fp32 oracle {e_32:.2e}, vs fp64 {e_64:.2e} (fp32 oracle vs fp64: {r_:.2e})" + (f"   ({int(tie.sum())} clip ties set aside)" if keep is not None else ""))
            if min(e_64, e_32) > max(tol, 1.5 * r_):
                bad.append((pn, e_32, e_64, r_, tol))
        assert not bad, (name, step, bad)
        # weight-index ties, layer by layer (part 1's rule: a device / oracle difference only where it is verified to be a tie, at most TIE_CHANNEL_CAP of the channels): the
        # running statistics of a channel that holds one -- in this step or an earlier one, they are moving averages -- move with it and get run_layer_case's relaxed bound
        for l in run.E.layers:
            c_ = l.name.split(".")[-1]
            wd = np.argwhere(q32[c_] != device_int_weights(l))
            # (from step 1 on the fold carries the running variance, which in a chain differs between device and oracle downstream of an earlier tie: measured, conv1 at step 1,
            # weights 8.7e-4 / 2.4e-4 of a level from the oracle's rounding boundary on the other side.  Such a difference is accepted where the device's index is the
            # rounding of ITS OWN folded weight -- its weight, gamma, the running variance it had before the step, its per-channel scale -- up to the same tie window.)
            with torch.no_grad():
                t_dev = ((l.w * (l.gamma / torch.sqrt(rv_dev[c_] + O.BN_EPS)).reshape(-1, 1, 1, 1)).double() / l.wscale[: l.cout].double().reshape(-1, 1, 1, 1)).reshape(l.cout, -1).cpu().numpy()
            q_dev = device_int_weights(l)
            for a_, b_ in wd:
                tt = float(t32[c_][a_, b_])
                own = step > 0 and abs(float(t_dev[a_, b_]) - int(q_dev[a_, b_])) <= 0.5 + TIE
                assert abs(int(q_dev[a_, b_]) - int(q32[c_][a_, b_])) == 1 and (abs(abs(tt - np.floor(tt)) - 0.5) <= TIE or own), \
                    (name, step, c_, "weight quantised differently away from a tie", int(a_), int(b_), tt, float(t_dev[a_, b_]), int(q_dev[a_, b_]))
            tie_chs.setdefault(c_, set()).update(int(a_) for a_, _ in wd)
            # the cap is a statement about step 0, where the differences are last-bit ties of equal inputs; later the device's fold and the oracle's start from running
            # variances a few 1e-5 apart, and a layer with 768 / 1440 weights per channel has one within that distance of a boundary in most channels (measured at step 1:
            # 71 of 104 / 150 of 192 channels of reduce_conv, each difference verified above against the device's own fold)
            if step == 0:
                assert len(tie_chs[c_]) <= TIE_CHANNEL_CAP * l.cout, (name, step, c_, len(tie_chs[c_]))
        print(f"    weight-tie channels so far: { {c_: len(v) for c_, v in tie_chs.items()} }")
        # The share of output indices a step apart.  test_g4_block_true_shapes' 2e-3 holds where no weight differs; here weights do (above), and each one moves its channel's
        # outputs by a fraction of a step, which reduce_conv mixes into every output.  The oracle measures that effect on itself: its fp32 and fp64 evaluations differ in n_ref
        # weight indices and in ref_flips of the outputs.  Small perturbations add in quadrature and flip indices in proportion to their size, so n_dev differing weights
        # between device and fp32 oracle account for ref_flips x sqrt(n_dev / n_ref); the bound is 1.5 x that (measured at step 0: 6.1e-2 / 3.6e-2 against 1.75e-1 / 1.51e-1
        # between the evaluations, with about a tenth as many differing weights).
        n_dev = sum(int((q32[l.name.split(".")[-1]] != device_int_weights(l)).sum()) for l in run.E.layers)
        n_ref = sum(int((q32[c_] != q64[c_]).sum()) for c_ in convs)
        flip_bound = max(2e-3, 1.5 * ref_flips * (n_dev / max(n_ref, 1)) ** 0.5)
        print(f"    weights a level apart: device vs fp32 oracle {n_dev}, fp32 vs fp64 oracle {n_ref}; index flips {flips:.2e}, bound {flip_bound:.2e}")
        assert flips <= flip_bound, (name, step, flips, flip_bound, n_dev, n_ref, ref_flips)
        sd = m.state_dict()
        n_state = 0
        for key, v in qs32.sd.items():
            if key.endswith(("scale", "running_var", "running_mean", "min_val", "max_val")):
                # (that test's rtol 2e-3 / atol 2e-4, plus 1.5 x the distance between the oracle's own two evaluations: an observer's min / max is ONE element of a tensor that
                # the tie weights upstream move by a fraction of a step -- measured: reduce_conv's min_val 2.3e-3 from the fp32 evaluation on the 14 x 14 block)
                mine, r32, r64 = sd[key[2:]].detach().double().cpu().numpy().reshape(-1), v.detach().double().numpy().reshape(-1), qs64.sd[key].detach().double().numpy().reshape(-1)
                ok = np.abs(mine - r32) <= 2e-3 * np.abs(r32) + 2e-4 + 1.5 * np.abs(r32 - r64)
                if key.endswith(("running_mean", "running_var")):
                    tc = sorted(tie_chs.get(key.split(".")[1], ()))
                    if tc:
                        ok[tc] |= np.isclose(mine[tc], r32[tc], rtol=2e-2, atol=2e-3)
                if not ok.all():
                    bad.append((key, mine[~ok][:4], r32[~ok][:4], r64[~ok][:4]))
                n_state += 1
        assert not bad, (name, step, bad)
        assert n_state >= 38          # 4 layers x (3 weight-observer + 3 activation-observer + 2 running) entries, + 3 each for quant_cat and skip_add


# ------------------------------------------------------------------------------------------ 6. fp32-gradient mode, per-channel (frost_g32_wq / frost_g32_dgrad with wscale)
@pytest.mark.parametrize("plain", [0, 1], ids=["fast", "plain"])
@pytest.mark.parametrize("name", ["pw16_96_112", "dw5s2_144_56"])
def test_fbgemm_fp32_gradient_mode_layer_vs_oracle(engine, name, plain):
    from frostnet_amd import _lib as L
    lib = L.load_library()
    lib.frost_g32_set_plain(plain)
    try:
        run_case(engine, name, expect=("frost_g32_wq", "frost_g32_dgrad", "frost_g32_wgrad"), g32=True)
    finally:
        lib.frost_g32_set_plain(0)


if __name__ == "__main__":          # one case in a process of its own (environment switches are read at library load): `saturated <name> <qconfig>`
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import engine as EN
    assert sys.argv[1] == "saturated"
    _saturated(EN, sys.argv[2], sys.argv[3], True)

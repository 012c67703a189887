"""Post-training quantisation on the device: histogram calibration of a fused float FrostNet and its conversion to the int8 engine.

The reference's post-quantisation flow (README "Post quantization examples"): float checkpoint -> `fuse_model()` -> `get_default_qconfig(backend)` ->
`torch.quantization.prepare` -> calibration forwards -> `torch.quantization.convert`.  Both default PTQ qconfigs observe activations with
`HistogramObserver` (2048 bins, upsample rate 16; quant range 0..255 for 'qnnpack', 0..127 for 'fbgemm') and weights with plain min/max
(per tensor / per output channel).

This module holds
  * the CPU DEFINITION of one observer update (`hist_update`, fp32 arithmetic restated with numpy) -- what csrc/frost_ptq.hip implements and what the GPU
    tests compare against where stock torch is not called directly;
  * `PtqRunner`: the calibration forward on the device -- the fused float network in fp32 on the float kernels (a fused layer is the coefficient row
    (1, bias)), one observe launch group per activation site, the observers' `min_val` / `max_val` / `histogram` buffers aliased onto one device arena;
  * `PtqConvertedRunner` / `convert`: qparams of every site from stock torch's own `HistogramObserver.calculate_qparams` on ONE host copy of the arena,
    weight qparams by the converted engine's first-observation rule, then the existing converted int8 engine (QNNPACK form for 'qnnpack', FBGEMM form
    for 'fbgemm').
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import call, ptr, stream

BINS, UPSAMPLE = 2048, 16
HDR = 16                               # FROST_PTQ_HDR: words in front of a site's histogram [min, max, batch min, batch max, ...]
SITE_WORDS = HDR + 2 * BINS            # FROST_PTQ_SITE_WORDS: header, fp32 histogram, int32 counts of the running call
ARENA_HDR = 16                         # words in front of the first site; word 0 = count of non-finite activations seen (int32)

_F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------- CPU definition
def _linspace(a, b, n):
    """torch.linspace in fp32: step = (b - a) / (n - 1); element i < n // 2 is fma(step, i, a), the rest fma(-step, n - 1 - i, b) -- ONE rounding each
    (the product of a 24-bit step and an index below 2^16 is exact in fp64, so is its sum with an fp32 value of comparable exponent)."""
    a, b = _F(a), _F(b)
    step = _F((b - a) / _F(n - 1))
    i = np.arange(n, dtype=np.float64)
    lo = (np.float64(step) * i + np.float64(a)).astype(_F)
    hi = (-np.float64(step) * (np.float64(n - 1) - i) + np.float64(b)).astype(_F)
    return np.where(np.arange(n) < n // 2, lo, hi).astype(_F)


def histc(x, lo, hi, bins=BINS):
    """torch.histc(x, bins, lo, hi) on the CPU in fp32, as an fp32 vector of exact integer counts."""
    x = np.asarray(x, dtype=_F).reshape(-1)
    lo, hi = _F(lo), _F(hi)
    if lo == hi:
        lo, hi = _F(lo - _F(1)), _F(hi + _F(1))
    x = x[(x >= lo) & (x <= hi)]
    pos = (((x - lo) / _F(hi - lo)) * _F(bins)).astype(np.int64)
    pos[pos == bins] = bins - 1
    return np.bincount(pos, minlength=bins).astype(_F)


def upscale(hist, mn, mx, nmin, nmax, bins=BINS, rate=UPSAMPLE):
    """HistogramObserver._upscale_histogram: the old histogram (range mn..mx) in the bins of the range nmin..nmax."""
    mn, mx, nmin, nmax = _F(mn), _F(mx), _F(nmin), _F(nmax)
    fine = np.repeat(np.asarray(hist, dtype=_F), rate) / _F(rate)
    bin_size = _F((mx - mn) / _F(bins * rate))
    mid = _linspace(mn, mx, bins * rate + 1)[:-1] + _F(0.5) * bin_size
    bounds = _linspace(nmin, nmax, bins + 1)
    dst = np.clip(np.searchsorted(bounds, mid, side="right") - 1, 0, bins - 1)          # bucketize(right=True) - 1
    out = np.zeros(bins, dtype=_F)
    # every destination bin sums its fine bins in ascending source order, in fp32 (np.add.at is unbuffered and sequential)
    np.add.at(out, dst, fine)
    return out


def hist_init():
    """State of a fresh observer: (min_val, max_val, histogram)."""
    return _F(np.inf), _F(-np.inf), np.zeros(BINS, dtype=_F)


def hist_update(state, x):
    """One HistogramObserver.forward(x) on the state (min_val, max_val, histogram); returns the new state.  Non-finite values are outside the contract."""
    mn, mx, hist = state
    x = np.asarray(x, dtype=_F).reshape(-1)
    if x.size == 0:
        return state
    xmin, xmax = _F(x.min()), _F(x.max())
    if mn == _F(np.inf) or mx == _F(-np.inf):
        return xmin, xmax, histc(x, xmin, xmax)
    nmin, nmax = min(mn, xmin), max(mx, xmax)
    u = histc(x, nmin, nmax)
    if nmin == mn and nmax == mx:
        return mn, mx, (hist + u).astype(_F)
    if mn == mx:                                              # a constant history: all of its mass goes into the bin of that value
        total = _F(np.sum(hist, dtype=_F))
        return nmin, nmax, (histc([mn], nmin, nmax) * total + u).astype(_F)
    return nmin, nmax, (u + upscale(hist, mn, mx, nmin, nmax)).astype(_F)


# ---------------------------------------------------------------------------------------------------------------------------------- public surface
def _check_scope(model):
    from .frostnet import FrostNet
    if type(model).__name__ == "SSDLiteFrostNet" or not isinstance(model, FrostNet):
        raise NotImplementedError("post-training quantisation on the device covers the FrostNet classifier (not the features backbone / SSDLiteFrostNet)")
    if getattr(model, "act", "relu") != "relu":
        raise NotImplementedError("post-training quantisation on the device covers the ReLU FrostNet (act='hswish' is not supported)")
    if not getattr(model, "quantized", False):
        raise NotImplementedError("ptq_prepare needs a frostnet_quant_* model (QuantStub / FloatFunctional sites)")


def ptq_prepare(model, backend="qnnpack"):
    """Classification post-quantisation flow of the reference: eval -> fuse -> default PTQ qconfig -> torch.quantization.prepare.  The tree is stock torch's."""
    from torch.ao.quantization import get_default_qconfig, prepare
    _check_scope(model)
    if backend not in ("qnnpack", "fbgemm"):
        raise NotImplementedError("ptq_prepare supports the default 'qnnpack' and 'fbgemm' qconfigs")
    model.eval()
    model.fuse_model()
    model.qconfig = get_default_qconfig(backend)
    prepare(model, inplace=True)
    return model


class PtqArena:
    """Observer state of every activation site in ONE device tensor: ARENA_HDR words (word 0: non-finite count), then SITE_WORDS per site."""

    def __init__(self, nsites, device):
        self.t = torch.zeros(ARENA_HDR + nsites * SITE_WORDS, dtype=torch.float32, device=device)
        self.nsites, self.next = nsites, 0
        sites = self.t[ARENA_HDR:].view(nsites, SITE_WORDS)
        sites[:, 0] = float("inf")
        sites[:, 1] = float("-inf")
        sites[:, 2] = float("inf")
        sites[:, 3] = float("-inf")

    def alloc(self):
        i = self.next
        self.next += 1
        return self.t[ARENA_HDR + i * SITE_WORDS: ARENA_HDR + (i + 1) * SITE_WORDS]


def _observer_ok(obs):
    return type(obs).__name__ == "HistogramObserver" and obs.bins == BINS and obs.upsample_rate == UPSAMPLE and obs.dtype == torch.quint8


from .float_train import FAct, EMIT, DESC_BYTES      # noqa: E402  (after the CPU definition: importing it needs no device)
from .topology import FloatLayer, bind_trunk, conv_out_hw, model_signature, plan_tree      # noqa: E402


class _PLayer(FloatLayer):
    """One fused layer (Conv2d with the BatchNorm folded into weight and bias, ReLU or not) on the fp32 float kernels."""
    def __init__(self, name, mod, dev, stem=False):
        relu = type(mod).__name__ == "ConvReLU2d"
        conv = mod[0] if relu else mod
        if not isinstance(conv, torch.nn.Conv2d) or conv.bias is None:
            raise RuntimeError(f"{name}: the calibration path expects the fused model (Conv2d with the BatchNorm folded in); call ptq_prepare")
        super().__init__(conv, dev, stem, 16)
        self.name, self.mod, self.relu = name, mod, 1 if relu else 0
        self.stat = torch.zeros(8 * 4 * self.cpad, dtype=torch.float64, device=dev)
        self.coef = torch.zeros(8 * self.cpad, dtype=torch.float32, device=dev)
        self.site = None
        self.desc_ptr = None

    def desc(self):
        # the conv bias travels in the `beta` slot: frost_ptq_coef writes the coefficient rows (scale, bias) = (1, beta)
        return L.FrostFDesc(self.conv.weight.data_ptr(), None, self.conv.bias.data_ptr(), None, None, None, self.pack.data_ptr(), None,
                            self.stat.data_ptr(), self.coef.data_ptr(), None, None, self.cout, self.cin_g, self.k * self.k, self.kind, self.cpad,
                            self.kpad, 0, 1)


class PtqRunner:
    """Calibration forward of a PTQ-prepared FrostNet on the device: fp32 logits, every HistogramObserver updated, no host synchronisation."""
    is_qat, is_ptq, converted, precision = False, True, False, "fp32"

    def __init__(self, model):
        L.load_library()
        _check_scope(model)
        params = list(model.parameters())
        self.model, self.device = model, params[0].device
        if self.device.type != "cuda":
            raise RuntimeError("the calibration runner needs the model on the GPU (a CPU tensor takes the stock modules)")
        dev = self.device
        self.layers, self._obs = [], []
        nsites = sum(1 for m in model.modules() if type(m).__name__ == "HistogramObserver")
        self.qa = PtqArena(nsites, dev)
        plan = plan_tree(model)
        self.q_in = self._site("quant", plan.quant)
        self.stem, self.blocks, self.last = bind_trunk(plan, self._add, self._site)
        self.fc = plan.classifier
        self.q_fc = self._site("classifier.2", self.fc)
        # a block that does not cat / add still owns the FloatFunctional: its observer never sees data on either side (stock convert gives it scale 1, zero-point 0)
        idle = sum((e["q_cat"] is None) + (e["q_add"] is None) for e in self.blocks)
        if self.qa.next + idle != nsites:
            raise NotImplementedError(f"{nsites} HistogramObserver sites in the tree, {self.qa.next} + {idle} idle known to the calibration forward")
        arr = (L.FrostFDesc * len(self.layers))()
        for i, l in enumerate(self.layers):
            arr[i] = l.desc()
        self._table = L.struct_to_tensor(arr, dev)
        for i, l in enumerate(self.layers):
            l.desc_ptr = C.c_void_p(self._table.data_ptr() + i * DESC_BYTES)
        self._err = self.qa.t[:1]
        self._sig = model_signature(model)

    # ------------------------------------------------------------------------------------------ binding
    def _site(self, name, mod):
        """The module's HistogramObserver state moves into a site of the arena; its buffers become views of it (state_dict / load_state_dict keep working)."""
        obs = getattr(mod, "activation_post_process", None)
        if obs is None or not _observer_ok(obs):
            raise NotImplementedError(f"{name}: the device calibration supports the default PTQ qconfigs (HistogramObserver, {BINS} bins, upsample rate {UPSAMPLE})")
        site = self.qa.alloc()
        with torch.no_grad():
            site[0] = obs.min_val.reshape(-1)[0].float() if obs.min_val.numel() else float("inf")
            site[1] = obs.max_val.reshape(-1)[0].float() if obs.max_val.numel() else float("-inf")
            if obs.histogram.numel() == BINS:
                site[HDR: HDR + BINS] = obs.histogram.float()
        obs._buffers["min_val"] = site[0]
        obs._buffers["max_val"] = site[1]
        obs._buffers["histogram"] = site[HDR: HDR + BINS]
        self._obs.append((name, obs, site))
        return site

    def _add(self, name, wrapper, kind):
        mod = wrapper.conv[0]
        l = _PLayer(name, mod, self.device, kind == "stem")
        l.site = self._site(name, mod)
        self.layers.append(l)
        return l

    def still_valid(self):
        return self._sig == model_signature(self.model)

    # ------------------------------------------------------------------------------------------ forward
    def _new(self, n, h, w, c):
        return FAct(torch.empty(n * h * w * c + 64, dtype=torch.float32, device=self.device), n, h, w, c)

    def _observe(self, buf, numel, site):
        call("frost_ptq_observe", ptr(buf), numel, ptr(site), ptr(self._err), stream())

    def _conv(self, l, a):
        if l.kind == 1:
            y = self._new(a.n, *conv_out_hw(a.h, a.w, l.k, l.stride), l.cout)
            call("frost_float_dw_f32", l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, l.relu, EMIT, None, ptr(y.buf), stream())
        else:
            y = self._new(a.n, a.h, a.w, l.cout)
            call("frost_float_pw_f32", l.desc_ptr, ptr(a.buf), ptr(l.pack), y.npix, a.c, l.cout, l.relu, EMIT, None, 0, ptr(y.buf), l.cout, stream())
        self._observe(y.buf, y.npix * y.c, l.site)
        return y

    def forward(self, x):
        if self.model.training:
            raise RuntimeError("a PTQ-prepared model calibrates in eval mode (ptq_prepare leaves it there): call model.eval()")
        if x.dim() != 4 or x.shape[1] != 3 or x.device != self.device:
            raise ValueError("expected an (N,3,H,W) tensor on the model's device")
        if x.numel() == 0:
            raise ValueError("empty batch")
        if x.dtype != torch.float32:
            x = x.float()
        with torch.cuda.device(self.device):
            return self._forward(x.detach())

    def _forward(self, x):
        n, c, h, w = x.shape
        nl = len(self.layers)
        call("frost_float_weight_prep", ptr(self._table), nl, stream())
        call("frost_ptq_coef", ptr(self._table), nl, stream())
        call("frost_ptq_observe_strided", ptr(x), n, c, h, w, *x.stride(), ptr(self.q_in), ptr(self._err), stream())          # QuantStub's observer
        col = self._new(n, *conv_out_hw(h, w, 3, 2), 64)
        call("frost_float_stem_im2col_f32", ptr(x), n, h, w, *x.stride(), ptr(col.buf), stream())
        a = self._conv(self.stem, col)
        for ent in self.blocks:
            inp = a
            if ent["conv1"] is not None:
                if ent["squeeze"] is not None:
                    sq = self._conv(ent["squeeze"], a)
                    cat = self._new(a.n, a.h, a.w, sq.c + a.c)
                    call("frost_float_cat_f32", ptr(sq.buf), sq.c, ptr(a.buf), a.c, a.npix, ptr(cat.buf), stream())
                    self._observe(cat.buf, cat.npix * cat.c, ent["q_cat"])
                    a = cat
                a = self._conv(ent["conv1"], a)
            a = self._conv(ent["reduce"], self._conv(ent["conv2"], a))
            if ent["q_add"] is not None:
                out = self._new(a.n, a.h, a.w, a.c)
                call("frost_float_add_f32", ptr(inp.buf), ptr(a.buf), a.npix * a.c, ptr(out.buf), stream())
                self._observe(out.buf, out.npix * out.c, ent["q_add"])
                a = out
        a = self._conv(self.last, a)
        pooled = torch.empty(a.n, a.c, dtype=torch.float32, device=self.device)
        call("frost_float_avgpool_f32", ptr(a.buf), a.n, a.h * a.w, a.c, None, ptr(pooled), stream())
        nclass = self.fc.out_channels
        logits = torch.empty(a.n, nclass, dtype=torch.float32, device=self.device)
        call("frost_linear_f32", ptr(pooled), ptr(self.fc.weight), ptr(self.fc.bias), a.n, a.c, nclass, ptr(logits), stream())
        self._observe(logits, logits.numel(), self.q_fc)
        return logits

    # ------------------------------------------------------------------------------------------ conversion
    def site_qparams(self):
        """ONE device -> host read of the arena; every site's (scale, zero_point) from stock torch's HistogramObserver.calculate_qparams on the host copy."""
        host = self.qa.t.cpu()
        bad = int(host[:1].view(torch.int32)[0])
        if bad:
            raise RuntimeError(f"hip_convert: {bad} non-finite activation values were seen during calibration (NaN / inf inputs are outside the contract)")
        out = {}
        for i, (name, obs, _) in enumerate(self._obs):
            s = host[ARENA_HDR + i * SITE_WORDS: ARENA_HDR + (i + 1) * SITE_WORDS]
            if not (torch.isfinite(s[0]) and torch.isfinite(s[1])):
                raise RuntimeError(f"hip_convert: the observer of '{name}' has seen no data -- calibrate the PTQ-prepared model first (harness.calibrate)")
            ref = self.model.qconfig.activation()
            ref.min_val, ref.max_val, ref.histogram = s[0].clone(), s[1].clone(), s[HDR: HDR + BINS].clone()
            scale, zp = ref.calculate_qparams()
            out[name] = (float(scale.reshape(-1)[0]), int(zp.reshape(-1)[0]), int(ref.quant_max))
        return out


def convert(model):
    """model.hip_convert() of a PTQ-prepared, calibrated model: returns the runner of the converted int8 engine."""
    cal = model.hip_runner()
    if getattr(cal, "converted", False):
        return cal
    return PtqConvertedRunner(model, cal)


from .runner import FrostRunner       # noqa: E402
from .engine import ConvLayer, Engine, QArena      # noqa: E402


class PtqConvertedRunner(FrostRunner):
    """The converted int8 engine bound to a PTQ tree: every layer in the engine's "bias, no gamma" form (fuse_model() folded the BatchNorm already),
    activation records from the calibrated observers, weight records fresh (their first observation at convert() is plain min/max)."""
    is_qat, is_ptq = False, True

    def __init__(self, model, cal):
        L.load_library()
        self.model, self.device = model, cal.device
        self.flags_dirty = False
        self.ptq_arena = cal.qa.t          # the observers' buffers stay aliased onto the calibration arena
        self._qp = cal.site_qparams()
        wobs = model.qconfig.weight()
        self._pc = type(wobs).__name__ == "PerChannelMinMaxObserver"
        if type(wobs).__name__ not in ("MinMaxObserver", "PerChannelMinMaxObserver") or wobs.dtype != torch.qint8:
            raise NotImplementedError("hip_convert of a PTQ model supports the default weight observers (MinMaxObserver / PerChannelMinMaxObserver, qint8)")
        self.E = Engine(self.device)
        self._recs = {}
        with torch.cuda.device(self.device):
            self._build()
            self.convert()

    def _site(self, name, mod):
        """Activation record of a site, frozen: scale / zero-point of the calibrated observer, its own observer flag off."""
        scale, zp, qmax = self._qp[name]
        rec = self.qa.alloc()
        QArena.set_qparams(rec, scale, zp)
        with torch.no_grad():
            rec[L.Q_QMAX] = float(qmax)
            rec.view(torch.int32)[L.Q_OBS_EN] = 0
        self.E.act_qmax = qmax
        self._recs[id(mod.activation_post_process)] = rec
        return rec

    def _conv_layer(self, name, blk, kind):
        m = blk if kind == "cls" else blk.conv[0]
        relu = type(m).__name__ == "ConvReLU2d"
        conv = m[0] if relu else m
        l = ConvLayer(name, kind, conv.weight, None, None, None, None, None, conv.bias, conv.kernel_size[0], conv.stride[0], relu, self.qa.alloc(),
                      self._site(name, m))
        if self._pc:
            l.per_channel = True
            l.wmin = torch.full((l.cout,), float("inf"), dtype=torch.float32, device=self.device)
            l.wmax = torch.full((l.cout,), float("-inf"), dtype=torch.float32, device=self.device)
        l.qmod = m
        return self.E.add_layer(l)

    def _new_arena(self):
        return QArena(2 * len(self._qp) + 16, self.device)

    def _bind_params(self, params):
        self._params = params          # a converted model has no gradients: no arena

    def _site_qparams(self, obs):
        rec = self._recs.get(id(obs))
        if rec is None:          # the FloatFunctional of a block that does not cat / add: never observed, stock calculate_qparams answers (1, 0)
            return (torch.ones(1), torch.zeros(1, dtype=torch.int64)) if type(obs).__name__ == "HistogramObserver" else None
        return rec[L.Q_SCALE: L.Q_SCALE + 1], rec.view(torch.int32)[L.Q_ZP: L.Q_ZP + 1]

"""Exponential moving average of a model's weights on the device -- the `--model-ema --model-ema-decay 0.9999` of the published FrostNet recipe
(timm `ModelEmaV3` semantics, restated here) as ONE multi-tensor HIP launch (`frost_ema_update`, csrc/frost_ema.hip) that a `harness.GraphedStep` captures
next to the optimizer launch.

    ema = ModelEma(model, decay=0.9999)
    step = GraphedStep(model, criterion, optimizer, ema=ema)          # or: train(..., ema=ema), or ema.update(model) after optimizer.step()
    val(val_loader, ema.module, criterion)

Semantics.  The model's and the shadow's tensors are walked in `state_dict()` key order (parameters and persistent buffers).  Floating-point tensors move by
`shadow = fmaf(w, model - shadow, shadow)`, w = float32(1 - decay_t), which is bit-equal to CPU `shadow.lerp_(model, w)` for w < 0.5; every other dtype is
copied; with `exclude_buffers=True` every buffer is copied.  decay_t = decay, or with `warmup=True` min(decay, (1 + t) / (10 + t)), t = updates made so far.
ONE deliberate departure from the stock loop: where the model's value is not finite the shadow takes it as it is.  An observer that never saw data holds
min_val = +inf / max_val = -inf (FrostNet has such sites for good: the FloatFunctional of a block that neither cats nor adds) and `lerp_` would turn
inf - inf into NaN, which defeats the first-observation test of the observer kernels once the shadow is trained or evaluated.  (A shadow value that is itself
not finite under a finite model value still averages to NaN, as in the stock loop: make the shadow after the model's first training forward, or `set()` it.)

The device table holds raw pointers of the LIVE tensors of both trees (never of `state_dict()`, which clones the buffers a bound model aliases onto its qrecord
arena).  Those tensors are replaced when a runner binds (the shadow's first device forward, `model.to()`, a rebuilt runner), so `prepare_step()` compares a
signature of every pointer and rewrites the table in place in the same device memory: a launch captured earlier reads the new pointers without a recapture.
Only when the entries themselves change (count, sizes, dtypes) is the plan rebuilt; `plan_id` then changes and a `GraphedStep` captures again.

A model that is not on the HIP device takes `update_reference()`: the same definition as torch code, the yardstick of the tests.
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import call, ptr, stream
from .optimizer import _upload

SMALL_UNITS = 1024          # entries below this many units are packed many per workgroup
SMALL_SLICE = 2048          # units of one such workgroup at most (8 per lane)


def _walk(module, prefix=""):
    """(key, owner dict, name, is_parameter) of every entry of `module.state_dict()`, in its order -- the dictionaries, not the tensors: a runner that binds
    replaces the tensor objects in `_buffers`."""
    for name, p in module._parameters.items():
        if p is not None:
            yield prefix + name, module._parameters, name, True
    for name, b in module._buffers.items():
        if b is not None and name not in module._non_persistent_buffers_set:
            yield prefix + name, module._buffers, name, False
    for name, child in module._modules.items():
        if child is not None:
            yield from _walk(child, prefix + name + ".")


def build_map(units):
    """The flat workgroup map of `frost_ema_update` (include/frost_hip.h) for entries of `units[i]` units each: int32 [rows, 4], and the workgroup count.
    One workgroup per FROST_EMA_CHUNK units of a large entry; entries below SMALL_UNITS are packed, at most FROST_EMA_SMALL_ROWS entries and SMALL_SLICE
    units per workgroup.  Entries without units get no work."""
    large, groups, cur, tot = [], [], [], 0
    for i, u in enumerate(units):
        if u <= 0:
            continue
        if u >= SMALL_UNITS:
            large.extend((0, i, c, 0) for c in range((u + L.EMA_CHUNK - 1) // L.EMA_CHUNK))
            continue
        if cur and (len(cur) == L.EMA_SMALL_ROWS or tot + u > SMALL_SLICE):
            groups.append((cur, tot))
            cur, tot = [], 0
        cur.append((i, tot, 0, 0))
        tot += u
    if cur:
        groups.append((cur, tot))
    nwg = len(large) + len(groups)
    head, rows = list(large), []
    for g, tot in groups:
        head.append((1, nwg + len(rows), len(g), tot))
        rows.extend(g)
    return np.asarray(head + rows, dtype=np.int32).reshape(-1, 4), nwg


class ModelEma:
    """`module` is the shadow (`copy.deepcopy(model).eval()`, no gradients); `update(model)` = `launch(prepare_step(model))`; `set(model)` copies; `updates` counts."""

    def __init__(self, model, decay=0.9999, warmup=False, exclude_buffers=False):
        decay = float(decay)
        if not 0.5 < decay <= 1.0:
            raise ValueError(f"ModelEma: decay must be in (0.5, 1] (got {decay}): the update is dst + w * (src - dst) with w = 1 - decay, exact against lerp_ for w < 0.5")
        self.decay, self.warmup, self.exclude_buffers = decay, bool(warmup), bool(exclude_buffers)
        self.module = copy.deepcopy(model).eval()
        self.module.requires_grad_(False)
        self.updates = 0
        self.plan_id = 0            # changes whenever the device plan is rebuilt: a captured launch of an older plan must not be replayed
        self._plan, self._w = None, None

    # ---- the definition ----
    def decay_at(self, t):
        """decay_t for the update that follows `t` earlier ones."""
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    @staticmethod
    def _weight(decay_t):
        """w = 1 - decay_t as the fp32 word the kernel reads."""
        return float(np.float32(1.0 - decay_t))

    def _pairs(self, model):
        src, dst = list(_walk(model)), list(_walk(self.module))
        if [k for k, *_ in src] != [k for k, *_ in dst]:
            raise RuntimeError("ModelEma: the model's state_dict keys differ from the shadow's (the model was restructured after the ModelEma was made, e.g. "
                               "fused / QAT-prepared): make a new ModelEma")
        return src, dst

    def _lerped(self, tensor, is_param):
        return tensor.is_floating_point() and (is_param or not self.exclude_buffers)

    @torch.no_grad()
    def update_reference(self, model, w=None):
        """One update as plain torch code on the live tensors of both trees (any device): the stock loop plus the non-finite rule."""
        if w is None:
            w = self._weight(self.decay_at(self.updates))
            self.updates += 1
        src, dst = self._pairs(model)
        for (_, sd, sn, is_param), (_, dd, dn, _) in zip(src, dst):
            s, d = sd[sn].detach(), dd[dn]
            s = s.to(d.device)
            if w != 1.0 and self._lerped(d, is_param):
                old = d.clone()
                if w < 0.5:
                    d.lerp_(s, w)
                else:                       # (lerp_ switches to another formula there) the same fma through fp64: the product is exact in it
                    d.copy_((old.double() + float(w) * (s - old).double()).to(d.dtype))
                bad = ~torch.isfinite(s)
                if bool(bad.any()):
                    d.copy_(torch.where(bad, s, d))
            else:
                d.copy_(s)

    # ---- the device plan ----
    def _device(self, model):
        for _, d, n, _ in _walk(model):
            return d[n].device
        raise RuntimeError("ModelEma: the model has no parameters or persistent buffers")

    def _entries(self, src, dst, dev):
        """(src tensor, dst tensor, elements, kind) per walked pair; a tensor that occurs twice in the shadow is averaged once."""
        out, seen = [], set()
        for (key, sd, sn, is_param), (_, dd, dn, _) in zip(src, dst):
            s, d = sd[sn], dd[dn]
            if s.device != dev or d.device != dev:
                raise RuntimeError(f"ModelEma: '{key}' is on {s.device} (model) / {d.device} (shadow), the launch runs on {dev}: move both with .to() first")
            if s.dtype != d.dtype or s.numel() != d.numel():
                raise RuntimeError(f"ModelEma: '{key}' is {s.dtype} x {s.numel()} in the model and {d.dtype} x {d.numel()} in the shadow")
            if not (s.is_contiguous() and d.is_contiguous()) and s.numel() > 1:
                raise NotImplementedError(f"ModelEma: '{key}' is not contiguous")
            n = s.numel()
            if d.data_ptr() in seen and n:
                n = 0
            seen.add(d.data_ptr())
            if self._lerped(s, is_param):
                if s.dtype != torch.float32:
                    raise NotImplementedError(f"ModelEma: '{key}' is {s.dtype}; the device launch averages fp32 tensors")
                kind = L.EMA_LERP
            else:
                kind = {1: L.EMA_COPY1, 4: L.EMA_COPY4, 8: L.EMA_COPY8}.get(s.element_size())
                if kind is None:
                    raise NotImplementedError(f"ModelEma: '{key}' has {s.element_size()}-byte elements; the device launch copies 1-, 4- and 8-byte elements")
            if kind != L.EMA_COPY1 and n and (s.data_ptr() % 4 or d.data_ptr() % 4):
                raise NotImplementedError(f"ModelEma: '{key}' is not 4-byte aligned")
            out.append((s, d, n, kind))
        return out

    @staticmethod
    def _tables(entries):
        """Host bytes of the averaging table and of its all-copy twin (`set`)."""
        arr, arr_set = (L.FrostEmaEntry * len(entries))(), (L.FrostEmaEntry * len(entries))()
        for i, (s, d, n, kind) in enumerate(entries):
            for a, k in ((arr, kind), (arr_set, L.EMA_COPY4 if kind == L.EMA_LERP else kind)):
                a[i].src, a[i].dst, a[i].n, a[i].kind = s.data_ptr(), d.data_ptr(), n, k
        return [torch.frombuffer(bytearray(bytes(memoryview(a).cast("B"))), dtype=torch.uint8) for a in (arr, arr_set)]

    @staticmethod
    def _signature(src, dst):
        return tuple(d[n].data_ptr() for _, d, n, _ in src) + tuple(d[n].data_ptr() for _, d, n, _ in dst)

    def _revalidate(self, model):
        """The plan for `model`, its table pointing at the tensors both trees hold NOW."""
        plan = self._plan
        if getattr(self.module, "_hip_converted", False):
            raise RuntimeError("ModelEma: the shadow was hip_convert()-ed (its int8 weights are frozen): convert a copy.deepcopy of ema.module instead")
        if plan is not None and plan["model"] is model:
            try:
                sig = self._signature(plan["src"], plan["dst"])
            except KeyError:                      # a buffer or parameter was removed
                sig = None
            if sig == plan["sig"]:
                return plan
        src, dst = self._pairs(model)
        dev = self._device(model)
        if dev.type != "cuda":
            raise RuntimeError("ModelEma: the launch runs on the HIP device (a model elsewhere takes update_reference)")
        entries = self._entries(src, dst, dev)
        shape = [(n, kind) for _, _, n, kind in entries]
        host, host_set = self._tables(entries)
        sig = self._signature(src, dst)
        if plan is not None and plan["model"] is model and plan["shape"] == shape and plan["device"] == dev:
            # same entries at other addresses (a runner bound and re-aliased its buffers): the same device table, rewritten in place and in stream order
            _upload(plan["table"], host)
            _upload(plan["table_set"], host_set)
            plan.update(src=src, dst=dst, sig=sig, keep=[(s, d) for s, d, _, _ in entries])
            return plan
        wgmap, nwg = build_map([2 * n if kind == L.EMA_COPY8 else n for n, kind in shape])
        fbytes = sum(4 * n for n, kind in shape if kind == L.EMA_LERP)
        cbytes = sum(n * {L.EMA_COPY1: 1, L.EMA_COPY4: 4, L.EMA_COPY8: 8}[kind] for n, kind in shape if kind != L.EMA_LERP)
        if self._w is None or self._w.device != dev:
            self._w = torch.zeros(1, dtype=torch.float32, device=dev)
        self.plan_id += 1
        self._plan = dict(model=model, device=dev, src=src, dst=dst, sig=sig, shape=shape, keep=[(s, d) for s, d, _, _ in entries], table=host.to(dev),
                          table_set=host_set.to(dev), wgmap=torch.from_numpy(wgmap).to(dev), nwg=nwg, nentries=len(entries), id=self.plan_id,
                          traffic=3 * fbytes + 2 * cbytes)
        return self._plan

    def bind_shadow(self):
        """Build the shadow's device executor now (it re-aliases the shadow's observer / qparam buffers onto its own arena), so that the table does not move later."""
        if hasattr(self.module, "hip_runner") and self._device(self.module).type == "cuda":
            self.module.hip_runner()

    def prepare_step(self, model=None):
        """Host side of an update: advance the update count, upload w (pinned staging, stream-ordered), revalidate the table.  Returns the plan for `launch`."""
        model = model if model is not None else (self._plan["model"] if self._plan is not None else None)
        if model is None:
            raise RuntimeError("ModelEma.prepare_step: pass the model on the first call")
        plan = self._revalidate(model)
        w = self._weight(self.decay_at(self.updates))
        self.updates += 1
        _upload(self._w, torch.tensor([w], dtype=torch.float32))
        return plan

    def launch(self, plan=None, table="table"):
        """The one C call (capturable: everything it reads is in device memory)."""
        plan = plan or self._plan
        L.note_raw_write()          # the shadow changes through raw pointers: version-keyed caches must not trust torch's counters
        with torch.cuda.device(plan["device"]):
            call("frost_ema_update", ptr(plan[table]), plan["nentries"], ptr(plan["wgmap"]), plan["nwg"], ptr(self._w), stream(),
                 prof=("ema_update", plan["traffic"]))

    def _on_device(self, model):
        return self._device(model).type == "cuda" and self._device(self.module).type == "cuda"

    @torch.no_grad()
    def update(self, model):
        if not self._on_device(model):
            return self.update_reference(model)
        self.launch(self.prepare_step(model))

    @torch.no_grad()
    def set(self, model):
        """shadow := model, every entry copied (the same launch over the all-copy twin of the table); the update count stays."""
        if not self._on_device(model):
            return self.update_reference(model, w=1.0)
        self.launch(self._revalidate(model), table="table_set")

    # ---- checkpoints ----
    def state_dict(self):
        sd = self.module.state_dict()
        sd["updates"] = self.updates
        return sd

    def load_state_dict(self, state_dict):
        sd = copy.copy(state_dict)                # (a shallow copy that keeps the mapping's `_metadata`)
        self.updates = int(sd.pop("updates", self.updates))
        return self.module.load_state_dict(sd)

"""The FLOAT (not fake-quantised) FrostNet on the HIP kernels: train-mode forward + backward and eval-mode forward.

This is the StatAssist warm-up phase of the reference's schedule (`Classification/train.py:149-165`: the float model is trained
for `FP_epoch` epochs with the same GradBoost optimizer, `is_warmup=True`, before `prepare_qat`), i.e. stock
`Conv2d(bias=False) -> BatchNorm2d -> ReLU` modules in the `frostnet.py:14-145` topology, cross-entropy on the logits.

Reference semantics kept: BatchNorm2d training semantics (batch mean / biased variance to normalise, running statistics updated
with momentum 0.1 and the unbiased variance, `num_batches_tracked += 1`), eval mode uses the running statistics, dropout before the
classifier, parameter gradients accumulated into `p.grad`.  Deviation from the reference (stated tolerance in
`tests/test_gpu_float.py`): by default activations and activation gradients are stored as NHWC bf16 (fp32 accumulation everywhere,
fp32 parameters / statistics / weight gradients).  `precision="fp32"` (FloatRunner argument, `model.float_precision`, or the environment
variable FROST_FLOAT_PRECISION) keeps them in fp32 like the reference and runs the products on the fp32 MFMA: the reference's FP32-train
end-to-end gate applies to that mode (tests/test_gpu_float.py::test_fp32_mode_*).

The module tree stays the owner of every Parameter and buffer; parameter gradients live in one flat fp32 arena (views assigned to
`p.grad`), the same contract as the fake-quant runner, so the multi-tensor GradBoost step and the data-parallel all-reduce work
on it unchanged and `statassist_qat_switch` keeps the optimizer state attached.  No CPU / torch-eager fallback: a missing library raises.
"""
import contextlib
import ctypes as C
import os

import torch

from . import _lib as L
from ._lib import call, ptr, stream
from .topology import (FEATURE_TAPS, SEG_TAPS, SSD_TAPS, FloatLayer, GradArena, act_code, bind_block, bind_detector, bind_trunk, conv_out_hw, model_signature,
                       plan_block, plan_tree, round_up)

STATS, EMIT, BRED, BDC = 0, 1, 2, 3
DESC_BYTES = C.sizeof(L.FrostFDesc)


class FAct:
    """NHWC activation, bf16 (int16 storage) or fp32; 64 elements of slack for the 16-byte tail loads."""
    __slots__ = ("buf", "n", "h", "w", "c", "src")

    def __init__(self, buf, n, h, w, c, src=None):
        self.buf, self.n, self.h, self.w, self.c = buf, n, h, w, c
        self.src = src          # (descriptor pointer, relu) of the producing layer when `buf` holds its CONV OUTPUT (the consumer applies BN + ReLU on load)

    @property
    def npix(self):
        return self.n * self.h * self.w

    def float(self):
        v = self.buf[: self.npix * self.c]
        v = v.view(torch.bfloat16).float() if v.dtype == torch.int16 else v
        return v.view(self.n, self.h, self.w, self.c).permute(0, 3, 1, 2)


_KEEP_CONV = os.environ.get("FROST_FLOAT_KEEP_CONV", "1") != "0"        # training keeps each layer's conv output for element-wise passes (A/B knob)
_WGRAD_SIDE = os.environ.get("FROST_FLOAT_WGRAD_SIDE", "1") != "0"      # weight gradients on a second stream (A/B knob)
_LAZY_EMIT = os.environ.get("FROST_FLOAT_LAZY_EMIT", "1") != "0"        # training: conv1's activation is never written -- the depthwise kernels apply BN + ReLU to its kept conv output on load (A/B knob)


class _FLayer(FloatLayer):
    def __init__(self, name, seq, relu, dev, stem=False, fp32=False):
        conv, bn = seq[0], seq[1]
        if not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d):
            raise RuntimeError("the float device path expects the un-fused float model (Conv2d + BatchNorm2d per layer)")
        kq = 16 if fp32 else 32
        super().__init__(conv, dev, stem, kq)
        self.name, self.bn, self.relu, self.fp32 = name, bn, relu, fp32
        self.pack_t, self.kpad_t = None, 0
        if self.kind == 0:               # the transposed pack of the data gradient's GEMM
            self.kpad_t = round_up(self.cout, kq)
            self.pack_t = torch.zeros(self.pack_bytes(self.cin_g, self.kpad_t, kq), dtype=torch.uint8, device=dev)
        self.stat = torch.zeros(8 * 4 * self.cpad, dtype=torch.float64, device=dev)       # FST_SLOTS copies of [sum, sum of squares, S1, S2]
        self.coef = torch.zeros(8 * self.cpad, dtype=torch.float32, device=dev)
        self.x = None          # saved input of the last recorded forward
        self.c = None          # kept conv output of the last recorded training forward (element-wise backward passes)
        self.desc_ptr = None   # device address of this layer's FrostFDesc

    def desc(self, gviews):
        bn = self.bn
        return L.FrostFDesc(self.conv.weight.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                            bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(), self.pack.data_ptr(),
                            self.pack_t.data_ptr() if self.pack_t is not None else None, self.stat.data_ptr(), self.coef.data_ptr(),
                            gviews[id(bn.weight)].data_ptr(), gviews[id(bn.bias)].data_ptr(), self.cout, self.cin_g,
                            self.k * self.k, self.kind, self.cpad, self.kpad, self.kpad_t, 1 if self.fp32 else 0)


class _FloatFunction(torch.autograd.Function):
    """autograd boundary: image -> logits; backward() runs the hand-written backward pass, which writes the parameter gradients
    into the gradient arena (p.grad views) -- nothing is returned through autograd."""

    @staticmethod
    def forward(ctx, anchor, x, runner):
        ctx.runner = runner
        return runner._forward_impl(x, record=True)

    @staticmethod
    def backward(ctx, dlogits):
        ctx.runner._backward_impl(dlogits)
        return None, None, None


class _FloatFeatFunction(torch.autograd.Function):
    """image -> the four feature maps [x1, x2, x3, x5] (fp32 NCHW) of the features backbone (frostnet_features.py:342-352)."""

    @staticmethod
    def forward(ctx, anchor, x, runner):
        acts = runner._features_impl(x, record=True)
        ctx.runner, ctx.acts = runner, acts
        return tuple(a.float().contiguous() for a in acts)

    @staticmethod
    def backward(ctx, *grads):
        ctx.runner._backward_features(ctx.acts, grads)
        return None, None, None


class FloatRunner(GradArena):
    """Binds a float FrostNet (classification model or features backbone) to the float HIP kernels."""

    def __init__(self, model, precision=None):
        L.load_library()
        self._set_precision(precision or getattr(model, "float_precision", None))
        params = list(model.parameters())
        if not params[0].is_cuda:
            raise RuntimeError("FloatRunner needs the model on the GPU (no CPU fallback on the product path)")
        if model._is_qat_prepared():
            raise RuntimeError("FloatRunner binds the float model; a QAT-prepared model runs through FrostRunner")
        self.model, self.device = model, params[0].device
        self._bind_params(params)
        self.layers = []
        plan = plan_tree(model)
        self.stem, self.blocks, self.last = bind_trunk(plan, self._add)
        self.stage_ends, self.fc, self.drop_rate = plan.stage_ends, plan.classifier, plan.drop_rate
        self.extras, self.heads = bind_detector(plan, self._add)
        self._bind_more()
        self._finish()
        self._stem_tmp = torch.zeros(self.stem.cout * 64, dtype=torch.float32, device=self.device)

    def _bind_more(self):
        """Layers a subclass binds behind the trunk's and the detector's (FloatSegRunner: the segmentation head)."""

    def _set_precision(self, precision):
        precision = precision or os.environ.get("FROST_FLOAT_PRECISION", "bf16")
        if precision not in ("bf16", "fp32"):
            raise ValueError("float path precision is 'bf16' or 'fp32'")
        self.precision, self.fp32 = precision, precision == "fp32"
        self._adt = torch.float32 if self.fp32 else torch.int16          # activation / activation-gradient storage
        sfx = "_f32" if self.fp32 else ""
        self._fn = {n: n + sfx for n in ("frost_float_pw", "frost_float_dw", "frost_float_ew", "frost_float_dw_dgrad", "frost_float_dw_wgrad", "frost_float_pw_wgrad", "frost_float_dw_src", "frost_float_dw_wgrad_src",
                                         "frost_float_grad_merge", "frost_float_avgpool", "frost_float_head_bwd")}
        self._fn["cat"] = "frost_float_cat_f32" if self.fp32 else "frost_infer_cat"
        self._fn["add"] = "frost_float_add_f32" if self.fp32 else "frost_infer_add"
        self._fn["im2col"] = "frost_float_stem_im2col_f32" if self.fp32 else "frost_infer_stem_im2col"

    def _store(self, dst, src_nhwc):
        """fp32 NHWC tensor -> the activation storage type."""
        dst.copy_(src_nhwc.reshape(-1) if self.fp32 else src_nhwc.to(torch.bfloat16).view(torch.int16).reshape(-1))

    @classmethod
    def for_block(cls, block, precision=None):
        """Bind a single float CascadePreExBottleneck (teacher-forced block tests: `block_step`)."""
        L.load_library()
        r = cls.__new__(cls)
        r._set_precision(precision)
        r.model, r.device = block, next(block.parameters()).device
        r._bind_params(list(block.parameters()))
        r.layers, r.stem, r.last, r.fc = [], None, None, None
        r.blocks = [bind_block(plan_block("B", block), r._add)]
        r._finish()
        return r

    def _finish(self):
        arr = (L.FrostFDesc * len(self.layers))()
        for i, l in enumerate(self.layers):
            arr[i] = l.desc(self._gv)
        self._table = L.struct_to_tensor(arr, self.device)
        for i, l in enumerate(self.layers):
            l.desc_ptr = C.c_void_p(self._table.data_ptr() + i * DESC_BYTES)
        self._sig = model_signature(self.model)
        self.on_grads_ready = None      # data-parallel hook: called once when the backward has written every gradient

    def to_act(self, x):
        """fp32 (N,C,H,W) -> NHWC bf16 activation."""
        n, c, h, w = x.shape
        a = self._new(n, h, w, c)
        self._store(a.buf[: n * h * w * c], x.permute(0, 2, 3, 1).contiguous())
        return a

    def block_step(self, x, gy):
        """One teacher-forced train-mode forward + backward of the bound block: returns (y, dx) as fp32 NCHW; p.grad is written."""
        call("frost_float_weight_prep", ptr(self._table), len(self.layers), stream())
        y = self._block(self.blocks[0], self.to_act(x), True, True)
        yf = y.float().contiguous()
        self._grads_written = False              # a test entry: p.grad is overwritten, not accumulated
        self._begin_backward()
        dx = self._block_bwd(self.blocks[0], self.to_act(gy))
        self._end_backward()
        return yf, dx.float().contiguous()

    def _add(self, name, wrapper, kind):
        l = _FLayer(name, wrapper.conv, act_code(wrapper), self.device, kind == "stem", self.fp32)
        self.layers.append(l)
        return l

    def rng_state(self):
        """Dropout Philox stream {seed, draws}: the float warm-up shares the device generator of the fake-quant runner (runner.dropout_mask),
        so harness.save_checkpoint / load_checkpoint resume it the same way."""
        from .runner import rng_state
        return rng_state(self)

    def set_rng_state(self, state):
        from .runner import set_rng_state
        set_rng_state(self, state)

    def still_valid(self):
        return self._sig == model_signature(self.model)

    def enable_data_parallel(self, nbuckets=1, group=None):
        """Data-parallel warm-up: the same one exchange step as the fake-quant path (frostnet_amd.parallel.GradSync over the flat
        gradient arena); the float backward hands the whole arena over when it ends, `grad_sync.finish()` waits and averages."""
        self.on_grads_ready = lambda: self.grad_sync.ready(0)
        return self._attach_grad_sync(nbuckets, group)

    def _new(self, n, h, w, c):
        return FAct(torch.empty(n * h * w * c + 64, dtype=self._adt, device=self.device), n, h, w, c)

    # ------------------------------------------------------------------------------------------ forward
    def _conv(self, l, a, training, record, out=None, ldy=None, lazy=False):
        """Conv -> BN -> [ReLU] (frostnet.py:14-60).  `out`/`ldy`: write into a slice of a wider buffer (the cat).
        lazy (training, kept conv output): no emit pass -- the returned activation carries the conv output and `src`, its only consumer (the depthwise layer)
        applies BN + ReLU on load (frost_float_dw_src / frost_float_dw_wgrad_src)."""
        ho, wo = conv_out_hw(a.h, a.w, l.k, l.stride) if l.kind == 1 else (a.h, a.w)
        lazy = bool(lazy and out is None and training and _KEEP_CONV)
        y = self._new(a.n, ho, wo, l.cout) if (out is None and not lazy) else None
        npix_o = a.n * ho * wo
        dst, ld = (ptr(y.buf) if y is not None else None, l.cout) if out is None else (out, ldy)
        if training and _KEEP_CONV:
            # training: ONE convolution per layer.  The statistics pass stores the conv output c; y = [relu](c*scale + bias) is an element-wise pass
            # over c, and so are the backward's statistics and dc (frost_float_ew) -- c is kept until the layer's backward
            cbuf = torch.empty(npix_o * l.cout + 64, dtype=self._adt, device=self.device)
            if l.kind == 1:
                if a.src is not None:
                    call(self._fn["frost_float_dw_src"], l.desc_ptr, ptr(a.buf), a.src[0], a.src[1], a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), STATS, ptr(cbuf), stream())
                else:
                    call(self._fn["frost_float_dw"], l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), STATS, None, ptr(cbuf), stream())
            else:
                call(self._fn["frost_float_pw"], l.desc_ptr, ptr(a.buf), ptr(l.pack), npix_o, a.c, l.cout, int(l.relu), STATS, None, 0, ptr(cbuf), l.cout, stream())
            call("frost_float_bn_finalize", l.desc_ptr, l.cout, npix_o, stream())
            L.note_raw_write()          # running_mean / running_var change through raw pointers: the bf16-inference weight cache must not trust torch's version counters
            if lazy:
                y = FAct(cbuf, a.n, ho, wo, l.cout, src=(l.desc_ptr, int(l.relu)))
            else:
                call(self._fn["frost_float_ew"], l.desc_ptr, ptr(cbuf), npix_o, l.cout, int(l.relu), EMIT, None, 0, dst, ld, stream())
            if record:
                l.c = cbuf
        elif l.kind == 1:
            if training:
                call(self._fn["frost_float_dw"], l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), STATS, None, None, stream())
                call("frost_float_bn_finalize", l.desc_ptr, l.cout, npix_o, stream())
                L.note_raw_write()
            call(self._fn["frost_float_dw"], l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), EMIT, None, dst, stream())
        else:
            if training:
                call(self._fn["frost_float_pw"], l.desc_ptr, ptr(a.buf), ptr(l.pack), npix_o, a.c, l.cout, int(l.relu), STATS, None, 0, None, 0, stream())
                call("frost_float_bn_finalize", l.desc_ptr, l.cout, npix_o, stream())
                L.note_raw_write()
            call(self._fn["frost_float_pw"], l.desc_ptr, ptr(a.buf), ptr(l.pack), npix_o, a.c, l.cout, int(l.relu), EMIT, None, 0, dst, ld, stream())
        if record:
            l.x = a
        return y

    def _block(self, ent, a, training, record):
        """CascadePreExBottleneck.forward (frostnet.py:124-145)."""
        blk, inp = ent["blk"], a
        if ent["conv1"] is not None:
            if ent["squeeze"] is not None:
                cs = ent["squeeze"].cout
                cat = self._new(a.n, a.h, a.w, cs + a.c)
                sq = self._conv(ent["squeeze"], a, training, record)
                call(self._fn["cat"], ptr(sq.buf), cs, ptr(a.buf), a.c, a.npix, ptr(cat.buf), stream())     # cat([squeezed, x], 1)
                a = cat
            c2 = ent["conv2"]
            a = self._conv(ent["conv1"], a, training, record,
                           lazy=bool(training and _KEEP_CONV and _LAZY_EMIT and c2.kind == 1 and c2.k in (3, 5) and c2.stride in (1, 2)))
        a = self._conv(ent["conv2"], a, training, record)
        a = self._conv(ent["reduce"], a, training, record)
        if not blk.reduction:
            out = self._new(a.n, a.h, a.w, a.c)
            call(self._fn["add"], ptr(inp.buf), ptr(a.buf), a.npix * a.c, ptr(out.buf), stream())
            a = out
        if record:
            ent["inp"], ent["out"] = inp, a
        return a

    def _trunk(self, x, training, record):
        if x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
            raise ValueError("expected an (N,3,H,W) tensor on the model's device")
        if x.numel() == 0:
            raise ValueError("empty batch")
        if x.dtype != torch.float32:
            x = x.float()
        n, _, h, w = x.shape
        if training:
            for l in self.layers:
                if not l.bn.training:
                    raise NotImplementedError(f"{l.name}: BatchNorm in eval mode inside a training forward of the FLOAT model (_freeze_stages): the float HIP "
                                              "backward implements the batch-statistics gradient only; the QAT-prepared model supports frozen BatchNorm")
        call("frost_float_weight_prep", ptr(self._table), len(self.layers), stream())
        if not training:
            call("frost_float_bn_eval", ptr(self._table), len(self.layers), stream())
        col = self._new(n, *conv_out_hw(h, w, 3, 2), 64)
        call(self._fn["im2col"], ptr(x), n, h, w, x.stride(0), x.stride(1), x.stride(2), x.stride(3), ptr(col.buf), stream())
        a = self._conv(self.stem, col, training, record)
        outs = []
        for ent in self.blocks:
            a = self._block(ent, a, training, record)
            outs.append(a)
        return a, outs

    def forward(self, x):
        if self.model.training and torch.is_grad_enabled():
            return _FloatFunction.apply(self._params[0], x, self)
        return self._forward_impl(x, record=False)

    def _forward_impl(self, x, record):
        training = self.model.training
        a, _ = self._trunk(x, training, record)
        a = self._conv(self.last, a, training, record)
        drop = None
        if training and self.drop_rate > 0.0:
            keep = 1.0 - self.drop_rate
            from .runner import dropout_mask          # the same device Philox stream as the fake-quant runner (seed from torch + rank, resumable)
            drop = dropout_mask(self, a.n * a.c, keep).view(a.n, a.c)
        pooled = torch.empty(a.n, a.c, dtype=torch.float32, device=self.device)
        call(self._fn["frost_float_avgpool"], ptr(a.buf), a.n, a.h * a.w, a.c, ptr(drop), ptr(pooled), stream())
        nclass = self.fc.out_channels
        logits = torch.empty(a.n, nclass, dtype=torch.float32, device=self.device)
        call("frost_linear_f32", ptr(pooled), ptr(self.fc.weight), ptr(self.fc.bias), a.n, a.c, nclass, ptr(logits), stream())
        if record:
            self._head = (a, pooled, drop)
        return logits

    def forward_features(self, x):
        if self.model.training and torch.is_grad_enabled():
            return list(_FloatFeatFunction.apply(self._params[0], x, self))
        return [a.float().contiguous() for a in self._features_impl(x, record=False)]

    def _features_impl(self, x, record):
        _, outs = self._trunk(x, self.model.training, record)
        return [outs[self.stage_ends[i]] for i in FEATURE_TAPS]

    # ------------------------------------------------------------------------------------------ backward
    def _conv_bwd(self, l, gy, ldg, need_dx):
        """gy: device pointer (c_void_p) of the bf16 output gradient, rows of ldg elements.  Returns dx (FAct) or None."""
        a = l.x
        ho, wo = conv_out_hw(a.h, a.w, l.k, l.stride) if l.kind == 1 else (a.h, a.w)
        npix_o = a.n * ho * wo
        dc = torch.empty(npix_o * l.cout + 64, dtype=self._adt, device=self.device)
        gw = self._gv[id(l.conv.weight)]
        dx = None
        kept = getattr(l, "c", None)
        if kept is not None:          # the conv output of the forward is at hand: statistics and dc are element-wise
            call(self._fn["frost_float_ew"], l.desc_ptr, ptr(kept), npix_o, l.cout, int(l.relu), BRED, gy, ldg, None, 0, stream())
            call("frost_float_bwd_finalize", l.desc_ptr, l.cout, npix_o, stream())
            call(self._fn["frost_float_ew"], l.desc_ptr, ptr(kept), npix_o, l.cout, int(l.relu), BDC, gy, ldg, ptr(dc), l.cout, stream())
            l.c = None
        if l.kind == 1:
            if kept is None:
                if ldg != l.cout:
                    raise RuntimeError("depthwise gradients are dense")
                call(self._fn["frost_float_dw"], l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), BRED, gy, None, stream())
                call("frost_float_bwd_finalize", l.desc_ptr, l.cout, npix_o, stream())
                call(self._fn["frost_float_dw"], l.desc_ptr, ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, int(l.relu), BDC, gy, ptr(dc), stream())
            if need_dx:
                dx = self._new(a.n, a.h, a.w, a.c)
                call(self._fn["frost_float_dw_dgrad"], l.desc_ptr, ptr(dc), a.n, a.h, a.w, a.c, l.k, l.stride, ptr(dx.buf), stream())
            if a.src is not None:
                self._on_side(lambda: call(self._fn["frost_float_dw_wgrad_src"], ptr(dc), ptr(a.buf), a.src[0], a.src[1], a.n, a.h, a.w, a.c, l.k, l.stride, ptr(gw), stream()), dc, a)
            else:
                self._on_side(lambda: call(self._fn["frost_float_dw_wgrad"], ptr(dc), ptr(a.buf), a.n, a.h, a.w, a.c, l.k, l.stride, ptr(gw), stream()), dc, a)
        else:
            if kept is None:
                call(self._fn["frost_float_pw"], l.desc_ptr, ptr(a.buf), ptr(l.pack), npix_o, a.c, l.cout, int(l.relu), BRED, gy, ldg, None, 0, stream())
                call("frost_float_bwd_finalize", l.desc_ptr, l.cout, npix_o, stream())
                call(self._fn["frost_float_pw"], l.desc_ptr, ptr(a.buf), ptr(l.pack), npix_o, a.c, l.cout, int(l.relu), BDC, gy, ldg, ptr(dc), l.cout, stream())
            if need_dx:
                dx = self._new(a.n, a.h, a.w, a.c)
                # data gradient = a plain bf16 GEMM with the transposed pack: the tuned pointwise skeleton (DMA double-buffered tiles,
                # resident weights, LDS-staged output) that also serves the fake-quant dgrad and the bf16 inference layers
                if self.fp32:     # the same GEMM on the fp32 MFMA (mode 4 of the float pointwise kernel)
                    call("frost_float_pw_f32", None, ptr(dc), ptr(l.pack_t), npix_o, l.cout, a.c, 0, 4, None, 0, ptr(dx.buf), a.c, stream())
                elif l.kind == 0 and L.load_library().frost_pw_dgrad_wide_ok(npix_o, a.c, l.cout):
                    call("frost_pw_dgrad_wide", ptr(dc), ptr(l.pack_t), None, npix_o, a.c, l.cout, ptr(dx.buf), 0, stream())      # the stand-alone bf16 GEMM (frost_wgrad.hip)
                else:
                    call("frost_infer_pw", ptr(dc), ptr(l.pack_t), None, npix_o, l.cout, a.c, 0, ptr(dx.buf), stream())
            if l.kind == 2:
                self._stem_tmp.zero_()
                call(self._fn["frost_float_pw_wgrad"], ptr(dc), ptr(a.buf), npix_o, 64, 64, l.cout, ptr(self._stem_tmp), 64, stream())
                call("frost_float_stem_wscatter", ptr(self._stem_tmp), l.cout, ptr(gw), stream())
            else:
                self._on_side(lambda: call(self._fn["frost_float_pw_wgrad"], ptr(dc), ptr(a.buf), npix_o, a.c, a.c, l.cout, ptr(gw), a.c, stream()), dc, a)
        l.x = None
        return dx

    def _block_bwd(self, ent, g, need_dx=True):
        """g: FAct gradient of the block output.  Returns the gradient of the block input."""
        blk, inp = ent["blk"], ent["inp"]
        res = g if not blk.reduction else None            # add: the gradient reaches both branches unchanged
        d = self._conv_bwd(ent["reduce"], ptr(g.buf), g.c, True)
        d = self._conv_bwd(ent["conv2"], ptr(d.buf), d.c, ent["conv1"] is not None or need_dx or res is not None)
        cat, cs, sq = None, 0, None
        if ent["conv1"] is not None:
            d = self._conv_bwd(ent["conv1"], ptr(d.buf), d.c, True)
            if ent["squeeze"] is not None:
                cs = ent["squeeze"].cout
                cat = d                                       # gradient of cat([squeezed, x]): columns [0, cs) -> squeeze, [cs, ..) -> x
                sq = self._conv_bwd(ent["squeeze"], ptr(cat.buf), cat.c, True)
                d = None
        ent["inp"] = ent["out"] = None
        if res is None and cat is None:
            return d
        out = self._new(inp.n, inp.h, inp.w, inp.c)
        direct = d if cat is None else sq                     # dense gradient w.r.t. the block input from the conv chain
        call(self._fn["frost_float_grad_merge"], ptr(res.buf) if res is not None else None, ptr(cat.buf) if cat is not None else None, cs,
             cat.c if cat is not None else 8, ptr(direct.buf) if direct is not None else None, inp.npix, inp.c, ptr(out.buf), stream())
        return out

    def _begin_backward(self):
        """torch semantics: backward() accumulates into p.grad until zero_grad().  Gradients the caller has not cleared are set aside (one copy of
        the arena) and added back by _end_backward; in the usual loop (zero_grad() -> p.grad is None) nothing is copied."""
        prev = None
        live = [getattr(self, "_grads_written", False) and p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                for p, v in zip(self._params, self._grad_views)]
        if any(live):
            if getattr(self, "grad_sync", None) is not None:
                raise RuntimeError("gradient accumulation over several backward passes is not supported together with the data-parallel exchange")
            prev = self.grad_arena.clone()
            for ok, v in zip(live, self._grad_views):
                if not ok:
                    prev[v.storage_offset(): v.storage_offset() + v.numel()].zero_()
        self.bind_grads()
        self.grad_arena.zero_()
        self._carry = prev
        self._keep = []

    def _on_side(self, launch, *keep):
        """Weight gradients are off the backward's critical path (nothing reads them before the optimizer): they run on a second stream under
        the next layers' passes, which at the 14x14 / 7x7 stages leave most of the GPU idle.  `keep`: the buffers the launch reads -- held until
        the join in _end_backward, so the caching allocator cannot hand them to the main stream while the side stream still reads them."""
        if not _WGRAD_SIDE:
            return launch()
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            launch()
        self._keep.extend(keep)

    def _end_backward(self):
        if getattr(self, "_side", None) is not None and self._keep:
            torch.cuda.current_stream().wait_stream(self._side)
        self._keep = []
        if getattr(self, "_carry", None) is not None:
            self.grad_arena.add_(self._carry)
        self._carry = None
        self._grads_written = True

    def _trunk_bwd(self, g, taps=None):
        for i in range(len(self.blocks) - 1, -1, -1):
            if taps is not None and i in taps:
                t = taps[i]
                if g is None:
                    g = t
                else:
                    s = self._new(g.n, g.h, g.w, g.c)
                    call(self._fn["add"], ptr(g.buf), ptr(t.buf), g.npix * g.c, ptr(s.buf), stream())
                    g = s
            if g is None:
                continue
            g = self._block_bwd(self.blocks[i], g)
        self._conv_bwd(self.stem, ptr(g.buf), g.c, False)
        self._end_backward()
        if self.on_grads_ready is not None:
            self.on_grads_ready()

    def _backward_impl(self, dlogits):
        self._begin_backward()
        a, pooled, drop = self._head
        self._head = None
        dl = dlogits.contiguous().float()
        n, nclass = dl.shape
        g = self._new(a.n, a.h, a.w, a.c)
        scratch = torch.empty(n, a.c, dtype=torch.float32, device=self.device)
        call(self._fn["frost_float_head_bwd"], ptr(dl), ptr(pooled), ptr(self.fc.weight), n, a.c, nclass, a.h * a.w, ptr(drop),
             ptr(self._gv[id(self.fc.weight)]), ptr(self._gv[id(self.fc.bias)]), ptr(g.buf), ptr(scratch), stream())
        g = self._conv_bwd(self.last, ptr(g.buf), g.c, True)
        self._trunk_bwd(g)

    def _backward_features(self, acts, grads):
        self._begin_backward()
        taps = {}
        for bi, a, gr in zip((self.stage_ends[i] for i in FEATURE_TAPS), acts, grads):
            if gr is None:
                continue
            t = self._new(a.n, a.h, a.w, a.c)
            self._store(t.buf[: a.npix * a.c], gr.float().permute(0, 2, 3, 1).contiguous())
            taps[bi] = t
        # blocks after the last tap (x4 -> x5 are all used; nothing is dead in the reference's backbone)
        self._trunk_bwd(None, taps)


# ---------------------------------------------------------------------------------------------------------------------------------- SSDLite detector
class _FloatSSDFunction(torch.autograd.Function):
    """image -> (loc [N,P,4], conf [N,P,C]) of the float SSDLite detector; backward scatters their gradients onto the twelve maps and runs the
    hand-written backward.  A loss that uses only one of the two hands None for the other (materialize_grads off): a zero gradient."""

    @staticmethod
    def forward(ctx, anchor, x, runner):
        ctx.set_materialize_grads(False)
        heads = runner._maps_impl(x, record=True, lazy_heads=_LAZY_EMIT)
        ctx.runner, ctx.heads = runner, heads
        return runner._gather(heads)

    @staticmethod
    def backward(ctx, dloc, dconf):
        heads, ctx.heads = ctx.heads, None
        ctx.runner._backward_ssd(heads, dloc=dloc, dconf=dconf)
        return None, None, None


class _FloatSSDMapsFunction(torch.autograd.Function):
    """image -> the twelve prediction maps [loc0, conf0, loc1, ...] as fp32 NCHW (SSDRunner.forward_maps' surface, for debugging)."""

    @staticmethod
    def forward(ctx, anchor, x, runner):
        heads = runner._maps_impl(x, record=True, lazy_heads=False)
        ctx.runner, ctx.heads = runner, heads
        return tuple(o.float().contiguous() for o, _ in heads)

    @staticmethod
    def backward(ctx, *grads):
        heads, ctx.heads, run = ctx.heads, None, ctx.runner
        gs = []
        for (o, _), g in zip(heads, grads):
            t = run._new(o.n, o.h, o.w, o.c)
            if g is None:
                t.buf.zero_()
            else:
                run._store(t.buf[: o.npix * o.c], g.float().permute(0, 2, 3, 1).contiguous())
            gs.append(t)
        run._backward_ssd(heads, grads=gs)
        return None, None, None


class FloatSSDRunner(FloatRunner):
    """frostnet_amd.ssdlite.SSDLiteFrostNet in float mode on the float kernels (the StatAssist warm-up of the detector, Object_Detection/qtrainval.py:187-238,
    or a whole float run): backbone sources at strides 8 / 16 / 32, the SSDLite extras (1x1 -> depthwise 3x3 stride 2 -> 1x1, BN + ReLU each) and the
    separable heads (depthwise 3x3 + BN + ReLU, 1x1 + BN), then the twelve maps gathered into (loc, conf) by one HIP launch (frost_float_ssd_gather).
    Training: each head's 1x1 conv output is kept for its backward anyway, so the gather applies that layer's BatchNorm on load and the head emit passes
    never run (fp32 outputs to the loss in both precisions); eval reads the emitted maps.  Backward: frost_float_ssd_scatter -> heads -> per-source sum of
    the loc / conf head gradients and the next extra stage's -> extras in reverse -> the trunk with taps at the three backbone sources."""

    def _set_precision(self, precision):
        super()._set_precision(precision)
        sfx = "_f32" if self.fp32 else ""
        self._fn["ssd_gather"] = "frost_float_ssd_gather" + sfx
        self._fn["ssd_scatter"] = "frost_float_ssd_scatter" + sfx

    def __init__(self, model, precision=None):
        super().__init__(model, precision)
        self.anchors, self.num_classes = list(model.ANCHORS), int(model.num_classes)

    def _check_train_input(self, x):
        """torch BatchNorm2d refuses a training forward with one value per channel; here the 1x1 tail maps would otherwise be normalised with var = 0."""
        if x.dim() != 4 or not x.is_cuda:
            raise ValueError("expected an (N,3,H,W) tensor on the model's device")
        n, h, w = x.shape[0], x.shape[2], x.shape[3]
        for l in self.layers:               # forward order; only the stride-2 layers change the map size (every one pads (k - 1) / 2)
            if l.stride == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if n * h * w == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([{n}, {self.extras[-1][2].cout}, {h}, {w}])")

    def forward(self, x):
        """(loc [N,P,4], conf [N,P,C]) fp32 -- SSDLiteFrostNet._assemble of the twelve maps."""
        if self.model.training and torch.is_grad_enabled():
            return _FloatSSDFunction.apply(self._params[0], x, self)
        return self._gather(self._maps_impl(x, record=False, lazy_heads=_LAZY_EMIT))

    def forward_maps(self, x):
        """The twelve maps [loc0, conf0, loc1, ...] as fp32 NCHW (conf maps with their padding channels), like SSDRunner.forward_maps."""
        if self.model.training and torch.is_grad_enabled():
            return list(_FloatSSDMapsFunction.apply(self._params[0], x, self))
        return [o.float().contiguous() for o, _ in self._maps_impl(x, record=False, lazy_heads=False)]

    def _maps_impl(self, x, record, lazy_heads):
        """-> [(head output FAct, its 1x1 layer)] x 12.  lazy_heads (training): the FAct holds the 1x1 conv output, BatchNorm not yet applied."""
        training = self.model.training
        if training:
            self._check_train_input(x)
        a, outs = self._trunk(x, training, record)
        sources = [outs[self.stage_ends[i]] for i in SSD_TAPS]
        for pw1, dw, pw2 in self.extras:           # pw1 -> dw like conv1 -> conv2 of a block: the depthwise layer applies pw1's BN + ReLU on load
            t = self._conv(pw1, a, training, record, lazy=_LAZY_EMIT)
            a = self._conv(pw2, self._conv(dw, t, training, record), training, record)
            sources.append(a)
        heads = []
        for s, (ldw, lpw, cdw, cpw) in zip(sources, self.heads):
            for dw, pw in ((ldw, lpw), (cdw, cpw)):
                heads.append((self._conv(pw, self._conv(dw, s, training, record), training, record, lazy=lazy_heads), pw))
        return heads

    def _ssd_table(self, heads, grads=None):
        """FrostSSDMap host table of the twelve maps (include/frost_hip.h) -> (table, N, P)."""
        tab = (L.FrostSSDMap * len(heads))()
        offs, p = [], 0
        for k, a in enumerate(self.anchors):
            o = heads[2 * k][0]
            offs.append(p)
            p += o.h * o.w * a
        for i, (o, pw) in enumerate(heads):
            k, which = divmod(i, 2)
            width = 4 if which == 0 else self.num_classes
            m = tab[i]
            m.buf = (grads[i] if grads is not None else o).buf.data_ptr()
            m.coef = pw.coef.data_ptr() if (grads is None and o.src is not None) else None
            m.hw, m.doff, m.stored, m.used, m.cpad, m.which = o.h * o.w, offs[k] * width, o.c, self.anchors[k] * width, pw.cpad, which
        return tab, heads[0][0].n, p

    def _gather(self, heads):
        tab, n, p = self._ssd_table(heads)
        c = self.num_classes
        loc = torch.empty(n, p, 4, dtype=torch.float32, device=self.device)
        conf = torch.empty(n, p, c, dtype=torch.float32, device=self.device)
        call(self._fn["ssd_gather"], tab, len(heads), n, p * 4, p * c, ptr(loc), ptr(conf), stream())
        return loc, conf

    def _sum(self, a, b):
        s = self._new(a.n, a.h, a.w, a.c)
        call(self._fn["add"], ptr(a.buf), ptr(b.buf), a.npix * a.c, ptr(s.buf), stream())
        return s

    def _backward_ssd(self, heads, dloc=None, dconf=None, grads=None):
        """grads: the twelve map gradients (FAct) -- or None: scattered from dloc / dconf (fp32 [N,P,4] / [N,P,C]; None = zero)."""
        self._begin_backward()
        if grads is None:
            grads = [self._new(o.n, o.h, o.w, o.c) for o, _ in heads]
            tab, n, p = self._ssd_table(heads, grads)
            dl = dloc.contiguous().float() if dloc is not None else None
            dc = dconf.contiguous().float() if dconf is not None else None
            call(self._fn["ssd_scatter"], tab, len(heads), n, p * 4, p * self.num_classes, ptr(dl), ptr(dc), stream())
        self._keep.extend(g.buf for g in grads)         # (held until the side stream's join in _end_backward, with the heads' kept conv outputs)
        self._keep.extend(o.buf for o, _ in heads)
        srcg = []
        for k, (ldw, lpw, cdw, cpw) in enumerate(self.heads):
            gl, gc = grads[2 * k], grads[2 * k + 1]
            d = self._conv_bwd(lpw, ptr(gl.buf), gl.c, True)
            dl_ = self._conv_bwd(ldw, ptr(d.buf), d.c, True)
            d = self._conv_bwd(cpw, ptr(gc.buf), gc.c, True)
            srcg.append(self._sum(dl_, self._conv_bwd(cdw, ptr(d.buf), d.c, True)))
        g = srcg[5]
        for i in range(len(self.extras) - 1, -1, -1):      # extra stage i maps source i + 2 to source i + 3
            pw1, dw, pw2 = self.extras[i]
            d = self._conv_bwd(pw2, ptr(g.buf), g.c, True)
            d = self._conv_bwd(dw, ptr(d.buf), d.c, True)
            d = self._conv_bwd(pw1, ptr(d.buf), d.c, True)
            g = self._sum(srcg[i + 2], d)
        self._trunk_bwd(None, dict(zip((self.stage_ends[i] for i in SSD_TAPS), (srcg[0], srcg[1], g))))


# ---------------------------------------------------------------------------------------------------------------------------------- segmentation network
class _FloatSegFunction(torch.autograd.Function):
    """image -> stride-8 logits of the float FrostNetSeg; backward runs head -> trunk by hand and writes the parameter gradients into the arena."""

    @staticmethod
    def forward(ctx, anchor, x, runner):
        ctx.runner = runner
        return runner._seg_impl(x, record=True)

    @staticmethod
    def backward(ctx, dout):
        run = ctx.runner
        run._begin_backward()
        dc1, dc4 = run._head_bwd(dout)
        run._trunk_bwd(None, dict(zip((run.stage_ends[i] for i in SEG_TAPS), (dc1, dc4))))
        return None, None, None


class FloatSegRunner(FloatRunner):
    """frostnet_amd.seg_model.FrostNetSeg in float mode on the float kernels: the trunk with taps at x2 (stride 8) and x5 (stride 32), then the Lite R-ASPP head.
    b0 and b1's conv + BatchNorm are ordinary float layers (_conv / _conv_bwd: batch statistics, running statistics, backward); the pool, the gate, `project`,
    `auxlayer` and both upsamplings are csrc/frost_seghead.hip.  project(up(z)) is computed as up(project(z)): nothing of 128 channels exists at c1's resolution.
    The logits are fp32 NHWC memory returned as a channels-last NCHW view; frost_seg_forward reads them through strides and hands back its gradient in the same
    layout, which frost_seghead_logits_bwd reads through strides again: no copy on the way to the criterion or back."""

    def _set_precision(self, precision):
        def table(prec):
            FloatRunner._set_precision(self, prec)
            sfx = "_f32" if self.fp32 else ""
            for n in ("pool", "pool_bwd", "gate_project", "gate_project_bwd", "logits", "logits_bwd"):
                self._fn["sh_" + n] = "frost_seghead_" + n + sfx
            return self._fn
        self._fn32 = table("fp32")          # the entries of the head's c4-resolution part (_c4_scope)
        table(precision)

    @contextlib.contextmanager
    def _c4_scope(self):
        """The head's c4-resolution part -- b0, the pool, b1, gate + project and their backward -- runs in fp32 storage in BOTH modes: at stride 32 it is a few
        per cent of the head's own traffic, and in bf16 storage b0's ReLU mask taken from a rounded conv output and the bf16 weight packs would put 3e-2 on dc4 and
        on the head's parameter gradients, the first gradients of the whole backward.  Inside the scope the runner's entry table, storage type and `_new` are the
        fp32 mode's; c4 is widened on entry (_widen) and the tap gradient at x5 is rounded once to the storage type on exit."""
        if self.fp32:
            yield
            return
        saved = (self.precision, self.fp32, self._adt, self._fn)
        self.precision, self.fp32, self._adt, self._fn = "fp32", True, torch.float32, self._fn32
        try:
            yield
        finally:
            self.precision, self.fp32, self._adt, self._fn = saved

    def _widen(self, a):
        """The activation in fp32 storage (itself in fp32 mode)."""
        if a.buf.dtype == torch.float32:
            return a
        f = FAct(torch.empty(a.npix * a.c + 64, dtype=torch.float32, device=self.device), a.n, a.h, a.w, a.c)
        f.buf[: a.npix * a.c].copy_(a.buf[: a.npix * a.c].view(torch.bfloat16))
        return f

    def _bind_more(self):
        self._bind_head(self.model.head, "head.")

    def _bind_head(self, head, prefix=""):
        if not 2 <= head.nclass <= 255:
            raise ValueError(f"FloatSegRunner: 2 <= nclass <= 255 (the criterion's range), got {head.nclass}")
        self.head = head
        with self._c4_scope():              # fp32 layer records: fp32 weight packs, the fp32 MFMA
            self.b0 = self._add(prefix + "lr_aspp.b0", head.lr_aspp.b0, "pw")
            self.b1 = self._add(prefix + "lr_aspp.b1.1", head.lr_aspp.b1[1], "pw")

    @classmethod
    def for_head(cls, head, precision=None):
        """Bind a single LRASPPHead (teacher-forced head tests: `head_step`, `head_eval`)."""
        L.load_library()
        r = cls.__new__(cls)
        r._set_precision(precision)
        r.model, r.device = head, next(head.parameters()).device
        r._bind_params(list(head.parameters()))
        r.layers, r.stem, r.last, r.fc, r.blocks = [], None, None, None, []
        r._bind_head(head)
        r._finish()
        return r

    def head_step(self, c1, c4, gout):
        """One teacher-forced train-mode forward + backward of the bound head: (out, dc1, dc4) as fp32 NCHW; p.grad is written."""
        call("frost_float_weight_prep", ptr(self._table), len(self.layers), stream())
        out = self._head_fwd(self.to_act(c1), self.to_act(c4), True, True).contiguous()
        self._grads_written = False              # a test entry: p.grad is overwritten, not accumulated
        self._begin_backward()
        dc1, dc4 = self._head_bwd(gout)
        self._end_backward()
        return out, dc1.float().contiguous(), dc4.float().contiguous()

    def head_eval(self, c1, c4):
        """Eval-mode forward of the bound head (running statistics) -> out as fp32 NCHW."""
        call("frost_float_weight_prep", ptr(self._table), len(self.layers), stream())
        call("frost_float_bn_eval", ptr(self._table), len(self.layers), stream())
        return self._head_fwd(self.to_act(c1), self.to_act(c4), False, False).contiguous()

    def _pooled_hw(self, h, w):
        from .seg_model import check_pool_fits
        (kh, kw), (sh, sw) = self.head.pool_kernel, self.head.pool_stride
        check_pool_fits(h, w, (kh, kw))
        return (h - kh) // sh + 1, (w - kw) // sw + 1

    def _check_input(self, x, training):
        """Before anything is launched: the c4 map holds the pool window, and (torch's BatchNorm2d rule) b1's BatchNorm sees more than one value per channel."""
        if x.dim() != 4 or not x.is_cuda:
            raise ValueError("expected an (N,3,H,W) tensor on the model's device")
        n, h, w = x.shape[0], x.shape[2], x.shape[3]
        for l in self.layers:               # forward order; only the stride-2 layers change the map size (every one pads (k - 1) / 2)
            if l.stride == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        ph, pw = self._pooled_hw(h, w)
        if training and n * ph * pw == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([{n}, {self.b1.cout}, {ph}, {pw}])")

    def forward(self, x):
        """Stride-8 logits [N, nclass, h/8, w/8], fp32, channels-last."""
        if self.model.training and torch.is_grad_enabled():
            return _FloatSegFunction.apply(self._params[0], x, self)
        return self._seg_impl(x, record=False)

    def _seg_impl(self, x, record):
        training = self.model.training
        self._check_input(x, training)
        _, outs = self._trunk(x, training, record)
        c1, c4 = (outs[self.stage_ends[i]] for i in SEG_TAPS)
        return self._head_fwd(c1, c4, training, record)

    def _head_fwd(self, c1, c4, training, record):
        head = self.head
        if training and not (self.b0.bn.training and self.b1.bn.training):
            raise NotImplementedError("BatchNorm in eval mode inside a training forward of the FLOAT model: the float HIP backward implements the batch-statistics gradient only")
        if c1.c != head.inter_channels or c4.c != head.in_channels or c1.n != c4.n:
            raise ValueError(f"LRASPPHead: expected c1 with {head.inter_channels} and c4 with {head.in_channels} channels, got {c1.c} and {c4.c}")
        ph, pw = self._pooled_hw(c4.h, c4.w)
        if training and c4.n * ph * pw == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([{c4.n}, {self.b1.cout}, {ph}, {pw}])")
        (kh, kw), (sh, sw) = head.pool_kernel, head.pool_stride
        nclass, cf = head.nclass, self.b0.cout
        with self._c4_scope():
            c4 = self._widen(c4)
            feat1 = self._conv(self.b0, c4, training, record)
            pooled = self._new(c4.n, ph, pw, c4.c)
            call(self._fn["sh_pool"], ptr(c4.buf), c4.n, c4.h, c4.w, c4.c, kh, kw, sh, sw, ptr(pooled.buf), stream())
            g = self._conv(self.b1, pooled, training, record)
            p = torch.empty(c4.npix * nclass, dtype=torch.float32, device=self.device)
            call(self._fn["sh_gate_project"], ptr(feat1.buf), ptr(g.buf), ptr(head.project.weight), ptr(head.project.bias), c4.n, c4.h, c4.w, ph, pw, cf, nclass,
                 ptr(p), stream())
        out = torch.empty(c1.n, c1.h, c1.w, nclass, dtype=torch.float32, device=self.device)
        call(self._fn["sh_logits"], ptr(p), ptr(c1.buf), ptr(head.auxlayer.weight), ptr(head.auxlayer.bias), c1.n, c1.h, c1.w, c4.h, c4.w, c1.c, nclass,
             ptr(out), stream())
        if record:
            self._seg = (c1, c4, feat1, g)
        return out.permute(0, 3, 1, 2)

    def _head_bwd(self, dout):
        """dout: gradient of the logits (NCHW-contiguous or channels-last, read through strides) -> (dc1, dc4) FActs, the tap gradients at x2 and x5; the
        gradients of project / auxlayer go into their arena views, b0's and b1's through _conv_bwd.  Call between _begin_backward and _end_backward."""
        c1, c4, feat1, g = self._seg
        self._seg = None
        head = self.head
        (kh, kw), (sh, sw) = head.pool_kernel, head.pool_stride
        nclass, cf = head.nclass, self.b0.cout
        d = dout if dout.dtype == torch.float32 else dout.float()
        if tuple(d.shape) != (c1.n, nclass, c1.h, c1.w):
            raise ValueError(f"the logits' gradient is {tuple(d.shape)}, expected {(c1.n, nclass, c1.h, c1.w)}")
        if not (d.is_contiguous() or d.is_contiguous(memory_format=torch.channels_last)):
            d = d.contiguous()
        sn, sc, s_h, s_w = d.stride()
        gv = self._gv
        dc1 = self._new(c1.n, c1.h, c1.w, c1.c)
        dp = torch.empty(c4.npix * nclass, dtype=torch.float32, device=self.device)
        call(self._fn["sh_logits_bwd"], ptr(d), sn, sc, s_h, s_w, ptr(c1.buf), ptr(head.auxlayer.weight), c1.n, c1.h, c1.w, c4.h, c4.w, c1.c, nclass,
             ptr(dc1.buf), ptr(gv[id(head.auxlayer.weight)]), ptr(gv[id(head.auxlayer.bias)]), ptr(dp), stream())
        with self._c4_scope():
            dfeat1 = self._new(c4.n, c4.h, c4.w, cf)
            dg = self._new(g.n, g.h, g.w, cf)
            scratch = torch.empty(c4.npix * cf, dtype=torch.float32, device=self.device)
            call(self._fn["sh_gate_project_bwd"], ptr(feat1.buf), ptr(g.buf), ptr(dp), ptr(head.project.weight), c4.n, c4.h, c4.w, g.h, g.w, cf, nclass,
                 ptr(gv[id(head.project.weight)]), ptr(gv[id(head.project.bias)]), ptr(dfeat1.buf), ptr(dg.buf), ptr(scratch), stream())
            d0 = self._conv_bwd(self.b0, ptr(dfeat1.buf), cf, True)
            dpool = self._conv_bwd(self.b1, ptr(dg.buf), cf, True)
            dc4 = self._new(c4.n, c4.h, c4.w, c4.c)
            call(self._fn["sh_pool_bwd"], ptr(dpool.buf), ptr(d0.buf), c4.n, c4.h, c4.w, c4.c, kh, kw, sh, sw, ptr(dc4.buf), stream())
        if dc4.buf.dtype != self._adt:          # the tap gradient at x5 in the storage type of the trunk
            wide, dc4 = dc4, self._new(c4.n, c4.h, c4.w, c4.c)
            self._store(dc4.buf[: c4.npix * c4.c], wide.buf[: c4.npix * c4.c])
        return dc1, dc4

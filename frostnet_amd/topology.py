"""The shape of a FrostNet / SSDLite module tree, stated ONCE for every runner that binds one (runner.py, float_train.py, infer.py, ptq.py).

Pure Python over nn.Module attributes -- no kernel library, no device needed: `plan_tree` reads which layers and FloatFunctional sites a tree has, `bind_trunk` /
`bind_block` / `bind_detector` hand them to a runner's callbacks in the canonical order.  That order is load-bearing: it is the descriptor-table index of
`runner.layers` / `E.layers`, the record index of the qrecord / calibration arena, and what pairs PtqConvertedRunner with PtqRunner.site_qparams() by name.
Beside the walk: the geometry of a float layer (`FloatLayer`), the flat gradient arena (`GradArena`), the validity signature and the small size arithmetic.
"""
from collections import namedtuple

import torch

STAGES = ("layer1", "layer2", "layer3", "layer4", "layer5")
FEATURE_TAPS = (0, 1, 2, 4)      # stage ends the features backbone returns: [x1, x2, x3, x5], x4 is skipped (frostnet_features.py:350)
SSD_TAPS = (1, 2, 4)             # stage ends that are SSD sources (strides 8 / 16 / 32)
SEG_TAPS = (1, 4)                # stage ends the segmentation head reads: x2 (stride 8, c1) and x5 (stride 32, c4)


def round_up(a, b):
    return (a + b - 1) // b * b


def conv_out_hw(h, w, k, stride):
    """Output size of a k x k convolution with padding (k - 1) / 2 (every spatial convolution of the network: the stem, conv2, the extras' and heads' depthwise)."""
    pad = (k - 1) // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def act_code(wrapper):
    """Activation code of the float kernels' `relu` argument (csrc/frost_float.hip: 0 none, 1 ReLU, 2 hard-swish) for a ConvBN / ConvBNReLU / ConvBNHswish."""
    return {"ConvBN": 0, "ConvBNHswish": 2}.get(type(wrapper).__name__, 1)


def model_signature(model):
    """Addresses of every parameter and buffer: a runner bound to the tree is valid while they stay where they were (`still_valid`)."""
    return tuple(p.data_ptr() for p in model.parameters()) + tuple(b.data_ptr() for b in model.buffers())


# ---------------------------------------------------------------------------------------------------------------------------------- the plan
# members a block does not use are None; the site members (quant_cat, skip_add) are None on a tree without FloatFunctionals, too
Block = namedtuple("Block", "prefix block squeeze_conv quant_cat conv1 conv2 reduce_conv skip_add")
# extras / heads: per extra stage three, per source four (name, wrapper, kind) entries; quant / last_layer / classifier are None where the tree has none
Plan = namedtuple("Plan", "quant stem blocks stage_ends last_layer classifier drop_rate extras heads")


def plan_block(prefix, blk):
    """CascadePreExBottleneck (frostnet.py:81-145): conv1 exists unless expand_ratio is 1; a 'CAS' block squeezes and cats in front of it; a block that keeps
    the map size and width adds its input."""
    expand = blk.expand_ratio != 1
    cas = expand and blk.block_type == "CAS"
    return Block(prefix, blk, blk.squeeze_conv if cas else None, getattr(blk, "quant_cat", None) if cas else None, blk.conv1 if expand else None,
                 blk.conv2, blk.reduce_conv, getattr(blk, "skip_add", None) if not blk.reduction else None)


def plan_tree(model):
    """Plan of a classifier, a features backbone or an SSDLite detector, in any state (float, fused, QAT- or PTQ-prepared): the wrapper modules, not their
    contents -- each runner unwraps what it needs (`.conv`, `.conv[0]`, `.act`)."""
    blocks, ends = [], []
    for stage in STAGES:
        blocks += [plan_block(f"{stage}.{i}", b) for i, b in enumerate(getattr(model, stage))]
        ends.append(len(blocks) - 1)
    cls = getattr(model, "classifier", None)
    extras = [tuple((f"extras.{i}.{n}", getattr(e, n), kind) for n, kind in (("pw1", "pw"), ("dw", "dw"), ("pw2", "pw")))
              for i, e in enumerate(getattr(model, "extras", ()))]
    heads = [tuple((f"{h}.{i}.{n}", getattr(m, n), n) for h, m in (("loc", l), ("conf", c)) for n in ("dw", "pw"))
             for i, (l, c) in enumerate(zip(getattr(model, "loc", ()), getattr(model, "conf", ())))]
    return Plan(getattr(model, "quant", None), model.conv1, blocks, ends, getattr(model, "last_layer", None), cls[2] if cls is not None else None,
                float(cls[1].p) if cls is not None else 0.0, extras, heads)


# ---------------------------------------------------------------------------------------------------------------------------------- the binding order
def bind_block(rec, layer, site=None, key="blk"):
    """A runner's block dict from a Block: `layer(name, wrapper, kind)` per convolution and, for a runner with activation sites, `site(name, functional)` --
    ALWAYS squeeze, cat site, conv1, conv2, reduce, add site."""
    d = {key: rec.block, "squeeze": None, "conv1": None}
    if site is not None:
        d["q_cat"] = d["q_add"] = None
    if rec.squeeze_conv is not None:
        d["squeeze"] = layer(rec.prefix + ".squeeze_conv", rec.squeeze_conv, "pw")
        if site is not None and rec.quant_cat is not None:
            d["q_cat"] = site(rec.prefix + ".quant_cat", rec.quant_cat)
    if rec.conv1 is not None:
        d["conv1"] = layer(rec.prefix + ".conv1", rec.conv1, "pw")
    d["conv2"] = layer(rec.prefix + ".conv2", rec.conv2, "dw")
    d["reduce"] = layer(rec.prefix + ".reduce_conv", rec.reduce_conv, "pw")
    if site is not None and rec.skip_add is not None:
        d["q_add"] = site(rec.prefix + ".skip_add", rec.skip_add)
    return d


def bind_trunk(plan, layer, site=None, key="blk"):
    """(stem, [block dict], last_layer or None): the stem, every bottleneck, then the classifier's 1x1 expansion where the tree has one."""
    stem = layer("conv1", plan.stem, "stem")
    blocks = [bind_block(b, layer, site, key) for b in plan.blocks]
    return stem, blocks, layer("last_layer", plan.last_layer, "pw") if plan.last_layer is not None else None


def bind_detector(plan, layer):
    """(extras [(pw1, dw, pw2)], heads [(loc dw, loc pw, conf dw, conf pw)]) of a detector: every extra stage, then the heads source by source; two empty lists otherwise."""
    return [tuple(layer(*e) for e in stage) for stage in plan.extras], [tuple(layer(*e) for e in src) for src in plan.heads]


# ---------------------------------------------------------------------------------------------------------------------------------- float layer geometry
class FloatLayer:
    """Geometry of one convolution on the float kernels (training, bf16 inference, PTQ calibration) and its packed weights: kind 0 pointwise, 1 depthwise,
    2 stem (im2col, K = 64); `kq` = elements per 64-byte K step of the MFMA A-fragment pack (32 bf16, 16 fp32); `pack_dtype` with 1024 bytes per fragment."""
    __slots__ = ("conv", "cout", "cin_g", "k", "stride", "kind", "cpad", "kpad", "pack")

    def __init__(self, conv, dev, stem, kq, pack_dtype=torch.uint8):
        self.conv = conv
        self.cout, self.cin_g, self.k, self.stride = conv.out_channels, conv.in_channels // conv.groups, conv.kernel_size[0], conv.stride[0]
        self.kind = 2 if stem else (1 if conv.groups > 1 else 0)
        self.cpad = round_up(self.cout, 16)
        if self.kind == 1:
            self.kpad = 0
            self.pack = torch.zeros(self.k * self.k * self.cpad, dtype=torch.float32, device=dev)
        else:
            self.kpad = 64 if stem else round_up(self.cin_g, kq)
            self.pack = torch.zeros(self.pack_bytes(self.cpad, self.kpad, kq) // pack_dtype.itemsize, dtype=pack_dtype, device=dev)

    @staticmethod
    def pack_bytes(rows, kpad, kq):
        return (round_up(rows, 16) // 16) * (kpad // kq) * 1024


# ---------------------------------------------------------------------------------------------------------------------------------- gradient arena
class GradArena:
    """Mixin of the training runners: parameter gradients in ONE flat fp32 arena (views assigned to `p.grad`), parameter order = the given list
    (model.parameters(): the reference's registration order) -- what the multi-tensor optimizer and the data-parallel all-reduce operate on."""

    def _bind_params(self, params):
        self._params = params
        self.grad_arena = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=self.device)
        self._grad_views, self._grad_offsets, self._gv, off = [], [], {}, 0
        for p in params:
            v = self.grad_arena[off: off + p.numel()].view_as(p)
            self._grad_views.append(v)
            self._grad_offsets.append(off)
            self._gv[id(p)] = v
            off += p.numel()

    def bind_grads(self):
        for p, v in zip(self._params, self._grad_views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    def _attach_grad_sync(self, nbuckets, group):
        """The bucketed gradient all-reduce over the arena (frostnet_amd.parallel.GradSync)."""
        from .parallel import GradSync
        self.grad_sync = GradSync(self.grad_arena, self._grad_offsets, nbuckets, group)
        return self.grad_sync

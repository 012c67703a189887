"""bf16 inference of the FLOAT (not fake-quantised) FrostNet on the HIP kernels -- BASELINE.json config c2.

Reference semantics: `model.eval(); model(x)` of a float `frostnet_*` model (`frostnet.py:14-60, 108-121, 271-300`): Conv ->
BatchNorm(running stats) -> ReLU per layer, block wiring squeeze -> cat -> conv1 -> conv2 -> reduce_conv -> (+x), global average
pool -> (dropout is identity in eval) -> 1x1 classifier.  Here BatchNorm is folded into the convolution once per call
(`frost_infer_weight_prep`), activations are NHWC bf16, accumulation is fp32.  Deviation from the reference: bf16 storage of
weights and activations (the c2 configuration asks for bf16); the parity test holds the logits to the fp32 oracle within bf16
tolerance.  No CPU / torch-eager fallback: a missing library raises.

The same kernels serve the feature backbone (`Bf16Inference.features`: the trunk's stage ends) and the float SSDLite detector (`Bf16SSDInference`: trunk taps,
the extras on the layer kernels, both prediction heads of a source in one launch of csrc/frost_ihead.hip that stores fp32 loc / conf in their final layout).
"""
import ctypes as C
import os

import torch

from . import _lib as L
from ._lib import call, ptr, stream
from .topology import FEATURE_TAPS, SSD_TAPS, FloatLayer, act_code, bind_detector, bind_trunk, conv_out_hw, plan_tree


# Whole-bottleneck fused kernel (csrc/frost_iblock.hip): "1" = every bottleneck the kernel takes (tile from pick_tile), "0" = layer-by-layer launches, "auto"
# (default) = MEASURED per bottleneck: the first forward outside a hipGraph capture times the layer-by-layer launches and the fused launch with each candidate
# tile (3 runs each) and keeps the fastest for that (map size, batch) -- results are bit-identical whichever is chosen (tests/test_gpu_infer.py).
_FUSED = {"0": False, "1": True}.get(os.environ.get("FROST_INFER_FUSED", "auto"), "auto")
# the stem straight from the fp32 image (frost_infer_stem) instead of im2col + GEMM: bit-identical, no 128-byte-per-pixel patch buffer
_STEM_DIRECT = os.environ.get("FROST_INFER_STEM", "direct") != "im2col"
# the wave-per-tile block kernel (csrc/frost_iblockw.hip) as a further candidate of the measured choice for the bottlenecks without a squeeze conv ("0": not offered)
_WAVE = os.environ.get("FROST_INFER_WAVE", "1") != "0"
TILE_CANDIDATES = ((0, 0), (-1, 0), (7, 14), (8, 16), (16, 16), (7, 7), (8, 8), (4, 16), (4, 8))          # (0, 0) = the whole map, (-1, 0) = half of it


def candidate_tiles(lib, h, w, cin, r, cexp, cout, k, stride):
    ho, wo = conv_out_hw(h, w, k, stride)
    out = []
    for th, tw in TILE_CANDIDATES:
        th, tw = (ho, wo) if th == 0 else (((ho + 1) // 2, wo) if th < 0 else (min(th, ho), min(tw, wo)))
        if (th, tw) not in out and th * tw <= 256 and lib.frost_infer_block_ok(h, w, cin, r, cexp, cout, k, stride, th, tw) > 0:
            out.append((th, tw))
    return out


def pick_tile(lib, h, w, cin, r, cexp, cout, k, stride):
    """Spatial output tile (th, tw) of one workgroup of frost_infer_block by a cost model (FROST_INFER_FUSED=1; the default mode "auto" measures the candidates
    instead, Bf16Inference._block): region pixels conv1 computes per output pixel plus a fixed per-tile cost, mildly weighted by the residency the tile's LDS
    footprint allows.  None: the fused kernel does not take this geometry."""
    ho, wo = conv_out_hw(h, w, k, stride)
    cands = [(ho, wo), ((ho + 1) // 2, wo), (7, 14), (8, 16), (7, 7), (8, 8), (4, 8), (4, 4)]
    if os.environ.get("FROST_IB_TILE"):
        cands = [tuple(int(v) for v in os.environ["FROST_IB_TILE"].split(","))] + cands[-1:]
    best = None
    for th, tw in cands:
        th, tw = min(th, ho), min(tw, wo)
        lds = lib.frost_infer_block_ok(h, w, cin, r, cexp, cout, k, stride, th, tw) if th * tw <= 256 else 0
        if lds <= 0:
            continue
        waste = (-(-ho // th) * th) * (-(-wo // tw) * tw) / float(ho * wo)            # ragged edge tiles
        rp = ((th - 1) * stride + k) * ((tw - 1) * stride + k)                            # region pixels conv1 computes for th * tw outputs (halo included)
        wgs = min(3, (160 * 1024) // lds)                                                 # resident workgroups per CU by LDS
        # cost per output pixel: region pixels plus a fixed per-tile cost (prologue, barriers: ~150 pixel-equivalents), mildly weighted by residency --
        # fitted to tools/prof_iblock.py (104 -> 624 -> 96 @14x14, k5: 7x14 157 us, 7x7 198, 4x8 235, 4x4 475; 16 -> 96 -> 24 @112, k3 s2: 8x8 best)
        score = waste * (rp + 150.0) / (th * tw) * (1.0 + 0.1 * (3 - wgs))
        if best is None or score < best[0] - 1e-9:
            best = (score, th, tw)
    return None if best is None else (best[1], best[2])


class _ILayer(FloatLayer):
    __slots__ = ("relu", "biasf", "bn")

    def __init__(self, seq, relu, dev, stem=False):
        conv, bn = seq[0], seq[1]
        if not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d):
            raise RuntimeError("bf16 inference expects the un-fused float model (Conv2d + BatchNorm2d per layer)")
        super().__init__(conv, dev, stem, 32, torch.int16)
        self.bn, self.relu = bn, relu
        self.biasf = torch.zeros(self.cpad, dtype=torch.float32, device=dev)

    def desc(self):
        bn, w = self.bn, self.conv.weight
        return L.FrostIDesc(w.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                            bn.running_var.data_ptr(), self.pack.data_ptr(), self.biasf.data_ptr(), self.cout, self.cin_g,
                            self.k * self.k, self.kind, self.cpad, self.kpad, 0, 0)


class Bf16Inference:
    """Binds a float FrostNet (eval mode) to the bf16 HIP inference kernels.  `__call__(x)` -> fp32 logits [N, nclass] (a model with `last_layer` / `classifier`);
    `features(x)` -> the stage ends [x1, x2, x3, x5] as fp32 NCHW (any FrostNet trunk)."""

    def __init__(self, model):
        L.load_library()
        # act='hswish' networks (frostnet.py ConvBNHswish): the layer kernels take the activation as a code (0 none, 1 ReLU, 2 hard-swish); the fused
        # bottleneck kernels (frost_infer_block / _block_w) are written for ReLU, so such a network runs layer by layer
        self.hswish = getattr(model, "act", "relu") == "hswish"
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("Bf16Inference needs the model on the GPU (no CPU fallback on the product path)")
        self.model, self.device = model, p.device
        self.layers = []
        # the classifier's tail where the tree has one (the feature backbone and the detector have none); a detector's extras and heads behind the trunk in the
        # same descriptor table (one prep launch for all of them)
        plan = plan_tree(model)
        self.stem, self.blocks, self.last = bind_trunk(plan, self._add)
        self.stage_ends, self.fc = plan.stage_ends, plan.classifier
        self.extras, self.heads = bind_detector(plan, self._add)
        self._table, self._ptrs, self._versions = None, None, None

    def _prepare_weights(self):
        """BatchNorm folding + fragment packing (frost_infer_weight_prep) once per state of the parameters, as the reference folds once before it evaluates
        (Classification/evaluate.py:131-143): the descriptor table follows re-assigned tensors (data pointers), the packs follow in-place updates (tensor
        version counters).  `refresh()` forces it (for writes the counters do not see, e.g. through a raw pointer)."""
        ts = [t for l in self.layers for t in (l.conv.weight, l.bn.weight, l.bn.bias, l.bn.running_mean, l.bn.running_var)]
        # + the generation of raw-pointer writers (the HIP optimizer step and the training forwards update parameters / running statistics behind torch's back);
        # once such a writer sits in a captured hipGraph its replays are invisible here: prepare on every call then
        ptrs, versions = [t.data_ptr() for t in ts], [t._version for t in ts] + [L.RAW_WRITE_GEN]
        if L.RAW_WRITES_CAPTURED:
            versions = None
        if ptrs != self._ptrs:
            arr = (L.FrostIDesc * len(self.layers))()
            for i, l in enumerate(self.layers):
                arr[i] = l.desc()
            self._table, self._ptrs, self._versions = L.struct_to_tensor(arr, self.device), ptrs, None
        if versions is None or versions != self._versions:
            call("frost_infer_weight_prep", ptr(self._table), len(self.layers), stream())
            self._versions = versions

    def refresh(self):
        self._versions = None

    def _add(self, name, wrapper, kind):
        l = _ILayer(wrapper.conv, act_code(wrapper), self.device, kind == "stem")
        self.layers.append(l)
        return l

    # ---------------------------------------------------------------------------------------------- kernels
    def _pw(self, l, x, npix, cin):
        y = torch.empty(npix * l.cout + 64, dtype=torch.int16, device=self.device)
        call("frost_infer_pw", ptr(x), ptr(l.pack), ptr(l.biasf), npix, cin, l.cout, int(l.relu), ptr(y), stream())
        return y

    def _dw(self, l, x, n, h, w):
        ho, wo = conv_out_hw(h, w, l.k, l.stride)
        y = torch.empty(n * ho * wo * l.cout + 64, dtype=torch.int16, device=self.device)
        call("frost_infer_dw", ptr(x), ptr(l.pack), ptr(l.biasf), n, h, w, l.cout, l.k, l.stride, int(l.relu), ptr(y), stream())
        return y, ho, wo

    def _block_plain(self, ent, a, c, n, h, w):
        """One bottleneck as layer-by-layer launches: [squeeze -> cat] -> conv1 -> conv2 -> reduce_conv [-> + x]."""
        x_in, npix = a, n * h * w
        if ent["conv1"] is not None:
            if ent["squeeze"] is not None:
                s = self._pw(ent["squeeze"], a, npix, c)
                cs = ent["squeeze"].cout
                cat = torch.empty(npix * (cs + c) + 64, dtype=torch.int16, device=self.device)
                call("frost_infer_cat", ptr(s), cs, ptr(a), c, npix, ptr(cat), stream())     # cat([squeezed, x], 1)
                a, c = cat, cs + c
            a, c = self._pw(ent["conv1"], a, npix, c), ent["conv1"].cout
        a, h2, w2 = self._dw(ent["conv2"], a, n, h, w)
        npix2 = n * h2 * w2
        a, c = self._pw(ent["reduce"], a, npix2, c), ent["reduce"].cout
        if not ent["blk"].reduction:
            out = torch.empty_like(a)
            call("frost_infer_add", ptr(x_in), ptr(a), npix2 * c, ptr(out), stream())
            a = out
        return a, c, h2, w2

    def _block_fused(self, ent, a, c, n, h, w, tile):
        """The same bottleneck as ONE launch of frost_infer_block with the spatial output tile `tile`."""
        l2, l3, sq, l1 = ent["conv2"], ent["reduce"], ent["squeeze"], ent["conv1"]
        r = sq.cout if sq is not None else 0
        h2, w2 = conv_out_hw(h, w, l2.k, l2.stride)
        out = torch.empty(n * h2 * w2 * l3.cout + 64, dtype=torch.int16, device=self.device)
        call("frost_infer_block", ptr(a), ptr(sq.pack) if sq is not None else None, ptr(sq.biasf) if sq is not None else None,
             ptr(l1.pack) if l1 is not None else None, ptr(l1.biasf) if l1 is not None else None, ptr(l2.pack), ptr(l2.biasf),
             ptr(l3.pack), ptr(l3.biasf), n, h, w, c, r, l2.cout, l3.cout, l2.k, l2.stride, 0 if ent["blk"].reduction else 1, tile[0], tile[1],
             tile[2] if len(tile) > 2 else 0, tile[3] if len(tile) > 3 else 0, ptr(out), stream())
        return out, l3.cout, h2, w2

    def _block_wave(self, ent, a, c, n, h, w, tile):
        """A bottleneck without a squeeze conv as ONE launch of frost_infer_block_w: one wave per (th, tw) output tile, no workgroup barriers."""
        l2, l3, l1 = ent["conv2"], ent["reduce"], ent["conv1"]
        h2, w2 = conv_out_hw(h, w, l2.k, l2.stride)
        out = torch.empty(n * h2 * w2 * l3.cout + 64, dtype=torch.int16, device=self.device)
        call("frost_infer_block_w", ptr(a), ptr(l1.pack) if l1 is not None else None, ptr(l1.biasf) if l1 is not None else None, ptr(l2.pack), ptr(l2.biasf),
             ptr(l3.pack), ptr(l3.biasf), n, h, w, c, l2.cout, l3.cout, l2.k, l2.stride, 0 if ent["blk"].reduction else 1, tile[1], tile[2], ptr(out), stream())
        return out, l3.cout, h2, w2

    def _run_choice(self, ent, a, c, n, h, w, choice):
        if choice == "plain":
            return self._block_plain(ent, a, c, n, h, w)
        if choice[0] == "w":
            return self._block_wave(ent, a, c, n, h, w, choice)
        return self._block_fused(ent, a, c, n, h, w, choice)

    def _block(self, ent, a, c, n, h, w):
        if _FUSED is False or self.hswish:
            return self._block_plain(ent, a, c, n, h, w)
        # the measured choice is kept per (resolution, batch BUCKET): a last partial batch or a slightly different batch size reuses its bucket's choice instead of
        # re-running dozens of timed launches inside the caller's forward, and the table stays bounded
        bucket = 1 << max(0, int(n) - 1).bit_length()
        key = ("choice", bucket, h, w, _FUSED)
        choice = ent.get(key)
        if choice is not None:
            ent[key] = ent.pop(key)                   # re-inserted on a hit: the eviction below drops the LEAST RECENTLY USED entry, not the oldest insertion
        if choice is None:
            l2, l3, sq = ent["conv2"], ent["reduce"], ent["squeeze"]
            r = sq.cout if sq is not None else 0
            lib = L.load_library()
            if _FUSED is True:
                choice = pick_tile(lib, h, w, c, r, l2.cout, l3.cout, l2.k, l2.stride) or "plain"
            elif torch.cuda.is_current_stream_capturing():
                return self._block_plain(ent, a, c, n, h, w)          # nothing can be timed inside a capture: run one eager forward first (bench.py does)
            else:
                timed = []
                tiles = candidate_tiles(lib, h, w, c, r, l2.cout, l3.cout, l2.k, l2.stride)
                narrow = -(-(r + c) // 32) <= 2                       # conv1 K <= 64 (the high-resolution blocks): 32-channel chunks are an option
                # every tile with 4 and with 8 waves per workgroup (and, for the narrow blocks, with 64- and 32-channel chunks of the expanded width)
                # bottlenecks without a squeeze conv on small Cin (the high-resolution blocks): the wave-per-tile kernel with its two tiles
                wave = [("w", 4, tw) for tw in (4, 8) if _WAVE and sq is None and
                        lib.frost_infer_block_w_ok(c, 0, l2.cout, l3.cout, l2.k, l2.stride, 1 if ent["conv1"] is not None else 0, 4, tw)]
                # (16 waves: only for whole small maps -- one workgroup per image, so with few images per CU only more waves shorten the serial phases)
                wide16 = [(th, tw, 16, 64) for th, tw in tiles if th * tw <= 64]
                for cand in ["plain"] + [(th, tw, nw, ch) for th, tw in tiles for nw in (4, 8) for ch in ((64, 32) if narrow else (64,))] + wide16 + wave:
                    run = (lambda t=cand: self._run_choice(ent, a, c, n, h, w, t))
                    try:
                        run()
                    except RuntimeError as e:         # only the library's own "this tile / wave count does not fit" refusals mean "not a candidate"
                        if not any(m in str(e) for m in ("too many output tiles per wave", "unsupported geometry / tile", "chunk = 64, or 32", "16 waves take 64-channel chunks only")):
                            raise                     # a genuine launch failure must not be read as "candidate not applicable"
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(3):
                        run()
                    e1.record()
                    e1.synchronize()
                    timed.append((e0.elapsed_time(e1) / 3.0, cand))
                choice = min(timed, key=lambda t: t[0])[1]
                ent[("timing", bucket, h, w)] = timed
            stale = [k for k in ent if isinstance(k, tuple) and k[0] == "choice"]
            for k in stale[:-7]:                      # at most 8 (bucket, resolution) entries per bottleneck
                ent.pop(k, None); ent.pop(("timing",) + k[1:4], None)
            ent[key] = choice
        return self._run_choice(ent, a, c, n, h, w, choice)

    def _check_input(self, x):
        if self.model.training:
            raise RuntimeError("bf16 inference is the eval-mode graph: call model.eval() first")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("expected an fp32 (N,3,H,W) tensor on the model's device")

    def _trunk(self, x):
        """Stem + the five stages -> [(activation NHWC bf16, channels, h, w)] at the end of every stage (the last entry is the trunk's output)."""
        n, _, h, w = x.shape
        self._prepare_weights()
        ho, wo = conv_out_hw(h, w, 3, 2)
        npix = n * ho * wo
        if _STEM_DIRECT and L.load_library().frost_infer_stem_ok(self.stem.cout):
            a = torch.empty(npix * self.stem.cout, dtype=torch.int16, device=self.device)
            call("frost_infer_stem", ptr(x), n, h, w, x.stride(0), x.stride(1), x.stride(2), x.stride(3), ptr(self.stem.pack), ptr(self.stem.biasf),
                 self.stem.cout, int(self.stem.relu), ptr(a), stream())
        else:
            col = torch.empty(npix * 64 + 64, dtype=torch.int16, device=self.device)
            call("frost_infer_stem_im2col", ptr(x), n, h, w, x.stride(0), x.stride(1), x.stride(2), x.stride(3), ptr(col), stream())
            a = self._pw(self.stem, col, npix, 64)
        c, h, w = self.stem.cout, ho, wo
        outs, ends = [], set(self.stage_ends)
        for i, ent in enumerate(self.blocks):
            a, c, h, w = self._block(ent, a, c, n, h, w)
            if i in ends:
                outs.append((a, c, h, w))
        return outs

    @staticmethod
    def _nchw_f32(a, n, c, h, w):
        """NHWC bf16 activation buffer -> fp32 NCHW tensor (an output conversion, not conv math)."""
        return a[:n * h * w * c].view(torch.bfloat16).view(n, h, w, c).permute(0, 3, 1, 2).float().contiguous()

    @torch.no_grad()
    def features(self, x):
        """[x1, x2, x3, x5] of the feature backbone (frostnet_features.py:342-352: strides 4 / 8 / 16 / 32, x4 skipped) as fp32 NCHW."""
        self._check_input(x)
        outs = self._trunk(x)
        return [self._nchw_f32(outs[i][0], x.shape[0], *outs[i][1:]) for i in FEATURE_TAPS]

    @torch.no_grad()
    def __call__(self, x):
        self._check_input(x)
        if self.last is None or self.fc is None:
            raise RuntimeError("this model has no classifier: Bf16Inference.features(x) / Bf16SSDInference serve the backbone and the detector")
        n = x.shape[0]
        a, c, h, w = self._trunk(x)[-1]
        npix = n * h * w
        a, c = self._pw(self.last, a, npix, c), self.last.cout
        pooled = torch.empty(n, c, dtype=torch.float32, device=self.device)
        call("frost_infer_avgpool", ptr(a), n, h * w, c, ptr(pooled), stream())
        logits = torch.empty(n, self.fc.out_channels, dtype=torch.float32, device=self.device)
        wfc = self.fc.weight.view(self.fc.out_channels, -1)
        call("frost_linear_f32", ptr(pooled), ptr(wfc), ptr(self.fc.bias), n, c, self.fc.out_channels, ptr(logits), stream())
        return logits


# the fused prediction-head kernel (csrc/frost_ihead.hip); "0": every head as frost_infer_dw + frost_infer_pw and an fp32 placement (bf16(loc / conf) bit-identical)
_HEAD_FUSED = os.environ.get("FROST_INFER_HEAD", "1") != "0"


def ssd_head_offsets(anchors, map_sizes):
    """Prior offset of every SSD source in SSDLiteFrostNet._assemble's order: source k (map h_k x w_k, A_k anchors per pixel) owns the priors
    [poff_k, poff_k + h_k * w_k * A_k), and element j of pixel `pix` of its loc map ([.., 4 A_k] per pixel) / conf map ([.., C A_k]) sits at
    poff_k * 4 + pix * 4 A_k + j of an image's flattened loc row / poff_k * C + pix * C A_k + j of its conf row.  map_sizes: (h, w) pairs or edge lengths."""
    offs, p = [], 0
    for a, m in zip(anchors, map_sizes):
        h, w = (m, m) if isinstance(m, int) else m
        offs.append(p)
        p += int(h) * int(w) * int(a)
    return offs


def cvt_place_torch(idx, scale, zero_point, width, out, off):
    """The definition of frost_cvt_place (and of the store of frost_cvt_head) as torch stages on any device: idx [n, hw, cout] int8 offset-binary indices (index - 128)
    of one head map under (scale, zero_point); the first `width` channels of every pixel, dequantised as (float)(index - zero_point) * scale in fp32, go to
    out[:, off : off + hw * width] of the image rows out [n, stride]; nothing else of `out` is written."""
    n, hw, _ = idx.shape
    v = (idx.to(torch.int32) + 128 - int(zero_point)).to(torch.float32) * torch.tensor(float(scale), dtype=torch.float32, device=idx.device)
    out[:, off:off + hw * width] = v[:, :, :width].reshape(n, -1)
    return out


class Bf16SSDInference(Bf16Inference):
    """Binds a float SSDLiteFrostNet (eval mode) to the bf16 HIP inference kernels.  `__call__(x)` -> (loc [N,P,4], conf [N,P,C]) fp32 in _assemble's order:
    the trunk on the fused bottleneck kernels with taps at the ends of stages 1, 2 and 4 (0-based), every extra stage as frost_infer_pw -> frost_infer_dw
    (stride 2) -> frost_infer_pw, and ONE frost_infer_head launch per source that computes both heads and stores straight into loc / conf."""

    def __init__(self, model):
        if getattr(model, "act", "relu") == "hswish":
            raise RuntimeError("the detector's bf16 inference path is written for ReLU networks")
        super().__init__(model)
        self.anchors, self.num_classes, self._offsets = list(model.ANCHORS), int(model.num_classes), {}

    def head_offsets(self, sizes):
        """(prior offsets, P) of the source maps `sizes`, built once per input size (host integers: the launches take them as arguments)."""
        key = tuple(sizes)
        hit = self._offsets.get(key)
        if hit is None:
            offs = ssd_head_offsets(self.anchors, sizes)
            hit = (offs, offs[-1] + sizes[-1][0] * sizes[-1][1] * self.anchors[-1])
            if len(self._offsets) >= 8:
                self._offsets.pop(next(iter(self._offsets)))
            self._offsets[key] = hit
        return hit

    def _head(self, src, layers, k, n, loc, conf, poff, p):
        a, c, h, w = src
        ldw, lpw, cdw, cpw = layers
        A, C = self.anchors[k], self.num_classes
        if _HEAD_FUSED and L.load_library().frost_infer_head_ok(h, w, c, 4 * A, C * A):
            call("frost_infer_head", ptr(a), ptr(ldw.pack), ptr(ldw.biasf), ptr(lpw.pack), ptr(lpw.biasf), ptr(cdw.pack), ptr(cdw.biasf), ptr(cpw.pack),
                 ptr(cpw.biasf), n, h, w, c, 4 * A, C * A, ptr(loc), p * 4, poff * 4, ptr(conf), p * C, poff * C, stream())
            return
        # layer launches + an fp32 placement of the used channels (geometries the fused kernel does not take; FROST_INFER_HEAD=0)
        for dw, pw, out, width in ((ldw, lpw, loc, 4), (cdw, cpw, conf, C)):
            t, _, _ = self._dw(dw, a, n, h, w)
            y = self._pw(pw, t, n * h * w, c)
            y = y[:n * h * w * pw.cout].view(torch.bfloat16).view(n, h * w, pw.cout)[:, :, :A * width]
            out.view(n, -1)[:, poff * width:(poff + h * w * A) * width] = y.reshape(n, -1).float()

    def _sources(self, x):
        """The six source maps [(activation, channels, h, w)]: stage ends 1, 2 and 4 (0-based) of the trunk, then the output of every extra stage."""
        n = x.shape[0]
        outs = self._trunk(x)
        sources = [outs[i] for i in SSD_TAPS]
        a, c, h, w = outs[4]
        for pw1, dw, pw2 in self.extras:
            t = self._pw(pw1, a, n * h * w, c)
            t, h, w = self._dw(dw, t, n, h, w)
            a, c = self._pw(pw2, t, n * h * w, pw1.cout), pw2.cout
            sources.append((a, c, h, w))
        return sources

    def _heads(self, sources, n):
        offs, p = self.head_offsets([(s[2], s[3]) for s in sources])
        loc = torch.empty(n, p, 4, dtype=torch.float32, device=self.device)
        conf = torch.empty(n, p, self.num_classes, dtype=torch.float32, device=self.device)
        for k, (src, layers) in enumerate(zip(sources, self.heads)):
            self._head(src, layers, k, n, loc, conf, offs[k], p)
        return loc, conf

    @torch.no_grad()
    def __call__(self, x):
        self._check_input(x)
        return self._heads(self._sources(x), x.shape[0])

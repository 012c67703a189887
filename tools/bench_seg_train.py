"""Time the float segmentation training iteration on one GPU at the VOC shape (FrostNetSeg Large, B = 32, 513 x 513), in bf16 and fp32 storage:

    SegmentationAugmentation -> FrostNetSeg -> SegmentationLoss with its SegMeter -> backward -> optimizer step (QSGD)

    python tools/bench_seg_train.py [--out profiles/seg_train.txt] [--iters 5] [--rounds 5] [--batch 32] [--mode large]

Reported per precision: the whole iteration; its parts from device events between them (input pipeline, forward, criterion, backward, optimizer) with their share of
the iteration; the head's forward and backward alone (events around FloatSegRunner._head_fwd / _head_bwd inside the same iterations); and the same head as stock torch
modules in the reference's order -- b0, b1, both F.interpolate, the product, project on the 128-channel map at c1's resolution, auxlayer, the add, and autograd's
backward -- on the same c1 / c4 tensors on the same device, with the peak memory of one call of either.  Times are device-event times; the figure per variant is the
median over `rounds` rounds, the two precisions and the torch head interleaved, with the spread beside it.  Nothing is compared against a fixed ratio."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

PARTS = ("input pipeline", "forward", "criterion", "backward", "optimizer")


def batch(n, size, seed):
    from frostnet_amd import seg_augment
    rng = np.random.default_rng(seed)
    pics, labs = [], []
    for i in range(n):
        h, w = int(rng.integers(size * 3 // 4, size + 1)), int(rng.integers(size * 3 // 4, size + 1))
        pics.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        coarse = rng.integers(0, 21, (h // 32 + 1, w // 32 + 1))
        lab = np.kron(coarse, np.ones((32, 32), dtype=np.int64))[:h, :w]
        labs.append(np.where(rng.random((h, w)) < 0.03, 255, lab).astype(np.uint8))
    return [t.cuda() for t in seg_augment.pad_pairs(pics, labs)]


class Events:
    def __init__(self):
        self.marks = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def spans(self):
        torch.cuda.synchronize()
        return [(b[0], a[1].elapsed_time(b[1])) for a, b in zip(self.marks, self.marks[1:])]


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})"


class Variant:
    """One precision: model, optimizer, criterion, transform; `iteration` returns {part: ms} with the head's two spans beside the five parts."""

    def __init__(self, base, prec, size):
        from frostnet_amd import harness, seg, seg_augment
        from frostnet_amd.optimizer import QSGD
        self.model = copy.deepcopy(base)
        self.model.float_precision = prec
        self.model.cuda().train()
        self.opt = QSGD(harness.make_param_groups(self.model, 1e-5), lr=1e-4, momentum=0.9)
        self.meter = seg.SegMeter(21, "cuda")
        self.crit = seg.SegmentationLoss(n_classes=21, device="cuda", meter=self.meter)
        self.aug = seg_augment.SegmentationAugmentation(crop_size=(size, size), seed=3, channels_last=True)
        self.head_ms, self.taps = {}, None
        run = self.model.hip_runner()
        fwd, bwd = run._head_fwd, run._head_bwd

        def head_fwd(c1, c4, training, record):
            self.taps = (c1, c4)
            ev = Events(); ev.mark("")
            out = fwd(c1, c4, training, record)
            ev.mark("head forward"); self._head_ev.append(ev)
            return out

        def head_bwd(dout):
            ev = Events(); ev.mark("")
            out = bwd(dout)
            ev.mark("head backward"); self._head_ev.append(ev)
            return out
        run._head_fwd, run._head_bwd = head_fwd, head_bwd

    def iteration(self, images, labels, sizes):
        self._head_ev = []
        ev = Events()
        ev.mark("")
        x, t = self.aug(images, labels, sizes)
        ev.mark("input pipeline")
        out = self.model(x)
        ev.mark("forward")
        loss = self.crit(out, t)
        ev.mark("criterion")
        self.opt.zero_grad()
        loss.backward()
        ev.mark("backward")
        self.opt.step()
        ev.mark("optimizer")
        res = dict(ev.spans())
        for h in self._head_ev:
            res.update(dict(h.spans()))
        # the criterion's backward (one multiply) is inside "backward"; the head's spans are inside "forward" / "backward"
        res["iteration"] = sum(res[p] for p in PARTS)
        return res


def torch_head_step(head, c1, c4, gout):
    c1, c4 = c1.detach().requires_grad_(True), c4.detach().requires_grad_(True)
    for p in head.parameters():
        p.grad = None
    ev = Events(); ev.mark("")
    out = head(c1, c4)
    ev.mark("forward")
    out.backward(gout)
    ev.mark("backward")
    return dict(ev.spans())


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--mode", default="large")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_train: needs the GPU (no CPU timing is reported)")
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import seg_model
    torch.manual_seed(1)
    base = seg_model.FrostNetSeg(21, args.mode)
    images, labels, sizes = batch(args.batch, args.size, 7)
    variants = {p: Variant(base, p, args.size) for p in ("bf16", "fp32")}
    lines = [f"# tools/bench_seg_train.py --iters {args.iters} --rounds {args.rounds} --batch {args.batch} --size {args.size} --mode {args.mode}   "
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}",
             "# device-event times per iteration; median over interleaved rounds (min, max)"]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for v in variants.values():                     # warm-up: descriptor tables, optimizer state, allocator
        for _ in range(2):
            v.iteration(images, labels, sizes)
    # the stock-module head on the device, fed with the fp32 variant's taps
    c1a, c4a = variants["fp32"].taps
    c1, c4 = c1a.float().contiguous(), c4a.float().contiguous()
    thead = copy.deepcopy(variants["fp32"].model.head).cuda().train()
    gout = torch.randn(args.batch, 21, c1.shape[2], c1.shape[3], device="cuda")
    for _ in range(2):
        torch_head_step(thead, c1, c4, gout)
    times = {p: {k: [] for k in PARTS + ("iteration", "head forward", "head backward")} for p in variants}
    ttimes = {"forward": [], "backward": []}
    for _ in range(args.rounds):
        for p, v in variants.items():
            acc = {}
            for _ in range(args.iters):
                for k, ms in v.iteration(images, labels, sizes).items():
                    acc[k] = acc.get(k, 0.0) + ms / args.iters
            for k, ms in acc.items():
                times[p][k].append(ms)
        acc = {"forward": 0.0, "backward": 0.0}
        for _ in range(args.iters):
            for k, ms in torch_head_step(thead, c1, c4, gout).items():
                acc[k] += ms / args.iters
        for k in acc:
            ttimes[k].append(acc[k])
    for p, v in variants.items():
        emit()
        emit(f"## {args.mode} B = {args.batch} {args.size} x {args.size}, {p} storage: augmentation -> FrostNetSeg -> SegmentationLoss + SegMeter -> backward -> QSGD")
        it = statistics.median(times[p]["iteration"])
        emit(f"   {'iteration':16s} {fmt(times[p]['iteration'])}   {args.batch / it * 1e3:8.1f} images/s")
        for k in PARTS:
            emit(f"   {k:16s} {fmt(times[p][k])}   {100 * statistics.median(times[p][k]) / it:5.1f} % of the iteration")
        hf, hb = statistics.median(times[p]["head forward"]), statistics.median(times[p]["head backward"])
        emit(f"   {'head forward':16s} {fmt(times[p]['head forward'])}   (inside forward)")
        emit(f"   {'head backward':16s} {fmt(times[p]['head backward'])}   (inside backward)   head forward + backward {100 * (hf + hb) / it:.1f} % of the iteration")
    emit()
    emit(f"## the same head as stock torch modules in the reference's order, fp32, c1 {tuple(c1.shape)} c4 {tuple(c4.shape)}")
    emit(f"   {'forward':16s} {fmt(ttimes['forward'])}")
    emit(f"   {'backward':16s} {fmt(ttimes['backward'])}")
    run = variants["fp32"].model.hip_runner()
    v = variants["fp32"]

    def dev_head():
        from frostnet_amd._lib import call, ptr, stream
        call("frost_float_weight_prep", ptr(run._table), len(run.layers), stream())
        run._head_fwd(c1a, c4a, True, True)
        run._begin_backward()
        run._head_bwd(gout)
        run._end_backward()
    mt, md = peak_rise(lambda: torch_head_step(thead, c1, c4, gout)), peak_rise(dev_head)
    for p in variants:
        hf, hb = statistics.median(times[p]["head forward"]), statistics.median(times[p]["head backward"])
        tf, tb = statistics.median(ttimes["forward"]), statistics.median(ttimes["backward"])
        emit(f"   torch / device ({p}): forward {tf / hf:.2f}x, backward {tb / hb:.2f}x, both {(tf + tb) / (hf + hb):.2f}x")
    emit(f"   peak memory of one forward + backward of the head: device (fp32 storage) {md / 1e6:.1f} MB, torch {mt / 1e6:.1f} MB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Time the fused segmentation criterion (frostnet_amd.seg: loss + gradient + mean-IoU counts from stride-8 logits, upsampling inside the kernel) against the torch
formulation of the same step on the same device, interleaved in one process:

    torch:  u = F.interpolate(x, size, mode='bilinear', align_corners=True); F.cross_entropy(u, t, weight, ignore_index=255) forward + backward to x;
            pred = u.argmax(1); three bincounts over the valid pixels

    python tools/bench_seg_loss.py [--out profiles/seg_loss.txt] [--iters 20] [--rounds 5]

Per shape: eager and replayed from a captured graph (torch.bincount reads its bin count back to the host and cannot be captured: the captured torch variant counts
with scatter_add_ into C + 1 bins instead, the eager one uses bincount), the peak-memory difference of one call, and the rate of the fused call on the bytes it
actually touches (logits once, gradient once, targets twice: the W_sum pass and the main pass) as a fraction of the 6.29 TB/s copy rate.  The equal-size case
(full-resolution logits, the one-read kernel) is timed against F.cross_entropy forward + backward alone.  Times are device-event times of `iters` back-to-back
calls; the figure per variant is the median over `rounds` interleaved rounds, with the spread beside it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

COPY_RATE = 6.29e12
SHAPES = [("voc", 32, 21, (64, 64), (512, 512)), ("cityscapes", 16, 20, (64, 128), (512, 1024))]
EQUAL = ("equal-size", 8, 21, (512, 512), (512, 512))


def inputs(n, c, hw, HW, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn((n, c) + hw, generator=gen) * 3.0).cuda().requires_grad_(True)
    # labels in blocks, as a label map has them, with ignored borders between
    coarse = torch.randint(0, c, (n, HW[0] // 32, HW[1] // 32), generator=gen)
    t = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)
    t[torch.rand(t.shape, generator=gen) < 0.03] = 255
    wt = torch.rand(c, generator=gen) * 9.0 + 1.0
    return x, t.cuda(), wt.cuda()


def torch_step(x, t, wt, c, counts, capturable, with_counts=True, interpolate=True):
    u = F.interpolate(x, tuple(t.shape[1:]), mode="bilinear", align_corners=True) if interpolate else x
    loss = F.cross_entropy(u, t, weight=wt, ignore_index=255)
    (g,) = torch.autograd.grad(loss, x)
    if with_counts:
        pred = u.detach().argmax(1)
        valid = t < c
        p, m = torch.where(valid, pred, c).flatten(), torch.where(valid, t, c).flatten()
        i = torch.where(valid & (pred == t), t, c).flatten()
        if capturable:
            one = torch.ones_like(p)
            counts.zero_()
            counts[0].scatter_add_(0, i, one); counts[1].scatter_add_(0, p, one); counts[2].scatter_add_(0, m, one)
        else:
            counts[0] += torch.bincount(i, minlength=c + 1); counts[1] += torch.bincount(p, minlength=c + 1); counts[2] += torch.bincount(m, minlength=c + 1)
    return loss.detach(), g          # (a loss that lives on keeps its autograd graph, and the leaf's gradient node with the stream it was made on, alive)


def fused_step(crit, x, t):
    loss = crit(x, t)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_loss: needs the GPU (no CPU timing is reported)")
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import seg
    lines = [f"# tools/bench_seg_loss.py --iters {args.iters} --rounds {args.rounds}   device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}",
             "# per call, device-event time of back-to-back calls; median over interleaved rounds (min, max)"]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, n, c, hw, HW in SHAPES + [EQUAL]:
        equal = hw == HW
        x, t, wt = inputs(n, c, hw, HW, seed=5)
        meter = None if equal else seg.SegMeter(c, "cuda")
        crit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt, meter=meter)
        counts = torch.zeros(3, c + 1, dtype=torch.int64, device="cuda")
        variants = {
            "fused eager": lambda: fused_step(crit, x, t),
            "torch eager": lambda: torch_step(x, t, wt, c, counts, False, with_counts=not equal, interpolate=not equal),
        }
        # results agree before anything is timed
        lf, gf = variants["fused eager"]()
        lt, gt = variants["torch eager"]()
        dl = abs(float(lf) - float(lt)) / abs(float(lt))
        dg = float((gf - gt).norm() / gt.norm())
        del lf, gf, lt, gt
        variants["fused graph"] = capture(lambda: fused_step(crit, x, t))
        variants["torch graph"] = capture(lambda: torch_step(x, t, wt, c, counts, True, with_counts=not equal, interpolate=not equal))
        for fn in variants.values():
            timed(fn, 3)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
        mem = {k: peak_rise(variants[k]) for k in ("fused eager", "torch eager")}
        tb = t.element_size()
        touched = 2 * x.numel() * 4 + 2 * t.numel() * tb
        full = n * c * HW[0] * HW[1] * 4
        emit()
        emit(f"## {name}: N = {n}, C = {c}, {hw[0]} x {hw[1]} -> {HW[0]} x {HW[1]}, int64 targets, class weights"
             + ("" if not equal else "   (identity: against F.cross_entropy forward + backward alone, no counts)"))
        emit(f"   agreement before timing: loss {dl:.1e} relative, gradient {dg:.1e} norm-wise; full-resolution logits would be {full / 1e6:.0f} MB")
        for k in variants:
            emit(f"   {k:12s} {fmt(times[k])}")
        fe, te, fg, tg = (statistics.median(times[k]) for k in ("fused eager", "torch eager", "fused graph", "torch graph"))
        emit(f"   torch / fused: eager {te / fe:.2f}x, graph {tg / fg:.2f}x")
        emit(f"   peak memory of one call: fused {mem['fused eager'] / 1e6:.1f} MB, torch {mem['torch eager'] / 1e6:.1f} MB (difference {(mem['torch eager'] - mem['fused eager']) / 1e6:.1f} MB)")
        rate = touched / (fg * 1e-3)
        emit(f"   fused graph: {touched / 1e6:.1f} MB touched -> {rate / 1e12:.3f} TB/s = {100 * rate / COPY_RATE:.1f} % of the 6.29 TB/s copy rate")
        del variants, x, t, counts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

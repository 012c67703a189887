"""dev: what the loops a user calls cost per iteration on one MI355X, eager against graph=True (harness.GraphedStep), next to the bare replay of the same graph.
  classifier: FrostNet-Large QAT, B = 512, ClassificationAugmentation in front of the model, `harness.train` over a synthetic in-memory loader of PINNED uint8 batches
              (slots of 375 x 500), --iters iterations per epoch
  detector:   SSDLite-FrostNet-Large QAT at 512 x 512, B = 32, SSDAugmentation in front of the model, `harness.train_detector` likewise
Eager and graphed epochs alternate in one process, --repeats each, wall clock of the whole call (it ends with the loop's single host read) / iterations.  Then, for the
attribution of what is left above the bare replay: the replay alone (prepare_step + replay, static inputs untouched), the graphed step fed from a batch that is already
on the device (in-stream copy only), and the host time of the three things a graphed iteration does on the host (input copy enqueue, prepare_step, replay launch).

    python tools/bench_train_loop.py [--iters 12] [--repeats 3] [--mode large] [--only classifier|detector] [--out profiles/train_loop.txt]
"""
import argparse, os, sys, time, warnings
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
from frostnet_amd import ClassificationAugmentation, SSDAugmentation, frostnet as F, harness as H, ssdlite as S
from frostnet_amd.optimizer import QSGD

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--mode", default="large")
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--det-batch", type=int, default=32)
ap.add_argument("--slot-h", type=int, default=375)
ap.add_argument("--slot-w", type=int, default=500)
ap.add_argument("--only", default=None, choices=("classifier", "detector"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_train_loop: no GPU (a timing needs the device; there is no fallback)")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


class Cycle:
    """An in-memory loader: `iters` iterations over a few pinned host batches."""

    def __init__(self, batches, iters):
        self.batches, self.iters = batches, iters

    def __iter__(self):
        return (self.batches[i % len(self.batches)] for i in range(self.iters))


def slots(rng, b):
    hs, ws = args.slot_h, args.slot_w
    sizes = np.stack([rng.integers(hs * 2 // 3, hs + 1, b), rng.integers(ws * 2 // 3, ws + 1, b)], 1).astype(np.int32)
    return torch.from_numpy(rng.integers(0, 256, (b, hs, ws, 3), dtype=np.uint8)).pin_memory(), torch.from_numpy(sizes).pin_memory()


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def host_us(fn, reps):
    """Host time of fn() alone (the stream is drained first and afterwards, outside the clock)."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
    return float(np.median(ts))


def report(name, run_eager, run_graphed, step, opt, batch, iters):
    """The interleaved repeats, then the bare replay of `step`'s graph and the attribution legs."""
    run_eager(), run_graphed(), run_graphed()          # tables, optimizer state, the capture
    assert step.captures >= 1, "the graphed loop did not capture"
    eager, graphed = [], []
    for _ in range(args.repeats):
        eager.append(wall(run_eager, iters))
        graphed.append(wall(run_graphed, iters))
    spread = max(max(eager) - min(eager), max(graphed) - min(graphed))
    say(f"{name}: eager loop    " + "  ".join(f"{v:8.3f}" for v in eager) + f"   ms / iteration (median {np.median(eager):.3f})")
    say(f"{name}: graphed loop  " + "  ".join(f"{v:8.3f}" for v in graphed) + f"   ms / iteration (median {np.median(graphed):.3f})")
    say(f"    graphed below eager by {np.median(eager) - np.median(graphed):.3f} ms = {(1 - np.median(graphed) / np.median(eager)) * 100:.1f} %; spread of the repeats "
        f"{spread:.3f} ms; largest graphed {max(graphed):.3f} against smallest eager {min(eager):.3f}")
    graph = step.graph_for(*batch)

    def bare():
        for _ in range(iters):
            opt.prepare_step()
            graph.replay()
    bare()
    ts = [wall(bare, iters) for _ in range(args.repeats)]
    bare_ms = float(np.median(ts))
    say(f"    bare replay of the same graph (prepare_step + replay, static inputs untouched)   " + "  ".join(f"{v:8.3f}" for v in ts) + f"   ms / step (median {bare_ms:.3f})")
    dev = tuple(t.cuda() for t in batch)

    def fed():
        for _ in range(iters):
            step(*dev)
    fed()
    ts = [wall(fed, iters) for _ in range(args.repeats)]
    fed_ms = float(np.median(ts))
    say(f"    graphed step fed from a device-resident batch (in-stream copy only)              " + "  ".join(f"{v:8.3f}" for v in ts) + f"   ms / step (median {fed_ms:.3f})")
    g = step._graphs[step._signature(batch)]
    say(f"    gap of the graphed loop to the bare replay {np.median(graphed) - bare_ms:+.3f} ms = {(np.median(graphed) / bare_ms - 1) * 100:+.1f} %: in-stream input copy "
        f"{fed_ms - bare_ms:+.3f} ms, host -> device leg and the loop around the step {np.median(graphed) - fed_ms:+.3f} ms")
    def h2d():
        for i, t in enumerate(batch):
            g.staging[i].copy_(t, non_blocking=True)
    h2d_ms = wall(h2d, 1)
    say(f"    host -> device copy of one batch ({sum(t.numel() * t.element_size() for t in batch) / 1e6:.0f} MB, pinned) {h2d_ms:.3f} ms: under the previous replay from the second "
        f"iteration on, exposed once per call = {h2d_ms / iters:.3f} ms / iteration here; the call's closing host read waits for the last replay")
    say(f"    host time per iteration: input copy enqueue {host_us(lambda: step._load(g, batch), 10):.0f} us, prepare_step {host_us(opt.prepare_step, 10):.0f} us, "
        f"replay launch {host_us(graph.replay, 10):.0f} us (all run ahead of the device: the replay before is still executing)")
    return float(np.median(eager)), float(np.median(graphed)), bare_ms


say(f"harness loops, eager against graph=True (GraphedStep); {torch.cuda.get_device_name(0)}; {args.iters} iterations per call, {args.repeats} interleaved repeats, wall clock "
    f"of the whole call / iterations")
rng = np.random.default_rng(1882)
if args.only in (None, "classifier"):
    B = args.batch
    model = F.MODEL_REGISTRY[f"frostnet_quant_{args.mode}_1_0"]()
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
    opt.is_warmup = False
    aug = ClassificationAugmentation(size=224, seed=7, channels_last=True)
    batches = [slots(rng, B) + (torch.randint(0, 1000, (B,)).pin_memory(),) for _ in range(2)]
    loader = Cycle(batches, args.iters)
    crit = H.CrossEntropyLoss()
    step = H.GraphedStep(model, crit, opt, transform=aug)
    say(f"classifier: FrostNet-{args.mode} QAT, B = {B}, ClassificationAugmentation (224 x 224, channels-last) on pinned uint8 slots {args.slot_h} x {args.slot_w} "
        f"({batches[0][0].numel() / 1e6:.0f} MB per batch)")
    report("classifier", lambda: H.train(loader, model, crit, opt, 0, transform=aug), lambda: H.train(loader, model, crit, opt, 0, transform=aug, graph=step),
           step, opt, batches[0], args.iters)
    del model, opt, step, batches, loader
    torch.cuda.empty_cache()

if args.only in (None, "detector"):
    B = args.det_batch
    model = S.SSDLiteFrostNet(num_classes=21, mode=args.mode)
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
    opt.is_warmup = False
    aug = SSDAugmentation(size=512, seed=7, channels_last=True)
    tr = torch.Generator().manual_seed(1882)
    batches = []
    for _ in range(2):
        tg = []
        for i in range(B):
            k = 1 + i % 4
            c, wh = torch.rand(k, 2, generator=tr) * 0.5 + 0.25, torch.rand(k, 2, generator=tr) * 0.3 + 0.1
            tg.append(torch.cat([c - wh / 2, c + wh / 2, torch.randint(0, 20, (k, 1), generator=tr).float()], 1))
        boxes, valid = S.pad_targets(tg, torch.device("cpu"))
        batches.append(slots(rng, B) + (boxes.pin_memory(), valid.pin_memory()))
    loader = Cycle(batches, args.iters)
    crit = S.MultiBoxLoss(21)
    step = H.GraphedStep(model, crit, opt, transform=aug)
    say()
    say(f"detector: SSDLite-FrostNet-{args.mode} QAT 512 x 512, B = {B}, SSDAugmentation (channels-last) on pinned uint8 slots {args.slot_h} x {args.slot_w} "
        f"({batches[0][0].numel() / 1e6:.0f} MB per batch)")
    n = args.iters
    report("detector", lambda: H.train_detector(loader, model, crit, opt, 0, n, 5e-3, 0.1, (), transform=aug),
           lambda: H.train_detector(loader, model, crit, opt, 0, n, 5e-3, 0.1, (), transform=aug, graph=step), step, opt, batches[0], n)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

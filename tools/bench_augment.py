"""dev: what augmenting a detector training batch costs on one MI355X (B = 32 uint8 images in slots of 500 x 500, G = 16 box rows, 512 x 512 fp32 output),
HIP-event timed, median of --reps:
  (a) SSDAugmentation.__call__ on device tensors, eager (frost_aug_plan: 2 launches, frost_aug_apply: 1 launch), NCHW and channels-last
  (b) the same call as one replayed hipGraph (every replay draws fresh decisions)
  (c) the apply kernel's achieved bytes/s: output bytes (12 B per output pixel) + the source bytes its taps touch (3 B per pixel of the pasted image inside the
      clipped crop, from the plans of the timed calls), as a fraction of the copy rate this project quotes as achievable (6.29 TB/s)
  (d) the CPU definition (the same class on CPU tensors, numpy) for the same batch, wall clock
  (e) for scale, the detector's QAT step (SSDLite-FrostNet 512 x 512 fake-quant fwd + MultiBoxLoss + bwd + QSGD step, eager) from the same process

    python tools/bench_augment.py [--batch 32] [--reps 30] [--mode large] [--out profiles/augment_b32_512.txt]
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
from frostnet_amd import SSDAugmentation, augment as A, frostnet as F, harness as H, ssdlite as S
from frostnet_amd.optimizer import QSGD

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--slot", type=int, default=500)
ap.add_argument("--boxes", type=int, default=16)
ap.add_argument("--mode", default="large")
ap.add_argument("--no-step", action="store_true", help="skip (e)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_augment: no GPU (a timing needs the device; there is no fallback)")
COPY_RATE = 6.29e12          # bytes/s, the achievable copy rate this project quotes (README)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, G, size, slot = args.batch, args.boxes, args.size, args.slot
rng = np.random.default_rng(1882)
sizes = np.full((B, 2), slot, dtype=np.int32)          # VOC-like: the longer side fills the slot, the other is 2/3 .. 1 of it
short = rng.integers(slot * 2 // 3, slot + 1, B)
sizes[np.arange(B), rng.integers(0, 2, B)] = short
c, half = rng.uniform(0.2, 0.8, (B, G, 2)), rng.uniform(0.05, 0.3, (B, G, 2))
boxes = np.concatenate([np.clip(c - half, 0, 1), np.clip(c + half, 0, 1), rng.integers(0, 20, (B, G, 1))], 2).astype(np.float32)
valid = np.arange(G)[None, :] < (1 + np.arange(B) % 4)[:, None]
host = [torch.from_numpy(a) for a in (rng.integers(0, 256, (B, slot, slot, 3), dtype=np.uint8), sizes, boxes, valid)]
dev = [t.cuda() for t in host]
out_bytes = B * 3 * size * size * 4


def touched_bytes(plan, sz):
    """Source bytes the taps of one batch can touch: per image 3 B x the pasted image's pixels inside the clipped crop."""
    p, s = plan.cpu().numpy().astype(np.int64), sz.cpu().numpy().astype(np.int64)
    x1, y1 = p[:, A.P_X1], p[:, A.P_Y1]
    x2, y2 = np.minimum(p[:, A.P_X2], p[:, A.P_CANVAS_W]), np.minimum(p[:, A.P_Y2], p[:, A.P_CANVAS_H])
    w = np.clip(np.minimum(x2, p[:, A.P_PASTE_X] + s[:, 1]) - np.maximum(x1, p[:, A.P_PASTE_X]), 0, None)
    h = np.clip(np.minimum(y2, p[:, A.P_PASTE_Y] + s[:, 0]) - np.maximum(y1, p[:, A.P_PASTE_Y]), 0, None)
    return int((w * h).sum()) * 3


def timed(fn):
    """HIP-event times of --reps calls of fn, ms."""
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.asarray(ts)


say(f"SSDAugmentation, B = {B}, slots {slot} x {slot} uint8 BGR, G = {G}, output {size} x {size} fp32 ({out_bytes / 1e6:.1f} MB per batch); {torch.cuda.get_device_name(0)}")
say(f"median (min) of {args.reps} calls, HIP events; every call draws new decisions, so the touched source bytes vary from call to call")
for cl in (False, True):
    name = "channels-last" if cl else "NCHW         "
    aug = SSDAugmentation(size=size, seed=7, channels_last=cl)
    for _ in range(3):
        aug(*dev)
    torch.cuda.synchronize()
    ts = timed(lambda: aug(*dev))
    say(f"(a) __call__ eager, {name} (plan + advance + apply)      {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = aug(*dev)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    ts = timed(graph.replay)
    say(f"(b) __call__ as one replayed hipGraph, {name}            {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s")
    # the two halves on their own; the plan of every timed apply is kept for the byte count
    ts = timed(lambda: aug.plan(*dev[1:]))
    say(f"    plan alone (frost_aug_plan: k_aug_plan + k_aug_advance)          {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us")
    plans = [aug.plan(*dev[1:])[0] for _ in range(args.reps)]
    it = iter(plans)
    ts = timed(lambda: aug.apply(dev[0], dev[1], next(it)))
    src = np.asarray([touched_bytes(p, dev[1]) for p in plans], dtype=np.float64)
    rate = (out_bytes + src) / (ts * 1e-3)
    say(f"(c) apply alone (k_aug_apply), {name}                    {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   output {out_bytes / 1e6:.1f} MB + touched source "
        f"{np.median(src) / 1e6:.1f} MB (median): {np.median(rate) / 1e12:.3f} TB/s median = {np.median(rate) / COPY_RATE:.3f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
    ident = A.identity_plan(dev[1])
    ts = timed(lambda: aug.apply(dev[0], dev[1], ident))
    src_i = touched_bytes(ident, dev[1])
    say(f"    apply under the identity plan (= BaseTransform), {name}  {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   "
        f"{(out_bytes + src_i) / (np.median(ts) * 1e-3) / 1e12:.3f} TB/s = {(out_bytes + src_i) / (np.median(ts) * 1e-3) / COPY_RATE:.3f} of the copy rate")
    del graph, out, plans

cpu = SSDAugmentation(size=size, seed=7)
ts = []
for _ in range(2):
    t0 = time.perf_counter()
    cpu(*host)
    ts.append(time.perf_counter() - t0)
say(f"(d) the CPU definition (numpy, one process), same batch                {np.median(ts) * 1e3:8.1f} ({min(ts) * 1e3:8.1f}) ms   {B / np.median(ts):8.1f} img/s")

if not args.no_step:
    model = S.SSDLiteFrostNet(num_classes=21, mode=args.mode)
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
    opt.is_warmup = False
    crit = S.MultiBoxLoss(21)
    aug = SSDAugmentation(size=size, seed=7, channels_last=True)
    x, bo, vo = aug(*dev)

    def step():
        opt.zero_grad(set_to_none=True)
        loc, conf, pri = model(x)
        ll, lc = crit((loc, conf, pri), (bo, vo))
        (ll + lc).backward()
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ts = timed(step)
    say(f"(e) SSDLite-FrostNet-{args.mode} {size} x {size} QAT step on the augmented batch, eager  {np.median(ts):8.3f} ({ts.min():8.3f}) ms   {B / np.median(ts):8.2f} k img/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

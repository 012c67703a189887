"""dev: what the classifier's input pipeline costs on one MI355X (B = 512 uint8 images in slots of 375 x 500, 224 x 224 fp32 output), HIP-event timed, median of
--reps:
  (a) ClassificationAugmentation.__call__ on device tensors, eager (frost_caug_plan: 2 launches, frost_caug_apply: 1 launch), NCHW and channels-last
  (b) the same call as one replayed hipGraph (every replay draws fresh crops)
  (c) the apply kernel's achieved bytes/s: output bytes (12 B per output pixel) + the source bytes of the crops (3 B per pixel of every plan rect, from the plans of
      the timed calls), as a fraction of the copy rate this project quotes as achievable (6.29 TB/s)
  (d) the same batch and the same crops through Pillow itself (crop, resize BILINEAR, flip, ToTensor + Normalize in numpy) on --threads host threads, wall clock;
      where Pillow does not import, the numpy definition on the same threads -- the line says which
  (e) ClassificationEvalTransform.__call__ likewise (eager, graph, host leg)
  (f) the FrostNet QAT step the pipeline feeds (fake-quant fwd + CE + bwd + QSGD step at 224 x 224, eager) from the same process, and the pipeline's share of it

    python tools/bench_cls_augment.py [--batch 512] [--reps 30] [--mode large] [--out profiles/cls_augment_b512.txt]
"""
import argparse, os, sys, time, warnings
from concurrent.futures import ThreadPoolExecutor
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
from frostnet_amd import ClassificationAugmentation, ClassificationEvalTransform, cls_augment as C, frostnet as F, harness as H
from frostnet_amd.optimizer import QSGD
try:
    from PIL import Image
except ImportError:
    Image = None

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--resize", type=int, default=256)
ap.add_argument("--slot-h", type=int, default=375)
ap.add_argument("--slot-w", type=int, default=500)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--mode", default="large")
ap.add_argument("--no-step", action="store_true", help="skip (f)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_cls_augment: no GPU (a timing needs the device; there is no fallback)")
COPY_RATE = 6.29e12          # bytes/s, the achievable copy rate this project quotes (README)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, size, hs, ws = args.batch, args.size, args.slot_h, args.slot_w
rng = np.random.default_rng(1882)
sizes = np.stack([rng.integers(hs * 2 // 3, hs + 1, B), rng.integers(ws * 2 // 3, ws + 1, B)], 1).astype(np.int32)          # ImageNet-like: 2/3 .. 1 of the slot per side
sizes[::8] = (hs, ws)
host = [torch.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)), torch.from_numpy(sizes)]
dev = [t.cuda() for t in host]
out_bytes = B * 3 * size * size * 4


def timed(fn, reps=None):
    """HIP-event times of --reps calls of fn, ms."""
    ts = []
    for _ in range(reps or args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.asarray(ts)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return graph, out


def host_leg(obj, plan):
    """The batch under `plan` on the host, one image per task on --threads threads: Pillow where it imports, else the numpy definition.  Returns (seconds, which)."""
    table = C.norm_table(obj.mean, obj.std)
    im, pl = host[0].numpy(), plan.cpu().numpy()
    out = np.empty((B, 3, size, size), dtype=np.float32)

    def one(i):
        x0, y0, w, h, rw, rh, ox, oy = (int(v) for v in pl[i, C.P_X0:C.P_OY + 1])
        if Image is not None:
            win = np.asarray(Image.fromarray(im[i]).crop((x0, y0, x0 + w, y0 + h)).resize((rw, rh), Image.BILINEAR))[oy:oy + size, ox:ox + size]
        else:
            win = C.resize_crop(im[i, y0:y0 + h, x0:x0 + w], rw, rh, ox, oy, size, size)
        if int(pl[i, C.P_FLAGS]) & C.F_MIRROR:
            win = win[:, ::-1]
        for c in range(3):
            out[i, c] = table[c][win[..., c]]
    ts = []
    with ThreadPoolExecutor(args.threads) as pool:
        for _ in range(2):
            t0 = time.perf_counter()
            list(pool.map(one, range(B)))
            ts.append(time.perf_counter() - t0)
    return min(ts), out, "Pillow " + Image.__version__ if Image is not None and hasattr(Image, "__version__") else ("Pillow" if Image is not None else "the numpy definition")


say(f"ClassificationAugmentation / ClassificationEvalTransform, B = {B}, slots {hs} x {ws} uint8 (sizes 2/3 .. 1 of the slot per side), output {size} x {size} fp32 "
    f"({out_bytes / 1e6:.1f} MB per batch); {torch.cuda.get_device_name(0)}")
say(f"median (min) of {args.reps} calls, HIP events; every training call draws new crops, so the touched source bytes vary from call to call")
call_us = {}
for cl in (False, True):
    name = "channels-last" if cl else "NCHW         "
    aug = ClassificationAugmentation(size=size, seed=7, channels_last=cl)
    for _ in range(3):
        aug(*dev)
    torch.cuda.synchronize()
    ts = timed(lambda: aug(*dev))
    say(f"(a) __call__ eager, {name} (plan + advance + apply)      {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s")
    graph, out = graphed(lambda: aug(*dev))
    ts = timed(graph.replay)
    call_us[cl] = float(np.median(ts)) * 1e3
    say(f"(b) __call__ as one replayed hipGraph, {name}            {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s")
    ts = timed(lambda: aug.plan(dev[1]))
    say(f"    plan alone (frost_caug_plan: k_caug_plan + k_caug_advance)       {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us")
    plans = [aug.plan(dev[1]) for _ in range(args.reps)]
    it = iter(plans)
    ts = timed(lambda: aug.apply(dev[0], dev[1], next(it)))
    src = np.asarray([int((p[:, C.P_W].long() * p[:, C.P_H].long()).sum()) * 3 for p in plans], dtype=np.float64)
    rate = (out_bytes + src) / (ts * 1e-3)
    say(f"(c) apply alone (k_caug_apply), {name}                   {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   output {out_bytes / 1e6:.1f} MB + crop source "
        f"{np.median(src) / 1e6:.1f} MB (median): {np.median(rate) / 1e12:.3f} TB/s median = {np.median(rate) / COPY_RATE:.3f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
    if not cl:
        secs, ref, which = host_leg(aug, plans[-1])
        same = bool(torch.equal(aug.apply(dev[0], dev[1], plans[-1]).cpu(), torch.from_numpy(ref)))
        say(f"(d) the same batch and crops through {which} on {args.threads} host threads   {secs * 1e3:8.1f} ms (best of 2)   {B / secs / 1e3:8.2f} k img/s   "
            f"device output bit-equal to it: {same}")
        say(f"    __call__ (b) is {secs * 1e6 / call_us[cl]:.0f} x faster than the host leg")
    del graph, out, plans

ev_us = None
for cl in (False, True):
    name = "channels-last" if cl else "NCHW         "
    ev = ClassificationEvalTransform(size=size, resize=args.resize, channels_last=cl)
    for _ in range(3):
        ev(*dev)
    torch.cuda.synchronize()
    ts = timed(lambda: ev(*dev))
    say(f"(e) eval transform eager, {name} (plan + apply)          {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s")
    graph, out = graphed(lambda: ev(*dev))
    ts = timed(graph.replay)
    plan = ev.plan(dev[1])
    src = int((plan[:, C.P_W].long() * plan[:, C.P_H].long()).sum()) * 3
    say(f"    eval transform as one replayed hipGraph, {name}      {np.median(ts) * 1e3:8.1f} ({ts.min() * 1e3:8.1f}) us   {B / np.median(ts):8.1f} k img/s   "
        f"output + whole images {(out_bytes + src) / 1e6:.1f} MB: {(out_bytes + src) / (np.median(ts) * 1e-3) / COPY_RATE:.3f} of the copy rate")
    if not cl:
        ev_us = float(np.median(ts)) * 1e3
        secs, ref, which = host_leg(ev, plan)
        same = bool(torch.equal(out.cpu(), torch.from_numpy(ref)))
        say(f"    the same through {which} on {args.threads} host threads                     {secs * 1e3:8.1f} ms (best of 2)   {B / secs / 1e3:8.2f} k img/s   "
            f"device output bit-equal to it: {same}; the device is {secs * 1e6 / ev_us:.0f} x faster")
    del graph, out

if not args.no_step:
    model = F.MODEL_REGISTRY[f"frostnet_quant_{args.mode}_1_0"]()
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
    opt.is_warmup = False
    crit = H.CrossEntropyLoss()
    aug = ClassificationAugmentation(size=size, seed=7, channels_last=True)
    x = aug(*dev)
    target = torch.randint(0, 1000, (B,), device="cuda")
    for _ in range(3):
        H.train_one_iter(model, crit, opt, x, target)
    torch.cuda.synchronize()
    ts = timed(lambda: H.train_one_iter(model, crit, opt, x, target), reps=min(args.reps, 10))
    step_ms = float(np.median(ts))
    say(f"(f) FrostNet-{args.mode} {size} x {size} QAT step on the augmented batch, eager  {step_ms:8.3f} ({ts.min():8.3f}) ms   {B / step_ms:8.2f} k img/s")
    ts = timed(lambda: H.train_one_iter(model, crit, opt, aug(*dev), target), reps=min(args.reps, 10))
    say(f"    the same step with __call__ in front of it, eager               {np.median(ts):8.3f} ({ts.min():8.3f}) ms   "
        f"measured share of the pipeline: (b) / (f) = {call_us[True] / (step_ms * 1e3) * 100:.2f} % of a step")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

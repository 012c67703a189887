"""dev: what the segmentation input pipeline costs on one MI355X, HIP-event timed, median over --rounds interleaved rounds of --reps calls, for the two recipes:
  voc         B = 32, slots 375 x 500, crop 513 x 513, scale (0.5, 1.0), the mirror in front of the resizes
  cityscapes  B = 16, slots 1024 x 2048, crop 1024 x 512 (w x h), scale (0.5, 2.0), the mirror behind the crop
per recipe:
  (a) SegmentationAugmentation.__call__ on device tensors, eager (frost_saug_plan: 2 launches, frost_saug_apply: 3 launches)
  (b) the same call as one replayed hipGraph (every replay draws fresh scales and crops)
  (c) each launch of frost_saug_apply alone (the index tables, the picture, the label map) under the plans of the timed calls, and the picture + label launches'
      achieved bytes/s on output + touched-source bytes as a fraction of the copy rate this project quotes as achievable (6.29 TB/s).  Touched source: per image the
      rect of the picture that the window's taps reach (3 B per pixel) and one label byte per distinct (row, column) of the two index tables.
  (d) the same batch and the same decisions through Pillow itself (transpose, resize LANCZOS / NEAREST, pad + crop, ToTensor + Normalize in numpy) on --threads host
      threads, wall clock, and whether the device output is bit-equal to it
  (e) SegmentationEvalTransform.__call__ likewise (VOC: Resize to the crop size; Cityscapes: Normalize alone)
  (f) the segmentation criterion the pipeline feeds (SegmentationLoss forward + backward on stride-8 logits at the crop size, the recipe's class count) in the same
      process, and the pipeline's time relative to it.  The share of a whole training iteration is measured by tools/bench_seg_train.py.

    python tools/bench_seg_augment.py [--reps 20] [--rounds 5] [--out profiles/seg_augment.txt]
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
from frostnet_amd import SegmentationAugmentation, SegmentationEvalTransform, SegmentationLoss, _lib as L, cls_augment as C, seg_augment as S
import PIL
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--recipes", default="voc,cityscapes")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_seg_augment: no GPU (a timing needs the device; there is no fallback)")
COPY_RATE = 6.29e12          # bytes/s, the achievable copy rate this project quotes (README)
RECIPES = {"voc": dict(batch=32, slot=(375, 500), crop=(513, 513), scale=(0.5, 1.0), flip_first=True, classes=21, eval_size=(513, 513)),
           "cityscapes": dict(batch=16, slot=(1024, 2048), crop=(1024, 512), scale=(0.5, 2.0), flip_first=False, classes=20, eval_size=None)}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """HIP-event time per call of `reps` back-to-back calls of fn, ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fns):
    """{name: fn} -> {name: (median, min, max) ms}: the candidates alternate inside every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, args.reps))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def fmt(t):
    return f"{t[0] * 1e3:9.1f} us  (min {t[1] * 1e3:.1f}, max {t[2] * 1e3:.1f})"


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


def touched(plan, sizes, cw, ch):
    """Source bytes the picture and label launches have to read under `plan` (host arithmetic from the plan words)."""
    pic = lab = 0
    for (flags, rw, rh, ox, oy, *_), (h, w) in zip(plan.tolist(), sizes.tolist()):
        x0, x1, y0, y1 = max(ox, 0), min(ox + cw, rw), max(oy, 0), min(oy + ch, rh)
        if x0 >= x1 or y0 >= y1:
            continue
        sup = 3.0 if flags & S.F_LANCZOS else 1.0
        sx, sy = w / rw, h / rh
        cols = min(w, int((x1 - x0) * sx + 2 * sup * max(sx, 1.0)) + 1)
        rows = min(h, int((y1 - y0) * sy + 2 * sup * max(sy, 1.0)) + 1)
        pic += cols * rows * 3
        lab += min(x1 - x0, int((x1 - x0) * sx) + 1) * min(y1 - y0, int((y1 - y0) * sy) + 1)
    return pic + lab


def host_leg(obj, host, plan, cw, ch):
    """The batch under `plan` through Pillow, one pair per task on --threads threads.  Returns (seconds, x, target)."""
    table = C.norm_table(obj.mean, obj.std)
    im, lb, sz, pl = host[0].numpy(), host[1].numpy(), host[2].numpy(), plan.cpu().numpy()
    n = im.shape[0]
    x, t = np.empty((n, 3, ch, cw), dtype=np.float32), np.empty((n, ch, cw), dtype=np.int64)

    def one(i):
        flags, rw, rh, ox, oy = (int(v) for v in pl[i, :5])
        h, w = int(sz[i, 0]), int(sz[i, 1])
        pic, lab = Image.fromarray(im[i, :h, :w]), Image.fromarray(lb[i, :h, :w])
        mirror, first = flags & S.F_MIRROR, flags & S.F_FLIP_FIRST
        if mirror and first:
            pic, lab = pic.transpose(Image.FLIP_LEFT_RIGHT), lab.transpose(Image.FLIP_LEFT_RIGHT)
        if flags & (S.F_LANCZOS | S.F_TRIANGLE):
            pic, lab = pic.resize((rw, rh), Image.LANCZOS if flags & S.F_LANCZOS else Image.BILINEAR), lab.resize((rw, rh), Image.NEAREST)
        cp, cl = Image.new("RGB", (cw, ch), 0), Image.new("L", (cw, ch), obj.ignore_idx)          # Pad + crop: the window of the padded grid
        cp.paste(pic, (-ox, -oy))
        cl.paste(lab, (-ox, -oy))
        if mirror and not first:
            cp, cl = cp.transpose(Image.FLIP_LEFT_RIGHT), cl.transpose(Image.FLIP_LEFT_RIGHT)
        a = np.asarray(cp)
        for c in range(3):
            x[i, c] = table[c][a[..., c]]
        t[i] = np.asarray(cl)
    ts = []
    with ThreadPoolExecutor(args.threads) as pool:
        for _ in range(2):
            t0 = time.perf_counter()
            list(pool.map(one, range(n)))
            ts.append(time.perf_counter() - t0)
    return min(ts), x, t


say(f"# tools/bench_seg_augment.py --reps {args.reps} --rounds {args.rounds}   device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}   Pillow {PIL.__version__}")
say("# per call, device-event time of back-to-back calls; median over interleaved rounds (min, max); every training call draws new scales and crops")
for name in args.recipes.split(","):
    r = RECIPES[name]
    B, (hs, ws), (cw, ch) = r["batch"], r["slot"], r["crop"]
    rng = np.random.default_rng(1882)
    sizes = np.tile(np.asarray([[hs, ws]], dtype=np.int32), (B, 1))
    if name == "voc":          # PASCAL VOC: the longer side is 500, the other 2/3 .. 1 of its slot side; every fourth image is a portrait
        sizes[:, 0] = rng.integers(hs * 2 // 3, hs + 1, B)
        sizes[::4] = np.stack([np.full(B // 4, hs), rng.integers(ws // 2, hs + 1, B // 4)], 1)
    host = [torch.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)), torch.from_numpy(rng.integers(0, r["classes"], (B, hs, ws)).astype(np.uint8)),
            torch.from_numpy(sizes)]
    host[1][torch.from_numpy(rng.random((B, hs, ws)) < 0.05)] = 255
    dev = [t.cuda() for t in host]
    out_bytes = B * ch * cw * (12 + 8)
    say()
    say(f"## {name}: B = {B}, slots {hs} x {ws} uint8 + uint8 labels, crop {cw} x {ch} (w x h), scale {r['scale']}, flip_first = {r['flip_first']}; "
        f"output fp32 NCHW + int64 target = {out_bytes / 1e6:.1f} MB per batch")
    kw = dict(crop_size=(cw, ch), scale=r["scale"], flip_first=r["flip_first"], seed=7)
    aug, aug_g = SegmentationAugmentation(**kw), SegmentationAugmentation(**kw)
    aug_g(*dev)
    graph, out = graphed(lambda: aug_g(*dev))
    plans = [aug.plan(dev[2]) for _ in range(8)]
    tables = torch.empty(B, cw + ch, dtype=torch.int32, device="cuda")
    x, t = torch.empty(B, 3, ch, cw, device="cuda"), torch.empty(B, ch, cw, dtype=torch.int64, device="cuda")
    state = {"k": 0}

    def part(parts):
        def run():
            p = plans[state["k"] % len(plans)]
            state["k"] += 1
            L.call("frost_saug_apply", L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), L.ptr(p), B, hs, ws, cw, ch, *aug.mean, *aug.std, 255, 0, 1, parts, L.ptr(tables), L.ptr(x),
                   L.ptr(t), L.stream())
        return run

    part(7)()
    res = rounds({"eager": lambda: aug(*dev), "graph": graph.replay, "plan": lambda: aug.plan(dev[2]), "tables": part(1), "picture": part(2), "labels": part(4),
                  "apply": part(7)})
    say(f"(a) __call__ eager (plan + advance + tables + picture + labels)      {fmt(res['eager'])}   {B / res['eager'][0]:8.1f} k img/s")
    say(f"(b) __call__ as one replayed hipGraph                                {fmt(res['graph'])}   {B / res['graph'][0]:8.1f} k img/s")
    say(f"(c) plan alone (k_saug_plan + k_saug_advance)                        {fmt(res['plan'])}")
    say(f"    index tables alone (k_saug_tables, {2 * B} waves, serial fp64 adds)    {fmt(res['tables'])}")
    say(f"    picture alone (k_saug_apply)                                     {fmt(res['picture'])}")
    say(f"    label map alone (k_saug_labels)                                  {fmt(res['labels'])}")
    say(f"    frost_saug_apply, all three launches                             {fmt(res['apply'])}")
    src = float(np.median([touched(p.cpu(), host[2], cw, ch) for p in plans]))
    both = res["picture"][0] + res["labels"][0]
    rate = (out_bytes + src) / (both * 1e-3)
    say(f"    picture + label launches: output {out_bytes / 1e6:.1f} MB + touched source {src / 1e6:.1f} MB (median of the plans) in {both * 1e3:.1f} us = "
        f"{rate / 1e12:.3f} TB/s = {rate / COPY_RATE:.3f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
    grids = torch.stack(plans).cpu()
    say(f"    grids of the timed plans: width {int(grids[..., S.P_RW].min())} .. {int(grids[..., S.P_RW].max())}, height {int(grids[..., S.P_RH].min())} .. "
        f"{int(grids[..., S.P_RH].max())}; records with padding {int(((grids[..., S.P_PADW] > 0) | (grids[..., S.P_PADH] > 0)).sum())} of {grids.shape[0] * B}")
    secs, rx, rt = host_leg(aug, host, plans[-1], cw, ch)
    dx, dt = aug.apply(dev[0], dev[1], dev[2], plans[-1])
    same = bool(torch.equal(dx.cpu().view(torch.int32), torch.from_numpy(rx).view(torch.int32))) and bool(torch.equal(dt.cpu(), torch.from_numpy(rt)))
    say(f"(d) the same batch and decisions through Pillow on {args.threads} host threads      {secs * 1e3:9.1f} ms (best of 2)   {B / secs / 1e3:8.3f} k img/s   "
        f"device output bit-equal to it: {same}; __call__ (b) is {secs * 1e3 / res['graph'][0]:.0f} x faster")
    del graph, out

    ev = SegmentationEvalTransform(size=r["eval_size"])
    ew, eh = r["eval_size"] if r["eval_size"] is not None else (ws, hs)
    ev(*dev)
    graph, out = graphed(lambda: ev(*dev))
    res_e = rounds({"eager": lambda: ev(*dev), "graph": graph.replay})
    what = f"Resize({ew} x {eh}) + Normalize" if r["eval_size"] is not None else f"Normalize alone ({ew} x {eh})"
    say(f"(e) eval transform, {what}: eager {fmt(res_e['eager'])}; replayed {fmt(res_e['graph'])}   {B / res_e['graph'][0]:8.1f} k img/s")
    secs, rx, rt = host_leg(ev, host, ev.plan(dev[2]), ew, eh)
    same = bool(torch.equal(out[0].cpu().view(torch.int32), torch.from_numpy(rx).view(torch.int32))) and bool(torch.equal(out[1].cpu(), torch.from_numpy(rt)))
    say(f"    the same through Pillow on {args.threads} host threads   {secs * 1e3:9.1f} ms (best of 2)   device output bit-equal to it: {same}; the device is "
        f"{secs * 1e3 / res_e['graph'][0]:.0f} x faster")
    del graph, out

    c = r["classes"]
    crit = SegmentationLoss(n_classes=c, device="cuda")
    logits = torch.randn(B, c, (ch + 7) // 8, (cw + 7) // 8, device="cuda", requires_grad=True)
    target = aug.apply(dev[0], dev[1], dev[2], plans[0])[1]

    def loss_step():
        logits.grad = None
        crit(logits, target).backward()

    res_l = rounds({"criterion": loss_step})
    say(f"(f) SegmentationLoss forward + backward, {c} classes, stride-8 logits -> {cw} x {ch}, same process   {fmt(res_l['criterion'])}; the pipeline (b) takes "
        f"{res['graph'][0] / res_l['criterion'][0]:.2f} x the criterion's time (the share of a whole training iteration: tools/bench_seg_train.py)")
    del host, dev, x, t, tables, plans, logits, target
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

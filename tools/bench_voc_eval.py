"""dev: what scoring the detector costs per batch and per evaluation on one MI355X (B = 32, C = 21, K = 200, scene inputs from tests/voc_scenes.py), HIP-event
timed, median of --reps:
  (a) VOCEvaluator.update on device tensors (one frost_voc_update call: matching + records + the images-seen advance)
  (b) the same batch the reference's way: copy the detections to the host and run the CPU definition's update (wall clock)
  (c) compute() on a record set of VOC07-test size (4 952 images fed as 155 batches), split into the torch.sort of the rows and frost_voc_ap, both metrics
  (d) for scale, model.hip_detect_bf16 of SSDLite-FrostNet for the same batch size at 512 x 512 (the replayed graph)

    python tools/bench_voc_eval.py [--batch 32] [--reps 20] [--mode large] [--out profiles/voc_eval_b32.txt]
"""
import argparse, os, sys, time, warnings
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
import voc_scenes as V
from frostnet_amd import VOCEvaluator, _lib as L, ssdlite as S

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--images", type=int, default=4952)
ap.add_argument("--mode", default="large")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_voc_eval: no GPU (a timing needs the device; there is no fallback)")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn, before=None):
    ts = []
    for _ in range(args.reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


B, C, K = args.batch, 21, 200
det, gt, difficult, valid, sizes, info = V.build(1, N=B, C=C, K=K, G=8, offset=0.0, fill=0.15)
host = [torch.from_numpy(a) for a in (det, gt, difficult, valid, sizes)]
dev = [t.cuda() for t in host]
nb = (args.images + B - 1) // B
say(f"VOC evaluator, B = {B}, C = {C}, K = {K}, G = 8: {int((det[..., 0] > 0).sum())} detections and {int(valid.sum())} ground-truth boxes per batch; {torch.cuda.get_device_name(0)}")

ev = VOCEvaluator(device="cuda", max_images=nb * B, top_k=K)
for _ in range(3):
    ev.update(*dev)
torch.cuda.synchronize()
med, mn = event_ms(lambda: ev.update(*dev), before=ev.reset)
say(f"(a) update on the device (frost_voc_update, 2 launches)        median {med * 1e3:8.1f} us   min {mn * 1e3:8.1f} us")

cpu = VOCEvaluator(max_images=nb * B, top_k=K)
ts = []
for _ in range(args.reps):
    cpu.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cpu.update(dev[0].cpu(), *host[1:])
    ts.append((time.perf_counter() - t0) * 1e3)
say(f"(b) detections to the host + the CPU definition's update        median {np.median(ts) * 1e3:8.1f} us   min {min(ts) * 1e3:8.1f} us")

ev.reset()
for _ in range(nb):
    ev.update(*dev)
torch.cuda.synchronize()
say(f"(c) compute() after {nb} batches = {nb * B} images, {int(ev._ctr[:C].sum())} records in rows of {ev.capacity} slots")
med, mn = event_ms(ev.sorted_records)
say(f"    torch.sort of the [21, {ev.capacity}] rows                       median {med:8.3f} ms   min {mn:8.3f} ms")
srt = ev.sorted_records()
for metric in (True, False):
    ev.use_07_metric = metric
    ap_t, cnt_t = torch.empty(C, dtype=torch.float64, device="cuda"), torch.empty(5, C, dtype=torch.int64, device="cuda")
    fn = lambda: L.call("frost_voc_ap", L.ptr(srt), L.ptr(ev._ctr), C, ev.capacity, 0, int(metric), L.ptr(ap_t), L.ptr(cnt_t), L.stream())
    fn()
    med, mn = event_ms(fn)
    say(f"    frost_voc_ap, {'07 metric  ' if metric else 'area metric'}                                   median {med:8.3f} ms   min {mn:8.3f} ms")
    med, mn = event_ms(lambda: float(ev.compute()["mean_ap"]))
    say(f"    compute() + the host read of mean_ap, {'07' if metric else 'area'}                     median {med:8.3f} ms   min {mn:8.3f} ms")
del srt

model = S.SSDLiteFrostNet(num_classes=C, mode=args.mode).cuda().eval()
x = torch.randn(B, 3, 512, 512, device="cuda")
for _ in range(3):
    model.hip_detect_bf16(x)
torch.cuda.synchronize()
med, mn = event_ms(lambda: model.hip_detect_bf16(x))
say(f"(d) hip_detect_bf16, SSDLite-FrostNet-{args.mode} 512 x 512, B = {B}      median {med:8.3f} ms   min {mn:8.3f} ms")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

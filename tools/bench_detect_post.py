"""dev: time of the SSD Detect layer (softmax + decode + per-class top-k + NMS) on the device, on scene inputs (tests/detect_scenes.py) at config c5's size:
(a) the HIP kernels (csrc/frost_detect.hip), (b) Detect.forward_torch on the same device tensors (the only other way to get detections on the device), and,
for scale, (c) the eval-mode forward of the QAT SSDLite-FrostNet-Large that feeds it.  HIP-event timed, median over --steps after --warmup.

    python tools/bench_detect_post.py [--batch 32] [--res 512] [--steps 20] [--warmup 3] [--only hip,torch,forward] [--out FILE]
"""
import argparse, json, os, sys, warnings
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
import detect_scenes as D
from frostnet_amd import frostnet as F, ssdlite as S

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--top-k", type=int, default=200)
ap.add_argument("--only", default="hip,torch,forward")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.steps >= 20, "median of at least 20"


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


B, C = args.batch, 21
cfg = S.ssd_cfg_for(args.res)
pri = S.prior_boxes(cfg)
P = pri.shape[0]
oi, ol, oc = D.object_rows(pri.numpy(), B, C, 1)                  # (timing needs no decision margins: the scene of seed 1 as it comes)
loc, conf = (torch.from_numpy(a).cuda() for a in D.assemble(B, P, C, 1, oi, ol, oc))
pri_d = pri.cuda()
det = S.Detect(C, 0, args.top_k, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
res = dict(batch=B, res=args.res, priors=P, classes=C, top_k=args.top_k, steps=args.steps)
which = args.only.split(",")
if "hip" in which:
    res["hip_ms"], res["hip_min_ms"] = median_ms(lambda: det.forward_hip(loc, conf, pri_d))
    cnt = det.last_counts
    res["kept_rows"], res["candidates"] = int(cnt.sum()), int((torch.softmax(conf, 2)[..., 1:] > 0.01).sum())
if "torch" in which:
    res["torch_ms"], res["torch_min_ms"] = median_ms(lambda: det.forward_torch(loc, conf, pri_d))
    if "hip" in which:
        res["paths_agree_on_counts"] = bool(torch.equal(det.last_counts, cnt))      # (informative: this scene carries no decision margins)
if "forward" in which:
    torch.manual_seed(0)
    model = S.SSDLiteFrostNet(num_classes=C, mode="large", cfg=cfg)
    F.qat_prepare(model, version=0)
    model.cuda().train()
    x = torch.randn(B, 3, args.res, args.res, device="cuda").contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        for _ in range(2):
            model(x)
        model.apply(torch.quantization.disable_observer)
        model.eval()
        res["qat_eval_forward_ms"], res["qat_eval_forward_min_ms"] = median_ms(lambda: model(x))
        res["model_detect_ms"], _ = median_ms(lambda: model.detect(x, top_k=args.top_k))
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")

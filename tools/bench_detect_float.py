"""dev: throughput of one float SSDLite detector training step on the device (the StatAssist warm-up of the detection recipe):
forward + MultiBoxLoss + backward + QSGD step (is_warmup), Large backbone, in the bf16 and the fp32 storage mode.

    python tools/bench_detect_float.py [--batch 32] [--res 512] [--steps 8] [--warmup 3] [--prec bf16,fp32]
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
from frostnet_amd import harness as H, ssdlite as S
from frostnet_amd.optimizer import QSGD

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--prec", default="bf16,fp32")
args = ap.parse_args()


def targets(n):
    rng = np.random.Generator(np.random.PCG64(7))
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 6))
        c = rng.random((k, 2)) * 0.6 + 0.2
        wh = rng.random((k, 2)) * 0.3 + 0.05
        out.append(torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2, rng.integers(0, 20, (k, 1))], 1).astype(np.float32)))
    return out


torch.manual_seed(0)
B = args.batch
model = S.SSDLiteFrostNet(num_classes=21, mode="large", cfg=S.ssd_cfg_for(args.res)).cuda().train()
opt = QSGD(H.make_param_groups(model, 1e-5), lr=1e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2)
assert opt.is_warmup
mbox = S.MultiBoxLoss(21)
crit = lambda out, t: sum(mbox(out, t))
x = torch.randn(B, 3, args.res, args.res, device="cuda")
tg = S.pad_targets(targets(B), "cuda")
for prec in args.prec.split(","):
    model.float_precision = prec
    for _ in range(args.warmup):
        H.train_one_iter(model, crit, opt, x, tg)
    assert type(model.hip_runner()).__name__ == "FloatSSDRunner" and model.hip_runner().precision == prec
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    for _ in range(args.steps):
        loss, _ = H.train_one_iter(model, crit, opt, x, tg)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / args.steps
    print(f"float SSDLite-Large {prec} B={B} @{args.res}: {dt * 1e3:.2f} ms/step  {B / dt:.0f} img/s  peak mem {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB"
          f"  loss {float(loss):.4f}", flush=True)

"""dev: what the weight EMA costs on one MI355X -- FrostNet-Large QAT at 224 x 224, B = 512, model and shadow bound on the device; legs interleaved round by round in
one process, median of --reps:
  (a) `ModelEma.update` alone: eager (prepare_step + the one launch; HIP events, and the host time of the call) and the launch replayed from a hipGraph; the launch's
      bytes/s on 3 x the float bytes + 2 x the integer bytes next to the copy rate this project quotes as achievable (6.29 TB/s); and the same launch over the
      large-entry rows of the workgroup map alone and over the packed small entries alone (which part of the map the time belongs to)
  (b) the stock loop on the same two models, wall clock with a drained stream: through `state_dict()` as a user would write it, and its best torch form
      (`torch._foreach_lerp_` over the float tensors + one `copy_` per other tensor, live tensors collected once)
  (c) `harness.GraphedStep` with and without `ema=`, alternating, --repeats times --iters iterations, wall clock / iteration

    python tools/bench_ema.py [--batch 512] [--reps 20] [--iters 12] [--repeats 3] [--mode large] [--out profiles/ema_b512.txt]
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
from frostnet_amd import frostnet as F, harness as H, _lib as L
from frostnet_amd.ema import ModelEma, _walk, build_map
from frostnet_amd.optimizer import QSGD

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--mode", default="large")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_ema: no GPU (a timing needs the device; there is no fallback)")
COPY_RATE = 6.29e12          # bytes/s, the achievable copy rate this project quotes (README)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn, iters=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


B, size = args.batch, args.size
torch.manual_seed(0)
model = F.MODEL_REGISTRY[f"frostnet_quant_{args.mode}_1_0"](drop_rate=0.2)
F.qat_prepare(model, version=0)
model.cuda().train()
opt = QSGD(H.make_param_groups(model, 1e-5), lr=1e-3, momentum=0.9, nesterov=True)
crit = H.CrossEntropyLoss()
g = torch.Generator().manual_seed(1)
x, t = torch.randn(B, 3, size, size, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda()
H.train_one_iter(model, crit, opt, x, t)                     # bound, observed
ema = ModelEma(model, decay=0.9999)
ema.bind_shadow()
ema.update(model)
plan = ema._plan
shape = plan["shape"]
units = [2 * n if k == L.EMA_COPY8 else n for n, k in shape]
nfloat = sum(n for n, k in shape if k == L.EMA_LERP)
say(f"weight EMA: FrostNet-{args.mode} QAT {size} x {size}, B = {B}; {torch.cuda.get_device_name(0)}")
say(f"{len(shape)} state-dict entries: {sum(1 for n, k in shape if k == L.EMA_LERP)} fp32 ({nfloat} elements, {sum(1 for n, k in shape if k == L.EMA_LERP and n == 1)} single words), "
    f"{sum(1 for n, k in shape if k != L.EMA_LERP)} copied; {sum(1 for u in units if 0 < u < 1024)} packed small entries; {plan['nwg']} workgroups, "
    f"{plan['traffic'] / 1e6:.2f} MB of traffic (3 x float bytes + 2 x integer bytes)")

# ---- (a) the update alone
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
graph = torch.cuda.CUDAGraph()
with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
        ema.launch(plan)
torch.cuda.current_stream().wait_stream(side)


def sub_launch(keep):
    wg, nwg = build_map([u if keep(u) else 0 for u in units])
    wg = torch.from_numpy(wg).cuda()
    return lambda: L.call("frost_ema_update", L.ptr(plan["table"]), plan["nentries"], L.ptr(wg), nwg, L.ptr(ema._w), L.stream()), nwg


large_fn, nwg_large = sub_launch(lambda u: u >= 1024)
small_fn, nwg_small = sub_launch(lambda u: u < 1024)

# ---- (b) the stock loop
live_m = [d[n] for _, d, n, _ in _walk(model)]
live_e = [d[n] for _, d, n, _ in _walk(ema.module)]
fl = [(e, m) for e, m in zip(live_e, live_m) if e.is_floating_point()]
rest = [(e, m) for e, m in zip(live_e, live_m) if not e.is_floating_point()]
fe, fm = [e for e, _ in fl], [m.detach() for _, m in fl]


@torch.no_grad()
def stock_state_dict():
    # (on a bound model state_dict() returns clones of the aliased buffers: this form reads the model and averages into copies -- it costs what it costs, it is not a working EMA)
    for ev, mv in zip(ema.module.state_dict().values(), model.state_dict().values()):
        if ev.is_floating_point():
            ev.lerp_(mv, 1e-4)
        else:
            ev.copy_(mv)


@torch.no_grad()
def stock_foreach():
    torch._foreach_lerp_(fe, fm, 1e-4)
    for e, m in rest:
        e.copy_(m)


legs = {"eager": lambda: ema.update(model), "launch": lambda: ema.launch(plan), "replay": lambda: (ema.prepare_step(model), graph.replay()),
        "large": large_fn, "small": small_fn}
for fn in list(legs.values()) + [stock_state_dict, stock_foreach]:
    fn()
ts = {k: [] for k in legs}
host, w_sd, w_fe = [], [], []
for _ in range(args.reps):
    for k, fn in legs.items():
        ts[k].append(once(fn))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ema.update(model)
    host.append((time.perf_counter() - t0) * 1e6)
    w_sd.append(wall(stock_state_dict))
    w_fe.append(wall(stock_foreach))
med = {k: float(np.median(v)) * 1e3 for k, v in ts.items()}          # us
rate = plan["traffic"] / (med["launch"] * 1e-6)
say(f"median of {args.reps} interleaved rounds")
say(f"(a) ema.update, eager (prepare_step + launch)      {med['eager']:9.1f} us on the device (HIP events), {np.median(host):9.1f} us of host time per call")
say(f"(a) the launch alone                               {med['launch']:9.1f} us   {rate / 1e9:8.1f} GB/s = {rate / COPY_RATE:.3f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
say(f"(a) prepare_step + replay of the captured launch   {med['replay']:9.1f} us")
say(f"    large-entry rows alone ({nwg_large} workgroups)          {med['large']:9.1f} us;  packed small entries alone ({nwg_small} workgroups) {med['small']:9.1f} us")
say(f"(b) stock loop through state_dict()                {np.median(w_sd) * 1e3:9.1f} us wall clock (drained stream)   {np.median(w_sd) * 1e3 / med['eager']:.0f} x the eager update")
say(f"(b) stock loop, _foreach_lerp_ + copy_ per tensor  {np.median(w_fe) * 1e3:9.1f} us wall clock (drained stream)   {np.median(w_fe) * 1e3 / med['eager']:.0f} x the eager update")

# ---- (c) the graphed iteration with and without the average
plain, with_ema = H.GraphedStep(model, crit, opt), H.GraphedStep(model, crit, opt, ema=ema)


def run(step):
    def fn():
        for _ in range(args.iters):
            step(x, t)
    return fn


for s in (plain, with_ema):
    for _ in range(4):
        s(x, t)
    assert s.captures == 1 and s.graph_for(x, t) is not None
a, b = [], []
for _ in range(args.repeats):
    a.append(wall(run(plain), args.iters))
    b.append(wall(run(with_ema), args.iters))
say(f"(c) GraphedStep without ema   " + "  ".join(f"{v:8.3f}" for v in a) + f"   ms / iteration (median {np.median(a):.3f})")
say(f"(c) GraphedStep with ema=     " + "  ".join(f"{v:8.3f}" for v in b) + f"   ms / iteration (median {np.median(b):.3f})")
say(f"    the average adds {(np.median(b) - np.median(a)) * 1e3:.1f} us = {(np.median(b) / np.median(a) - 1) * 100:.2f} % per iteration; spread of the repeats "
    f"{max(max(a) - min(a), max(b) - min(b)) * 1e3:.1f} us")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

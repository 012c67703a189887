"""dev: what histogram calibration costs on one MI355X (FrostNet at 224 x 224, B = 256), HIP-event timed, legs interleaved round by round in one process, median of --reps:
  (a) the calibration forward of the PTQ-prepared model (fused fp32 network + one HistogramObserver update per activation site), eager
  (b) the same forward as one replayed hipGraph (every replay is the next calibration batch)
  (c) the fp32 float eval forward alone (FloatRunner, precision 'fp32') on the same weights: what the observers add is (a) - (c) / (b) - (c)
  (d) the observe entry alone on a tensor of the largest site's size: Gaussian values and post-ReLU values (about half of the elements in one bin), side by side, in GB/s
      of tensor bytes (the entry reads the tensor twice: range pass, count pass) and as a fraction of the copy rate this project quotes as achievable (6.29 TB/s)
  (e) the same calibration in stock torch on --threads host threads at --cpu-batch, wall clock

    python tools/bench_ptq.py [--batch 256] [--reps 20] [--mode large] [--out profiles/ptq_b256.txt]
"""
import argparse, copy, os, sys, time, warnings
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
from frostnet_amd import frostnet as F, _lib as L, ptq as P

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--mode", default="large")
ap.add_argument("--backend", default="qnnpack")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--cpu-batch", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_ptq: no GPU (a timing needs the device; there is no fallback)")
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


B, size = args.batch, args.size
torch.manual_seed(0)
base = F.MODEL_REGISTRY[f"frostnet_quant_{args.mode}_1_0"]().eval()
flt = copy.deepcopy(base)
flt.float_precision = "fp32"
flt.cuda().eval()
cal = F.ptq_prepare(copy.deepcopy(base), args.backend).cuda()
cal_g = F.ptq_prepare(copy.deepcopy(base), args.backend).cuda()
x = torch.randn(B, 3, size, size, device="cuda")
with torch.no_grad():
    for _ in range(2):
        flt(x), cal(x), cal_g(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cal_g(x)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()

    run = cal.hip_runner()
    sites = len(run._obs)
    # the largest activation site: the widest tensor any observer of the network sees at this batch
    seen, inner = [x.numel()], run._observe
    run._observe = lambda buf, numel, site: (seen.append(numel), inner(buf, numel, site))[1]
    cal(x)
    del run._observe
    n = max(seen)
    gauss = torch.randn(n, device="cuda")
    relu = torch.relu(torch.randn(n, device="cuda"))
    t = torch.zeros(P.ARENA_HDR + 2 * P.SITE_WORDS, dtype=torch.float32, device="cuda")
    s_g, s_r = t[P.ARENA_HDR: P.ARENA_HDR + P.SITE_WORDS], t[P.ARENA_HDR + P.SITE_WORDS:]
    for s in (s_g, s_r):
        s[0], s[1], s[2], s[3] = float("inf"), float("-inf"), float("inf"), float("-inf")
    obs = lambda v, s: L.call("frost_ptq_observe", L.ptr(v), n, L.ptr(s), L.ptr(t), L.stream())
    for _ in range(2):
        obs(gauss, s_g), obs(relu, s_r)
    legs = {"a": lambda: cal(x), "b": graph.replay, "c": lambda: flt(x), "dg": lambda: obs(gauss, s_g), "dr": lambda: obs(relu, s_r)}
    ts = {k: [] for k in legs}
    for _ in range(args.reps):          # interleaved: one call of every leg per round, so that clock and thermal drift hit all of them alike
        for k, fn in legs.items():
            ts[k].append(once(fn))
ts = {k: np.asarray(v) for k, v in ts.items()}
med = {k: float(np.median(v)) for k, v in ts.items()}

say(f"post-training quantisation, histogram calibration: FrostNet-{args.mode} {size} x {size}, B = {B}, '{args.backend}' qconfig, {sites} observed sites; {torch.cuda.get_device_name(0)}")
say(f"median (min) of {args.reps} interleaved rounds, HIP events")
say(f"(a) calibration forward, eager                         {med['a']:8.3f} ({ts['a'].min():8.3f}) ms   {B / med['a']:8.2f} k img/s")
say(f"(b) calibration forward, one replayed hipGraph         {med['b']:8.3f} ({ts['b'].min():8.3f}) ms   {B / med['b']:8.2f} k img/s")
say(f"(c) fp32 float eval forward alone (FloatRunner)        {med['c']:8.3f} ({ts['c'].min():8.3f}) ms   {B / med['c']:8.2f} k img/s   "
    f"observers add {med['a'] - med['c']:.3f} ms eager / {med['b'] - med['c']:.3f} ms graphed")
for k, name in (("dg", "Gaussian "), ("dr", "post-ReLU")):
    rate = 4.0 * n / (med[k] * 1e-3)
    say(f"(d) observe entry alone, {name}, {n} elements ({4 * n / 1e6:.1f} MB)   {med[k] * 1e3:8.1f} ({ts[k].min() * 1e3:8.1f}) us   {rate / 1e9:8.1f} GB/s of tensor bytes = "
        f"{rate / COPY_RATE:.3f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate (two reads of the tensor: {2 * rate / COPY_RATE:.3f})")

# (e) the stock flow on the host
torch.set_num_threads(args.threads)
cpu = F.ptq_prepare(copy.deepcopy(base), args.backend)
xc = x[: args.cpu_batch].cpu()
with torch.no_grad():
    cpu(xc)
    best = 1e30
    for _ in range(2):
        t0 = time.perf_counter()
        cpu(xc)
        best = min(best, time.perf_counter() - t0)
say(f"(e) the same calibration in stock torch, {args.threads} host threads, B = {args.cpu_batch}   {best * 1e3:8.1f} ms (best of 2)   {args.cpu_batch / best:8.1f} img/s   "
    f"the device (b) is {B / med['b'] * 1e3 / (args.cpu_batch / best):.0f} x faster")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

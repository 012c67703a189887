"""dev: what a deployed float SSDLite-FrostNet spends per batch at config c5's size (Large, 21 classes, B = 32, 512 x 512, eval), three ways in ONE process,
interleaved round by round so that drift of the machine hits all of them alike:
  (a) the eval-mode forward through the training executor + Detect:  model.detect(x)  (FloatSSDRunner, bf16: the only path before the inference kernels)
  (b) model.hip_detect_bf16(x), eager (fused bottleneck kernels, one head launch per source, Detect)
  (c) the same call replayed as one hipGraph
and, on the six source maps of that forward, the prediction heads alone: six frost_infer_head launches against the layer launches they replace (twelve
frost_infer_dw + frost_infer_pw pairs, with and without the fp32 placement of their bf16 maps).  HIP-event timed windows of --iters calls; median and minimum
of the per-call time over --rounds windows.  Launch counts come from _lib.CALL_LOG.

    python tools/bench_detect_infer.py [--batch 32] [--res 512] [--mode large] [--rounds 7] [--iters 10] [--out FILE]
"""
import argparse, collections, os, sys, warnings
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge
if not os.path.exists(ge.LIB):
    ge.build()
from frostnet_amd import _lib as L, infer as I, ssdlite as S

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--mode", default="large")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_detect_infer: no GPU (a timing needs the device; there is no fallback)")

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.iters


def interleaved(legs):
    """legs: [(name, fn)] -> {name: (median ms, min ms)}; every round times every leg once, in turn."""
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = collections.defaultdict(list)
    for _ in range(args.rounds):
        for name, fn in legs:
            ts[name].append(window_ms(fn))
    return {k: (float(np.median(v)), float(min(v))) for k, v in ts.items()}


def launches(fn):
    L.CALL_LOG = []
    try:
        fn()
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    return log


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


B = args.batch
torch.manual_seed(0)
cfg = S.ssd_cfg_for(args.res)
model = S.SSDLiteFrostNet(num_classes=21, mode=args.mode, cfg=cfg)
g = torch.Generator().manual_seed(1)
for m in model.modules():          # BatchNorm statistics as after training rather than the unit initialisation (timing does not depend on them; the comparison of outputs does)
    if isinstance(m, torch.nn.BatchNorm2d):
        m.weight.data = torch.rand(m.num_features, generator=g) * 0.8 + 0.6
        m.bias.data = torch.rand(m.num_features, generator=g) * 0.2 - 0.1
        m.running_mean.data = torch.randn(m.num_features, generator=g) * 0.1
        m.running_var.data = torch.rand(m.num_features, generator=g) * 0.5 + 0.5
model.cuda().eval()
x = torch.randn(B, 3, args.res, args.res, device="cuda")
say(f"SSDLite-FrostNet-{args.mode}, {model.num_classes} classes, B = {B}, {args.res} x {args.res}, eval, float model; {model.priors.shape[0]} priors; "
    f"{args.rounds} interleaved rounds of {args.iters} calls, median (min) ms per call; device {torch.cuda.get_device_name(0)}")

with torch.no_grad():
    # first calls: the float runner binds, the inference runner measures its per-bottleneck choices and folds the weights
    ploc, pconf, _ = model(x)
    iloc, iconf, _ = model.hip_infer_bf16(x)
    want = model.hip_detect_bf16(x).clone()
    say(f"outputs, hip_infer_bf16 against model(x) (both bf16 activations, norm-wise): loc {rel(iloc, ploc):.3e}  conf {rel(iconf, pconf):.3e}")
    log_a = launches(lambda: model.detect(x))
    log_b = launches(lambda: model.hip_detect_bf16(x))
    static = x.clone()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.hip_detect_bf16(static)
        with torch.cuda.graph(graph, stream=side):
            gout = model.hip_detect_bf16(static)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    say(f"graph replay equals the eager call: {bool(torch.equal(gout, want))}")
    res = interleaved([("a", lambda: model.detect(x)), ("b", lambda: model.hip_detect_bf16(x)), ("c", graph.replay)])

    run = model.__dict__["_bf16_infer"]
    sources = run._sources(x)

    def heads_layers(place):
        old = I._HEAD_FUSED
        I._HEAD_FUSED = False
        try:
            if place:
                return run._heads(sources, B)
            for (a, c, h, w), (ldw, lpw, cdw, cpw) in zip(sources, run.heads):
                for dw, pw in ((ldw, lpw), (cdw, cpw)):
                    run._pw(pw, run._dw(dw, a, B, h, w)[0], B * h * w, c)
        finally:
            I._HEAD_FUSED = old

    log_h = launches(lambda: run._heads(sources, B))
    log_l = launches(lambda: heads_layers(True))
    hres = interleaved([("fused", lambda: run._heads(sources, B)), ("layers", lambda: heads_layers(False)), ("layers+place", lambda: heads_layers(True))])


def count(log):
    c = collections.Counter(log)
    return f"{len(log)} launches (" + ", ".join(f"{v} {k}" for k, v in sorted(c.items(), key=lambda t: -t[1])) + ")"


say()
say("whole call -> detections [N, 21, 200, 5]")
say(f"  (a) model.detect(x): FloatSSDRunner + Detect      {res['a'][0]:8.3f} ({res['a'][1]:.3f}) ms   {B / res['a'][0] * 1e3:9.0f} img/s")
say(f"  (b) hip_detect_bf16(x), eager                     {res['b'][0]:8.3f} ({res['b'][1]:.3f}) ms   {B / res['b'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['b'][0]:.2f}x of (a)")
say(f"  (c) hip_detect_bf16 as one replayed hipGraph      {res['c'][0]:8.3f} ({res['c'][1]:.3f}) ms   {B / res['c'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['c'][0]:.2f}x of (a)")
say(f"  C-ABI launches of (a): {count(log_a)}")
say(f"  C-ABI launches of (b): {count(log_b)}")
say()
say("prediction heads alone, on the six source maps " + ", ".join(f"{h}x{w}x{c}" for _, c, h, w in sources))
say(f"  six frost_infer_head (fp32 loc / conf in place)   {hres['fused'][0]:8.3f} ({hres['fused'][1]:.3f}) ms   {count(log_h)}")
say(f"  twelve dw + pw pairs, bf16 maps only              {hres['layers'][0]:8.3f} ({hres['layers'][1]:.3f}) ms")
say(f"  twelve dw + pw pairs + fp32 placement             {hres['layers+place'][0]:8.3f} ({hres['layers+place'][1]:.3f}) ms   {count(log_l)} + the placement copies")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

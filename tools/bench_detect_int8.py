"""dev: what a deployed CONVERTED (int8) SSDLite-FrostNet spends per batch at config c5's size (Large, 21 classes, B = 32, 512 x 512), in ONE process, interleaved
round by round so that drift of the machine hits all legs alike:
  (a) model.detect(x): the twelve-map form (24 head layer launches, 12 frost_dequant_act, NCHW copies, _assemble's permute / slice / cat) + Detect -- the only path
      before hip_detect_int8
  (b) model.hip_detect_int8(x), eager, heads as the default picks them per source (runner._CVT_HEAD_LAYERWISE), fp32 loc / conf written in place, Detect
  (c) the same call replayed as one hipGraph
  (d) as (c) with FROST_CVT_HEAD=1: one fused head launch for EVERY source
  (e) as (c) with FROST_CVT_HEAD=0: head layer launches + frost_cvt_place for every source
and, per source map of that forward, the prediction heads alone: ONE frost_cvt_head launch against four conv_converted launches + two frost_cvt_place, each captured
--reps times into a hipGraph (device time without the host's launch cost, as inside (c)).  HIP-event timed windows of --iters calls; median and minimum of the
per-call time over --rounds windows.  Launch counts come from _lib.CALL_LOG.  Outputs of (a) and (b) are compared bit for bit.

    python tools/bench_detect_int8.py [--batch 32] [--res 512] [--mode large] [--backend qnnpack] [--rounds 7] [--iters 10] [--reps 20] [--out FILE]
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
from frostnet_amd import _lib as L, frostnet as F, infer as I, runner as R, ssdlite as S

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--mode", default="large")
ap.add_argument("--backend", default="qnnpack")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_detect_int8: no GPU (a timing needs the device; there is no fallback)")

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


def count(log):
    c = collections.Counter(log)
    return f"{len(log)} launches (" + ", ".join(f"{v} {k}" for k, v in sorted(c.items(), key=lambda t: -t[1])) + ")"


def captured(fn):
    """fn recorded into a hipGraph on a side stream after one warm-up call there; returns (graph, what fn returned during capture)."""
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph, out


def with_heads(mode, fn):
    def run():
        old = R._CVT_HEAD
        R._CVT_HEAD = mode
        try:
            return fn()
        finally:
            R._CVT_HEAD = old
    return run


B = args.batch
torch.manual_seed(0)
cfg = S.ssd_cfg_for(args.res)
model = S.SSDLiteFrostNet(num_classes=21, mode=args.mode, cfg=cfg)
F.qat_prepare(model, version=0, **({"backend": "fbgemm"} if args.backend == "fbgemm" else {}))
model.cuda().train()
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for _ in range(3):              # calibration: BatchNorm statistics and observers move (train-mode forwards), as in tests/test_gpu_convert.py
        model(torch.randn(max(2, B // 4), 3, args.res, args.res, generator=g).cuda())
model.hip_convert()
x = torch.randn(B, 3, args.res, args.res, device="cuda")
say(f"SSDLite-FrostNet-{args.mode}, {model.num_classes} classes, B = {B}, {args.res} x {args.res}, QAT-prepared ({args.backend}), calibrated and hip_convert()-ed; "
    f"{model.priors.shape[0]} priors; {args.rounds} interleaved rounds of {args.iters} calls, median (min) ms per call; device {torch.cuda.get_device_name(0)}")

with torch.no_grad():
    ploc, pconf, _ = model(x)
    iloc, iconf, _ = model.hip_infer_int8(x)
    say(f"hip_infer_int8(x) equals model(x) bit for bit: loc {bool(torch.equal(iloc, ploc))}  conf {bool(torch.equal(iconf, pconf))}")
    want = model.detect(x).clone()
    got = model.hip_detect_int8(x).clone()
    say(f"hip_detect_int8(x) equals model.detect(x) bit for bit: {bool(torch.equal(got, want))}")
    log_a = launches(lambda: model.detect(x))
    log_b = launches(with_heads("auto", lambda: model.hip_detect_int8(x)))
    log_d = launches(with_heads("1", lambda: model.hip_detect_int8(x)))
    log_e = launches(with_heads("0", lambda: model.hip_detect_int8(x)))
    static = x.clone()
    graph_c, out_c = captured(with_heads("auto", lambda: model.hip_detect_int8(static)))
    graph_d, out_d = captured(with_heads("1", lambda: model.hip_detect_int8(static)))
    graph_e, out_e = captured(with_heads("0", lambda: model.hip_detect_int8(static)))
    graph_c.replay(); graph_d.replay(); graph_e.replay()
    torch.cuda.synchronize()
    say(f"graph replays equal the eager call: default {bool(torch.equal(out_c, want))}  fused heads everywhere {bool(torch.equal(out_d, want))}  "
        f"layer launches + placement everywhere {bool(torch.equal(out_e, want))}")
    res = interleaved([("a", lambda: model.detect(x)), ("b", with_heads("auto", lambda: model.hip_detect_int8(x))), ("c", graph_c.replay), ("d", graph_d.replay),
                       ("e", graph_e.replay)])

    # ---- the heads alone, per source
    run = model.hip_runner()
    sources = run._sources_converted(x)
    run.E.tape = []
    anchors, C = list(model.ANCHORS), model.num_classes
    offs = I.ssd_head_offsets(anchors, [(s.h, s.w) for s in sources])
    P = offs[-1] + sources[-1].h * sources[-1].w * anchors[-1]
    loc = torch.empty(B, P, 4, device="cuda")
    conf = torch.empty(B, P, C, device="cuda")

    def heads(mode, ks):
        def fn():
            for _ in range(args.reps):
                for k in ks:
                    run._head_converted(k, sources[k], run.heads[k], loc, conf, offs[k], P)
            run.E.tape = []
        return with_heads(mode, fn)

    per = []
    for k in range(len(sources)):
        gf, _ = captured(heads("1", [k]))
        gl, _ = captured(heads("0", [k]))
        r_ = interleaved([("fused", gf.replay), ("layers", gl.replay)])
        per.append({n: (v[0] / args.reps, v[1] / args.reps) for n, v in r_.items()})
    gf, _ = captured(heads("1", range(len(sources))))
    gl, _ = captured(heads("0", range(len(sources))))
    allres = {n: (v[0] / args.reps, v[1] / args.reps) for n, v in interleaved([("fused", gf.replay), ("layers", gl.replay)]).items()}
    log_hf = launches(with_heads("1", lambda: [run._head_converted(k, sources[k], run.heads[k], loc, conf, offs[k], P) for k in range(len(sources))]))
    log_hl = launches(with_heads("0", lambda: [run._head_converted(k, sources[k], run.heads[k], loc, conf, offs[k], P) for k in range(len(sources))]))
    run.E.tape = []

say()
say("whole call -> detections [N, 21, 200, 5]")
say(f"  (a) model.detect(x): twelve maps + _assemble + Detect        {res['a'][0]:8.3f} ({res['a'][1]:.3f}) ms   {B / res['a'][0] * 1e3:9.0f} img/s")
say(f"  default heads: sources {sorted(R._CVT_HEAD_LAYERWISE)} as layer launches + frost_cvt_place, the others as one frost_cvt_head launch")
say(f"  (b) hip_detect_int8(x), eager                                {res['b'][0]:8.3f} ({res['b'][1]:.3f}) ms   {B / res['b'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['b'][0]:.2f}x of (a)")
say(f"  (c) hip_detect_int8 as one replayed hipGraph                 {res['c'][0]:8.3f} ({res['c'][1]:.3f}) ms   {B / res['c'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['c'][0]:.2f}x of (a)")
say(f"  (d) as (c), one fused head launch for every source           {res['d'][0]:8.3f} ({res['d'][1]:.3f}) ms   {B / res['d'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['d'][0]:.2f}x of (a)")
say(f"  (e) as (c), layer launches + frost_cvt_place everywhere      {res['e'][0]:8.3f} ({res['e'][1]:.3f}) ms   {B / res['e'][0] * 1e3:9.0f} img/s   {res['a'][0] / res['e'][0]:.2f}x of (a)")
say(f"  C-ABI launches of (a): {count(log_a)}; torch adds 12 NCHW copies, 12 reshape copies and 2 cats")
say(f"  C-ABI launches of (b), (c): {count(log_b)}")
say(f"  C-ABI launches of (d): {count(log_d)}")
say(f"  C-ABI launches of (e): {count(log_e)}")
say()
say(f"prediction heads alone, replayed from a hipGraph of {args.reps} repetitions, ms per repetition (fused = one frost_cvt_head; layers = 4 conv launches + 2 frost_cvt_place)")
for k, (s, r_) in enumerate(zip(sources, per)):
    say(f"  source {k}  {s.h:3d} x {s.w:3d} x {s.c:4d}   fused {r_['fused'][0]:8.4f} ({r_['fused'][1]:.4f})   layers + placement {r_['layers'][0]:8.4f} ({r_['layers'][1]:.4f})   "
        f"{r_['layers'][0] / r_['fused'][0]:.2f}x")
say(f"  all six sources          fused {allres['fused'][0]:8.4f} ({allres['fused'][1]:.4f})   layers + placement {allres['layers'][0]:8.4f} ({allres['layers'][1]:.4f})   "
    f"{allres['layers'][0] / allres['fused'][0]:.2f}x")
say(f"  launches, fused: {count(log_hf)}")
say(f"  launches, layers + placement: {count(log_hl)}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""Post-training quantisation on the device (frostnet_amd/ptq.py, csrc/frost_ptq.hip): the observe kernels against stock HistogramObserver, the calibration
forward, hip_convert() of a calibrated model against stock torch's convert on both CPU engines, graph capture and the refusals."""
import copy
import io
import warnings

import numpy as np
import pytest
import torch
from torch.ao.quantization import HistogramObserver

from test_cpu_ptq import SEQUENCES, make_sequence, stock_states

gpu = pytest.mark.gpu
NAME, RES, BATCH = "frostnet_quant_small_0_35", 64, 4


def _build():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import frostnet, ptq, _lib
    return frostnet, ptq, _lib


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=g) * 0.8 + 0.6
            m.bias.data = torch.rand(m.num_features, generator=g) * 0.2 - 0.1
            m.running_mean.data = torch.randn(m.num_features, generator=g) * 0.1
            m.running_var.data = torch.rand(m.num_features, generator=g) * 0.5 + 0.5


def _float_model(seed=11):
    from frostnet_amd import frostnet as F
    torch.manual_seed(seed)
    m = F.MODEL_REGISTRY[NAME]()
    _randomize_bn(m, 3)
    return m.eval()


def _prepared_pair(backend, seed=11):
    """A PTQ-prepared model on the CPU (fixed seed); deepcopy it for the stock side, .cuda() it for the device: both hold the same folded weights."""
    from frostnet_amd import frostnet as F
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return F.ptq_prepare(_float_model(seed), backend)


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(BATCH, 3, RES, RES, generator=g) * (1.0 + 0.25 * i) for i in range(n)]


def _observers(m):
    return {n: mod for n, mod in m.named_modules() if isinstance(mod, HistogramObserver)}


def _site_scales(m):
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n, o in _observers(m).items():
            ref = HistogramObserver(reduce_range=o.reduce_range)           # the stock search in fp32 arithmetic of its own, on a copy of the state
            ref.min_val, ref.max_val, ref.histogram = o.min_val.detach().cpu().clone(), o.max_val.detach().cpu().clone(), o.histogram.detach().cpu().clone()
            out[n] = float(ref.calculate_qparams()[0].reshape(-1)[0])
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).reshape(-1).view(np.uint32), np.asarray(b, dtype=np.float32).reshape(-1).view(np.uint32))


class _Site:
    """One observer site in device memory, driven through the C entries directly."""

    def __init__(self):
        _, self.ptq, self.L = _build()
        self.t = torch.zeros(self.ptq.ARENA_HDR + self.ptq.SITE_WORDS, dtype=torch.float32, device="cuda")
        self.site = self.t[self.ptq.ARENA_HDR:]
        self.site[0], self.site[1], self.site[2], self.site[3] = float("inf"), float("-inf"), float("inf"), float("-inf")
        assert self.L.load_library().frost_ptq_site_words() == self.ptq.SITE_WORDS

    def observe(self, x):
        L = self.L
        L.call("frost_ptq_observe", L.ptr(x), x.numel(), L.ptr(self.site), L.ptr(self.t), L.stream())

    def observe_strided(self, x):
        L = self.L
        L.call("frost_ptq_observe_strided", L.ptr(x), *x.shape, *x.stride(), L.ptr(self.site), L.ptr(self.t), L.stream())

    def state(self):
        h = self.site.cpu()
        H = self.ptq.HDR
        # the scratch words are re-armed after every call
        assert h[2] == float("inf") and h[3] == float("-inf") and int(h[H + 2048:].view(torch.int32).abs().sum()) == 0
        return h[0].numpy(), h[1].numpy(), h[H: H + 2048].numpy()

    def check(self, stock, tag):
        mn, mx, hist = self.state()
        assert _same_bits(mn, stock[0].numpy()) and _same_bits(mx, stock[1].numpy()), (tag, mn, mx, stock[0], stock[1])
        ref = stock[2].numpy()
        bad = np.flatnonzero(hist.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (tag, bad.size, bad[:6], hist[bad[:6]], ref[bad[:6]])
        assert int(self.t[:1].view(torch.int32)[0]) == 0


@gpu
@pytest.mark.parametrize("kind,seed", SEQUENCES)
def test_observe_kernel_bit_equal_to_stock_observer(kind, seed):
    xs = make_sequence(kind, seed)
    s = _Site()
    for i, (x, st) in enumerate(zip(xs, stock_states(xs))):
        s.observe(x.cuda())
        s.check(st, (kind, seed, i))


@gpu
def test_observe_kernel_many_workgroups_and_tail():
    """A 2^20 + 3 element tensor (more workgroups than the launch cap keeps busy at once, a scalar tail) between two small ones; also through an unaligned pointer."""
    xs = make_sequence("relu", 7, sizes=[5000, 2 ** 20 + 3, 30001])
    s, s2 = _Site(), _Site()
    for i, (x, st) in enumerate(zip(xs, stock_states(xs, reduce_range=True))):
        s.observe(x.cuda())
        s.check(st, ("big", i))
        pad = torch.cat([torch.full((1,), 1e9), x]).cuda()
        s2.observe(pad[1:])                                   # 4-byte aligned only: the scalar path
        s2.check(st, ("unaligned", i))


@gpu
def test_observe_kernel_strided_entry():
    g = torch.Generator().manual_seed(3)
    base = [torch.randn(3, 5, 40, 37, generator=g) * (1 + i) + 0.3 * i for i in range(3)]
    # a strided NCHW window, a transposed one, a channel slice of a channels_last tensor (channel stride 1, not dense)
    views = [lambda t: t[:, 1:4, ::2, 3:30], lambda t: t.permute(0, 1, 3, 2)[:, :3, 1:, :], lambda t: t.contiguous(memory_format=torch.channels_last)[:, 1:4]]
    xs = [v(b) for v, b in zip(views, base)]
    s = _Site()
    for i, (x, st) in enumerate(zip(xs, stock_states([x.contiguous() for x in xs]))):
        d = views[i](base[i].cuda())
        assert d.stride() == x.stride() and not d.is_contiguous()
        s.observe_strided(d)
        s.check(st, ("strided", i))


@gpu
def test_calibration_forward_logits_and_observer_state():
    """frostnet_quant_small_0_35 at 64^2, B = 4: fp32 logits against the stock fused float model on the CPU at the fp32 mode's tolerance of tests/test_gpu_float.py
    (3e-5 norm-wise against the fp64 evaluation of the stock modules); every site's range finite and its histogram summing to the site's element count."""
    F, ptq, _ = _build()
    from frostnet_amd import harness
    fused = _float_model()
    fused.fuse_model()
    ref64 = copy.deepcopy(fused).double()
    model = _prepared_pair("qnnpack").cuda()
    assert model._is_ptq_prepared()
    x = _batches(1)[0]
    counts = {}
    cpu = _prepared_pair("qnnpack")
    hooks = [mod.register_forward_hook(lambda m, i, o, n=n: counts.__setitem__(n, o.numel())) for n, mod in _observers(cpu).items()]
    with torch.no_grad():
        y_ref64, y_ref32 = ref64(x.double()), fused(x)
        cpu(x)
        y = model(x.cuda())
    for h in hooks:
        h.remove()
    assert y.dtype == torch.float32 and y.shape == (BATCH, 1000)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    e64, e32 = rel(y.cpu(), y_ref64), rel(y.cpu(), y_ref32)
    print(f"[ptq calibration forward] logits vs stock fused model: fp64 {e64:.1e}, fp32 {e32:.1e}")
    assert e64 <= 3e-5 and e32 <= 3e-5, (e64, e32)
    obs = _observers(model)
    assert set(counts) <= set(obs) and len(counts) > 40
    arena = model.hip_runner().qa.t
    for n, o in obs.items():
        if n not in counts:          # the FloatFunctional of a block that neither cats nor adds: no data on either side
            assert float(o.min_val) == float("inf") and float(o.max_val) == float("-inf") and "conv" not in n.rsplit(".", 2)[-2], n
            continue
        assert o.histogram.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr(), n          # aliased onto the arena
        assert torch.isfinite(o.min_val) and torch.isfinite(o.max_val) and float(o.min_val) <= float(o.max_val), n
        assert float(o.histogram.double().sum()) == counts[n], (n, float(o.histogram.double().sum()), counts[n])
    # state_dict / torch.save / deepcopy of the bound model, and harness.calibrate
    sd = model.state_dict()
    k = "layer2.0.conv1.conv.0.activation_post_process.histogram"
    assert sd[k].untyped_storage().data_ptr() != arena.untyped_storage().data_ptr() and torch.equal(sd[k], obs[k.rsplit(".", 1)[0]].histogram)
    buf = io.BytesIO()
    torch.save(sd, buf)
    assert buf.tell() < 4 * sum(v.numel() for v in sd.values() if torch.is_tensor(v)) + (1 << 20)
    twin = copy.deepcopy(model)
    assert harness.calibrate([(b, None) for b in _batches(2, seed=9)], model) == 2
    assert harness.calibrate([(b.cuda(), None) for b in _batches(2, seed=9)], twin) == 2
    for (n, a), (_, b) in zip(_observers(model).items(), _observers(twin).items()):
        assert torch.equal(a.histogram, b.histogram) and torch.equal(a.min_val, b.min_val) and torch.equal(a.max_val, b.max_val), n


@gpu
@pytest.mark.parametrize("backend", ["qnnpack", "fbgemm"])
def test_teacher_forced_flow_is_bit_exact_against_stock_convert(backend):
    """Prepare on the CPU, move to the device, calibrate on 3 batches, hip_convert(), hip_export_converted(): the stock CPU model that ran convert() after its own
    calibration on the same batches holds the same int8 weights, weight scales and biases; with the exported dict loaded (strict) its logits equal the device's."""
    F, ptq, _ = _build()
    prev = torch.backends.quantized.engine
    torch.backends.quantized.engine = backend
    try:
        cpu = _prepared_pair(backend)
        model = copy.deepcopy(cpu).cuda()
        xs = _batches(3)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for x in xs:
                cpu(x)
                model(x.cuda())
            assert model.hip_convert() is model
            exported = model.hip_export_converted()
            ref = torch.quantization.convert(cpu, inplace=False)
            y_dev = model(xs[0].cuda()).cpu()
            assert torch.equal(model(xs[0].cuda()).cpu(), y_dev)
        sd = ref.state_dict()
        assert sorted(sd.keys()) == sorted(exported.keys())
        nw = 0
        for k, v in sd.items():
            if k.endswith(".weight"):
                w = exported[k]
                assert torch.equal(w.int_repr(), v.int_repr()), k
                if backend == "fbgemm":
                    assert torch.equal(w.q_per_channel_scales(), v.q_per_channel_scales()) and torch.equal(w.q_per_channel_zero_points(), v.q_per_channel_zero_points()), k
                else:
                    assert w.q_scale() == v.q_scale() and w.q_zero_point() == v.q_zero_point() == 0, k
                nw += 1
            elif k.endswith(".bias"):
                assert torch.equal(exported[k], v), k
        assert nw > 30
        missing, unexpected = ref.load_state_dict(exported, strict=True)
        assert not missing and not unexpected
        with torch.no_grad():
            y_cpu = ref(xs[0])
        assert torch.equal(y_cpu, y_dev), float((y_cpu - y_dev).abs().max())
    finally:
        torch.backends.quantized.engine = prev


@gpu
def test_free_running_activation_qparams_close_to_cpu_calibration():
    """Activation scales, device-calibrated against CPU-calibrated, per site as |dscale| / scale.  The bound is the reference's own sensitivity: the stock flow run
    in fp64 and in fp32 on the CPU, maximum over the sites; the device, compared against the fp64 run, gets twice that maximum (two fp32 evaluations of one function
    lie within the sum of their distances to it).  Measured on one MI355X (profiles/ptq_b256.txt): CPU fp32 against fp64 4.154e-07, hence the bound 8.308e-07;
    device against fp64 3.444e-07."""
    F, ptq, _ = _build()
    cpu32 = _prepared_pair("qnnpack")
    cpu64 = copy.deepcopy(cpu32).double()
    model = copy.deepcopy(cpu32).cuda()
    with torch.no_grad():
        for x in _batches(3):
            cpu32(x)
            cpu64(x.double())
            model(x.cuda())
    s32, s64, sdev = _site_scales(cpu32), _site_scales(cpu64), _site_scales(model)
    assert s32.keys() == s64.keys() == sdev.keys()
    own = max(abs(s32[k] - s64[k]) / s64[k] for k in s64)
    dev = max(abs(sdev[k] - s64[k]) / s64[k] for k in s64)
    print(f"[ptq free-running] max |dscale|/scale over {len(s64)} sites: CPU fp32 vs fp64 {own:.3e}, device vs fp64 {dev:.3e}, bound {2 * own:.3e}")
    assert dev <= 2 * own, (dev, own)


@gpu
def test_calibration_forward_graph_capture_replays_next_batches():
    """One calibration forward captured with torch.cuda.graph and replayed on two further inputs leaves the observer state of the eager three-batch sequence."""
    F, ptq, _ = _build()
    base = _prepared_pair("fbgemm")
    eager, graphed = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    xs = [x.cuda() for x in _batches(3)]
    with torch.no_grad():
        ys = [eager(x) for x in xs]
        static = xs[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            graphed(static)                                  # batch 0, eager: binds the runner outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed(static)
        for x, y in zip(xs[1:], ys[1:]):
            static.copy_(x)
            g.replay()
            assert torch.equal(out, y)
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(_observers(eager).items(), _observers(graphed).items()):
        assert torch.equal(a.min_val, b.min_val) and torch.equal(a.max_val, b.max_val) and torch.equal(a.histogram, b.histogram), n


@gpu
def test_refusals():
    F, ptq, _ = _build()
    with pytest.raises(NotImplementedError):
        F.ptq_prepare(F.MODEL_REGISTRY[NAME](act="hswish"))
    with pytest.raises(RuntimeError, match="QAT-prepared"):
        F.MODEL_REGISTRY[NAME]().cuda().hip_convert()                      # a plain float model: as before
    model = _prepared_pair("qnnpack").cuda()
    with pytest.raises(RuntimeError, match="calibrate"):
        model.hip_convert()                                                # prepared, never calibrated
    x = _batches(1)[0].cuda()
    with torch.no_grad():
        model(x)
        with pytest.raises(RuntimeError, match="eval"):
            model.train()(x)
        model.eval()
        bad = x.clone()
        bad[1, 2, 5, 7] = float("nan")
        model(bad)
    with pytest.raises(RuntimeError, match="non-finite"):
        model.hip_convert()
    good = _prepared_pair("qnnpack").cuda()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        good(x)
        good.hip_convert()
        y = good(x)
        assert y.shape == (BATCH, 1000) and good.hip_convert() is good     # idempotent
        good.train()
        with pytest.raises(RuntimeError, match="converted"):
            good(x)
        good.eval()
        twin = copy.deepcopy(good)                                         # the frozen int8 weights stay behind: refused like a converted QAT model
        with pytest.raises(RuntimeError, match="hip_convert"):
            twin(x)

"""Post-training quantisation, CPU side: the numpy definition of one HistogramObserver update (frostnet_amd.ptq.hist_update) against stock torch,
and `ptq_prepare` against the hand-written stock flow."""
import numpy as np
import pytest
import torch
from torch.ao.quantization import HistogramObserver, convert, get_default_qconfig, prepare

from frostnet_amd import frostnet as F
from frostnet_amd import ptq

KINDS = ("relu", "shifted", "constant_first", "inside")


def make_sequence(kind, seed, sizes=None):
    """Five batches of 1 000 - 60 000 fp32 values (shared with tests/test_gpu_ptq.py)."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + seed)
    sizes = sizes or [int(torch.randint(1000, 60001, (1,), generator=g)) for _ in range(5)]
    xs = []
    for i, n in enumerate(sizes):
        z = torch.randn(n, generator=g)
        if kind == "relu":                    # post-ReLU: about half of the mass in one bin, the range grows with the batch scale
            x = torch.relu(z * (1.0 + 0.7 * i))
        elif kind == "shifted":               # Gaussians whose mean moves: the range grows on both sides
            x = z * (0.5 + 0.3 * i) + (1.5 * i - 2.0)
        elif kind == "constant_first":        # a constant history, then data
            x = torch.full((n,), 0.75) if i < 1 + seed % 2 else z * 2.0 + 0.5
        else:                                 # batches 2.. lie inside the range of the first
            x = z * 3.0 if i == 0 else torch.tanh(z) * 2.0
        xs.append(x.float().contiguous())
    return xs


SEQUENCES = [(k, s) for k in KINDS for s in range(3)]          # 12 sequences x 5 updates


def stock_states(xs, reduce_range=False):
    obs = HistogramObserver(reduce_range=reduce_range)
    out = []
    for x in xs:
        obs(x)
        out.append((obs.min_val.clone(), obs.max_val.clone(), obs.histogram.clone()))
    return out


@pytest.mark.parametrize("kind,seed", SEQUENCES)
def test_definition_equals_stock_observer(kind, seed):
    xs = make_sequence(kind, seed)
    state = ptq.hist_init()
    for i, (x, (mn, mx, hist)) in enumerate(zip(xs, stock_states(xs))):
        state = ptq.hist_update(state, x.numpy())
        assert np.float32(state[0]).tobytes() == mn.numpy().astype(np.float32).tobytes(), (kind, seed, i, "min_val")
        assert np.float32(state[1]).tobytes() == mx.numpy().astype(np.float32).tobytes(), (kind, seed, i, "max_val")
        ref = hist.numpy()
        bad = np.flatnonzero(state[2].view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (kind, seed, i, bad[:8], state[2][bad[:8]], ref[bad[:8]])


def _stock_prepare(name, backend):
    torch.manual_seed(0)
    m = F.MODEL_REGISTRY[name]()
    m.eval()
    m.fuse_model()
    m.qconfig = get_default_qconfig(backend)
    prepare(m, inplace=True)
    return m


def _observers(m):
    out = {}
    for n, mod in m.named_modules():
        if isinstance(mod, torch.ao.quantization.ObserverBase):
            out[n] = (type(mod).__name__, str(mod.dtype), str(getattr(mod, "qscheme", None)), getattr(mod, "bins", None), getattr(mod, "upsample_rate", None),
                      getattr(mod, "reduce_range", None), getattr(mod, "quant_min", None), getattr(mod, "quant_max", None))
    return out


@pytest.mark.parametrize("backend", ["qnnpack", "fbgemm"])
def test_ptq_prepare_is_the_stock_flow(backend):
    name = "frostnet_quant_small_0_35"
    ref = _stock_prepare(name, backend)
    torch.manual_seed(0)
    m = F.ptq_prepare(F.MODEL_REGISTRY[name](), backend)
    assert not m.training and m._is_ptq_prepared() and not m._is_qat_prepared()
    assert [n for n, _ in m.named_modules()] == [n for n, _ in ref.named_modules()]
    obs, obs_ref = _observers(m), _observers(ref)
    assert obs == obs_ref and len(obs) > 0
    assert all(v[0] == "HistogramObserver" and v[3] == 2048 and v[4] == 16 and v[5] == (backend == "fbgemm") for v in obs.values())
    wobs = m.qconfig.weight()
    assert type(wobs).__name__ == ("PerChannelMinMaxObserver" if backend == "fbgemm" else "MinMaxObserver")
    x = torch.randn(2, 3, 64, 64)
    prev = torch.backends.quantized.engine
    torch.backends.quantized.engine = backend
    try:
        with torch.no_grad():
            m(x), ref(x)
        keys = list(convert(m, inplace=False).state_dict().keys())
        assert keys == list(convert(ref, inplace=False).state_dict().keys())
    finally:
        torch.backends.quantized.engine = prev
    # the same sites as the QAT-prepared tree (the converted engine binds them by name)
    torch.manual_seed(0)
    q = F.qat_prepare(F.MODEL_REGISTRY[name](), backend=backend)
    sfx = ".activation_post_process"
    qat_sites = sorted(n[:-len(sfx)] for n, mod in q.named_modules()
                       if n.endswith(sfx) and n.count("activation_post_process") == 1 and "weight_fake_quant" not in n and type(mod).__name__ != "Identity")
    assert sorted(n[:-len(sfx)] for n in obs) == qat_sites


def test_ptq_prepare_refusals():
    with pytest.raises(NotImplementedError):
        F.ptq_prepare(F.frostnet_quant_small_0_35(act="hswish"))
    with pytest.raises(NotImplementedError):
        F.ptq_prepare(F.frostnet_quant_small_0_35(), backend="x86")
    from frostnet_amd import frostnet_features as FF
    feat = [v for k, v in vars(FF).items() if k.startswith("frostnet_quant_small_0_35")]
    if feat:
        with pytest.raises(NotImplementedError):
            F.ptq_prepare(feat[0]())


def test_hip_convert_on_plain_float_model_still_raises():
    with pytest.raises(RuntimeError, match="QAT-prepared"):
        F.frostnet_quant_small_0_35().hip_convert()

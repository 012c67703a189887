"""frostnet_amd.topology on the CPU: the plan of every tree the runners bind (classifier, features backbone, detector; float, QAT-prepared and PTQ-prepared)
covers each convolution exactly once, names what `named_modules()` names, does not change with the state of the tree, and the binding helpers call a
runner's callbacks in the canonical order."""
import pytest
import torch
import torch.nn as nn

from frostnet_amd import frostnet as F
from frostnet_amd import frostnet_features as FF
from frostnet_amd import ssdlite as S
from frostnet_amd import topology as T

ARCHS = {
    "quant_large": lambda: F.frostnet_quant_large_1_0(),
    "quant_base": lambda: F.frostnet_quant_base_1_0(),
    "quant_small": lambda: F.frostnet_quant_small_1_0(),
    "float_large": lambda: F.frostnet_large_1_0(),
    "features_large": lambda: FF.FrostNet(mode="large", quantized=True),
    "ssd_small": lambda: S.SSDLiteFrostNet(mode="small", cfg=S.ssd_cfg_for(128)),
    "ssd_large": lambda: S.SSDLiteFrostNet(mode="large", cfg=S.ssd_cfg_for(128)),
}
QUANT = {a for a in ARCHS if a != "float_large"}
STATES = [(a, s) for a in ARCHS for s in ("float", "qat") + (("ptq",) if a.startswith("quant_") else ())]
MEMBERS = ("squeeze_conv", "quant_cat", "conv1", "conv2", "reduce_conv", "skip_add")
_CACHE = {}


def tree(arch, state):
    """(model, plan), built once per (architecture, state) and left unchanged."""
    if (arch, state) not in _CACHE:
        m = ARCHS[arch]()
        if state == "qat":
            F.qat_prepare(m)
        elif state == "ptq":
            F.ptq_prepare(m)
        _CACHE[arch, state] = (m, T.plan_tree(m))
    return _CACHE[arch, state]


def calls(plan):
    """(kind, name, module) of every callback a runner with sites receives, in order: QuantStub, trunk, classifier, extras, heads."""
    out = []

    def layer(name, mod, kind):
        out.append((kind, name, mod))

    def site(name, mod):
        out.append(("site", name, mod))
    if plan.quant is not None:
        site("quant", plan.quant)
    T.bind_trunk(plan, layer, site)
    if plan.classifier is not None:
        layer("classifier.2", plan.classifier, "cls")
    T.bind_detector(plan, layer)
    return out


def events(plan):
    return [(kind, name) for kind, name, _ in calls(plan)]


def layers(plan):
    """Every (name, module, kind) that owns a convolution, in table order; the classifier conv is the module itself, every other entry a wrapper."""
    return [(name, mod, kind) for kind, name, mod in calls(plan) if kind != "site"]


@pytest.mark.parametrize("arch,state", STATES)
def test_every_conv_is_owned_by_exactly_one_layer(arch, state):
    model, plan = tree(arch, state)
    table = layers(plan)
    owned = []
    for name, mod, kind in table:
        convs = [c for c in mod.modules() if isinstance(c, nn.Conv2d)]
        assert len(convs) == 1, (name, len(convs))
        owned.append(id(convs[0]))
    every = [id(c) for _, c in model.named_modules() if isinstance(c, nn.Conv2d)]
    assert len(owned) == len(set(owned)) == len(every) and set(owned) == set(every), (len(owned), len(every))
    assert len({name for name, _, _ in table}) == len(table)


@pytest.mark.parametrize("arch,state", STATES)
def test_names_resolve(arch, state):
    model, plan = tree(arch, state)
    mods = dict(model.named_modules())
    for name, mod, _ in layers(plan):
        assert mods[name] is mod, name
    for b in plan.blocks:
        assert mods[b.prefix] is b.block
        for member in MEMBERS:
            if getattr(b, member) is not None:
                assert mods[f"{b.prefix}.{member}"] is getattr(b, member), (b.prefix, member)
    if plan.quant is not None:
        assert mods["quant"] is plan.quant
    assert (plan.last_layer is not None) == ("last_layer" in mods) and (plan.classifier is not None) == ("classifier.2" in mods)
    assert (len(plan.extras), len(plan.heads)) == ((3, 6) if arch.startswith("ssd") else (0, 0))
    if plan.classifier is not None:
        assert plan.drop_rate == model.classifier[1].p


@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_events_do_not_depend_on_the_state(arch):
    seqs = {s: events(tree(a, s)[1]) for a, s in STATES if a == arch}
    assert len(seqs) >= 2 and all(v == seqs["float"] for v in seqs.values()), {s: len(v) for s, v in seqs.items()}


@pytest.mark.parametrize("arch,state", STATES)
def test_stage_ends(arch, state):
    model, plan = tree(arch, state)
    ends, n = [], 0
    for stage in T.STAGES:
        n += len(getattr(model, stage))
        ends.append(n - 1)
    assert plan.stage_ends == ends and len(plan.blocks) == n
    assert [b.prefix for b in plan.blocks] == [f"{stage}.{i}" for stage in T.STAGES for i in range(len(getattr(model, stage)))]
    assert T.FEATURE_TAPS == (0, 1, 2, 4) and T.SSD_TAPS == (1, 2, 4)


@pytest.mark.parametrize("arch,state", STATES)
def test_members_follow_the_block(arch, state):
    """The block's own forward (frostnet.py:124-145) restated from its constructor arguments: a squeeze conv exists iff the block cats, the input is added
    iff the block keeps stride 1 and its width."""
    _, plan = tree(arch, state)
    full = 0
    for b in plan.blocks:
        blk = b.block
        cats = getattr(blk, "squeeze_conv", None) is not None
        adds = blk.stride == 1 and blk.in_channels == blk.out_channels
        assert (b.squeeze_conv is not None) == cats and (b.conv1 is not None) == (getattr(blk, "conv1", None) is not None), b.prefix
        assert b.conv2 is blk.conv2 and b.reduce_conv is blk.reduce_conv
        if arch in QUANT:
            assert (b.quant_cat is not None) == cats and (b.skip_add is not None) == adds, b.prefix
            full += cats and adds
        else:
            assert b.quant_cat is None and b.skip_add is None, b.prefix
    assert full > 0 or arch not in QUANT           # every quant tree has blocks that use all six members


@pytest.mark.parametrize("arch,state", STATES)
def test_binding_order(arch, state):
    _, plan = tree(arch, state)
    for b in plan.blocks:
        calls = []

        def layer(name, mod, kind):
            calls.append((name, mod, kind))
            return ("L", name)

        def site(name, mod):
            calls.append((name, mod, "site"))
            return ("S", name)
        d = T.bind_block(b, layer, site, key="mod")
        kinds = dict(squeeze_conv="pw", quant_cat="site", conv1="pw", conv2="dw", reduce_conv="pw", skip_add="site")
        want = [(f"{b.prefix}.{m}", getattr(b, m), kinds[m]) for m in MEMBERS if getattr(b, m) is not None]
        assert [(n, k) for n, _, k in calls] == [(n, k) for n, _, k in want] and all(c[1] is w[1] for c, w in zip(calls, want))
        assert set(d) == {"mod", "squeeze", "conv1", "conv2", "reduce", "q_cat", "q_add"} and d["mod"] is b.block
        got = dict(squeeze_conv=d["squeeze"], quant_cat=d["q_cat"], conv1=d["conv1"], conv2=d["conv2"], reduce_conv=d["reduce"], skip_add=d["q_add"])
        for m in MEMBERS:
            assert got[m] == (None if getattr(b, m) is None else ("S" if kinds[m] == "site" else "L", f"{b.prefix}.{m}")), (b.prefix, m)
        calls.clear()
        d = T.bind_block(b, layer)                  # a runner without sites: the float / inference dict
        assert [k for _, _, k in calls] == [k for _, _, k in want if k != "site"] and set(d) == {"blk", "squeeze", "conv1", "conv2", "reduce"}
    calls = []
    extras, heads = T.bind_detector(plan, lambda name, mod, kind: calls.append((name, kind)) or name)
    assert calls == [(f"extras.{i}.{n}", k) for i in range(len(plan.extras)) for n, k in (("pw1", "pw"), ("dw", "dw"), ("pw2", "pw"))] + \
        [(f"{h}.{i}.{n}", n) for i in range(len(plan.heads)) for h in ("loc", "conf") for n in ("dw", "pw")]
    assert all(len(e) == 3 for e in extras) and all(len(h) == 4 and h[0] == f"loc.{i}.dw" and h[3] == f"conf.{i}.pw" for i, h in enumerate(heads))


def test_conv_out_hw_and_round_up():
    for h, w, k, s in ((7, 9, 3, 1), (7, 9, 3, 2), (8, 8, 5, 2), (1, 1, 3, 2), (224, 224, 3, 2), (13, 5, 5, 1)):
        y = torch.nn.functional.conv2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, k, k), stride=s, padding=(k - 1) // 2)
        assert T.conv_out_hw(h, w, k, s) == tuple(y.shape[2:])
    assert [T.round_up(a, 16) for a in (0, 1, 16, 17)] == [0, 16, 16, 32]


@pytest.mark.parametrize("kq,dtype", [(32, torch.int16), (32, torch.uint8), (16, torch.uint8)])
def test_float_layer_geometry(kq, dtype):
    """kind / padding / pack size of the three layer kinds: 1024 bytes per (16 rows x one 64-byte K step) fragment, fp32 taps for a depthwise layer."""
    pw, dw, stem = nn.Conv2d(24, 40, 1, bias=False), nn.Conv2d(72, 72, 5, 2, 2, groups=72, bias=False), nn.Conv2d(3, 24, 3, 2, 1, bias=False)
    a, b, c = T.FloatLayer(pw, "cpu", False, kq, dtype), T.FloatLayer(dw, "cpu", False, kq, dtype), T.FloatLayer(stem, "cpu", True, kq, dtype)
    assert (a.kind, a.cout, a.cin_g, a.k, a.stride, a.cpad, a.kpad) == (0, 40, 24, 1, 1, 48, 32)
    assert (b.kind, b.cout, b.cin_g, b.k, b.stride, b.cpad, b.kpad) == (1, 72, 1, 5, 2, 80, 0)
    assert (c.kind, c.cout, c.cin_g, c.k, c.stride, c.cpad, c.kpad) == (2, 24, 3, 3, 2, 32, 64)
    assert a.pack.dtype == dtype and a.pack.numel() * a.pack.element_size() == 3 * (32 // kq) * 1024
    assert c.pack.numel() * c.pack.element_size() == 2 * (64 // kq) * 1024
    assert b.pack.dtype == torch.float32 and b.pack.numel() == 25 * 80


def test_grad_arena_and_signature():
    class Owner(T.GradArena):
        device = torch.device("cpu")
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
    params = list(m.parameters())
    o = Owner()
    o._bind_params(params)
    assert o.grad_arena.numel() == sum(p.numel() for p in params) and o.grad_arena.dtype == torch.float32
    off = 0
    for p, v, start in zip(params, o._grad_views, o._grad_offsets):
        assert start == off and v.shape == p.shape and v.data_ptr() == o.grad_arena.data_ptr() + 4 * off and o._gv[id(p)] is v
        off += p.numel()
    o.bind_grads()
    assert all(p.grad is v for p, v in zip(params, o._grad_views))
    sig = T.model_signature(m)
    assert sig == T.model_signature(m) and len(sig) == len(params) + len(list(m.buffers()))
    m[1].running_mean = torch.zeros(4)
    assert T.model_signature(m) != sig

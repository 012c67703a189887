"""Weight EMA (frostnet_amd.ema.ModelEma), host side: the C-ABI binding, the workgroup map, the reference loop against the stock loop, the decay schedule and
the checkpoint keys.  No GPU."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import frostnet_amd
    return frostnet_amd


def _qat_small(seed=0):
    from frostnet_amd import frostnet as F
    torch.manual_seed(seed)
    m = F.frostnet_quant_small_0_35(drop_rate=0.0)
    F.qat_prepare(m, version=0)
    return m


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def test_binding(built):
    from frostnet_amd import _lib as L
    assert "frost_ema_update" in built.SYMBOLS and "frost_ema_entry_bytes" in built.SYMBOLS
    lib = built.load_library()
    assert lib.frost_ema_entry_bytes() == ctypes.sizeof(L.FrostEmaEntry) == 32
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frost_hip.h")).read()
    for name, val in (("LERP", L.EMA_LERP), ("COPY1", L.EMA_COPY1), ("COPY4", L.EMA_COPY4), ("COPY8", L.EMA_COPY8), ("CHUNK", L.EMA_CHUNK),
                      ("SMALL_ROWS", L.EMA_SMALL_ROWS)):
        assert f"#define FROST_EMA_{name} {val}\n" in hdr


def _covered(units, wgmap, nwg):
    """Runs the map the way the kernel reads it: how often every unit of every entry is visited."""
    from frostnet_amd import _lib as L
    hits = [np.zeros(max(u, 0), dtype=np.int32) for u in units]
    for kind, a, b, c in wgmap[:nwg]:
        if kind == 0:
            assert c == 0 and 0 <= a < len(units)
            lo = b * L.EMA_CHUNK
            assert lo < units[a]
            hits[a][lo:min(lo + L.EMA_CHUNK, units[a])] += 1
        else:
            assert kind == 1 and a >= nwg and 1 <= b <= L.EMA_SMALL_ROWS and a + b <= len(wgmap)
            rows = wgmap[a:a + b]
            pref = rows[:, 1].tolist() + [c]
            assert pref[0] == 0 and all(x < y for x, y in zip(pref, pref[1:]))
            for (entry, p, _, _), nxt in zip(rows, pref[1:]):
                assert nxt - p == units[entry]
                hits[entry] += 1
    return hits


def test_workgroup_map_covers_every_unit_once(built):
    from frostnet_amd import _lib as L
    from frostnet_amd.ema import SMALL_SLICE, build_map
    rng = np.random.default_rng(3)
    units = [1, 0, 3, 1023, 1024, 1025, 4096, 4097, 2 ** 20 + 3, 2] + [1] * 700 + rng.integers(1, 1024, 300).tolist() + [5000, 1, 1]
    wgmap, nwg = build_map(units)
    assert wgmap.dtype == np.int32 and wgmap.shape[1] == 4
    for u, h in zip(units, _covered(units, wgmap, nwg)):
        assert h.shape[0] == u and bool((h == 1).all())
    # the target shape: about (total units / chunk) workgroups plus a handful, not one per entry
    large = sum(-(-u // L.EMA_CHUNK) for u in units if u >= 1024)
    small = sum(u for u in units if u < 1024)
    assert nwg <= large + small // (SMALL_SLICE // 2) + 700 // L.EMA_SMALL_ROWS + 4
    assert build_map([0, 0])[1] == 0


def test_fma_definition_equals_lerp_below_half(built):
    """The two forms of the definition the device test uses agree on the CPU: lerp_ and the fp64 evaluation of fmaf(w, src - dst, dst)."""
    g = torch.Generator().manual_seed(5)
    dst = torch.randn(1 << 16, generator=g) * torch.logspace(-6, 6, 1 << 16)
    src = dst + torch.randn(1 << 16, generator=g) * dst.abs() * 0.1
    for w in (1e-4, 0.1):
        w32 = float(np.float32(w))
        a = dst.clone().lerp_(src, w32)
        b = (dst.double() + w32 * (src - dst).double()).float()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_reference_loop_is_the_stock_loop_plus_the_nonfinite_rule(built):
    from frostnet_amd.ema import ModelEma
    m = _qat_small()
    m.train()
    x = torch.randn(4, 3, 32, 32)
    m(x)
    ema = ModelEma(m, decay=0.9)
    assert not ema.module.training and all(not p.requires_grad for p in ema.module.parameters())
    with torch.no_grad():                                 # the model moves on: parameters, BatchNorm statistics, observers, num_batches_tracked
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    m(torch.randn(4, 3, 32, 32) * 2)
    stock = copy.deepcopy(ema.module)
    w = float(np.float32(1.0 - 0.9))
    with torch.no_grad():
        for (k, ev), (k2, mv) in zip(stock.state_dict().items(), m.state_dict().items()):
            assert k == k2
            if ev.is_floating_point():
                ev.lerp_(mv, w)
            else:
                ev.copy_(mv)
    ema.update(m)                                          # a CPU model: update_reference
    assert ema.updates == 1
    never = [k for k, v in m.state_dict().items() if k.endswith("min_val") and v.numel() == 1 and bool(torch.isinf(v).all())]
    assert len(never) > 0
    msd = m.state_dict()
    excepted = []
    got = ema.module.state_dict()
    assert list(got.keys()) == list(msd.keys())
    for k, sv in stock.state_dict().items():
        if sv.is_floating_point() and bool(torch.isnan(sv).any()):
            excepted.append(k)
            assert torch.equal(_bits(got[k]), _bits(msd[k])), k           # there the shadow holds the model's value
        else:
            assert torch.equal(_bits(got[k]), _bits(sv)), k
    assert len(excepted) == 2 * len(never)
    assert sorted(excepted) == sorted(never + [k[:-len("min_val")] + "max_val" for k in never])
    changed = sum(1 for k, v in got.items() if v.is_floating_point() and v.numel() > 1 and not torch.equal(v, msd[k]))
    assert changed > 50                                    # an average, not a copy
    # exclude_buffers: parameters averaged, every buffer copied
    ema2 = ModelEma(m, decay=0.9, exclude_buffers=True)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.01)
        for b in m.buffers():
            if b.is_floating_point() and b.numel() > 1:
                b.add_(0.25)
    before = {k: v.clone() for k, v in ema2.module.state_dict().items()}
    ema2.update(m)
    names = {k for k, _ in m.named_parameters()}
    for k, v in ema2.module.state_dict().items():
        if k in names:
            assert torch.equal(_bits(v), _bits(before[k].lerp(m.state_dict()[k], w))), k
        else:
            assert torch.equal(_bits(v), _bits(m.state_dict()[k])), k
    # set(): a copy of everything, the count stays
    ema2.set(m)
    assert ema2.updates == 1
    for k, v in ema2.module.state_dict().items():
        assert torch.equal(_bits(v), _bits(m.state_dict()[k])), k


def test_decay_schedule(built):
    from frostnet_amd.ema import ModelEma
    m = torch.nn.Linear(2, 2)
    plain, warm = ModelEma(m, decay=0.9999), ModelEma(m, decay=0.9999, warmup=True)
    for t, want in ((0, 1 / 10), (1, 2 / 11), (9, 10 / 19), (10 ** 5, 0.9999)):
        assert plain.decay_at(t) == 0.9999
        assert warm.decay_at(t) == want
    with pytest.raises(ValueError):
        ModelEma(m, decay=0.4)
    # the update count drives it
    src = torch.nn.Linear(2, 2)
    w0 = warm.module.weight.clone()
    warm.update(src)
    assert warm.updates == 1
    want = (w0.double() + float(np.float32(0.9)) * (src.weight.detach() - w0).double()).float()
    assert torch.equal(warm.module.weight, want)


def test_train_loop_updates_the_average_after_every_step(built):
    """harness.train(..., ema=ema) on the eager path (a CPU model): one update behind every optimizer step, and graph=True refuses nothing it did not refuse before."""
    from frostnet_amd import harness as H
    from frostnet_amd.ema import ModelEma
    m = _qat_small(2)
    m.train()
    g = torch.Generator().manual_seed(9)
    loader = [(torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 1000, (4,), generator=g)) for _ in range(2)]
    m(loader[0][0])
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    ema = ModelEma(m, decay=0.75)
    stock = copy.deepcopy(ema.module)
    seen = []

    class Spy(list):                                   # the model as it stands when the loop comes back for the next batch = after the step and the update
        def __iter__(self):
            for b in list.__iter__(self):
                yield b
                seen.append(copy.deepcopy(m.state_dict()))
    H.train(Spy(loader), m, torch.nn.CrossEntropyLoss(), opt, 0, ema=ema)
    assert ema.updates == 2 and len(seen) == 2
    with torch.no_grad():
        for sd in seen:
            for (k, ev), mv in zip(stock.state_dict().items(), sd.values()):
                if ev.is_floating_point():
                    new = ev.clone().lerp_(mv, 0.25)
                    ev.copy_(torch.where(torch.isfinite(mv), new, mv))
                else:
                    ev.copy_(mv)
    for (k, a), (_, b) in zip(ema.module.state_dict().items(), stock.state_dict().items()):
        assert torch.equal(_bits(a), _bits(b)), k
    with pytest.raises(ValueError):
        H.GraphedStep(m, torch.nn.CrossEntropyLoss(), None, ema=ema)


def test_checkpoint_round_trip_and_ema_ingest(built, tmp_path):
    from frostnet_amd import frostnet_features as FF
    from frostnet_amd.ema import ModelEma
    from frostnet_amd.harness import checkpoint_state, load_checkpoint, save_checkpoint
    torch.manual_seed(1)
    m = FF.FrostNet(mode="small", width_mult=0.35)
    m._init_weights()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    ema = ModelEma(m, decay=0.99)
    for _ in range(3):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn_like(p))
        ema.update(m)
    path = str(tmp_path / "ck.pth.tar")
    state = checkpoint_state(m, opt, 4, ema=ema, acc1=12.5)
    assert state["ema_updates"] == 3 and list(state["state_dict_ema"].keys()) == list(m.state_dict().keys())
    save_checkpoint(state, path)
    m2 = FF.FrostNet(mode="small", width_mult=0.35)
    m2._init_weights()
    ema2 = ModelEma(m2, decay=0.99)
    ck = load_checkpoint(m2, torch.optim.SGD(m2.parameters(), lr=0.1), path, ema=ema2)
    assert ck["epoch"] == 5 and ck["acc1"] == 12.5 and ema2.updates == 3
    for (k, a), (_, b) in zip(ema.module.state_dict().items(), ema2.module.state_dict().items()):
        assert torch.equal(_bits(a), _bits(b)), k
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(_bits(a), _bits(b)), k
    # the backbone's checkpoint ingest prefers the average
    m3 = FF.FrostNet(mode="small", width_mult=0.35)
    FF.load_checkpoint(m3, path, use_ema=True)
    differs = 0
    for (k, a), (_, b), (_, c) in zip(m3.state_dict().items(), ema.module.state_dict().items(), m.state_dict().items()):
        assert torch.equal(_bits(a), _bits(b)), k
        differs += int(not torch.equal(_bits(a), _bits(c)))
    assert differs > 50
    # ModelEma's own state_dict carries the count
    sd = ema.state_dict()
    assert sd["updates"] == 3
    ema4 = ModelEma(m3, decay=0.99)
    ema4.load_state_dict(sd)
    assert ema4.updates == 3 and torch.equal(ema4.module.conv1.conv[0].weight, ema.module.conv1.conv[0].weight)
    # a checkpoint without an average is refused when one is asked for
    save_checkpoint(checkpoint_state(m, opt, 4), path)
    with pytest.raises(KeyError):
        load_checkpoint(m2, None, path, ema=ema2)

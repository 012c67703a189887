"""Weight EMA on the device (frostnet_amd.ema.ModelEma, csrc/frost_ema.hip): the kernel on a synthetic table against the definition, the device shadow against the
stock loop on the CPU (with the non-finite rule) through eager training, a shadow whose runner binds in between, the graphed loops, the float model, the detector
and two data-parallel ranks.  Every comparison is bit for bit.  FrostNet-Small x0.35, QAT-prepared, 32 x 32, B = 4; the detector is Small @128, B = 2."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, B = 32, 4


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import ema, frostnet, harness
    return frostnet, harness, ema


@pytest.fixture(autouse=True)
def _raw_write_flags():
    """The graphed tests capture raw-pointer writers, which switches the version-keyed weight caches off for the rest of the PROCESS (`_lib.RAW_WRITES_CAPTURED`: such a
    graph may be replayed unseen).  Their graphs die with them, so the switch goes back to what it was: later test files find the process as this one found it."""
    from frostnet_amd import _lib as L
    before = L.RAW_WRITES_CAPTURED
    yield
    L.RAW_WRITES_CAPTURED = before


# ------------------------------------------------------------------------------------------------------------------- helpers
def _live(model):
    """key -> the tensor the module tree holds NOW, for every state_dict entry (not state_dict(): a bound model returns clones of its aliased buffers)."""
    out, params = {}, set()
    for mname, mod in model.named_modules(remove_duplicate=False):
        pre = mname + "." if mname else ""
        for n, p in mod._parameters.items():
            if p is not None:
                out[pre + n] = p
                params.add(pre + n)
        for n, b in mod._buffers.items():
            if b is not None and n not in mod._non_persistent_buffers_set:
                out[pre + n] = b
    return out, params


def _to_cpu(model):
    torch.cuda.synchronize()
    live, params = _live(model)
    return {k: v.detach().cpu().clone() for k, v in live.items()}, params


def _stock_step(shadow, model_cpu, params, w, exclude_buffers=False):
    """The stock loop on CPU tensors, plus the rule: where the model's value is not finite the shadow takes it."""
    for k, ev in shadow.items():
        mv = model_cpu[k]
        if ev.is_floating_point() and (k in params or not exclude_buffers):
            # (lerp_ changes its formula at 0.5 -- the first steps of the warm-up schedule: there the definition fmaf(w, src - dst, dst) through fp64)
            new = ev.clone().lerp_(mv, w) if w < 0.5 else (ev.double() + w * (mv - ev).double()).float()
            ev.copy_(torch.where(torch.isfinite(mv), new, mv))
        else:
            ev.copy_(mv)


def _raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def _assert_same(got, want, what):
    assert list(got.keys()) == list(want.keys())
    bad = [k for k in want if got[k].dtype != want[k].dtype or not torch.equal(_raw(got[k]), _raw(want[k]))]
    assert not bad, f"{what}: {len(bad)} of {len(want)} entries differ, first {bad[:5]}"


def _w(decay):
    return float(np.float32(1.0 - decay))


def _qat(F, seed=0, name="frostnet_quant_small_0_35"):
    torch.manual_seed(seed)
    m = F.MODEL_REGISTRY[name](drop_rate=0.0)
    F.qat_prepare(m, version=0)
    return m.cuda().train()


def _qsgd(model, lr=1e-2):
    from frostnet_amd.optimizer import QSGD
    return QSGD([{"params": [p]} for p in model.parameters()], lr=lr, momentum=0.9, nesterov=True)      # is_warmup: no noise


def _batch(seed=1, n=B, res=RES):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, res, res, generator=g).cuda(), torch.randint(0, 1000, (n,), generator=g).cuda()


# ------------------------------------------------------------------------------------------------------------------- 5. the kernel
_SIZES = [(), (1,), (3,), (63,), (64,), (65,), (255,), (256,), (257,), (1023,), (1024,), (1025,), (4099,), (2 ** 20 + 3,)]


def _synthetic(shift):
    """One host arena (bytes) with src / dst of every entry at offsets = 0, 4, 8, 12 mod 16 -- entry i: src at 4 * (i % 4), dst at 4 * ((i + shift) % 4), so shift 0
    puts both sides on the same offset (vector body behind a scalar head) and shift 1 never does (word by word) -- and 32 guard bytes around every region.
    -> arena, entries [(src offset, dst offset, n, kind, numpy dtype)]."""
    from frostnet_amd import _lib as L
    rng = np.random.default_rng(11)
    specs = [(int(np.prod(s)), L.EMA_LERP, np.float32) for s in _SIZES]
    specs += [(1, L.EMA_COPY4, np.int32), (1, L.EMA_COPY8, np.int64), (1, L.EMA_COPY1, np.uint8), (257, L.EMA_COPY4, np.int32), (1500, L.EMA_COPY1, np.uint8),
              (1100, L.EMA_COPY8, np.int64)]
    chunks, entries, off = [], [], 0

    def region(nbytes, mod):
        nonlocal off
        off += 32                                             # guard
        off += (mod - off) % 16
        start = off
        off += nbytes
        return start
    for i, (n, kind, dt) in enumerate(specs):
        size = n * np.dtype(dt).itemsize
        odd = 1 if kind == L.EMA_COPY1 else 0                 # bytes need no alignment at all
        so, do = region(size, 4 * (i % 4) + odd), region(size, 4 * ((i + shift) % 4) + 3 * odd)
        entries.append((so, do, n, kind, dt))
    off += 48
    arena = np.full(off, 0xA5, dtype=np.uint8)
    for i, (so, do, n, kind, dt) in enumerate(entries):
        if kind == L.EMA_LERP:
            d = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
            s = (d + rng.standard_normal(n).astype(np.float32) * np.abs(d) * 0.3).astype(np.float32)
            special = np.array([0.0, -0.0, 1e-40, -3e-42, np.inf, -np.inf, np.nan, 1.17549435e-38, 3e38], dtype=np.float32)
            k = min(n, 64)
            if n > 1:
                at = rng.choice(n, k, replace=False)
                s[at] = special[rng.integers(0, len(special), k)]
                at = rng.choice(n, k, replace=False)
                d[at] = special[[0, 1, 2, 3, 7]][rng.integers(0, 5, k)]        # the shadow side stays finite: zeros and denormals
            elif i % 2:
                s[0] = np.inf
        else:
            info = np.iinfo(dt)
            s = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            d = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        arena[so:so + s.nbytes] = s.view(np.uint8)
        arena[do:do + d.nbytes] = d.view(np.uint8)
    return arena, entries


def _define(arena, entries, w):
    """The definition on the host arena: dst = float32(float64(dst) + float64(w) * float64(float32(src - dst))), a src that is not finite is copied; copies are bytes."""
    from frostnet_amd import _lib as L
    out = arena.copy()
    for so, do, n, kind, dt in entries:
        size = n * np.dtype(dt).itemsize
        s = arena[so:so + size].copy().view(dt)
        if kind == L.EMA_LERP:
            d = arena[do:do + size].copy().view(np.float32)
            with np.errstate(all="ignore"):
                new = (d.astype(np.float64) + np.float64(np.float32(w)) * (s - d).astype(np.float64)).astype(np.float32)
            new = np.where(np.isfinite(s), new.view(np.uint32), s.view(np.uint32)).astype(np.uint32)
            out[do:do + size] = new.view(np.uint8)
        else:
            out[do:do + size] = s.view(np.uint8)
    return out


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("w", [1e-4, 0.1])
def test_kernel_on_a_synthetic_table(mods, w, shift):
    from frostnet_amd import _lib as L
    from frostnet_amd.ema import build_map
    arena, entries = _synthetic(shift)
    dev = torch.from_numpy(arena.copy()).cuda()
    assert dev.data_ptr() % 16 == 0
    tab = (L.FrostEmaEntry * len(entries))()
    for i, (so, do, n, kind, dt) in enumerate(entries):
        tab[i].src, tab[i].dst, tab[i].n, tab[i].kind = dev.data_ptr() + so, dev.data_ptr() + do, n, kind
        assert (dev.data_ptr() + so) % 16 == (4 * (i % 4) + (kind == L.EMA_COPY1)) % 16
    table = L.struct_to_tensor(tab, dev.device)
    wgmap, nwg = build_map([2 * n if kind == L.EMA_COPY8 else n for _, _, n, kind, _ in entries])
    total = sum(n for _, _, n, _, _ in entries)
    assert nwg <= total // L.EMA_CHUNK + 12                    # flat map: about bytes / chunk workgroups plus a handful
    wg = torch.from_numpy(wgmap).cuda()
    wd = torch.tensor([w], dtype=torch.float32, device="cuda")

    def launch():
        L.call("frost_ema_update", L.ptr(table), len(entries), L.ptr(wg), nwg, L.ptr(wd), L.stream())
        torch.cuda.synchronize()
        return dev.cpu().numpy()
    want1 = _define(arena, entries, w)
    got1 = launch()
    bad = np.nonzero(got1 != want1)[0]
    assert bad.size == 0, f"{bad.size} bytes differ from the definition (guards and src included), first at {bad[:8].tolist()}"
    # the same through CPU lerp_ where src is finite
    for so, do, n, kind, dt in entries:
        if kind != L.EMA_LERP:
            continue
        s, d = torch.from_numpy(arena[so:so + 4 * n].copy().view(np.float32)), torch.from_numpy(arena[do:do + 4 * n].copy().view(np.float32))
        ref = d.clone().lerp_(s, float(np.float32(w)))
        fin = torch.isfinite(s)
        got = torch.from_numpy(got1[do:do + 4 * n].copy().view(np.float32))
        assert torch.equal(got[fin].view(torch.int32), ref[fin].view(torch.int32)), n
        assert torch.equal(got[~fin].view(torch.int32), s[~fin].view(torch.int32)), n
    assert int((~np.isfinite(np.concatenate([arena[so:so + 4 * n].view(np.float32) for so, _, n, k, _ in entries if k == L.EMA_LERP]))).sum()) > 20
    # two launches in a row compose
    got2 = launch()
    want2 = _define(want1, entries, w)
    assert np.array_equal(got2, want2) and not np.array_equal(want2, want1)


# ------------------------------------------------------------------------------------------------------------------- 6. QAT training, eager
def test_qat_training_eager_matches_the_stock_loop(mods):
    F, H, E = mods
    model, (x, t) = _qat(F), _batch()
    opt, crit = _qsgd(model), H.CrossEntropyLoss()
    H.train_one_iter(model, crit, opt, x, t)                  # bound, every used site observed
    emas = {eb: E.ModelEma(model, decay=0.9, exclude_buffers=eb) for eb in (False, True)}
    shadows = {eb: _to_cpu(e.module)[0] for eb, e in emas.items()}
    for step in range(3):
        H.train_one_iter(model, crit, opt, *_batch(10 + step))
        for e in emas.values():
            e.update(model)
        mcpu, params = _to_cpu(model)
        for eb, e in emas.items():
            _stock_step(shadows[eb], mcpu, params, _w(0.9), eb)
            _assert_same(_to_cpu(e.module)[0], shadows[eb], f"step {step} exclude_buffers={eb}")
    n = len(shadows[False])
    never = sum(1 for k, v in shadows[False].items() if k.endswith("min_val") and bool(torch.isinf(v).all()))
    ints = sum(1 for v in shadows[False].values() if not v.is_floating_point())
    print(f"[ema eager] {n} entries, {ints} integer, {never} never-observed sites; plan {emas[False]._plan['nwg']} workgroups")
    assert n > 800 and ints > 200 and never > 0 and emas[False].plan_id == 1 and emas[False].updates == 3
    assert not any(bool(torch.isnan(v).any()) for v in shadows[False].values() if v.is_floating_point())
    moved = sum(1 for k, v in shadows[False].items() if k in params and not torch.equal(v, mcpu[k]))
    assert moved > 50                                         # an average, not a copy of the model
    # set(): shadow := model
    emas[False].set(model)
    _assert_same(_to_cpu(emas[False].module)[0], _to_cpu(model)[0], "set")
    assert emas[False].updates == 3


# ------------------------------------------------------------------------------------------------------------------- 7. the table goes stale
def test_table_follows_a_shadow_whose_runner_binds(mods):
    F, H, E = mods
    model, (x, t) = _qat(F), _batch()
    opt, crit = _qsgd(model), H.CrossEntropyLoss()
    H.train_one_iter(model, crit, opt, x, t)
    ema = E.ModelEma(model, decay=0.9)
    H.train_one_iter(model, crit, opt, *_batch(20))
    ema.update(model)
    sig0, table0 = ema._plan["sig"], ema._plan["table"].data_ptr()
    with torch.no_grad():
        ema.module(x)                                         # the shadow's runner binds: its observer / qparam buffers are re-aliased onto its own arena
    shadow = _to_cpu(ema.module)[0]                           # (an eval forward moves the live observers: the CPU shadow continues from here)
    for step in range(2):
        H.train_one_iter(model, crit, opt, *_batch(21 + step))
        ema.update(model)
        mcpu, params = _to_cpu(model)
        _stock_step(shadow, mcpu, params, _w(0.9))
        _assert_same(_to_cpu(ema.module)[0], shadow, f"update {step} after the shadow bound")
    assert ema._plan["sig"] != sig0                           # the pointers did move ...
    assert ema.plan_id == 1 and ema._plan["table"].data_ptr() == table0          # ... and the same device table was rewritten in place
    assert ema.module.hip_runner().still_valid()


# ------------------------------------------------------------------------------------------------------------------- 8. the shadow is a model
def test_shadow_is_a_model(mods):
    F, H, E = mods
    model, (x, t) = _qat(F), _batch()
    opt, crit = _qsgd(model), H.CrossEntropyLoss()
    H.train_one_iter(model, crit, opt, x, t)
    ema = E.ModelEma(model, decay=0.9)
    ema.bind_shadow()                                         # bound first: every update below writes the shadow's qrecords through the aliased views
    with torch.no_grad():
        ema.module(x)
    for step in range(3):
        H.train_one_iter(model, crit, opt, *_batch(30 + step))
        ema.update(model)
    fresh = _qat(F, seed=5)
    fresh.load_state_dict(ema.module.state_dict())
    fresh.eval()
    xe = _batch(40)[0]
    with torch.no_grad():
        y_fresh, y_shadow = fresh(xe), ema.module(xe)
    assert bool(torch.isfinite(y_shadow).all()) and float(y_shadow.abs().max()) > 0
    assert torch.equal(y_shadow, y_fresh)
    _assert_same(_to_cpu(ema.module)[0], _to_cpu(fresh)[0], "state after the eval forward")
    fresh.hip_convert()
    ema.module.hip_convert()
    with torch.no_grad():
        q_fresh, q_shadow = fresh(xe), ema.module(xe)
    assert torch.equal(q_shadow, q_fresh) and bool(torch.isfinite(q_shadow).all())
    with pytest.raises(RuntimeError):
        ema.update(model)                                     # a converted shadow's weights are frozen


# ------------------------------------------------------------------------------------------------------------------- 9. graphed
def test_graphed_step_against_the_stock_loop(mods):
    """A real learning rate: the captured EMA launch must see the parameters the captured optimizer launch left (the CPU stock loop runs on this run's own post-step
    tensors), with w = 1 - decay_t different at every replay."""
    F, H, E = mods
    model = _qat(F)
    opt, crit = _qsgd(model), H.CrossEntropyLoss()
    H.train_one_iter(model, crit, opt, *_batch())
    ema = E.ModelEma(model, decay=0.9999, warmup=True)
    step = H.GraphedStep(model, crit, opt, ema=ema, eager_warmup=2)
    shadow = _to_cpu(ema.module)[0]
    a = _batch(50)
    for i in range(5):
        step(*_batch(50 + i))
        mcpu, params = _to_cpu(model)
        w = _w(min(0.9999, (1 + i) / (10 + i)))
        _stock_step(shadow, mcpu, params, w)
        _assert_same(_to_cpu(ema.module)[0], shadow, f"graphed step {i}")
        assert (step.graph_for(*a) is not None) == (i >= 2)
    assert step.captures == 1 and ema.updates == 5 and ema.plan_id == 1


def _twin(mods, capture):
    F, H, E = mods
    model = _qat(F)
    opt, crit = _qsgd(model, lr=0.0), H.CrossEntropyLoss()
    H.train_one_iter(model, crit, opt, *_batch())
    ema = E.ModelEma(model, decay=0.9999, warmup=True)
    with torch.no_grad():
        for p in ema.module.parameters():                     # the average starts away from the model, so every step moves every parameter's shadow
            p.mul_(1.03125)
    step = H.GraphedStep(model, crit, opt, ema=ema, eager_warmup=2)
    step.capture = capture
    return model, opt, ema, step


def test_graphed_step_equals_its_eager_twin(mods):
    """The twin (capture = False) from the same seed, shadows compared after every step.  Two TRAINING runs of this engine branch (the backward's fp32 atomics, see
    tests/test_gpu_dp.py::test_graph_segments_replay_equals_eager; measured with these twins at lr = 1e-2, three trials: 29 - 38 of 1 259 shadow entries differ after the
    first step and about 600 after the fifth), while its forward is bit-reproducible; so the twins train with lr = 0 -- the optimizer launch runs,
    the parameters stay -- and what moves is what the forward moves (BatchNorm statistics, observers, qparams, counters) plus the average itself, started 3 % away from
    the model, with a different w at every step.  The captured launch after a real optimizer step is the test above."""
    _, gopt, gema, gstep = _twin(mods, True)
    _, eopt, eema, estep = _twin(mods, False)
    a = _batch(60)
    seen = []
    for i in range(5):
        b = _batch(60 + i)
        gstep(*b)
        estep(*b)
        got, want = _to_cpu(gema.module)[0], _to_cpu(eema.module)[0]
        _assert_same(got, want, f"step {i}")
        seen.append(hashlib.sha1(b"".join(_raw(v).numpy().tobytes() for v in got.values())).hexdigest())
        assert (gstep.graph_for(*a) is not None) == (i >= 2)
    assert len(set(seen)) == 5 and gstep.captures == 1 and estep.captures == 0
    for opt in (gopt, eopt):                                  # the optimizer's plan changes: the step is captured again, never replayed stale
        opt.load_state_dict(opt.state_dict())
    gstep(*a)
    estep(*a)
    _assert_same(_to_cpu(gema.module)[0], _to_cpu(eema.module)[0], "after the plan change")
    assert gstep.captures == 2 and gema.updates == eema.updates == 6


# ------------------------------------------------------------------------------------------------------------------- 10. float model, detector
def test_float_model_one_step(mods):
    F, H, E = mods
    torch.manual_seed(3)
    model = F.frostnet_small_0_35(drop_rate=0.0).cuda().train()
    opt, crit = _qsgd(model), H.CrossEntropyLoss()
    ema = E.ModelEma(model, decay=0.9)
    shadow = _to_cpu(ema.module)[0]
    H.train_one_iter(model, crit, opt, *_batch(70))
    assert type(model.hip_runner()).__name__ == "FloatRunner"
    ema.update(model)
    mcpu, params = _to_cpu(model)
    _stock_step(shadow, mcpu, params, _w(0.9))
    _assert_same(_to_cpu(ema.module)[0], shadow, "float model")
    assert sum(1 for k in params if not torch.equal(shadow[k], mcpu[k])) > 50


def test_detector_through_train_detector(mods):
    F, H, E = mods
    from frostnet_amd import ssdlite as S
    torch.manual_seed(2)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128))
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt, crit = _qsgd(model, lr=4e-3), S.MultiBoxLoss(21)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 128, 128, generator=g).cuda()
    boxes, valid = S.pad_targets([torch.tensor([[0.2, 0.2, 0.6, 0.7, 3.0]], device="cuda"),
                                  torch.tensor([[0.1, 0.3, 0.5, 0.9, 7.0], [0.5, 0.5, 0.9, 0.8, 1.0]], device="cuda")], torch.device("cuda"))
    model(x)                                                  # bound, sites observed
    ema = E.ModelEma(model, decay=0.9)
    shadow = _to_cpu(ema.module)[0]
    H.train_detector([(x, boxes, valid)], model, crit, opt, 0, 1, 4e-3, 0.5, (), graph=False, ema=ema)
    mcpu, params = _to_cpu(model)
    _stock_step(shadow, mcpu, params, _w(0.9))
    _assert_same(_to_cpu(ema.module)[0], shadow, "detector")
    assert ema.updates == 1 and sum(1 for k in params if not torch.equal(shadow[k], mcpu[k])) > 50


# ------------------------------------------------------------------------------------------------------------------- 11. two ranks on one device
def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    sys.path.insert(0, ROOT)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from frostnet_amd import ema as E, frostnet as F, harness as H
        from frostnet_amd.parallel import broadcast_model
        model = _qat(F, seed=100 + rank)                      # ranks start different ...
        broadcast_model(model)                                # ... rank 0's weights win
        opt, crit = _qsgd(model), H.CrossEntropyLoss()
        step = H.GraphedStep(model, crit, opt, nbuckets=3, group=dist.group.WORLD, eager_warmup=1)
        step(*_batch(80))                                     # (before the average is made: every used site observed)
        ema = E.ModelEma(model, decay=0.9)
        step = H.GraphedStep(model, crit, opt, nbuckets=3, group=dist.group.WORLD, eager_warmup=1, ema=ema)
        shadow, ok, digests = _to_cpu(ema.module)[0], True, []
        for i in range(4):                                    # eager segments, the capture, a replay: the same batch on both ranks; then one step on different shards
            step(*_batch(81 + i + (7 * rank if i == 3 else 0)))
            mcpu, params = _to_cpu(model)
            _stock_step(shadow, mcpu, params, _w(0.9))
            got = _to_cpu(ema.module)[0]
            ok = ok and all(torch.equal(_raw(got[k]), _raw(shadow[k])) for k in shadow)
            digests.append((hashlib.sha1(b"".join(_raw(got[k]).numpy().tobytes() for k in got)).hexdigest(),
                            hashlib.sha1(b"".join(_raw(got[k]).numpy().tobytes() for k in got if k in params)).hexdigest()))
        q.put((rank, ok, digests, step.captures, isinstance(step.graph_for(*_batch(81)), list), None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                    # the parent must not wait for a rank that died
        import traceback
        q.put((rank, False, [], 0, False, f"{e!r}\n{traceback.format_exc()}"))


def test_two_ranks_on_one_device():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + (os.getpid() % 40)
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[5] is None, r[5]
        assert r[1], f"rank {r[0]}: the shadow differs from the stock loop on its own post-step tensors"
        assert r[3] == 1 and r[4]                             # eager segments, one capture, replays: a chain of segment graphs
    for i in range(3):                                        # the same batch on both ranks: whole shadows equal
        assert res[0][2][i][0] == res[1][2][i][0], i
    assert res[0][2][3][1] == res[1][2][3][1]                 # different shards: equal parameters (all-reduced step), so equal parameter averages ...
    assert res[0][2][3][0] != res[1][2][3][0]                 # ... while BatchNorm statistics and observers are each rank's own
    assert len({d[0] for d in res[0][2]}) == 4

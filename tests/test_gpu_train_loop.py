"""The graphed loops on the device: `frost_softmax_ce_metrics` against the CPU definition (harness.EpochMeter.update_reference and a row-by-row restatement here),
harness.GraphedStep's replay against what a replay must consume and advance, one graphed step against one eager step from the same restored state (the bounds of
tests/test_gpu_dp.py::test_graph_segments_replay_equals_eager: a multi-step trajectory is not compared, for the reason its docstring gives), and the loops
(`train` / `val` with graph=True, `train_detector`).  FrostNet-Small, QAT-prepared, 64 x 64, B = 8; the detector is Small @128, B = 4."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
RES, B = 64, 8


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import frostnet, harness
    return frostnet, harness


# ------------------------------------------------------------------------------------------------------------------- 1. the kernel
def _kernel_case(n, c, seed):
    """Random logits (O(1) losses) with, as far as n and c allow: row 0 = target tied with a LOWER class index (both the row maximum), row 1 = target tied with a
    HIGHER one, row 2 = target -100, last row = target logit -inf.  Returns x, t and the mask of plain rows (valid, finite, tie-free)."""
    g = torch.Generator().manual_seed(seed)
    x, t = torch.randn(n, c, generator=g) * 3.0, torch.randint(0, c, (n,), generator=g)
    plain = torch.ones(n, dtype=torch.bool)
    if n >= 2 and c >= 2:
        t[0], t[1] = 1, 0
        x[0, 0] = x[0, 1] = 50.0
        x[1, 0] = x[1, 1] = 50.0
        plain[:2] = False
    if n >= 4:
        t[2] = -100
        plain[2] = False
    if n >= 5:
        x[n - 1, t[n - 1]] = float("-inf")
        plain[n - 1] = False
    for r in range(n):          # the plain rows really are tie-free at the target
        if plain[r]:
            assert int((x[r] == x[r, t[r]]).sum()) == 1
    return x, t, plain


def _rows_by_hand(x, t, topk):
    """(hits top-1, hits top-k, fp64 batch loss with the kernel's fp32 1 / n) row by row, independent of EpochMeter."""
    n, c = x.shape
    inv_n = float(torch.tensor(1.0 / n, dtype=torch.float32))
    h1 = hk = 0
    loss = 0.0
    for r in range(n):
        tr = int(t[r])
        if tr < 0 or tr >= c:
            continue
        row = x[r].double()
        xt = float(row[tr])
        loss += float(torch.logsumexp(row, 0)) - xt
        if not math.isfinite(xt):
            continue
        rank = int((row > xt).sum()) + int((row[:tr] == xt).sum())
        h1 += rank == 0
        hk += rank < min(topk, c)
    return h1, hk, loss * inv_n


def _launch(H, x, t, topk, with_grad=True, meter=None):
    meter = meter or H.EpochMeter("cuda", topk=topk)
    xd, td = x.cuda(), t.cuda()
    dl = torch.empty_like(xd) if with_grad else None
    loss = meter._launch(xd, td, dl)
    return meter, loss, dl


def _counts(rec, n):
    unit = 100.0 * float(torch.tensor(1.0 / n, dtype=torch.float32))
    c1, ck = round(rec[1] / unit), round(rec[2] / unit)
    assert abs(rec[1] - c1 * unit) <= 1e-12 * max(rec[1], 1.0) and abs(rec[2] - ck * unit) <= 1e-12 * max(rec[2], 1.0)
    return c1, ck


@pytest.mark.parametrize("n,c,topk", [(1, 2, 5), (5, 7, 5), (3, 1000, 5), (67, 21, 5), (9, 130, 1), (4, 3, 5)])
def test_softmax_ce_metrics_kernel(mods, n, c, topk):
    _, H = mods
    from frostnet_amd._lib import call, ptr, stream
    x, t, plain = _kernel_case(n, c, 100 + n)
    meter, loss, dl = _launch(H, x, t, topk)
    # dlogits: bit-equal to frost_softmax_ce
    xd, td = x.cuda(), t.cuda()
    loss0, dl0 = torch.zeros((), device="cuda"), torch.empty_like(xd)
    call("frost_softmax_ce", ptr(xd), ptr(td), n, c, 1.0 / n, ptr(loss0), ptr(dl0), stream())
    assert torch.equal(dl, dl0)
    # hit counts: exactly the definition's (restated row by row here, and EpochMeter's torch code)
    h1, hk, want_loss = _rows_by_hand(x, t, topk)
    ref = H.EpochMeter("cpu", topk=topk)
    ref.update_reference(x, t)
    rec = meter.record.tolist()
    print(f"[ce_metrics {n}x{c} top{topk}] loss {float(loss):.7f} want {want_loss:.7f}; record {rec}; hits by hand {h1} {hk}")
    assert _counts(rec, n) == (h1, hk) == _counts(ref.record.tolist(), n) and rec[3] == 1.0
    if n >= 2 and c >= 2:          # the tie rule itself: of rows 0 and 1 (both tied at the row maximum) only row 1, tied with a HIGHER index, is a top-1 hit
        m2, _, _ = _launch(H, x[:2], t[:2], 1)
        assert _counts(m2.record.tolist(), 2) == (1, 1)
    # loss: +inf with the -inf row (as cross-entropy defines it); within 1e-6 of the fp64 value on the finite rows
    if math.isinf(want_loss):
        assert math.isinf(float(loss)) and float(loss) > 0 and math.isinf(rec[0]) and float(loss0) == float(loss)
        x, t, plain = x[:n - 1].contiguous(), t[:n - 1].contiguous(), plain[:n - 1]
        n -= 1
        meter, loss, dl = _launch(H, x, t, topk)
        h1, hk, want_loss = _rows_by_hand(x, t, topk)
        rec = meter.record.tolist()
        assert _counts(rec, n) == (h1, hk)
    assert abs(float(loss) - want_loss) <= 1e-6 * want_loss and abs(rec[0] - want_loss) <= 1e-6 * want_loss, (float(loss), rec[0], want_loss)
    # a null dlogits is accepted and changes nothing else; three launches add up; reset() zeroes
    m3, loss3, _ = _launch(H, x, t, topk, with_grad=False)
    assert abs(float(loss3) - float(loss)) <= (0.0 if n <= 8 else 1e-6 * want_loss) and _counts(m3.record.tolist(), n) == (h1, hk)          # (up to 8 rows: the same bits)
    for _ in range(2):
        _launch(H, x, t, topk, with_grad=False, meter=m3)
    rec3 = m3.record.tolist()
    assert all(abs(a - 3 * b) <= 1e-12 * abs(3 * b) for a, b in zip(rec3, rec)), (rec3, rec)
    got = m3.read()
    assert abs(got[0] - rec[0]) <= 1e-12 * rec[0] and abs(got[1] - rec[1]) <= 1e-12 * max(rec[1], 1.0)
    m3.reset()
    assert m3.record.tolist() == [0.0] * 4
    # on the plain rows the hits are harness.accuracy's
    if int(plain.sum()) > 0:
        xs, ts = x[plain].contiguous(), t[plain].contiguous()
        ms, _, _ = _launch(H, xs, ts, topk)
        a1, ak = H.accuracy(xs.cuda(), ts.cuda(), topk=(1, min(topk, c)))
        ns = xs.size(0)
        assert _counts(ms.record.tolist(), ns) == (round(float(a1) * ns / 100.0), round(float(ak) * ns / 100.0))


def test_cross_entropy_with_metrics_module(mods):
    _, H = mods
    x, t, _ = _kernel_case(9, 130, 7)
    x, t = x[:8].cuda(), t[:8].clamp(min=0).cuda()
    meter = H.EpochMeter("cuda")
    crit, plain = H.CrossEntropyWithMetrics(meter), H.CrossEntropyLoss()
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la, lb = crit(a, t), plain(b, t)
    (la * 0.5).backward()
    (lb * 0.5).backward()
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-6 * float(lb.detach()) and torch.equal(a.grad, b.grad)          # (the two kernels add the rows up in different orders)
    with torch.no_grad():
        assert float(crit(x, t)) == float(la)
    assert meter.record.tolist()[3] == 2.0
    with pytest.raises(ValueError):
        crit(x, t.int())
    with pytest.raises(ValueError):
        H.EpochMeter("cpu")._launch(x, t, None)          # a meter on another device than the logits


# ------------------------------------------------------------------------------------------------------------------- 2. the graphed step
def _classifier(mods, drop_rate=0.2, **kw):
    F, H = mods
    from frostnet_amd.optimizer import QSGD
    torch.manual_seed(0)
    model = F.frostnet_quant_small_1_0(drop_rate=drop_rate)
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=1e-3, momentum=0.9, nesterov=True)          # is_warmup: no noise
    return model, opt, H.GraphedStep(model, H.CrossEntropyLoss(), opt, **kw)


def _batches(k, n=B, seed=1, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, RES, RES, generator=g).to(device), torch.randint(0, 1000, (n,), generator=g).to(device)) for _ in range(k)]


def _params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def _warm(step, batch, calls=3):
    for _ in range(calls):          # two eager calls, then the capture (which also runs the step once)
        step(*batch)
    assert step.captures == 1 and step.graph_for(*batch) is not None


def test_replay_consumes_the_batch_and_the_live_state(mods):
    model, opt, step = _classifier(mods)
    a, b = _batches(2)
    _warm(step, a)
    graph, runner = step.graph_for(*a), model.hip_runner()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rng0 = runner.rng_state()
    la = float(step(*a))
    lb = float(step(*b))
    assert la != lb and math.isfinite(la) and math.isfinite(lb)
    model.load_state_dict(sd0)
    runner.set_rng_state(rng0)
    assert float(step(*a)) == la                                         # bit for bit: the forward is reproducible
    assert step.captures == 1 and step.graph_for(*a) is graph
    # K = 3 replays: BatchNorm counters, observers, the dropout stream and the optimizer's step count all advance by 3
    sd1 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    draws, steps = runner.rng_state()["draws"], [int(opt.state[p]["step"]) for p in model.parameters()]
    for _ in range(3):
        step(*b)
    sd2 = model.state_dict()
    nbt = [k for k in sd1 if k.endswith("num_batches_tracked")]
    assert nbt and all(int(sd2[k]) == int(sd1[k]) + 3 for k in nbt)
    obs = [k for k in sd1 if k.endswith("min_val") or k.endswith("max_val")]
    moved = sum(not torch.equal(sd1[k], sd2[k]) for k in obs)
    print(f"[replay] {moved} of {len(obs)} observer ranges moved over 3 replays")
    assert moved > 0
    assert runner.rng_state()["draws"] == draws + 3
    assert [int(opt.state[p]["step"]) for p in model.parameters()] == [s + 3 for s in steps]
    assert step.captures == 1


def test_hyper_parameters_stay_live_and_a_new_plan_is_captured_again(mods):
    model, opt, step = _classifier(mods)
    (a,) = _batches(1)
    _warm(step, a)
    graph = step.graph_for(*a)
    saved = [(g["lr"], g["weight_decay"]) for g in opt.param_groups]
    for g in opt.param_groups:
        g["lr"], g["weight_decay"] = 0.0, 0.0
    step(*a)                                   # (the momentum buffers move; lr = 0 keeps the parameters)
    p0 = _params(model)
    step(*a)
    assert torch.equal(_params(model), p0)
    for g, (lr, wd) in zip(opt.param_groups, saved):
        g["lr"], g["weight_decay"] = lr, wd
    step(*a)
    p1 = _params(model)
    assert not torch.equal(p1, p0) and bool(torch.isfinite(p1).all())
    assert step.graph_for(*a) is graph and step.captures == 1
    # a new optimizer plan (load_state_dict replaces the state tensors the captured launch reads): captured again, and the step still updates
    opt.load_state_dict(opt.state_dict())
    step(*a)
    assert step.captures == 2 and step.graph_for(*a) is not graph
    p2 = _params(model)
    assert not torch.equal(p2, p1) and bool(torch.isfinite(p2).all())
    step(*a)
    assert step.captures == 2 and not torch.equal(_params(model), p2)
    # eval mode: the training graph is never replayed
    model.eval()
    with pytest.raises(RuntimeError):
        step(*a)
    model.train()
    step(*a)
    assert step.captures == 2


def test_partial_batch_and_the_meter_against_the_logits(mods):
    """An epoch of four batches of 8 and a last one of 5: the meter equals the definition recomputed on the CPU from the logits of every iteration (the short batch with
    its own 1 / n)."""
    F, H = mods
    model, opt, step = _classifier(mods)
    batches = _batches(4) + _batches(1, n=5, seed=9)
    step.reset_record()
    ref = H.EpochMeter("cpu")
    losses = []
    for x, t in batches:
        loss = step(x, t)
        assert tuple(step.logits.shape) == (x.size(0), 1000)
        losses.append(float(loss))
        ref.update_reference(step.logits.clone().cpu(), t.cpu())
    assert step.captures == 1 and step.graph_for(*batches[0]) is not None and step.graph_for(*batches[4]) is None
    got, want = step.meter.read(), ref.read()
    print(f"[meter] device {got} definition {want} losses {losses}")
    assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[0] - sum(losses) / 5) <= 1e-6 * want[0]
    assert abs(got[1] - want[1]) <= 1e-12 * max(want[1], 1.0) and abs(got[2] - want[2]) <= 1e-12 * max(want[2], 1.0)
    # the partial signature gets its own graph after its warm-up, beside the full one
    for _ in range(2):
        step(*batches[4])
    assert step.captures == 2 and step.graph_for(*batches[4]) is not None and step.graph_for(*batches[0]) is not None
    assert math.isfinite(float(step(*batches[0]))) and math.isfinite(float(step(*batches[4])))


def test_graphed_step_equals_eager_step_from_the_same_state(mods):
    """One step each from the SAME restored state, the comparison and the bounds of tests/test_gpu_dp.py::test_graph_segments_replay_equals_eager: the forward is
    reproducible (loss and forward state to 1e-6; measured bit-equal), the backward differs by the order of its fp32 atomics and the bf16 roundings that order flips
    (measured over four runs: eager against graph 2.3e-7 ... 7.1e-3, graph against graph 2.2e-4 ... 1.4e-2)."""
    model, opt, step = _classifier(mods, drop_rate=0.0)
    (a,) = _batches(1)
    _warm(step, a)
    runner = model.hip_runner()
    torch.cuda.synchronize()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def one(graph):
        model.load_state_dict(sd0)
        step.capture = graph
        loss = float(step(*a))
        torch.cuda.synchronize()
        post = torch.cat([v.detach().float().reshape(-1) for k, v in model.state_dict().items() if "running_" in k or "min_val" in k or "max_val" in k])
        return loss, runner.grad_arena.clone(), torch.nan_to_num(post, posinf=0.0, neginf=0.0)
    le, ge_, se = one(False)
    lg, gg, sg = one(True)
    lg2, gg2, _ = one(True)
    rel_g, rel_g2, rel_s = float((ge_ - gg).norm() / ge_.norm()), float((gg2 - gg).norm() / gg.norm()), float((se - sg).norm() / se.norm())
    print(f"[graphed step] loss eager {le:.7f} graph {lg:.7f}; gradient rel eager/graph {rel_g:.2e}, graph/graph {rel_g2:.2e}; forward state rel {rel_s:.2e}")
    assert step.captures == 1
    assert abs(le - lg) <= 1e-6 * abs(le) and lg2 == lg
    assert rel_s <= 1e-6
    assert rel_g <= 2e-2 and rel_g2 <= 2e-2


# ------------------------------------------------------------------------------------------------------------------- 3. the loops
def _tie_free_targets(model, xs, sd0):
    """One eval pass in the loop's order from the restored state; per row a class whose (fake-quantised) logit no other class shares: the row maximum where it is unique."""
    model.load_state_dict(sd0)
    model.eval()
    out = []
    with torch.no_grad():
        for x in xs:
            logits = model(x).cpu()
            t = torch.empty(x.size(0), dtype=torch.int64)
            for r in range(x.size(0)):
                vals, inv, cnt = torch.unique(logits[r], return_inverse=True, return_counts=True)
                uniq = (cnt[inv] == 1).nonzero().flatten()
                assert uniq.numel() > 0
                top = int(logits[r].argmax())
                t[r] = top if r % 2 == 0 and int(cnt[inv[top]]) == 1 else int(uniq[r % uniq.numel()])
            out.append(t.cuda())
    return out


def test_train_and_val_loops_graphed(mods):
    F, H = mods
    model, opt, _ = _classifier(mods)
    loader = _batches(4)
    tr = H.train(loader, model, H.CrossEntropyLoss(), opt, 0, graph=True)
    assert all(math.isfinite(v) for v in tr) and 0.0 <= tr[1] <= tr[2] <= 100.0
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    xs = [x for x, _ in loader]
    loader = list(zip(xs, _tie_free_targets(model, xs, sd0)))
    model.load_state_dict(sd0)
    eager = H.val(loader, model, H.CrossEntropyLoss())
    model.load_state_dict(sd0)
    vstep = H.GraphedStep(model, H.CrossEntropyLoss())
    graphed = H.val(loader, model, H.CrossEntropyLoss(), graph=vstep)
    print(f"[loops] train {tr} val eager {eager} graphed {graphed}")
    assert vstep.captures == 1 and not model.training
    assert all(math.isfinite(v) for v in graphed)
    assert abs(graphed[0] - eager[0]) <= 1e-6 * eager[0] and graphed[1] == eager[1] and graphed[2] == eager[2]
    assert eager[1] > 0.0                                              # the targets were chosen to hit on the even rows
    model.load_state_dict(sd0)
    again = H.val(loader, model, None, graph=vstep)                    # the capture survives: every batch replays
    assert vstep.captures == 1 and abs(again[0] - graphed[0]) <= 1e-12 * graphed[0] and again[1:] == graphed[1:]


def test_transform_draws_fresh_crops_at_every_replay(mods):
    """`(images uint8, sizes, target)` from pinned host memory through the copy stream, ClassificationAugmentation inside the graph: the same batch gives other crops, hence
    other logits, at every replay."""
    F, H = mods
    from frostnet_amd import ClassificationAugmentation
    model, opt, step = _classifier(mods, drop_rate=0.0, transform=ClassificationAugmentation(size=RES, seed=5))
    g = torch.Generator().manual_seed(2)
    images = torch.randint(0, 256, (B, 80, 96, 3), dtype=torch.uint8, generator=g).pin_memory()
    sizes = torch.tensor([[80 - i, 96 - 2 * i] for i in range(B)], dtype=torch.int32).pin_memory()
    target = torch.randint(0, 1000, (B,), generator=g).pin_memory()
    _warm(step, (images, sizes, target))
    seen0 = step.transform.images_seen()
    for g_ in opt.param_groups:          # the parameters stay: what differs between the replays is the crop
        g_["lr"], g_["weight_decay"] = 0.0, 0.0
    step(images, sizes, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    outs = []
    for _ in range(2):
        model.load_state_dict(sd0)
        step(images, sizes, target)
        outs.append(step.logits.clone())
    assert step.captures == 1 and step.transform.images_seen() == seen0 + 3 * B
    assert not torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    # and a replay reads the NEW host batch: other images, same stream position, other logits
    model.load_state_dict(sd0)
    state = step.transform.state_dict()
    step(images, sizes, target)
    ref = step.logits.clone()
    model.load_state_dict(sd0)
    step.transform.load_state_dict(state)
    step(images, sizes, target)
    assert torch.equal(step.logits, ref)
    model.load_state_dict(sd0)
    step.transform.load_state_dict(state)
    step((255 - images).pin_memory(), sizes, target)
    assert not torch.equal(step.logits, ref)


def _det_targets(n):
    g = torch.Generator().manual_seed(77)
    out = []
    for i in range(n):
        k = 1 + i % 3
        c, wh = torch.rand(k, 2, generator=g) * 0.5 + 0.25, torch.rand(k, 2, generator=g) * 0.3 + 0.1
        out.append(torch.cat([c - wh / 2, c + wh / 2, torch.randint(0, 20, (k, 1), generator=g).float()], 1))
    return out


class _RecordingLoader:
    """Two detector batches; notes the step's (loss_l, loss_c) of the iteration that just ran whenever the loop comes back for the next batch."""

    def __init__(self, batches):
        self.batches, self.step, self.terms, self.passes = batches, None, [], 0

    def __iter__(self):
        self.passes += 1
        for i, b in enumerate(self.batches):
            if i > 0 or self.passes > 1:
                self.terms.append(self.step.loss_terms.clone())
            yield b


def test_train_detector_graphed(mods):
    F, H = mods
    from frostnet_amd import ssdlite as S
    from frostnet_amd.optimizer import QSGD
    torch.manual_seed(2)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128))
    F.qat_prepare(model, version=0)
    model.cuda().train()
    lr, gamma = 4e-3, 0.5
    opt = QSGD(H.make_param_groups(model, 1e-5), lr=lr, momentum=0.9, nesterov=True)
    crit = S.MultiBoxLoss(21)
    boxes, valid = S.pad_targets(_det_targets(4), "cuda")
    g = torch.Generator().manual_seed(4)
    loader = _RecordingLoader([(torch.randn(4, 3, 128, 128, generator=g).cuda(), boxes, valid) for _ in range(2)])
    step = H.GraphedStep(model, crit, opt)
    loader.step = step
    p0 = _params(model)
    ll, lc = H.train_detector(loader, model, crit, opt, 0, 6, lr, gamma, (2, 4), graph=step)
    loader.terms.append(step.loss_terms.clone())
    terms = torch.stack(loader.terms).double().cpu()
    print(f"[train_detector] mean loss_l {ll:.6f} loss_c {lc:.6f}; per iteration {terms.tolist()}")
    assert terms.shape == (6, 2) and loader.passes == 3 and step.captures == 1
    assert all(g_["lr"] == lr * gamma ** 2 for g_ in opt.param_groups)
    want = terms.mean(0).tolist()
    assert abs(ll - want[0]) <= 1e-12 * want[0] and abs(lc - want[1]) <= 1e-12 * want[1]
    assert math.isfinite(ll) and math.isfinite(lc) and abs(float(step.loss) - float(terms[-1].sum())) <= 1e-6 * float(terms[-1].sum())
    assert [int(opt.state[p]["step"]) for p in model.parameters()] == [6] * len(list(model.parameters()))
    p1 = _params(model)
    assert not torch.equal(p0, p1) and bool(torch.isfinite(p1).all())
    # resumed at iteration 3: the entry at 2 lies behind it, so the entry at 4 is the second one
    for g_ in opt.param_groups:
        g_["lr"] = lr
    H.train_detector(loader, model, crit, opt, 3, 5, lr, gamma, (2, 4), graph=step)
    assert all(g_["lr"] == lr * gamma ** 2 for g_ in opt.param_groups) and step.captures == 1


def test_one_rank_process_group_routes_through_segmented_step(mods, tmp_path):
    import torch.distributed as dist
    F, H = mods
    from frostnet_amd.optimizer import QSGD
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(str(tmp_path), 'pg')}", rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        model = F.frostnet_quant_small_1_0(drop_rate=0.0)
        F.qat_prepare(model, version=0)
        model.cuda().train()
        opt = QSGD([{"params": [p]} for p in model.parameters()], lr=1e-3, momentum=0.9, nesterov=True)
        step = H.GraphedStep(model, H.CrossEntropyLoss(), opt, nbuckets=3, group=dist.group.WORLD)
        (a,) = _batches(1)
        step.reset_record()
        for _ in range(3):
            step(*a)
        graphs = step.graph_for(*a)
        assert isinstance(graphs, list) and len(graphs) >= 2 and step.captures == 1          # a chain of segments, collectives between them
        p0 = _params(model)
        loss = float(step(*a))
        p1 = _params(model)
        assert math.isfinite(loss) and not torch.equal(p0, p1) and bool(torch.isfinite(p1).all())
        got = step.meter.read()
        assert step.meter.record.tolist()[3] == 4.0 and math.isfinite(got[0])
    finally:
        dist.destroy_process_group()

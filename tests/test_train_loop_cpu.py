"""CPU side of the graphed loops (harness.EpochMeter / CrossEntropyWithMetrics / GraphedStep / train(graph=True)): the meter's definition against cases worked out
by hand (ties, an ignored target, a target logit of -inf, topk > C), a float CPU model through the graphed loop entry points (they run the same iteration eagerly
there), and the new export in header, binding and library."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import frostnet_amd
    return frostnet_amd


def _lse(row):
    m = max(row)
    return m + math.log(sum(math.exp(v - m) for v in row))


def test_epoch_meter_definition_by_hand():
    from frostnet_amd import harness as H
    rows = [[1.0, 3.0, 3.0, 0.0],      # target 2 ties with the LOWER index 1: rank 1 -> top-1 miss, top-2 hit
            [2.0, 2.0, 1.0, 0.0],      # target 0 ties with the HIGHER index 1: rank 0 -> hit, hit
            [0.0, 1.0, 2.0, 3.0],      # ignored target: miss, miss, no loss
            [5.0, 1.0, 1.0, 1.0],      # plain hit
            [0.0, 1.0, 2.0, 3.0]]      # target 1: rank 2 -> miss, miss at topk = 2
    tgt = [2, 0, -100, 0, 1]
    meter = H.EpochMeter("cpu", topk=2)
    loss = meter.update(torch.tensor(rows), torch.tensor(tgt))
    inv_n = float(torch.tensor(1.0 / 5, dtype=torch.float32))
    want_loss = sum(_lse(r) - r[t] for r, t in zip(rows, tgt) if t >= 0) * inv_n
    rec = meter.record.tolist()
    assert abs(rec[0] - want_loss) <= 1e-12 * want_loss and abs(float(loss) - want_loss) <= 1e-12 * want_loss
    assert rec[1] == 2 * (100.0 * inv_n) and rec[2] == 3 * (100.0 * inv_n) and rec[3] == 1.0
    meter.update(torch.tensor(rows), torch.tensor(tgt))
    l, a1, ak = meter.read()
    assert abs(l - want_loss) <= 1e-12 * want_loss and a1 == 2 * (100.0 * inv_n) and ak == 3 * (100.0 * inv_n)       # the mean over two equal batches
    meter.reset()
    assert meter.record.tolist() == [0.0] * 4
    with pytest.raises(ValueError):
        meter.read()


def test_epoch_meter_non_finite_target_and_topk_beyond_classes():
    from frostnet_amd import harness as H
    x = torch.tensor([[0.5, float("-inf"), 0.25], [0.1, 0.2, 0.3], [float("nan"), 0.0, 1.0]])
    meter = H.EpochMeter("cpu", topk=5)                      # topk > C: every finite, valid target is a top-k hit
    meter.update(x, torch.tensor([1, 0, 0]))
    rec = meter.record.tolist()
    inv_n = float(torch.tensor(1.0 / 3, dtype=torch.float32))
    assert rec[1] == 0.0 and rec[2] == 1 * (100.0 * inv_n)   # row 0: -inf target logit, row 2: NaN target logit -> misses; row 1: rank 2 < min(5, 3)
    assert not math.isfinite(rec[0])                         # the loss of a -inf target logit is +inf, as cross-entropy defines it
    with pytest.raises(ValueError):
        meter.update(torch.zeros(3), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        H.EpochMeter("cpu", topk=0)


def test_epoch_meter_matches_accuracy_without_ties():
    from frostnet_amd import harness as H
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(16, 10, generator=g), torch.randint(0, 10, (16,), generator=g)
    meter = H.EpochMeter("cpu", topk=5)
    crit = H.CrossEntropyWithMetrics(meter)
    xr = x.clone().requires_grad_(True)
    loss = crit(xr, t)
    loss.backward()
    ref = x.clone().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref, t)
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * float(want.detach()) and torch.allclose(xr.grad, ref.grad, rtol=1e-5, atol=1e-8)
    a1, a5 = H.accuracy(x, t, topk=(1, 5))
    l, m1, m5 = meter.read()
    assert m1 == float(a1) and m5 == float(a5) and abs(l - float(want)) <= 1e-6 * float(want)      # 100 / 16 is exact in fp32


def _tiny(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 32), torch.nn.ReLU(), torch.nn.Linear(32, 10))


def _loader():
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(8, 3, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(4)]


def test_float_cpu_model_runs_the_graphed_loops_eagerly():
    """On the CPU `graph=True` is the same iteration with eager launches: the triple equals graph=False's (fp32 rounding of the batch loss: 1e-6; 100 / 8 exact)."""
    from frostnet_amd import harness as H
    loader = _loader()
    out = []
    for graph in (False, True):
        model = _tiny(5)
        opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
        tr = H.train(loader, model, torch.nn.CrossEntropyLoss(), opt, 0, graph=graph)
        va = H.val(loader, model, H.CrossEntropyLoss(), graph=graph)
        out.append((tr, va, [p.detach().clone() for p in model.parameters()]))
    for a, b in zip(out[0][:2], out[1][:2]):
        assert abs(a[0] - b[0]) <= 1e-6 * abs(a[0]) and a[1] == b[1] and a[2] == b[2], (a, b)
    assert all(torch.allclose(p, q, rtol=1e-5, atol=1e-7) for p, q in zip(out[0][2], out[1][2]))      # the optimizer really stepped, the same way
    model = _tiny(5)
    step = H.GraphedStep(model, torch.nn.CrossEntropyLoss(), torch.optim.SGD(model.parameters(), lr=0.05))
    H.train(loader, model, None, step.optimizer, 0, graph=step)
    assert step.captures == 0 and step.graph_for(*loader[0]) is None and tuple(step.logits.shape) == (8, 10)
    with pytest.raises(ValueError):
        H.train(loader, _tiny(6), None, step.optimizer, 0, graph=step)          # a GraphedStep built for another model
    with pytest.raises(ValueError):
        H.train([], model, None, step.optimizer, 0, graph=step)


def test_own_criterion_records_its_loss_with_the_meters_hits():
    from frostnet_amd import harness as H
    loader = _loader()
    model = _tiny(7)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    want = sum(float(crit(model(x), t)) for x, t in loader) / len(loader)
    got = H.val(loader, model, crit, graph=True)
    ref = H.val(loader, model, crit)
    assert abs(got[0] - want) <= 1e-6 * want and got[1:] == ref[1:]


def test_new_symbol_in_header_binding_and_library(built):
    hdr = open(os.path.join(ROOT, "include", "frost_hip.h")).read()
    declared = set(re.findall(r"\b(frost_[a-z0-9_]+)\s*\(", hdr))
    assert "frost_softmax_ce_metrics" in declared and "frost_softmax_ce_metrics" in built.SYMBOLS
    assert hasattr(ctypes.CDLL(built.LIB_PATH), "frost_softmax_ce_metrics")
    from frostnet_amd import _lib
    assert len(_lib._PROTOS["frost_softmax_ce_metrics"]) == 10
    m = re.search(r"int frost_softmax_ce_metrics\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 10
    assert built.load_library().frost_abi_version() == 5          # an additive export

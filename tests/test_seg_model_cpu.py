"""frostnet_amd.seg_model on the CPU: LRASPPHead against the reference's own head (tests/golden/g20_seg_head.npz, written by tools/gen_golden_seg_head.py), and the
surface of FrostNetSeg -- output shapes, pool defaults, parameter order and names, the guard for a map smaller than the pool window."""
import pytest
import torch

from frostnet_amd import FrostNetSeg, LRASPPHead, frostnet_seg_base_1_0, frostnet_seg_large_1_0, frostnet_seg_small_1_0

N, C4, C1, NCLASS = 2, 16, 8, 6


def nrel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def golden_head(g):
    head = LRASPPHead(NCLASS, C4, C1, dataset="pascal", c4_stride=16)
    missing = head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w/")})
    assert not missing.missing_keys and not missing.unexpected_keys
    return head


def test_head_reproduces_the_reference_head(golden):
    g = golden("g20_seg_head")
    head = golden_head(g).train()
    assert (head.pool_kernel, head.pool_stride) == ((25, 25), (8, 8))
    c1, c4 = torch.from_numpy(g["c1"]).requires_grad_(True), torch.from_numpy(g["c4"]).requires_grad_(True)
    out = head(c1, c4)
    out.backward(torch.from_numpy(g["gout"]))
    assert nrel(out.detach(), torch.from_numpy(g["out"])) <= 2e-6
    assert nrel(c1.grad, torch.from_numpy(g["dc1"])) <= 1e-5 and nrel(c4.grad, torch.from_numpy(g["dc4"])) <= 1e-5
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    assert sorted(names) == sorted(n for n, _ in head.named_parameters())
    for n, p in head.named_parameters():
        assert nrel(p.grad, torch.from_numpy(g["grad/" + n])) <= 1e-5, n
    sd = head.state_dict()
    stats = [k[5:] for k in g.files if k.startswith("stat/")]
    assert len(stats) == 6
    for k in stats:
        if "num_batches" in k:
            assert int(sd[k]) == int(g["stat/" + k]) == 1
        else:
            torch.testing.assert_close(sd[k], torch.from_numpy(g["stat/" + k]), rtol=1e-5, atol=0)
    head.eval()
    with torch.no_grad():
        assert nrel(head(c1, c4), torch.from_numpy(g["out_eval"])) <= 2e-6


@pytest.mark.parametrize("mode,factory", [("large", frostnet_seg_large_1_0), ("base", frostnet_seg_base_1_0), ("small", frostnet_seg_small_1_0)])
def test_output_shapes(mode, factory):
    m = factory(21, pool_kernel=3, pool_stride=2).eval()
    assert isinstance(m, FrostNetSeg) and m.mode == mode and factory.__name__ == f"frostnet_seg_{mode}_1_0"
    assert m.head.inter_channels == (40 if mode == "large" else m.layer2[-1].out_channels) and m.head.in_channels == m.layer5[-1].out_channels
    x = torch.randn(2, 3, 129, 161)
    with torch.no_grad():
        assert tuple(m(x).shape) == (2, 21, 17, 21)
        m.upsample = True
        assert tuple(m(x).shape) == (2, 21, 129, 161)


def test_pool_defaults():
    want = {("pascal", 16): ((25, 25), (8, 8)), ("city", 16): ((37, 37), (12, 12)), ("pascal", 32): ((13, 13), (4, 4)), ("city", 32): ((19, 19), (6, 6))}
    for (ds, stride), (k, s) in want.items():
        h = LRASPPHead(21, 16, 8, dataset=ds, c4_stride=stride)
        assert (h.pool_kernel, h.pool_stride) == (k, s)
        assert (h.lr_aspp.b1[0].kernel_size, h.lr_aspp.b1[0].stride) == (k, s)
    h = LRASPPHead(21, 16, 8)                                   # the default is the FrostNet tap: stride 32, PASCAL; 513^2 -> 17^2 -> 2 x 2
    assert (h.pool_kernel, h.pool_stride) == ((13, 13), (4, 4)) and (17 - 13) // 4 + 1 == 2
    h = LRASPPHead(21, 16, 8, dataset="city", pool_kernel=(3, 5), pool_stride=2)
    assert (h.pool_kernel, h.pool_stride) == ((3, 5), (2, 2))
    assert FrostNetSeg(21, "small", dataset="city").head.pool_kernel == (19, 19)
    with pytest.raises(ValueError):
        LRASPPHead(21, 16, 8, c4_stride=8)


def test_parameter_order_and_names():
    h = LRASPPHead(6, 16, 8)
    assert [n for n, _ in h.named_parameters()] == [
        "lr_aspp.b0.conv.0.weight", "lr_aspp.b0.conv.1.weight", "lr_aspp.b0.conv.1.bias", "lr_aspp.b1.1.conv.0.weight", "lr_aspp.b1.1.conv.1.weight",
        "lr_aspp.b1.1.conv.1.bias", "project.weight", "project.bias", "auxlayer.weight", "auxlayer.bias"]
    assert tuple(h.project.weight.shape) == (6, 128, 1, 1) and tuple(h.auxlayer.weight.shape) == (6, 8, 1, 1)
    m = FrostNetSeg(6, "small")
    names = [n for n, _ in m.named_parameters()]
    assert names[0] == "conv1.conv.0.weight" and names[-10:] == ["head." + n for n, _ in h.named_parameters()]
    first_head = names.index("head.lr_aspp.b0.conv.0.weight")
    assert all(n.startswith(("conv1.", "layer")) for n in names[:first_head]) and len(names) - first_head == 10
    from frostnet_amd.topology import SEG_TAPS, plan_tree
    plan = plan_tree(m)
    assert SEG_TAPS == (1, 4) and plan.classifier is None and plan.last_layer is None and not plan.extras and not plan.heads
    assert [plan.blocks[plan.stage_ends[i]].block.out_channels for i in SEG_TAPS] == [m.head.inter_channels, m.head.in_channels]


def test_window_larger_than_the_map_and_class_range():
    m = FrostNetSeg(21, "small").eval()                            # default window 13: a 129 x 161 image gives a 5 x 6 map
    with pytest.raises(ValueError, match=r"5 x 6.*13 x 13"):
        m(torch.randn(1, 3, 129, 161))
    for bad in (1, 256):
        with pytest.raises(ValueError):
            LRASPPHead(bad, 16, 8)

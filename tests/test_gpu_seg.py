"""frost_seg_forward on the device (csrc/frost_seg.hip through frostnet_amd.seg) against its definition, seg_reference, in fp64 on the CPU.

Tolerances (nothing taken from the device).  Loss and dx: max(2e-6, 8 E32) norm-wise, E32 = fp32 seg_reference against fp64; twice that for the worst class
plane of dx.  Counts: exact.  The device interpolates in fp32 and may order two nearly equal classes differently from fp64, so before either side runs every pixel
whose fp64 top-2 margin is below BAND_RTOL * max|u| gets the target 255; the share of such pixels is asserted to stay below BAND_SHARE.  On the identity shape with
logits from a small integer grid (exact ties everywhere) counts are exact with no band: lowest index wins.
Every check prints `[seg] what: observed / bound / E32`; DESIGN.md ("Segmentation criterion") lists the worst."""
import pytest
import torch

from seg_common import T, bound, golden_val, hold, make_case, nrm

pytestmark = pytest.mark.gpu
BAND_RTOL, BAND_SHARE = 1e-5, 1e-3
SHAPES = [(2, 19, (1, 3), (5, 9)), (2, 20, (5, 7), (33, 41)), (2, 21, (8, 8), (64, 64)), (3, 21, (19, 23), (150, 181)), (2, 21, (9, 11), (9, 11)),
          (1, 2, (4, 4), (16, 16)), (1, 150, (6, 6), (24, 24))]
LARGEST = SHAPES[3]
_REF = {}


def _sid(s):
    return f"{s[0]}x{s[1]}_{s[2][0]}x{s[2][1]}_{s[3][0]}x{s[3][1]}"


@pytest.fixture(scope="module")
def seg():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import seg
    assert torch.cuda.is_available()
    return seg


def _case(seg, shape, weights, integer_grid=False):
    """Inputs with the near-tie band removed, and the fp64 / fp32 references: computed once per (shape, weights), never modified."""
    key = (shape, weights, integer_grid)
    if key not in _REF:
        n, c, hw, HW = shape
        x, t, wt = make_case(n, c, hw, HW, seed=13 + c, weights=weights, integer_grid=integer_grid)
        share = 0.0
        if not integer_grid:
            u = seg.upsample_reference(x.double(), HW)
            top2 = u.topk(2, dim=1).values
            band = (top2[:, 0] - top2[:, 1]) < BAND_RTOL * float(u.abs().max())
            share = float(band.double().mean())
            t = torch.where(band, torch.full_like(t, 255), t)
        ref64 = seg.seg_reference(x.double(), t, None if wt is None else wt.double())
        ref32 = seg.seg_reference(x, t, wt)
        _REF[key] = (x, t, wt, ref64, ref32, share)
    return _REF[key]


def _run(seg, x, t, wt, c, layout="nchw", meter=True):
    """One criterion call on the device -> (loss, dx, state or None)."""
    xd = x.cuda()
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    m = seg.SegMeter(c, "cuda") if meter else None
    crit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt, meter=m)
    loss = crit(xd, t.cuda())
    (dx,) = torch.autograd.grad(loss, xd)
    assert dx.stride() == xd.stride()
    return loss.detach(), dx, (m.state.clone() if meter else None), m


def _hold_planes(what, dx, d64, d32):
    e32 = nrm(d32, d64)
    worst = max(nrm(dx[:, k], d64[:, k]) for k in range(d64.size(1)))
    bnd = 2 * bound(e32)
    print(f"[seg] {what} worst class plane: observed {worst:.2e} bound {bnd:.2e} E32 {e32:.2e}")
    assert worst <= bnd


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("tdtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_loss_gradient_and_counts(seg, shape, layout, tdtype, weights):
    n, c, hw, HW = shape
    x, t, wt, ref64, ref32, share = _case(seg, shape, weights)
    assert share <= BAND_SHARE, f"near-tie share {share:.2e}"
    loss, dx, state, meter = _run(seg, x, t.to(tdtype), wt, c, layout)
    tag = f"{_sid(shape)} {layout}"
    hold(f"{tag} loss", loss.reshape(1), ref64[0].reshape(1), ref32[0].reshape(1))
    hold(f"{tag} dx", dx, ref64[1], ref32[1])
    _hold_planes(f"{tag} dx", dx.cpu(), ref64[1], ref32[1])
    st = state.cpu()
    assert torch.equal(st[:c], ref64[2]) and torch.equal(st[c:2 * c], ref64[3]) and torch.equal(st[2 * c:3 * c], ref64[4])
    assert int(st[3 * c]) == 1 and int(st[3 * c + 1]) == 0
    # counts alone (the meter's own launch) and loss alone (validation) are the same numbers
    meter.reset()
    meter.update(x.cuda(), t.to(tdtype).cuda())
    assert torch.equal(meter.state.cpu(), st)
    with torch.no_grad():
        lv = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt)(x.cuda(), t.cuda())
    hold(f"{tag} loss without gradient", lv.reshape(1), ref64[0].reshape(1), ref32[0].reshape(1))


@pytest.mark.parametrize("shape", [(3, 5, (32, 32), (272, 272)), (1, 5, (136, 136), (136, 136))], ids=_sid)
def test_more_than_64_workgroups(seg, shape):
    """Past 64 workgroups the ordered loss sum and the W_sum pass take the two-level ticket: 96 tiles and 109 W_sum workgroups on the first shape, 73 workgroups of
    the one-read kernel on the second.  Same bounds; and the result is the same bits on a second run."""
    n, c, hw, HW = shape
    x, t, wt, ref64, ref32, share = _case(seg, shape, True)
    assert share <= BAND_SHARE, f"near-tie share {share:.2e}"
    loss, dx, state, _ = _run(seg, x, t, wt, c)
    hold(f"{_sid(shape)} loss", loss.reshape(1), ref64[0].reshape(1), ref32[0].reshape(1))
    hold(f"{_sid(shape)} dx", dx, ref64[1], ref32[1])
    st = state.cpu()
    assert torch.equal(st[:c], ref64[2]) and torch.equal(st[c:2 * c], ref64[3]) and torch.equal(st[2 * c:3 * c], ref64[4])
    loss2, dx2, state2, _ = _run(seg, x, t, wt, c)
    assert torch.equal(loss2, loss) and torch.equal(dx2, dx) and torch.equal(state2, state)


def test_identity_ties_go_to_the_lowest_index(seg):
    shape = SHAPES[4]
    n, c, hw, HW = shape
    x, t, wt, ref64, ref32, _ = _case(seg, shape, True, integer_grid=True)
    for layout in ("nchw", "nhwc"):
        loss, dx, state, _ = _run(seg, x, t, wt, c, layout)
        st = state.cpu()
        assert torch.equal(st[:c], ref64[2]) and torch.equal(st[c:2 * c], ref64[3]) and torch.equal(st[2 * c:3 * c], ref64[4])
        hold(f"ties {layout} dx", dx, ref64[1], ref32[1])


def test_upsampled_ties_go_to_the_lowest_index(seg):
    """Constant logits per class pair: every upsampled pixel ties exactly (an interpolation of equal values), whatever the weights."""
    x = torch.zeros(1, 5, 4, 4)
    x[:, 1] = 1.0
    x[:, 3] = 1.0
    t = torch.randint(0, 5, (1, 16, 16), generator=torch.Generator().manual_seed(5))
    m = seg.SegMeter(5, "cuda")
    m.update(x.cuda(), t.cuda())
    inter, ap, am = m.areas()
    assert ap.tolist() == [0, 256, 0, 0, 0] and int(inter[1]) == int((t == 1).sum())


def test_golden_on_the_device(seg, golden):
    from frostnet_amd import harness
    g = golden("g18_seg")
    x, x2, t, wt = T(g["x"]), T(g["x2"]), T(g["target"]), T(g["class_wts"])
    for tag, w in (("", wt), ("_plain", None)):
        l64, d64, inter, ap, am = seg.seg_reference(x.double(), t, None if w is None else w.double())
        l32, d32, *_ = seg.seg_reference(x, t, w)
        loss, dx, state, _ = _run(seg, x, t, w, 19)
        hold(f"golden device loss{tag}", loss.reshape(1), l64.reshape(1), l32.reshape(1))
        hold(f"golden device gx{tag}", dx, d64, d32)
        hold(f"golden file loss{tag}", T(g["loss" + tag]).reshape(1), l64.reshape(1), l32.reshape(1))
        st = state.cpu()
        assert torch.equal(st[:19], T(g["inter"]).long())
        assert torch.equal(st[19:38] + st[38:57] - st[:19], T(g["union"]).double().round().long())
    # the tuple of two outputs: the sum of the two losses
    m = seg.SegMeter(19, "cuda")
    crit = seg.SegmentationLoss(n_classes=19, device="cuda", class_wts=wt, meter=m)
    xa, xb = x.cuda().requires_grad_(True), x2.cuda().requires_grad_(True)
    loss = crit((xa, xb), t.cuda())
    loss.backward()
    ra, rb = seg.seg_reference(x.double(), t, wt.double()), seg.seg_reference(x2.double(), t, wt.double())
    ra32, rb32 = seg.seg_reference(x, t, wt), seg.seg_reference(x2, t, wt)
    hold("golden device tuple loss", loss.detach().reshape(1), (ra[0] + rb[0]).reshape(1), (ra32[0] + rb32[0]).reshape(1))
    hold("golden device tuple gx", xa.grad, ra[1], ra32[1])
    hold("golden device tuple gx2", xb.grad, rb[1], rb32[1])
    assert torch.equal(m.areas()[0], T(g["inter"]).long()) and int(m.state[3 * 19]) == 1          # the meter saw inputs[0] once
    # val_seg's pair
    model, loader = golden_val(g, "cuda")
    crit = seg.SegmentationLoss(n_classes=19, device="cuda", class_wts=wt)
    miou, vloss = harness.val_seg(model, loader, criterion=crit, num_classes=19, device="cuda")
    assert abs(miou - float(g["val_miou"])) <= 3e-4, (miou, float(g["val_miou"]))
    sizes, l64, l32 = [2, 3, 1], [], []
    for i in range(3):
        xi, ti = T(g[f"val_x{i}"]), T(g[f"val_t{i}"])
        l64.append(seg.seg_reference(xi.double(), ti, wt.double())[0] * sizes[i])
        l32.append(seg.seg_reference(xi, ti, wt)[0].double() * sizes[i])
    hold("golden device val_seg loss", torch.tensor([vloss], dtype=torch.float64), (sum(l64) / 6).reshape(1), (sum(l32) / 6).reshape(1))


def test_no_valid_pixel(seg):
    for shape in (SHAPES[2], SHAPES[4]):
        n, c, hw, HW = shape
        x, t, wt = make_case(n, c, hw, HW, seed=1, weights=True)
        t = torch.where(t == 255, t, torch.full_like(t, 3))          # only the zero-weight class and ignored pixels: W_sum == 0
        assert float(wt[3]) == 0.0
        loss, dx, state, meter = _run(seg, x, t, wt, c)
        assert torch.isnan(loss) and not dx.any()
        t[:] = 255
        before = meter.state.clone()
        loss, dx, _, _ = _run(seg, x, t, wt, c, meter=False)
        assert torch.isnan(loss) and not dx.any()
        xd = x.cuda().requires_grad_(True)
        seg.SegmentationLoss(n_classes=c, device="cuda", meter=meter)(xd, t.cuda())
        after = meter.state
        assert torch.equal(after[:3 * c], before[:3 * c]) and int(after[3 * c]) == int(before[3 * c]) + 1


def test_out_of_range_target_is_counted_and_never_an_index(seg):
    for shape in (SHAPES[2], SHAPES[4]):
        n, c, hw, HW = shape
        x, t, wt, ref64, ref32, _ = _case(seg, shape, False)
        t2 = t.clone()
        t2[0, 0, 0] = 255                                           # the reference sees it ignored
        ref = seg.seg_reference(x.double(), t2)
        t2[0, 0, 0] = 200
        loss, dx, state, meter = _run(seg, x, t2, None, c)
        assert int(state[-1]) == 1 and torch.equal(state[:c].cpu(), ref[2])
        hold("out-of-range loss", loss.reshape(1), ref[0].reshape(1), seg.seg_reference(x, t2)[0].reshape(1))
        with pytest.raises(ValueError):
            meter.compute()


def test_run_to_run_bit_identical(seg):
    n, c, hw, HW = LARGEST
    x, t, wt, *_ = _case(seg, LARGEST, True)
    runs = [_run(seg, x, t, wt, c)[:3] for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])


def test_captured_criterion_and_meter_replay(seg):
    n, c, hw, HW = SHAPES[2]
    batches = [make_case(n, c, hw, HW, seed=40 + i, weights=True) for i in range(3)]
    wt = batches[0][2]
    sx = torch.zeros((n, c) + hw, device="cuda", requires_grad=True)
    st = torch.zeros((n,) + HW, dtype=torch.int64, device="cuda")
    gm, em = seg.SegMeter(c, "cuda"), seg.SegMeter(c, "cuda")
    gcrit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt, meter=gm)
    ecrit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt, meter=em)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(gcrit(sx, st), sx)                       # warm-up: workspace and weights exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    gm.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = gcrit(sx, st)
        (gdx,) = torch.autograd.grad(gloss, sx)
    gm.reset()
    for x, t, _ in batches:
        with torch.no_grad():
            sx.copy_(x)
        st.copy_(t)
        graph.replay()
        xe = x.cuda().requires_grad_(True)
        eloss = ecrit(xe, t.cuda())
        (edx,) = torch.autograd.grad(eloss, xe)
        assert torch.equal(gloss, eloss.detach()) and torch.equal(gdx, edx) and torch.equal(gm.state, em.state)
    assert int(gm.state[3 * c]) == 3 and gm.compute() == em.compute()


def test_full_resolution_logits_are_never_allocated(seg):
    n, c, hw, HW = 2, 21, (32, 32), (256, 256)
    x, t, wt = make_case(n, c, hw, HW, seed=9, weights=True)
    meter = seg.SegMeter(c, "cuda")
    crit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt, meter=meter)
    xd, td = x.cuda().requires_grad_(True), t.cuda()
    crit(xd, td).backward()                                          # workspace and weights allocated
    xd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    crit(xd, td).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    full = n * c * HW[0] * HW[1] * 4
    print(f"[seg] peak memory rise {rise} B, full-resolution logits {full} B")
    assert rise < full // 2


def test_autograd_through_a_conv_in_front(seg):
    n, c, hw, HW = 2, 21, (8, 8), (64, 64)
    _, t, wt = make_case(n, c, hw, HW, seed=21, weights=True)
    gen = torch.Generator().manual_seed(22)
    inp = torch.randn((n, 8) + hw, generator=gen)
    conv = torch.nn.Conv2d(8, c, 1)

    def wgrad(dtype, device):
        cv = torch.nn.Conv2d(8, c, 1).to(device=device, dtype=dtype)
        cv.load_state_dict({k: v.to(dtype) for k, v in conv.state_dict().items()})
        crit = seg.SegmentationLoss(n_classes=c, device=device, class_wts=wt)
        logits = cv(inp.to(device=device, dtype=dtype))
        logits.retain_grad()
        loss = crit(logits, t.to(device))
        loss.backward()
        return loss.detach(), cv.weight.grad, logits

    l64, w64, _ = wgrad(torch.float64, "cpu")
    l32, w32, _ = wgrad(torch.float32, "cpu")
    ld, wd, logits = wgrad(torch.float32, "cuda")
    hold("autograd conv weight gradient", wd, w64, w32)
    hold("autograd loss", ld.reshape(1), l64.reshape(1), l32.reshape(1))
    crit = seg.SegmentationLoss(n_classes=c, device="cuda", class_wts=wt)
    xd = logits.detach().clone().requires_grad_(True)
    (crit(xd, t.cuda()) * 3).backward()
    assert torch.equal(xd.grad, logits.grad * 3)


def _seg_model():
    torch.manual_seed(31)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, stride=2, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 5, 1))


def test_train_and_val_loops_against_the_cpu(seg):
    """train_seg for two iterations, then val_seg, on the device against the same loops on CPU copies.  The loss bound: max(2e-6, 8 E32) with E32 measured the
    same way on the whole pipeline (the fp32 CPU loop against the fp64 CPU loop), so it carries the model's own fp32 error."""
    import copy
    from frostnet_amd import harness
    c, gen = 5, torch.Generator().manual_seed(32)
    loader = [(torch.randn(2, 3, 16, 16, generator=gen), make_case(2, c, (8, 8), (32, 32), seed=33 + i)[1]) for i in range(2)]
    base = _seg_model()

    def loops(dtype, device):
        model = copy.deepcopy(base).to(device=device, dtype=dtype)
        data = [(a.to(dtype), b) for a, b in loader]
        crit = seg.SegmentationLoss(n_classes=c, device=device)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        tr = harness.train_seg(model, data, opt, crit, c, epoch=0, device=device)
        va = harness.val_seg(model, data, criterion=crit, num_classes=c, device=device)
        return tr, va

    r64, r32, rd = loops(torch.float64, "cpu"), loops(torch.float32, "cpu"), loops(torch.float32, "cuda")
    for k, name in enumerate(("train_seg", "val_seg")):
        assert abs(rd[k][0] - r64[k][0]) <= 1e-3, (name, rd[k][0], r64[k][0])
        hold(f"{name} loss", torch.tensor([rd[k][1]], dtype=torch.float64), torch.tensor([r64[k][1]], dtype=torch.float64),
             torch.tensor([r32[k][1]], dtype=torch.float64))


def test_refusals_on_the_device(seg):
    x, t, _ = make_case(2, 5, (4, 4), (8, 8), seed=2)
    crit = seg.SegmentationLoss(n_classes=5, device="cuda")
    with pytest.raises(ValueError):
        crit(x.cuda(), t[:, :3].cuda())
    with pytest.raises(ValueError):
        crit(x.cuda(), t.int().cuda())
    with pytest.raises(ValueError):
        crit(x.cuda(), t)                                            # targets on another device

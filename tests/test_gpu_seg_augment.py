"""The segmentation input pipeline on the device (csrc/frost_saug.hip behind frostnet_amd.seg_augment) against its CPU definition (the same classes on CPU tensors,
pinned to Pillow and to the reference by tests/test_seg_augment_cpu.py), at the smallest shapes at which the kernels can go wrong, and the plumbing: only
frost_saug_* entries run, capture into a HIP graph with a stream that advances per replay, the hand-over to harness.train_seg, argument errors.
Criterion: the decisions are fp64 in a written order with a written-out exp; the resampler's weights likewise, with a written-out sine, its passes integer
arithmetic; the label map is an index table of fp64 additions; the output is a table look-up.  So plan words, pixels and labels are expected EQUAL, and that is
what is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HMAX, WMAX = 80, 150
DIMS = [(80, 150), (64, 150), (80, 131), (37, 53)]          # (h, w) of the four pairs of one 80 x 150 slot


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib, seg_augment
    assert torch.cuda.is_available()
    return seg_augment, _lib


def _pairs(dims, hmax, wmax, sentinel, seed=31):
    """Random bytes and labels 0 .. 20 with 255 scattered in inside every image's own extent, the sentinel in the padding of its slot."""
    rng = np.random.default_rng(seed)
    images = np.full((len(dims), hmax, wmax, 3), sentinel, dtype=np.uint8)
    labels = np.full((len(dims), hmax, wmax), sentinel, dtype=np.uint8)
    for i, (h, w) in enumerate(dims):
        images[i, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 21, (h, w)).astype(np.uint8)
        lab[rng.random((h, w)) < 0.1] = 255
        labels[i, :h, :w] = lab
    return torch.from_numpy(images), torch.from_numpy(labels), torch.tensor(dims, dtype=torch.int32)


def _plan(S, rows, filt=None):
    """rows of (rw, rh, ox, oy, mirror, flip_first)."""
    filt = S.F_LANCZOS if filt is None else filt
    plan = torch.zeros(len(rows), S.PLAN_WORDS, dtype=torch.int32)
    for i, (rw, rh, ox, oy, mirror, first) in enumerate(rows):
        plan[i, S.P_FLAGS] = filt | (S.F_MIRROR if mirror else 0) | (S.F_FLIP_FIRST if first else 0)
        plan[i, S.P_RW], plan[i, S.P_RH], plan[i, S.P_OX], plan[i, S.P_OY] = rw, rh, ox, oy
    return plan


def _grids(which, crop):
    """Factors 2, 1 and 1/2 per axis, mixed across the two axes, the window in the middle of the grid (a negative offset: padding on both sides), both mirror orders.
    Set A: 2 x 1, 1/2 x 2, 1 x 1/2, 2 x 2; set B: 1/2 x 1/2, 1 x 1, 2 x 1/2, about 1/2 x 1 (53 -> 27: 13 taps, an odd source)."""
    cw, ch = crop
    if which == "A":
        g = [(300, 80, 1, 1), (75, 128, 1, 0), (131, 40, 0, 0), (106, 74, 1, 1)]
    else:
        g = [(75, 40, 1, 0), (150, 64, 1, 1), (262, 40, 1, 1), (27, 37, 1, 0)]
    return [(rw, rh, (rw - cw) // 2, (rh - ch) // 2, m, f) for rw, rh, m, f in g]


def _equal_bits(got, want):
    return torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("crop", [(7, 5), (33, 20), (261, 9), (36, 11)])
@pytest.mark.parametrize("which", ["A", "B"])
def test_apply_vs_cpu_definition_under_hand_written_plans(mods, which, crop):
    """Both memory layouts and both target types; the outputs lie inside larger buffers whose guard words must come back untouched.  Widths 7, 33 and 261 store
    scalars; width 36 stores 16 bytes at a time behind a guard of 64 elements, which keeps the outputs aligned, and scalars behind a guard of 65.  261 columns cross
    the 256-column chunk, 9 rows leave a band of one row."""
    S, L = mods
    cw, ch = crop
    images, labels, sizes = _pairs(DIMS, HMAX, WMAX, 255)
    clean = _pairs(DIMS, HMAX, WMAX, 0)
    plan = _plan(S, _grids(which, crop))
    want_x, want_t = S.SegmentationAugmentation(crop, seed=0).apply(clean[0], clean[1], sizes, plan)
    dimg, dlab, dsz, dplan = images.cuda(), labels.cuda(), sizes.cuda(), plan.cuda()
    aug = S.SegmentationAugmentation(crop, seed=0)
    numel, tel = 4 * 3 * ch * cw, 4 * ch * cw
    for cl in (False, True):
        for i64 in (True, False):
            guard = 64 if cl == i64 else 65
            ref = want_x.permute(0, 2, 3, 1).contiguous().reshape(-1) if cl else want_x.reshape(-1)
            buf = torch.full((numel + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
            tbuf = torch.full((tel + 2 * guard,), 99, dtype=torch.int64 if i64 else torch.uint8, device="cuda")
            tables = torch.empty(4 * (cw + ch), dtype=torch.int32, device="cuda")
            L.call("frost_saug_apply", L.ptr(dimg), L.ptr(dlab), L.ptr(dsz), L.ptr(dplan), 4, HMAX, WMAX, cw, ch, *aug.mean, *aug.std, 255, int(cl), int(i64), 7,
                   L.ptr(tables), L.ptr(buf[guard:]), L.ptr(tbuf[guard:]), L.stream())
            got, gt = buf.cpu(), tbuf.cpu()
            assert bool(torch.isnan(got[:guard]).all()) and bool(torch.isnan(got[guard + numel:]).all()), (which, crop, cl, guard)
            assert bool((gt[:guard] == 99).all()) and bool((gt[guard + tel:] == 99).all()), (which, crop, i64, guard)
            bad = (got[guard:guard + numel].view(torch.int32) != ref.view(torch.int32)).nonzero().reshape(-1)
            tbad = (gt[guard:guard + tel].long() != want_t.reshape(-1)).nonzero().reshape(-1)
            print(f"[apply {which} crop {crop} channels_last {cl} int64 {i64}] differing words: {bad.numel()} of {numel}, labels: {tbad.numel()} of {tel}")
            assert bad.numel() == 0 and tbad.numel() == 0, (which, crop, cl, i64, bad[:8].tolist(), tbad[:8].tolist())
    # the public call: the same values, in the memory format and the type asked for
    for cl, dt in ((False, torch.int64), (True, torch.uint8)):
        x, t = S.SegmentationAugmentation(crop, seed=0, channels_last=cl, target_dtype=dt).apply(dimg, dlab, dsz, dplan)
        assert x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format) and tuple(x.shape) == (4, 3, ch, cw)
        assert t.dtype == dt and tuple(t.shape) == (4, ch, cw) and _equal_bits(x, want_x) and torch.equal(t.cpu().long(), want_t)


def _both(S, crop, images, labels, sizes, plan, clean=None, **kw):
    """The device against the CPU, both layouts; returns the CPU pair."""
    aug = S.SegmentationAugmentation(crop, seed=0, **kw)
    src = (images, labels) if clean is None else clean
    want_x, want_t = aug.apply(src[0], src[1], sizes, plan)
    for cl, dt in ((False, torch.int64), (True, torch.uint8)):
        x, t = S.SegmentationAugmentation(crop, seed=0, channels_last=cl, target_dtype=dt, **kw).apply(images.cuda(), labels.cuda(), sizes.cuda(), plan.cuda())
        assert _equal_bits(x, want_x), (crop, cl, (x.cpu() != want_x).nonzero()[:6].tolist())
        assert torch.equal(t.cpu().long(), want_t), (crop, cl, (t.cpu().long() != want_t).nonzero()[:6].tolist())
    return want_x, want_t


def test_apply_with_the_window_outside_the_grid(mods):
    """Crop 33 x 20.  Set 1: the grid narrower than the crop (20 wide: the odd difference 13, pad 7, the offset at -7 and at -6), shorter (11 high), both at once.
    Set 2: the window entirely in the padding on the left, on the right, above and below; what comes out is table[c][0] and ignore_idx."""
    S, L = mods
    images, labels, sizes = _pairs(DIMS, HMAX, WMAX, 255, seed=35)
    clean = _pairs(DIMS, HMAX, WMAX, 0, seed=35)
    _both(S, (33, 20), images, labels, sizes, _plan(S, [(20, 30, -7, 4, 1, 1), (20, 30, -6, 9, 1, 0), (50, 11, 8, -5, 0, 0), (20, 11, -6, -4, 1, 1)]), clean)
    x, t = _both(S, (33, 20), images, labels, sizes, _plan(S, [(20, 30, -35, 4, 1, 1), (40, 30, 41, 2, 1, 0), (50, 11, 8, -20, 0, 0), (20, 11, 2, 11, 1, 1)]), clean,
                 ignore_idx=254)
    assert bool((t == 254).all()) and float(x.std()) > 0 and len(x[:, 0].unique()) == 1
    # half in, half out, on every side of a grid larger than the crop
    _both(S, (33, 20), images, labels, sizes, _plan(S, [(150, 80, -16, 30, 0, 0), (150, 64, 134, 30, 1, 0), (100, 60, 30, -9, 1, 1), (53, 37, 10, 27, 0, 1)]), clean)


def test_apply_beyond_the_lds_cap(mods):
    """Factor 0.3 (20 Lanczos taps) on one axis only, then on both: the general path, per axis mixed with the LDS path's factors; both mirror orders."""
    S, L = mods
    dims = [(100, 150), (100, 150), (100, 150), (90, 140)]
    images, labels, sizes = _pairs(dims, 100, 150, 255, seed=32)
    clean = _pairs(dims, 100, 150, 0, seed=32)
    plan = _plan(S, [(45, 100, 5, 40, 1, 1), (150, 30, 60, 4, 1, 0), (45, 30, 6, 5, 1, 1), (42, 27, -3, 12, 0, 0)])
    _both(S, (33, 20), images, labels, sizes, plan, clean)
    _both(S, (33, 20), images, labels, sizes, _plan(S, [(45, 30, 6, 5, 0, 0)] * 4, filt=S.F_TRIANGLE), clean)          # the triangle filter down by 0.3: 9 taps, 35 rows


def test_apply_on_an_unaligned_base_pointer_ending_at_the_last_byte(mods):
    """Both images fill their 24 x 20 slots and the windows show the grid's last pixel, whose taps end in the slot's last pixel: the last three bytes of the buffer
    for the second image.  The kernel reads the taps of a pixel as whole aligned dwords and has to fall back to byte loads where those would pass the end of the
    batch, and everywhere when the base pointer is not 4-byte aligned (a view one byte into its storage)."""
    S, L = mods
    dims = [(24, 20), (24, 20)]
    images, labels, sizes = _pairs(dims, 24, 20, 0, seed=34)
    for rw, rh in ((10, 12), (40, 48), (20, 24)):
        plan = _plan(S, [(rw, rh, rw - 16, rh - 16, 1, 1), (rw, rh, rw - 16, rh - 16, 1, 0)])          # (mirrored behind the crop: the same source bytes)
        aug = S.SegmentationAugmentation((16, 16), seed=0)
        want_x, want_t = aug.apply(images, labels, sizes, plan)
        for shift in (0, 1, 2):
            store = torch.zeros(images.numel() + shift, dtype=torch.uint8, device="cuda")
            dimg = store[shift:].view(images.shape)
            dimg.copy_(images)
            assert dimg.data_ptr() % 4 == shift and dimg.is_contiguous()
            x, t = aug.apply(dimg, labels.cuda(), sizes.cuda(), plan.cuda())
            assert _equal_bits(x, want_x) and torch.equal(t.cpu(), want_t), (rw, rh, shift)
    one = torch.tensor([[[[7, 99, 250]]]], dtype=torch.uint8)          # a 1 x 1 slot (three bytes in all) cannot be read as dwords at all
    lab1, sz1 = torch.tensor([[[4]]], dtype=torch.uint8), torch.tensor([[1, 1]], dtype=torch.int32)
    ev = S.SegmentationEvalTransform(size=(5, 3))
    x, t = ev(one.cuda(), lab1.cuda(), sz1.cuda())
    wx, wt = ev(one, lab1, sz1)
    assert _equal_bits(x, wx) and torch.equal(t.cpu(), wt) and bool((wt == 4).all())


CLOSED_FORM_WRONG = [(64, 88), (96, 132), (144, 102), (168, 119), (120, 85), (80, 110)]          # (n_in, n_out) on which (int)((x + 0.5) a) misses Pillow's table


def test_label_planes_where_the_closed_form_is_wrong(mods):
    """Grids whose nearest-neighbour table differs from the closed form on both axes; the whole grid is the window, so every entry of the table is used."""
    S, L = mods
    dims = [(96, 64), (144, 168), (120, 80)]
    grids = [(88, 132), (119, 102), (110, 85)]
    images, labels, sizes = _pairs(dims, 144, 168, 255, seed=36)
    clean = _pairs(dims, 144, 168, 0, seed=36)
    for (h, w), (rw, rh) in zip(dims, grids):
        assert (w, rw) in CLOSED_FORM_WRONG and (h, rh) in CLOSED_FORM_WRONG
    for mirror, first in ((0, 0), (1, 1), (1, 0)):
        plan = _plan(S, [(rw, rh, 0, 0, mirror, first) for rw, rh in grids])
        want_x, want_t = _both(S, (119, 132), images, labels, sizes, plan, clean)
        assert bool((want_t == 255).any())
        if not mirror:
            for i, ((h, w), (rw, rh)) in enumerate(zip(dims, grids)):
                cy = ((np.arange(rh) + 0.5) * (float(h) / float(rh))).astype(np.int64)
                cx = ((np.arange(rw) + 0.5) * (float(w) / float(rw))).astype(np.int64)
                closed = clean[1][i].numpy()[cy[:, None], cx[None, :]]
                assert not np.array_equal(closed, want_t[i, :rh, :rw].numpy()), i          # the wrong rule would have been caught


def _plan_sizes():
    """67 sizes from 1 x 1 to 160 x 300: more than one wave and no multiple of 64."""
    rng = np.random.default_rng(41)
    rows = [[1, 1], [160, 300], [8, 64], [64, 8], [1, 300], [160, 1], [2, 3], [20, 33], [40, 66], [10, 17]]
    rows += rng.integers(1, 301, (67 - len(rows), 2)).clip(1, [160, 300]).tolist()
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("kw", [dict(crop_size=(33, 20)), dict(crop_size=(64, 48), scale=(0.5, 2.0), flip_first=False), dict(crop_size=21, scale=(0.7, 0.7))])
def test_plan_vs_cpu_definition(mods, kw):
    """Two consecutive calls per stream, so the ordinal advances; a seed with the top bit set and a position past 2^32."""
    S, L = mods
    sizes = _plan_sizes()
    dsz = sizes.cuda()
    for seed, seen in ((1, 0), (2 ** 63 + 12345, 0), (7, 2 ** 32 + 1000)):
        cpu, dev = S.SegmentationAugmentation(seed=seed, **kw), S.SegmentationAugmentation(seed=seed, **kw)
        for o in (cpu, dev):
            o.load_state_dict({"seed": seed, "images_seen": seen})
        for call in range(2):
            pc = cpu.plan(sizes)
            L.CALL_LOG = []
            try:
                pd = dev.plan(dsz)
                log = list(L.CALL_LOG)
            finally:
                L.CALL_LOG = None
            assert log == ["frost_saug_plan"], log
            assert pd.dtype == torch.int32 and tuple(pd.shape) == (67, S.PLAN_WORDS)
            assert torch.equal(pd.cpu(), pc), (seed, seen, call, (pd.cpu() != pc).nonzero()[:8].tolist())
        assert dev.images_seen() == seen + 134 == cpu.images_seen()


def test_eval_transform_vs_cpu_definition(mods):
    """Resize(size) + Normalize on landscape, portrait and 1 x 1 images of one slot, down and up, and Normalize alone on images that fill their slots."""
    S, L = mods
    dims = [(60, 80), (80, 60), (70, 70), (1, 1)]
    images, labels, sizes = _pairs(dims, 80, 80, 255, seed=33)
    clean = _pairs(dims, 80, 80, 0, seed=33)
    full = _pairs([(36, 52)] * 3, 36, 52, 0, seed=37)
    for size, data, src in (((40, 24), (images, labels, sizes), clean), ((33, 100), (images, labels, sizes), clean), (None, full, full)):
        for cl, dt in ((False, torch.int64), (True, torch.uint8)):
            t = S.SegmentationEvalTransform(size=size, channels_last=cl, target_dtype=dt)
            wx, wt = t(src[0], src[1], data[2])
            L.CALL_LOG = []
            try:
                x, tg = t(data[0].cuda(), data[1].cuda(), data[2].cuda())
                log = list(L.CALL_LOG)
            finally:
                L.CALL_LOG = None
            assert log == ["frost_saug_eval_plan", "frost_saug_apply"], log
            assert torch.equal(t.plan(data[2].cuda()).cpu(), t.plan(data[2]))
            assert x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format) and tg.dtype == dt
            assert _equal_bits(x, wx) and torch.equal(tg.cpu(), wt), (size, cl)
    assert tuple(wx.shape) == (3, 3, 36, 52) and torch.equal(wt.long(), full[1].long())          # Normalize alone: the label map passes through


def _call_inputs(seed=8):
    dims = np.random.default_rng(seed).integers(20, 151, (4, 2)).clip(1, [HMAX, WMAX]).tolist()
    return _pairs([tuple(d) for d in dims], HMAX, WMAX, 255, seed=seed)


@pytest.mark.parametrize("first", [True, False])
def test_whole_call_equals_cpu_object_and_runs_only_its_own_entries(mods, first):
    S, L = mods
    images, labels, sizes = _call_inputs()
    dimg, dlab, dsz = images.cuda(), labels.cuda(), sizes.cuda()
    kw = dict(crop_size=(40, 36), scale=(0.5, 2.0), flip_first=first, seed=55)
    cpu, dev = S.SegmentationAugmentation(**kw), S.SegmentationAugmentation(**kw)
    dev(dimg, dlab, dsz)          # the first call creates the state tensor (one host-to-device copy); the stream is rewound below
    dev.load_state_dict({"seed": 55, "images_seen": 0})
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        L.CALL_LOG = []
        try:
            outs.append(dev(dimg, dlab, dsz))
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        assert log == ["frost_saug_plan", "frost_saug_apply"], log
    one = cpu(images, labels, sizes)
    plan1 = cpu.last_plan
    two = cpu(images, labels, sizes)
    assert _equal_bits(outs[0][0], one[0]) and torch.equal(outs[0][1].cpu(), one[1]) and _equal_bits(outs[1][0], two[0]) and torch.equal(outs[1][1].cpu(), two[1])
    assert not torch.equal(plan1, cpu.last_plan) and dev.images_seen() == 8
    assert torch.equal(dev.last_plan.cpu(), cpu.last_plan)


def test_graph_capture_replays_advance_the_stream(mods):
    """__call__ on static inputs records into one HIP graph; two replays and a third give different plans, those of the CPU stream at positions 4, 8 and 12
    (position 0 is the warm-up call that creates the state tensor).  A restored position reaches the captured graph: the state words are written in place."""
    S, L = mods
    images, labels, sizes = _call_inputs(seed=9)
    dimg, dlab, dsz = images.cuda(), labels.cuda(), sizes.cuda()
    kw = dict(crop_size=(40, 36), scale=(0.5, 2.0), flip_first=False, seed=77, channels_last=True)
    a, cpu = S.SegmentationAugmentation(**kw), S.SegmentationAugmentation(**kw)
    eager, plans = [], []
    for _ in range(4):
        eager.append(cpu(images, labels, sizes))
        plans.append(cpu.last_plan)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = a(dimg, dlab, dsz)
    torch.cuda.current_stream().wait_stream(s)
    assert _equal_bits(warm[0], eager[0][0]) and torch.equal(warm[1].cpu(), eager[0][1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a(dimg, dlab, dsz)
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a.last_plan.cpu(), plans[k]) and _equal_bits(out[0], eager[k][0]) and torch.equal(out[1].cpu(), eager[k][1]), k
    assert not torch.equal(plans[1], plans[2]) and not torch.equal(plans[2], plans[3]) and not torch.equal(plans[1], plans[3])
    assert a.images_seen() == 16
    a.load_state_dict({"seed": 77, "images_seen": 4})
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.last_plan.cpu(), plans[1]) and _equal_bits(out[0], eager[1][0]) and torch.equal(out[1].cpu(), eager[1][1])


def test_into_train_seg_and_val_seg(mods, monkeypatch):
    """pad_pairs -> SegmentationAugmentation((33, 20)) -> a one-convolution model -> SegmentationLoss through harness.train_seg(..., transform=...) on a two-batch
    loader: mean IoU and loss equal those of the same loop fed with what the CPU transform makes of the same batches under the same seed; val_seg likewise."""
    S, L = mods
    import copy
    from frostnet_amd import harness, seg
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    c, rng = 5, np.random.default_rng(14)
    loader = []
    for _ in range(2):
        pics = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((30, 41), (25, 50), (44, 38))]
        labs = [np.where(rng.random(p.shape[:2]) < 0.1, 255, rng.integers(0, c, p.shape[:2])).astype(np.uint8) for p in pics]
        loader.append(S.pad_pairs(pics, labs))
    torch.manual_seed(31)
    base = torch.nn.Conv2d(3, c, 1)
    kw = dict(crop_size=(33, 20), seed=3)
    results = []
    for on_device in (True, False):
        model = copy.deepcopy(base).cuda()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        crit = seg.SegmentationLoss(n_classes=c, device="cuda")
        aug, ev = S.SegmentationAugmentation(**kw), S.SegmentationEvalTransform(size=(33, 20))
        if on_device:
            tr = harness.train_seg(model, loader, opt, crit, c, transform=aug)
            va = harness.val_seg(model, loader, criterion=crit, num_classes=c, transform=ev)
            assert aug.images_seen() == 6
        else:
            tr = harness.train_seg(model, [aug(*b) for b in loader], opt, crit, c)
            va = harness.val_seg(model, [ev(*b) for b in loader], criterion=crit, num_classes=c)
        results.append((tr, va))
    print(f"[train_seg / val_seg] device transform {results[0]}, CPU transform {results[1]}")
    assert results[0] == results[1] and np.isfinite(results[0][0][1]) and 0.0 <= results[0][0][0] <= 100.0


def test_argument_errors_launch_nothing(mods):
    S, L = mods
    images, labels, sizes = [t.cuda() for t in _call_inputs()]
    aug, ev = S.SegmentationAugmentation((16, 12), seed=1), S.SegmentationEvalTransform(size=(16, 12))
    aug(images, labels, sizes)
    L.CALL_LOG = []
    try:
        for args in ((images.float(), labels, sizes), (images, labels.long(), sizes), (images, labels, sizes.long()), (images[0], labels, sizes),
                     (images, labels[:1], sizes), (images, labels, sizes[:1]), (images[..., :2], labels, sizes), (images.cpu(), labels, sizes),
                     (images, labels.cpu(), sizes), (images, labels, sizes.cpu())):
            with pytest.raises(ValueError):
                aug(*args)
            with pytest.raises(ValueError):
                ev(*args)
        with pytest.raises(ValueError):
            aug.apply(images, labels, sizes, torch.zeros(4, S.PLAN_WORDS, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            aug.apply(images, labels, sizes, torch.zeros(4, S.PLAN_WORDS, dtype=torch.int32))
        assert L.CALL_LOG == []
    finally:
        L.CALL_LOG = None
    assert aug.images_seen() == 4
    # the library's own checks: an error code and a message, no launch
    x, t, tables = torch.empty(4, 3, 12, 16, device="cuda"), torch.empty(4, 12, 16, dtype=torch.int64, device="cuda"), torch.empty(4, 28, dtype=torch.int32, device="cuda")
    plan = aug.last_plan

    def apply(hmax=HMAX, cw=16, parts=7, ignore=255):
        L.call("frost_saug_apply", L.ptr(images), L.ptr(labels), L.ptr(sizes), L.ptr(plan), 4, hmax, WMAX, cw, 12, *aug.mean, *aug.std, ignore, 0, 1, parts, L.ptr(tables),
               L.ptr(x), L.ptr(t), L.stream())

    for kw, msg in ((dict(cw=0), "crop side"), (dict(hmax=0), "Hmax"), (dict(parts=8), "parts"), (dict(ignore=256), "ignore_idx")):
        with pytest.raises(RuntimeError, match=msg):
            apply(**kw)
    with pytest.raises(RuntimeError, match="size is"):
        L.call("frost_saug_eval_plan", L.ptr(sizes), 4, 16, 0, L.ptr(plan), L.stream())
    with pytest.raises(RuntimeError, match="scale"):
        L.call("frost_saug_plan", L.ptr(sizes), 4, 16, 12, -1.0, 0.0, 1, L.ptr(aug._state), L.ptr(plan), L.stream())
    assert L.load_library().frost_saug_plan_words() == S.PLAN_WORDS and L.load_library().frost_abi_version() == 5
    torch.cuda.synchronize()
    assert aug.images_seen() == 4

"""The classifier's input pipeline on the device (csrc/frost_caug.hip behind frostnet_amd.cls_augment) against its CPU definition (the same classes on CPU tensors,
pinned to Pillow by tests/test_cls_augment_cpu.py), at the smallest shapes at which the kernels can go wrong, and the plumbing: only frost_caug_* entries run,
capture into a HIP graph with a stream that advances per replay, the hand-over to the classifier through harness.train, argument errors.
Criterion: the decisions are fp64 in a written order with correctly rounded sqrt and division and a written-out exp; the resampler's weights likewise, its passes
integer arithmetic; the output is a table look-up.  So plan words and output bits are expected EQUAL, and that is what is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HMAX, WMAX = 96, 80
DIMS = [(96, 80), (96, 80), (64, 80), (96, 50), (1, 1), (40, 33)]          # (h, w) of the six images of one 96 x 80 slot


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib, cls_augment
    assert torch.cuda.is_available()
    return cls_augment, _lib


def _images(dims, hmax, wmax, sentinel, seed=31):
    """Random bytes inside every image's own extent, the sentinel in the padding of its slot."""
    rng = np.random.default_rng(seed)
    images = np.full((len(dims), hmax, wmax, 3), sentinel, dtype=np.uint8)
    for i, (h, w) in enumerate(dims):
        images[i, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return torch.from_numpy(images), torch.tensor(dims, dtype=torch.int32)


def _rects(which, size):
    """Six hand-written (x0, y0, w, h, mirror) per set.  At size 32 set A holds an up-scale, scales in (1, 2), [2, 3] and (2, 3) x (1, 2), a 1 x 1 image and an
    unchanged axis, set B scales in (1, 2), (2, 3] and below 1 in one axis or both; at size 7 most crops exceed the LDS path's cap of 4 and take the general path; at
    224 every crop is scaled up."""
    if which == "A":
        return [(30, 40, 9, 11, 0),                       # an up-scale from the middle of the image
                (10, 20, 48, 40, 1),
                (0, 0, 80, 64, 1),                        # the whole image: all four borders
                (0, 0, 37, 70, 0),                        # the left and the top border
                (0, 0, 1, 1, 1),
                (1, 0, min(size, 32), 40, 0)]             # the width unchanged (sizes 7 and 32): the whole height of the image
    return [(35, 46, 45, 50, 1),                          # the right and the bottom border
            (0, 0, 80, 96, 0),                            # the whole image
            (0, 44, 30, 20, 0),                           # the left and the bottom border
            (30, 0, 20, 90, 1),                           # the right and the top border
            (0, 0, 1, 1, 0),
            (20, 25, 9, 11, 1)]


def _plan(C, rects, size):
    plan = torch.zeros(len(rects), C.PLAN_WORDS, dtype=torch.int32)
    for i, (x0, y0, w, h, mirror) in enumerate(rects):
        plan[i, C.P_FLAGS], plan[i, C.P_RW], plan[i, C.P_RH] = C.F_MIRROR if mirror else 0, size, size
        plan[i, C.P_X0], plan[i, C.P_Y0], plan[i, C.P_W], plan[i, C.P_H] = x0, y0, w, h
    return plan


_WANT = {}


def _want(C, which, size):
    """The CPU definition's answer, computed once per (set, size), from images whose padding holds the OTHER sentinel than the device's."""
    if (which, size) not in _WANT:
        images, sizes = _images(DIMS, HMAX, WMAX, 0)
        _WANT[which, size] = C.ClassificationAugmentation(size=size, seed=0).apply(images, sizes, _plan(C, _rects(which, size), size))
    return _WANT[which, size]


@pytest.mark.parametrize("size", [7, 32, 224])
@pytest.mark.parametrize("which", ["A", "B"])
def test_apply_vs_cpu_definition_under_hand_written_plans(mods, which, size):
    """Both memory layouts; the output lies inside a larger buffer whose guard words must come back untouched.  A guard of 64 floats keeps the output 16-byte aligned
    (the 16-byte stores at sizes 32 and 224), 65 does not (scalar stores); size 7 is no multiple of four and stores scalars either way."""
    C, L = mods
    images, sizes = _images(DIMS, HMAX, WMAX, 255)
    plan = _plan(C, _rects(which, size), size)
    want = _want(C, which, size)
    dimg, dsz, dplan = images.cuda(), sizes.cuda(), plan.cuda()
    aug = C.ClassificationAugmentation(size=size, seed=0)
    numel = 6 * 3 * size * size
    for cl in (False, True):
        ref = want.permute(0, 2, 3, 1).contiguous().reshape(-1) if cl else want.reshape(-1)
        for guard in (64, 65):
            buf = torch.full((numel + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
            L.call("frost_caug_apply", L.ptr(dimg), L.ptr(dsz), L.ptr(dplan), 6, HMAX, WMAX, size, *aug.mean, *aug.std, int(cl), L.ptr(buf[guard:]), L.stream())
            got = buf.cpu()
            assert bool(torch.isnan(got[:guard]).all()) and bool(torch.isnan(got[guard + numel:]).all()), (which, size, cl, guard)
            body = got[guard:guard + numel]
            bad = (body.view(torch.int32) != ref.view(torch.int32)).nonzero().reshape(-1)
            print(f"[apply {which} size {size} channels_last {cl} guard {guard}] differing words: {bad.numel()} of {numel}")
            assert bad.numel() == 0, (which, size, cl, guard, bad[:8].tolist())
    # the public call: the same values, in the memory format asked for
    for cl in (False, True):
        got = C.ClassificationAugmentation(size=size, seed=0, channels_last=cl).apply(dimg, dsz, dplan)
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format) and tuple(got.shape) == (6, 3, size, size)
        assert torch.equal(got.cpu(), want), (which, size, cl)


def test_apply_beyond_the_lds_cap(mods):
    """Crop 8 x 640 -> 16 x 16: 40 source columns per output column, far beyond the nine taps of the LDS path: the general path.  The second image is the same crop
    of a 20-row image, lower down and mirrored; the third one scales 640 -> 16 in x and 64 -> 16 in y (four rows per row: at the cap in y, beyond it in x)."""
    C, L = mods
    dims = [(8, 640), (20, 640), (64, 640)]
    images, sizes = _images(dims, 64, 640, 255, seed=32)
    plan = _plan(C, [(0, 0, 640, 8, 0), (0, 11, 640, 8, 1), (0, 0, 640, 64, 1)], 16)
    want = C.ClassificationAugmentation(size=16, seed=0).apply(_images(dims, 64, 640, 0, seed=32)[0], sizes, plan)
    for cl in (False, True):
        got = C.ClassificationAugmentation(size=16, seed=0, channels_last=cl).apply(images.cuda(), sizes.cuda(), plan.cuda())
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), cl


def test_apply_reads_the_last_pixel_of_the_batch(mods):
    """Both images fill their 24 x 20 slots and the crops end in the slot's last pixel, whose three bytes are the last of the buffer for the second image: the kernel
    reads the taps of a pixel as whole aligned dwords and has to fall back to byte loads where those would pass the end of the batch.  A 1 x 1 slot (three bytes in
    all) cannot be read as dwords at all."""
    C, L = mods
    dims = [(24, 20), (24, 20)]
    images, sizes = _images(dims, 24, 20, 0, seed=34)
    plan = _plan(C, [(0, 0, 20, 24, 0), (11, 15, 9, 9, 1)], 16)
    for cl in (False, True):
        aug = C.ClassificationAugmentation(size=16, seed=0, channels_last=cl)
        assert torch.equal(aug.apply(images.cuda(), sizes.cuda(), plan.cuda()).cpu().view(torch.int32), aug.apply(images, sizes, plan).view(torch.int32)), cl
    one = torch.tensor([[[[7, 99, 250]]]], dtype=torch.uint8)
    sz = torch.tensor([[1, 1]], dtype=torch.int32)
    ev = C.ClassificationEvalTransform(size=5, resize=6)
    assert torch.equal(ev(one.cuda(), sz.cuda()).cpu().view(torch.int32), ev(one, sz).view(torch.int32))


def _plan_sizes():
    """67 sizes from 1 x 1 to 96 x 80: more than one wave and no multiple of 64; the strips take the fallback often (8 x 64: in 4 of 5 streams)."""
    rng = np.random.default_rng(41)
    rows = [[1, 1], [96, 80], [8, 64], [64, 8], [1, 80], [96, 1], [2, 3], [8, 64], [64, 8], [8, 64], [64, 8], [5, 80], [96, 6]]
    rows += rng.integers(1, 97, (67 - len(rows), 2)).clip(1, [96, 80]).tolist()
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("kw", [dict(), dict(scale=(0.5, 1.0)), dict(scale=(0.2, 0.7), ratio=(0.6, 1.9), size=32)])
def test_plan_vs_cpu_definition(mods, kw):
    """Two consecutive calls per stream, so the ordinal advances; a seed with the top bit set and a position past 2^32.  scale = (0.5, 1) sends every strip to the
    fallback."""
    C, L = mods
    sizes = _plan_sizes()
    dsz = sizes.cuda()
    fallbacks = 0
    for seed, seen in ((1, 0), (2 ** 63 + 12345, 0), (7, 2 ** 32 + 1000)):
        cpu, dev = C.ClassificationAugmentation(seed=seed, **kw), C.ClassificationAugmentation(seed=seed, **kw)
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
            assert log == ["frost_caug_plan"], log
            assert pd.dtype == torch.int32 and tuple(pd.shape) == (67, C.PLAN_WORDS)
            diff = (pd.cpu() != pc).nonzero()
            assert torch.equal(pd.cpu(), pc), (seed, seen, call, diff[:8].tolist())
            fallbacks += int(((pc[:, C.P_FLAGS] & C.F_FALLBACK) != 0).sum())
        assert dev.images_seen() == seen + 134 == cpu.images_seen()
    assert fallbacks > 0


def test_eval_transform_vs_cpu_definition(mods):
    """Landscape, portrait, square and 1 x 1 images of one 80 x 80 slot; 36 -> 32 scales most of them down (80 -> 48: the window does not start at the grid's origin),
    256 -> 224 scales all of them up."""
    C, L = mods
    dims = [(60, 80), (80, 60), (70, 70), (1, 1), (33, 80), (80, 31)]
    images, sizes = _images(dims, 80, 80, 255, seed=33)
    clean = _images(dims, 80, 80, 0, seed=33)[0]
    for size, resize in ((32, 36), (224, 256), (20, 20)):
        for cl in (False, True):
            t = C.ClassificationEvalTransform(size=size, resize=resize, channels_last=cl)
            want = t(clean, sizes)
            L.CALL_LOG = []
            try:
                got = t(images.cuda(), sizes.cuda())
                log = list(L.CALL_LOG)
            finally:
                L.CALL_LOG = None
            assert log == ["frost_caug_eval_plan", "frost_caug_apply"], log
            assert torch.equal(t.plan(sizes.cuda()).cpu(), t.plan(sizes))
            assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (size, resize, cl)


def _call_inputs(seed=8):
    dims = np.random.default_rng(seed).integers(20, 97, (6, 2)).clip(1, [HMAX, WMAX]).tolist()
    return _images([tuple(d) for d in dims], HMAX, WMAX, 255, seed=seed)


def test_whole_call_equals_cpu_object_and_runs_only_its_own_entries(mods):
    C, L = mods
    images, sizes = _call_inputs()
    dimg, dsz = images.cuda(), sizes.cuda()
    cpu, dev = C.ClassificationAugmentation(size=40, seed=55), C.ClassificationAugmentation(size=40, seed=55)
    dev(dimg, dsz)          # the first call creates the state tensor (one host-to-device copy); the stream is rewound below
    dev.load_state_dict({"seed": 55, "images_seen": 0})
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        L.CALL_LOG = []
        try:
            outs.append(dev(dimg, dsz))
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        assert log == ["frost_caug_plan", "frost_caug_apply"], log
    first = cpu(images, sizes)
    plan1 = cpu.last_plan
    second = cpu(images, sizes)
    assert torch.equal(outs[0].cpu(), first) and torch.equal(outs[1].cpu(), second)
    assert not torch.equal(plan1, cpu.last_plan) and dev.images_seen() == 12
    assert torch.equal(dev.last_plan.cpu(), cpu.last_plan)


def test_graph_capture_replays_advance_the_stream(mods):
    """__call__ on static inputs records into one HIP graph; three replays give three different plans, those of the CPU stream at positions 6, 12 and 18 (position 0 is
    the warm-up call that creates the state tensor).  A restored position reaches the captured graph: the state words are written in place."""
    C, L = mods
    images, sizes = _call_inputs(seed=9)
    dimg, dsz = images.cuda(), sizes.cuda()
    a, cpu = C.ClassificationAugmentation(size=40, seed=77, channels_last=True), C.ClassificationAugmentation(size=40, seed=77, channels_last=True)
    eager, plans = [], []
    for _ in range(4):
        eager.append(cpu(images, sizes))
        plans.append(cpu.last_plan)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = a(dimg, dsz)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(warm.cpu(), eager[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a(dimg, dsz)
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a.last_plan.cpu(), plans[k]) and torch.equal(out.cpu(), eager[k]), k
    assert not torch.equal(plans[1], plans[2]) and not torch.equal(plans[2], plans[3]) and not torch.equal(plans[1], plans[3])
    assert a.images_seen() == 24
    a.load_state_dict({"seed": 77, "images_seen": 6})
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.last_plan.cpu(), plans[1]) and torch.equal(out.cpu(), eager[1])


def test_into_the_classifier(mods, monkeypatch):
    """pad_images -> ClassificationAugmentation(size=64) -> FrostNet-Small QAT steps through harness.train(..., transform=...) on a two-batch loader: the loss is finite,
    the stream moved by the epoch's images, and the epoch reads the device as often as it does without a transform: once."""
    C, L = mods
    from frostnet_amd import frostnet as F
    from frostnet_amd import harness as Hn
    from frostnet_amd import pad_images
    from frostnet_amd.optimizer import QSGD
    torch.manual_seed(1882)
    model = F.MODEL_REGISTRY["frostnet_quant_small_1_0"](drop_rate=0.0)
    F.qat_prepare(model, version=0)
    model.cuda().train()
    opt = QSGD(Hn.make_param_groups(model, 1e-5), lr=5e-3, momentum=0.9, nesterov=True, clip_by=1e-3, toss_coin=True, noise_decay=1e-2, weight_decay=1e-5)
    opt.is_warmup = False
    crit = Hn.CrossEntropyLoss()
    rng = np.random.default_rng(14)
    loader, plain = [], []
    for _ in range(2):
        images, sizes = pad_images([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((90, 120), (128, 100), (60, 60), (150, 97))])
        target = torch.from_numpy(rng.integers(0, 1000, 4))
        loader.append((images, sizes, target))
        plain.append((torch.from_numpy(rng.standard_normal((4, 3, 64, 64)).astype(np.float32)), target))
    reads = []
    for name in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    aug = C.ClassificationAugmentation(size=64, seed=3)
    Hn.train(plain, model, crit, opt, 0)          # (also the warm-up: whatever a first step sets up is behind us)
    reads.clear()
    Hn.train(plain, model, crit, opt, 0)
    before = list(reads)
    aug(loader[0][0].cuda(), loader[0][1].cuda())          # creates the state tensor
    reads.clear()
    loss, a1, a5 = Hn.train(loader, model, crit, opt, 0, transform=aug)
    after = list(reads)
    assert np.isfinite(loss) and 0.0 <= a1 <= a5 <= 100.0
    assert after == before and after.count("tolist") == 1, (before, after)
    assert aug.images_seen() == 12
    ev = C.ClassificationEvalTransform(size=64, resize=72)
    lv, _, _ = Hn.val(loader, model, crit, transform=ev)
    assert np.isfinite(lv) and not model.training


def test_argument_errors_launch_nothing(mods):
    C, L = mods
    images, sizes = [t.cuda() for t in _call_inputs()]
    with pytest.raises(ValueError):
        C.ClassificationAugmentation(size=0)
    with pytest.raises(ValueError):
        C.ClassificationEvalTransform(size=224, resize=223)
    aug, ev = C.ClassificationAugmentation(size=16, seed=1), C.ClassificationEvalTransform(size=16, resize=18)
    aug(images, sizes)
    L.CALL_LOG = []
    try:
        for args in ((images.float(), sizes), (images, sizes.long()), (images[0], sizes), (images, sizes[:1]), (images[..., :2], sizes), (images.cpu(), sizes),
                     (images, sizes.cpu())):
            with pytest.raises(ValueError):
                aug(*args)
            with pytest.raises(ValueError):
                ev(*args)
        with pytest.raises(ValueError):
            aug.apply(images, sizes, torch.zeros(6, C.PLAN_WORDS, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            aug.apply(images, sizes, torch.zeros(6, C.PLAN_WORDS, dtype=torch.int32))
        assert L.CALL_LOG == []
    finally:
        L.CALL_LOG = None
    assert aug.images_seen() == 6
    # the library's own checks: an error code and a message, no launch
    x = torch.empty(6, 3, 16, 16, device="cuda")
    plan = aug.last_plan
    with pytest.raises(RuntimeError, match="size outside"):
        L.call("frost_caug_apply", L.ptr(images), L.ptr(sizes), L.ptr(plan), 6, HMAX, WMAX, 0, *aug.mean, *aug.std, 0, L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="Hmax"):
        L.call("frost_caug_apply", L.ptr(images), L.ptr(sizes), L.ptr(plan), 6, 0, WMAX, 16, *aug.mean, *aug.std, 0, L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="resize"):
        L.call("frost_caug_eval_plan", L.ptr(sizes), 6, 16, 15, L.ptr(plan), L.stream())
    with pytest.raises(RuntimeError, match="ratio"):
        L.call("frost_caug_plan", L.ptr(sizes), 6, 16, 0.08, 1.0, 0.0, 1.0, 0.1, 4.0, L.ptr(aug._state), L.ptr(plan), L.stream())
    assert L.load_library().frost_caug_plan_words() == C.PLAN_WORDS and L.load_library().frost_abi_version() == 5
    torch.cuda.synchronize()
    assert aug.images_seen() == 6

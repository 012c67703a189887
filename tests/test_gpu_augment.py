"""The batch augmentation on the device (csrc/frost_augment.hip behind frostnet_amd.augment) against its CPU definition (the same classes on CPU tensors, pinned by
tests/test_augment_cpu.py), at the smallest shapes at which the kernels can go wrong, and the plumbing: only frost_aug_* entries run, capture into a HIP graph with
a stream that advances per replay, determinism, the hand-over to the detector and MultiBoxLoss, argument errors.
Criterion: tap indices are integer arithmetic and every value operation is one correctly rounded fp32 operation in the definition's order (the library builds with
contraction off), so pixels, plan words, boxes and masks are expected BIT-EQUAL, and that is what is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (33, 20), (64, 64), (1, 1)]          # (h, w) of the four images of one 64 x 64 slot


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as ge
    ge.build()
    from frostnet_amd import _lib, augment
    assert torch.cuda.is_available()
    return augment, _lib


@pytest.fixture(scope="module")
def batch():
    """uint8 [4, 64, 64, 3] with random bytes everywhere, also outside every image's own extent: a read past an image's size changes the result."""
    images = torch.from_numpy(np.random.default_rng(17).integers(0, 256, (4, 64, 64, 3), dtype=np.uint8))
    return images, torch.tensor(SIZES, dtype=torch.int32)


def _plan(A, sizes, rows):
    """identity_plan with words replaced per image: rows[i] = {word name: value}."""
    plan = A.identity_plan(sizes)
    for i, words in enumerate(rows):
        for name, v in words.items():
            w = getattr(A, "P_" + name.upper())
            if w in A.FLOAT_WORDS:
                plan.view(torch.float32)[i, w] = float(v)
            else:
                plan[i, w] = int(v)
    return plan


def _expand(h, w, **more):
    """Canvas twice the image, pasted at (w // 2, h // 3); a crop of the image's own extent from (w // 4, h // 4): it overhangs the paste on the left and the top and
    ends inside it (or beyond it, for the smallest images)."""
    return dict(flags=more.pop("flags", 0), canvas_w=2 * w, canvas_h=2 * h, paste_x=w // 2, paste_y=h // 3, ratio=2.0, mode=4,
                x1=w // 4, y1=h // 4, x2=min(2 * w, w // 4 + w), y2=min(2 * h, h // 4 + h), **more)


def _concerns(A):
    hsv = A.F_HSV
    both = lambda flags, **k: [dict(flags=flags, **k)] * 4
    c = {
        "identity": [{}] * 4,                                                   # = BaseTransform; image 2 is the down-scale from 64 x 64
        "brightness": both(0, delta=-20.5),
        "contrast_first": both(0, alpha_pre=1.37),
        "contrast_last": both(0, alpha_post=0.61),
        "round_trip": both(hsv),
        "saturation": both(hsv, sat=1.43),
        "hue_up": both(hsv, hue=17.5),
        "hue_down": both(hsv, hue=-17.5),
        "perms_a": [dict(perm=p) for p in (1, 2, 3, 4)],
        "perms_b": [dict(perm=p) for p in (5, 0, 5, 1)],
        "all_contrast_first": both(hsv, delta=12.25, alpha_pre=0.8, sat=0.7, hue=9.0, perm=3),
        "all_contrast_last": both(hsv, delta=-31.0, alpha_post=1.45, sat=1.2, hue=-11.0, perm=4),
        "expand_overhang": [_expand(h, w) for h, w in SIZES],
        "expand_all": [_expand(h, w, flags=hsv | A.F_MIRROR, delta=7.5, alpha_post=1.2, sat=1.3, hue=-6.0, perm=2) for h, w in SIZES],
        "rect_one_past": [dict(mode=5, x1=w // 3, y1=h // 3, x2=w + 1, y2=h + 1) for h, w in SIZES],
        "mirror": both(A.F_MIRROR),
        "mirror_crop": [dict(flags=A.F_MIRROR, mode=1, x1=w // 3, y1=0, x2=w, y2=max(h // 2, 1)) for h, w in SIZES],
        "upscale_3x3": [dict(mode=2, x1=1 if w >= 4 else 0, y1=1 if h >= 4 else 0, x2=4 if w >= 4 else w, y2=4 if h >= 4 else h) for h, w in SIZES],
    }
    return c


CONCERNS = ["identity", "brightness", "contrast_first", "contrast_last", "round_trip", "saturation", "hue_up", "hue_down", "perms_a", "perms_b", "all_contrast_first",
            "all_contrast_last", "expand_overhang", "expand_all", "rect_one_past", "mirror", "mirror_crop", "upscale_3x3"]


@pytest.mark.parametrize("size", [8, 20, 13])
@pytest.mark.parametrize("concern", CONCERNS)
def test_apply_vs_cpu_definition_under_hand_written_plans(mods, batch, concern, size):
    """Sizes 8 and 20 are whole four-pixel runs (16-byte stores); 13 is not a multiple of four, so the masked tail and the scalar stores run."""
    A, L = mods
    images, sizes = batch
    rows = _concerns(A)
    assert sorted(rows) == sorted(CONCERNS)
    plan = _plan(A, sizes, rows[concern])
    want = A.SSDAugmentation(size=size, seed=0).apply(images, sizes, plan)
    for cl in (False, True):
        aug = A.SSDAugmentation(size=size, seed=0, channels_last=cl)
        L.CALL_LOG = []
        try:
            got = aug.apply(images.cuda(), sizes.cuda(), plan.cuda())
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        assert log == ["frost_aug_apply"], log
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (4, 3, size, size)
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        g = got.cpu()
        print(f"[apply {concern} size {size} channels_last {cl}] max |device - cpu| = {float((g - want).abs().max()):.3e}")
        assert torch.equal(g, want), (concern, size, cl)
    if concern == "identity":
        assert torch.equal(A.BaseTransform(size)(images.cuda(), sizes.cuda()).cpu(), want)


def _scene(n, g, seed):
    """n images of random size in [32, 500]^2 with 1 .. g valid boxes; image 3 has no valid box, image 5's only box is centred at fraction (0, 0)."""
    r = np.random.default_rng(seed)
    sizes = r.integers(32, 501, (n, 2)).astype(np.int32)
    c, half = r.uniform(0.1, 0.9, (n, g, 2)), r.uniform(0.02, 0.3, (n, g, 2))
    boxes = np.concatenate([np.clip(c - half, 0, 1), np.clip(c + half, 0, 1), r.integers(0, 20, (n, g, 1))], 2).astype(np.float32)
    valid = np.arange(g)[None, :] < r.integers(1, g + 1, (n, 1))
    valid[3] = False
    boxes[5, 0, :4] = (-0.1, -0.2, 0.1, 0.2)
    valid[5] = np.arange(g) == 0
    return torch.from_numpy(sizes), torch.from_numpy(boxes), torch.from_numpy(valid)


@pytest.mark.parametrize("g", [1, 9, 70])
def test_plan_vs_cpu_definition(mods, g):
    """N = 64 images, three seeds at images seen = 0 and one at a position past 2^32; G = 70 is more boxes than lanes.  Plan words, boxes_out, valid_out identical word
    for word."""
    A, L = mods
    sizes, boxes, valid = _scene(64, g, 100 + g)
    dev_in = [t.cuda() for t in (sizes, boxes, valid)]
    for seed, seen in ((1, 0), (2 ** 63 + 12345, 0), (987654321, 0), (7, 2 ** 32 + 1000)):
        cpu, dev = A.SSDAugmentation(size=32, seed=seed), A.SSDAugmentation(size=32, seed=seed)
        for o in (cpu, dev):
            o.load_state_dict({"seed": seed, "images_seen": seen})
        pc, bc, vc = cpu.plan(sizes, boxes, valid)
        L.CALL_LOG = []
        try:
            pd, bd, vd = dev.plan(*dev_in)
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        assert log == ["frost_aug_plan"], log
        assert pd.dtype == torch.int32 and bd.dtype == torch.float32 and vd.dtype == torch.bool
        diff = (pd.cpu() != pc).nonzero()
        assert torch.equal(pd.cpu(), pc), (seed, seen, diff[:8].tolist())
        assert torch.equal(vd.cpu(), vc) and torch.equal(bd.cpu().view(torch.int32), bc.view(torch.int32)), (seed, seen)
        assert dev.images_seen() == seen + 64 == cpu.images_seen()
        assert int(pc[3, A.P_MODE]) == 0 and int(pc[3, A.P_ROUNDS]) == 0 and not bool(vc[3].any())
        modes = set(pc[:, A.P_MODE].tolist())
    assert len(modes) > 1


def _call_inputs(n=6, g=4, slot=96, seed=8):
    r = np.random.default_rng(seed)
    sizes = r.integers(20, slot + 1, (n, 2)).astype(np.int32)
    images = r.integers(0, 256, (n, slot, slot, 3), dtype=np.uint8)
    c, half = r.uniform(0.2, 0.8, (n, g, 2)), r.uniform(0.05, 0.3, (n, g, 2))
    boxes = np.concatenate([np.clip(c - half, 0, 1), np.clip(c + half, 0, 1), r.integers(0, 20, (n, g, 1))], 2).astype(np.float32)
    valid = np.arange(g)[None, :] < r.integers(1, g + 1, (n, 1))
    return [torch.from_numpy(a) for a in (images, sizes, boxes, valid)]


def _same(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def test_whole_call_equals_cpu_object_and_runs_only_its_own_entries(mods):
    A, L = mods
    parts = _call_inputs()
    dparts = [p.cuda() for p in parts]
    cpu, dev = A.SSDAugmentation(size=40, seed=55), A.SSDAugmentation(size=40, seed=55)
    dev(*dparts)          # the first call creates the state tensor (one host-to-device copy); the stream is rewound below
    dev.load_state_dict({"seed": 55, "images_seen": 0})
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        L.CALL_LOG = []
        try:
            outs.append(dev(*dparts))
            log = list(L.CALL_LOG)
        finally:
            L.CALL_LOG = None
        assert log == ["frost_aug_plan", "frost_aug_apply"], log
    first, second = cpu(*parts), cpu(*parts)
    assert _same(outs[0], first) and _same(outs[1], second)
    assert not torch.equal(outs[0][0], outs[1][0]) and dev.images_seen() == 12
    assert torch.equal(dev.last_plan.cpu(), cpu.last_plan)


def test_graph_capture_replays_advance_the_stream(mods):
    """__call__ on static inputs records into one HIP graph; replays 1 and 2 equal eager calls 2 and 3 of a twin with the same seed (call 1 is the warm-up that creates
    the state tensor).  Two fresh objects give identical results."""
    A, L = mods
    parts = [p.cuda() for p in _call_inputs(seed=9)]
    a, twin = A.SSDAugmentation(size=40, seed=77, channels_last=True), A.SSDAugmentation(size=40, seed=77, channels_last=True)
    eager = [[t.clone() for t in twin(*parts)] for _ in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = a(*parts)
    torch.cuda.current_stream().wait_stream(s)
    assert _same(warm, eager[0])          # determinism across two fresh objects
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a(*parts)
    for k in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager[k]), k
    assert not torch.equal(eager[1][0], eager[2][0]) and a.images_seen() == 18
    # a restored position reaches the captured graph: the state words are written in place
    a.load_state_dict({"seed": 77, "images_seen": 6})
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager[1])


def test_into_the_detector(mods):
    """pad_images + pad_targets -> SSDAugmentation -> the small float SSDLiteFrostNet @128 (the configuration tests/test_gpu_detect_float.py trains) -> MultiBoxLoss
    with the (boxes, valid) tuple -> backward: the loss is finite; the channels-last output gives the same logits."""
    A, L = mods
    from frostnet_amd import ssdlite as S
    torch.manual_seed(4)
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128)).cuda().train()
    r = np.random.default_rng(12)
    images, sizes = A.pad_images([r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((90, 120), (128, 100), (60, 60), (150, 97))])
    targets = [torch.tensor(t, dtype=torch.float32) for t in ([[0.1, 0.2, 0.6, 0.7, 3]], [[0.3, 0.3, 0.9, 0.8, 1], [0.05, 0.1, 0.5, 0.4, 7]], [[0.2, 0.1, 0.8, 0.9, 11]],
                                                              [[0.4, 0.4, 0.7, 0.95, 0], [0.1, 0.5, 0.3, 0.9, 19], [0.5, 0.05, 0.95, 0.5, 5]])]
    boxes, valid = S.pad_targets(targets, "cuda")
    images, sizes = images.cuda(), sizes.cuda()
    aug = A.SSDAugmentation(size=128, seed=3)
    x, bo, vo = aug(images, sizes, boxes, valid)
    assert tuple(x.shape) == (4, 3, 128, 128) and tuple(bo.shape) == tuple(boxes.shape) and bool(vo.any(1).all())
    loc, conf, pri = model(x)
    ll, lc = S.MultiBoxLoss(21)((loc, conf, pri), (bo, vo))
    (ll + lc).backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(ll)) and np.isfinite(float(lc)) and float(ll) > 0 and float(lc) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    x_cl = A.SSDAugmentation(size=128, seed=3, channels_last=True).apply(images, sizes, aug.last_plan)
    assert x_cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(x_cl, x)
    model.eval()
    with torch.no_grad():
        conf_a, conf_b = model(x)[1], model(x_cl)[1]
    assert torch.equal(conf_a, conf_b)


def test_argument_errors_launch_nothing(mods):
    A, L = mods
    images, sizes, boxes, valid = [p.cuda() for p in _call_inputs(n=2)]
    with pytest.raises(ValueError):
        A.SSDAugmentation(size=0)
    aug = A.SSDAugmentation(size=16, seed=1)
    aug(images, sizes, boxes, valid)
    L.CALL_LOG = []
    try:
        for args in ((images.float(), sizes, boxes, valid), (images, sizes.long(), boxes, valid), (images, sizes, boxes.double(), valid), (images, sizes, boxes, valid.int()),
                     (images[0], sizes, boxes, valid), (images, sizes, boxes[:, :, :4], valid), (images, sizes, boxes, valid[:, :1]), (images, sizes[:1], boxes, valid),
                     (images, sizes, boxes.cpu(), valid.cpu()), (images.cpu(), sizes, boxes, valid)):
            with pytest.raises(ValueError):
                aug(*args)
        with pytest.raises(ValueError):
            aug.apply(images, sizes, torch.zeros(2, A.PLAN_WORDS, dtype=torch.float32, device="cuda"))
        assert L.CALL_LOG == []
    finally:
        L.CALL_LOG = None
    assert aug.images_seen() == 2
    # the library's own checks: an error code and a message, no launch
    x = torch.empty(2, 3, 16, 16, device="cuda")
    plan = A.identity_plan(sizes)
    with pytest.raises(RuntimeError, match="size outside"):
        L.call("frost_aug_apply", L.ptr(images), L.ptr(sizes), L.ptr(plan), 2, images.size(1), images.size(2), 0, 0.0, 0.0, 0.0, 0, L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="Hmax"):
        L.call("frost_aug_apply", L.ptr(images), L.ptr(sizes), L.ptr(plan), 2, 0, images.size(2), 16, 0.0, 0.0, 0.0, 0, L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="G outside"):
        L.call("frost_aug_plan", L.ptr(sizes), L.ptr(boxes), L.ptr(valid), 2, 0, L.ptr(aug._state), L.ptr(plan), L.ptr(boxes), L.ptr(valid), L.stream())
    assert L.load_library().frost_aug_plan_words() == A.PLAN_WORDS and L.load_library().frost_abi_version() == 5
    torch.cuda.synchronize()
    assert aug.images_seen() == 2

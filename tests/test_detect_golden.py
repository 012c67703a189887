"""The SSD Detect layer's CPU definition (frostnet_amd.ssdlite.Detect.forward_torch) against the reference's test phase -- torch.softmax + Detect of
Object_Detection/layers/functions/detection.py, recorded by tools/gen_golden.py g15 on scenes with decision margins (tests/detect_scenes.py) -- and the
parts of the contract the reference leaves open: the tie rule, the refusal of nms_thresh <= 0, the zero background plane, the zero fill."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_scenes as D  # noqa: E402

from frostnet_amd import ssdlite as S  # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def golden_case(g, case):
    """(loc, conf, priors, cfg, top_k, expected out, expected counts) of a g15 case, inputs rebuilt from the seed + object rows and checked by CRC."""
    k = f"c{case}_"
    res, n, p, c, top_k, seed = (int(v) for v in g[k + "spec"])
    cfg = S.ssd_cfg_for(res)
    pri = S.prior_boxes(cfg)
    assert pri.shape[0] == p
    loc, conf = D.assemble(n, p, c, seed, g[k + "obj_idx"], g[k + "obj_loc"], g[k + "obj_conf"])
    assert D.crc(loc, conf, pri.numpy()) == g[k + "input_crc"], "g15 inputs do not reassemble to the recorded CRC"
    return T(loc), T(conf), pri, cfg, top_k, T(g[k + "out"]), T(g[k + "counts"])


def assert_same_detections(out, counts, ref, ref_counts, what=""):
    """Same kept rows in the same order (no exceptions: the scenes' margins make every decision deterministic), values within fp32 rounding of the < 30
    operations behind a score or a coordinate of magnitude <= 2: 1e-5 + 1e-5 |ref|."""
    out, ref, counts, ref_counts = out.cpu(), ref.cpu(), counts.cpu(), ref_counts.cpu()
    assert out.shape == ref.shape and out.dtype == torch.float32, (what, out.shape, ref.shape)
    assert torch.equal(counts.to(torch.int32), ref_counts.to(torch.int32)), (what, "kept-row counts differ", (counts != ref_counts).nonzero()[:8].tolist())
    assert torch.equal(out[..., 0] != 0, ref[..., 0] != 0), (what, "the sets of written rows differ")
    err = (out - ref).abs() - (1e-5 + 1e-5 * ref.abs())
    print(f"[detect {what}] kept rows {int(ref_counts.sum())}, max |d| {float((out - ref).abs().max()):.3e}")
    assert float(err.max()) <= 0.0, (what, float((out - ref).abs().max()))


@pytest.mark.parametrize("case", [0, 1])
def test_forward_torch_vs_reference_golden(golden, case):
    g = golden("g15_detect")
    loc, conf, pri, cfg, top_k, ref, ref_counts = golden_case(g, case)
    assert g[f"c{case}_margins"][0] >= D.M_THRESH and g[f"c{case}_margins"][1] >= D.M_GAP and g[f"c{case}_margins"][2] >= D.M_IOU
    over, empty, pairs, max_kept = (int(v) for v in g[f"c{case}_coverage"])
    assert over > 0 and empty > 0 and max_kept > 1 and float(g[f"c{case}_max_removed_fraction"]) >= 0.3
    det = S.Detect(21, 0, top_k, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    assert len(det.state_dict()) == 0 and not list(det.parameters()) and not list(det.buffers())
    out = det(loc, conf, pri)
    assert_same_detections(out, det.last_counts, ref, ref_counts, f"forward_torch vs g15 case {case}")
    assert int(ref_counts.sum()) > 0 and int(ref_counts.max()) > 1


def test_tie_rule_lower_prior_index_first():
    """Equal scores: the lower prior index comes first (and takes the last top_k place)."""
    cfg = S.ssd_cfg_for(128)
    pri = S.prior_boxes(cfg)[:40].clone()
    pri[:, :2] = torch.linspace(0.05, 0.95, 40)[:, None]          # disjoint small boxes along the diagonal: NMS removes nothing
    pri[:, 2:] = 0.01
    loc = torch.zeros(1, 40, 4)
    conf = torch.zeros(1, 40, 3)
    conf[..., 0] = 3.0
    conf[..., 2] = -10.0
    dup = [31, 7, 19, 12]                                          # four priors with the same row, one better, the rest background-like
    conf[0, dup, 1] = 2.5
    conf[0, 25, 1] = 4.0
    conf[0, :, 0][conf[0, :, 1] == 0] = 12.0
    det = S.Detect(3, 0, 4, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    out = det(loc, conf, pri)
    assert det.last_counts.tolist() == [[0, 4, 0]]
    x1 = out[0, 1, :, 1]
    want = torch.stack([pri[i, 0] - pri[i, 2] / 2 for i in (25, 7, 12, 19)])        # 31 ties with 7 / 12 / 19 and loses the last place to them
    assert torch.allclose(x1, want, atol=1e-6), (x1, want)
    assert out[0, 1, 1, 0] == out[0, 1, 2, 0] == out[0, 1, 3, 0] and out[0, 1, 0, 0] > out[0, 1, 1, 0]


def test_nms_thresh_must_be_positive():
    for t in (0.0, -0.1):
        with pytest.raises(ValueError):
            S.Detect(21, 0, 200, 0.01, t)


def test_background_plane_and_zero_fill():
    cfg = S.ssd_cfg_for(128)
    pri = S.prior_boxes(cfg)
    g = torch.Generator().manual_seed(3)
    loc = torch.randn(2, pri.shape[0], 4, generator=g) * 0.3
    conf = torch.randn(2, pri.shape[0], 5, generator=g) * 2.0
    for bkg in (0, 2):
        det = S.Detect(5, bkg, 50, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
        out = det(loc, conf, pri)
        assert out.shape == (2, 5, 50, 5) and not out[:, bkg].any() and int(det.last_counts[:, bkg].sum()) == 0
        assert int(det.last_counts.sum()) > 0
        written = out[..., 0] != 0
        assert torch.equal(written.sum(2).to(torch.int32), det.last_counts)
        assert torch.equal(written, torch.arange(50)[None, None, :] < det.last_counts[..., None]), "kept rows are not packed at the front"
        assert not out[~written].any()
    conf_bg = torch.zeros(2, pri.shape[0], 5)
    conf_bg[..., 0] = 15.0                                         # all background: nothing passes the threshold
    det = S.Detect(5, 0, 200, 0.01, 0.45, cfg["variance"], cfg["min_dim"])
    out = det(loc, conf_bg, pri)
    assert out.shape == (2, 5, 200, 5) and out.dtype == torch.float32 and not out.any() and not det.last_counts.any()
    assert det.last_counts.shape == (2, 5) and det.last_counts.dtype == torch.int32


def test_model_detect_is_eval_only_and_stateless():
    model = S.SSDLiteFrostNet(num_classes=21, mode="small", cfg=S.ssd_cfg_for(128))
    keys = list(model.state_dict().keys())
    x = torch.randn(1, 3, 128, 128)
    with pytest.raises(RuntimeError):
        model.train().detect(x)
    out = model.eval().detect(x, top_k=10)
    assert out.shape == (1, 21, 10, 5) and not out.requires_grad
    assert list(model.state_dict().keys()) == keys and not any(isinstance(m, S.Detect) for m in model.modules())

"""Host-side pieces of the converted detector's inference path (SSDLiteFrostNet.hip_infer_int8 / hip_detect_int8): the prior offsets the head launches take as
arguments and the placement definition (infer.cvt_place_torch: what frost_cvt_place and the store of frost_cvt_head compute) against SSDLiteFrostNet._assemble on
dequantised random index maps with padded class channels, and the guards of the public entries.  No HIP call here."""
import pytest
import torch

from frostnet_amd import infer as I
from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for


@pytest.mark.parametrize("res,mode,n", [(128, "small", 3), (96, "small", 1)])
def test_placement_definition_equals_assemble(res, mode, n):
    model = SSDLiteFrostNet(num_classes=21, mode=mode, cfg=ssd_cfg_for(res))
    C, anchors = model.num_classes, list(model.ANCHORS)
    sizes = [(f, f) for f in model.cfg["feature_maps"]]
    offs = I.ssd_head_offsets(anchors, sizes)
    P = offs[-1] + sizes[-1][0] * sizes[-1][1] * anchors[-1]
    assert P == model.priors.shape[0] and offs[0] == 0 and all(b - a == h * w * A for a, b, (h, w), A in zip(offs, offs[1:], sizes, anchors))
    assert model.conf_pad == [88, 128, 128, 128, 88, 88]              # 84 -> 88, 126 -> 128: the channels the placement drops
    g = torch.Generator().manual_seed(res)
    SENT = -777.0
    loc = torch.full((n, P * 4), SENT)
    conf = torch.full((n, P * C), SENT)
    maps = []
    for k, ((h, w), A) in enumerate(zip(sizes, anchors)):
        for cout, width, out, unit in ((4 * A, 4 * A, loc, 4), (model.conf_pad[k], C * A, conf, C)):
            idx = torch.randint(-128, 128, (n, h * w, cout), generator=g, dtype=torch.int8)
            scale, zp = float(torch.rand((), generator=g)) * 0.1 + 0.01, int(torch.randint(0, 256, (), generator=g))
            # what forward_maps hands to _assemble: the dequantised map as NCHW (Act.dequant's expression)
            deq = (idx.to(torch.int32) + 128 - zp).float() * torch.tensor(scale)
            maps.append(deq.view(n, h, w, cout).permute(0, 3, 1, 2).contiguous())
            I.cvt_place_torch(idx, scale, zp, width, out, offs[k] * unit)
    want_loc, want_conf, priors = model._assemble(maps)
    assert priors is model.priors
    assert not bool((loc == SENT).any()) and not bool((conf == SENT).any())          # the regions tile the rows exactly
    assert torch.equal(loc.view(n, P, 4), want_loc) and torch.equal(conf.view(n, P, C), want_conf)


def test_placement_writes_only_its_region():
    idx = torch.arange(-128, -128 + 2 * 6 * 16, dtype=torch.int32).remainder(256).sub(128).to(torch.int8).view(2, 6, 16)
    out = torch.full((2, 100), -1.0)
    I.cvt_place_torch(idx, 0.5, 3, 12, out, 7)
    assert bool((out[:, :7] == -1.0).all()) and bool((out[:, 7 + 72:] == -1.0).all())
    want = ((idx.int() + 128 - 3).float() * 0.5)[:, :, :12].reshape(2, -1)
    assert torch.equal(out[:, 7:79], want)


def test_public_entries_refuse_an_unconverted_model():
    model = SSDLiteFrostNet(num_classes=21, mode="small", cfg=ssd_cfg_for(128)).eval()
    x = torch.zeros(1, 3, 128, 128)
    for fn in (model.hip_infer_int8, model.hip_detect_int8):
        with pytest.raises(RuntimeError, match="hip_convert"):
            fn(x)
    from frostnet_amd import frostnet as F
    F.qat_prepare(model, version=0)
    model.eval()
    before = list(model.state_dict().keys())
    for fn in (model.hip_infer_int8, model.hip_detect_int8):
        with pytest.raises(RuntimeError, match="hip_convert"):          # QAT-prepared but not converted
            fn(x)
    assert "_detect" not in model.__dict__ and list(model.state_dict().keys()) == before

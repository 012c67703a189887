"""Where the fused prediction-head kernel stores: frostnet_amd.infer.ssd_head_offsets against SSDLiteFrostNet._assemble (CPU, no library).

Source k (h_k x w_k pixels, A_k anchors) owns the priors [poff_k, poff_k + h_k w_k A_k).  Its loc map has 4 A_k values per pixel, its conf map C A_k used (and a few
padding) channels, so element j of pixel `pix` sits at poff_k * 4 + pix * 4 A_k + j of an image's flattened loc row and at poff_k * C + pix * C A_k + j of its conf
row -- (poff + pix) * width + j where every earlier source has the same anchor count, and in general with poff counted in priors (the anchor counts differ:
4, 6, 6, 6, 4, 4).  Twelve index-valued maps go through _assemble and every element must land there."""
import torch


def _check(res, total):
    from frostnet_amd.infer import ssd_head_offsets
    from frostnet_amd.ssdlite import SSDLiteFrostNet, ssd_cfg_for
    cfg = ssd_cfg_for(res)
    model = SSDLiteFrostNet(mode="small", cfg=cfg).eval()
    A, C, n = model.ANCHORS, model.num_classes, 2
    sizes = [(f, f) for f in cfg["feature_maps"]]
    offs = ssd_head_offsets(A, sizes)
    assert offs == ssd_head_offsets(A, cfg["feature_maps"])                 # edge lengths and (h, w) pairs alike
    assert offs[0] == 0 and all(offs[k + 1] - offs[k] == sizes[k][0] * sizes[k][1] * A[k] for k in range(5))
    P = offs[-1] + sizes[-1][0] * sizes[-1][1] * A[-1]
    assert P == model.priors.shape[0] == total

    def code(k, hw, width):          # value of element (source k, pixel, j): exact in fp32 (< 2^24)
        return ((k * 4096 + torch.arange(hw)[:, None]) * 128 + torch.arange(width)[None, :]).float()

    maps = []
    for k, (h, w) in enumerate(sizes):
        for width in (4 * A[k], model.conf_pad[k]):
            m = code(k, h * w, width).view(h, w, width).permute(2, 0, 1)     # NCHW: channel j of pixel (y, x)
            maps.append(m[None].expand(n, -1, -1, -1).contiguous())
    loc, conf, priors = model._assemble(maps)
    assert loc.shape == (n, P, 4) and conf.shape == (n, P, C) and priors is model.priors
    loc, conf = loc.reshape(n, -1), conf.reshape(n, -1)
    for k, (h, w) in enumerate(sizes):
        for row, unit, width in ((loc, 4, 4 * A[k]), (conf, C, C * A[k])):
            seg = row[:, offs[k] * unit: offs[k] * unit + h * w * width].view(n, h * w, width)
            assert torch.equal(seg, code(k, h * w, width)[None].expand(n, -1, -1)), (k, unit)
            pix, j = h * w - 1, width - 1                                    # one element spelled out
            assert float(row[1, offs[k] * unit + pix * width + j]) == (k * 4096 + pix) * 128 + j


def test_head_offsets_reproduce_assemble_512():
    _check(512, 24528)


def test_head_offsets_reproduce_assemble_128():
    _check(128, 1536)


def test_head_offsets_rectangular_maps():
    from frostnet_amd.infer import ssd_head_offsets
    assert ssd_head_offsets([4, 6, 4], [(5, 3), (2, 2), (1, 1)]) == [0, 60, 84]

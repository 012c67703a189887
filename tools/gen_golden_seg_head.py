"""Generate tests/golden/g20_seg_head.npz by RUNNING the reference's Lite R-ASPP head (dev container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_seg_head.py

Imports Semantic_Segmentation/model/layers/LRASPP.py through tools/refshim.py, as the other gen_golden_* tools do.  The fixture holds DATA only: one train-mode step
of `_Head(nclass, in_channels, inter_channels, dataset='pascal')` followed by `project`, `auxlayer` and the add, exactly the lines of MobileNetV3Seg.forward between
the backbone and the final interpolation, then the eval-mode forward with the running statistics that step left.
Keys: c1, c4, gout (inputs and the upstream gradient on the stride-8 output), w/<name> (parameters and buffers before the step, under frostnet_amd.seg_model.LRASPPHead's
state_dict names: the reference's `cbr` / `cb` are `conv` here), out, dc1, dc4, grad/<name>, stat/<name> (running statistics and num_batches_tracked after the
step), out_eval.  Everything fp32.  The three seeded inputs are normal draws rounded to multiples of 1/8, which the archive's compression stores in about a byte each:
that keeps the file under the repository's size limit for a committed file at the sizes below; every other array is what the reference computed.
"""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import refshim

OUT = os.path.join(ROOT, "tests", "golden", "g20_seg_head.npz")
N, C4, H4, C1, H1, NCLASS = 2, 16, 33, 8, 65, 6


def project_name(k):
    return k.replace(".cbr.", ".conv.").replace(".cb.", ".conv.")


def coarse(gen, *shape):
    return torch.round(torch.randn(*shape, generator=gen) * 8) / 8


def main():
    _Head = refshim.load_seg_head()
    torch.manual_seed(20)
    head = _Head(NCLASS, C4, C1, dataset="pascal")
    project = torch.nn.Conv2d(256 // 2, NCLASS, 1, 1)
    auxlayer = torch.nn.Conv2d(C1, NCLASS, 1, 1)
    gen = torch.Generator().manual_seed(2020)
    for m in head.modules():                      # BatchNorm affine parameters and running statistics away from their initial values
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=gen) * 0.8 + 0.6
            m.bias.data = torch.rand(m.num_features, generator=gen) * 0.2 - 0.1
            m.running_mean.data = torch.randn(m.num_features, generator=gen) * 0.1
            m.running_var.data = torch.rand(m.num_features, generator=gen) * 0.5 + 0.5
    c1 = coarse(gen, N, C1, H1, H1).requires_grad_(True)
    c4 = coarse(gen, N, C4, H4, H4).requires_grad_(True)
    gout = coarse(gen, N, NCLASS, H1, H1)

    def state():
        sd = {project_name(k): v.detach().clone() for k, v in head.state_dict().items()}
        sd.update({"project." + k: v.detach().clone() for k, v in project.state_dict().items()})
        sd.update({"auxlayer." + k: v.detach().clone() for k, v in auxlayer.state_dict().items()})
        return sd

    def forward():
        a, b = head(c1, c4)                       # MobileNetV3Seg.forward: c1, c4 = self.head(c1, c4); c4 = self.project(c4); c1 = self.auxlayer(c1); out = c1 + c4
        return auxlayer(a) + project(b)

    data = {"c1": c1.detach().numpy(), "c4": c4.detach().numpy(), "gout": gout.numpy()}
    before = state()
    data.update({"w/" + k: v.float().numpy() if v.dtype.is_floating_point else v.numpy() for k, v in before.items()})
    head.train()
    out = forward()
    out.backward(gout)
    data["out"] = out.detach().numpy()
    data["dc1"], data["dc4"] = c1.grad.numpy(), c4.grad.numpy()
    named = {project_name(k): p for k, p in head.named_parameters()}
    named.update({"project." + k: p for k, p in project.named_parameters()})
    named.update({"auxlayer." + k: p for k, p in auxlayer.named_parameters()})
    data.update({"grad/" + k: p.grad.numpy() for k, p in named.items()})
    after = state()
    data.update({"stat/" + k: v.numpy() for k, v in after.items() if "running_" in k or "num_batches" in k})
    head.eval()
    with torch.no_grad():
        data["out_eval"] = forward().numpy()
    pooled = head.lr_aspp.b1[0](c4.detach())
    assert tuple(pooled.shape[2:]) == (2, 2), pooled.shape
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(data), "arrays")


if __name__ == "__main__":
    main()

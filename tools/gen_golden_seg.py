"""Generate tests/golden/g18_seg.npz by RUNNING the reference's segmentation criterion, mean-IoU meter and validation loop (dev container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_seg.py

Imports the reference through tools/refshim.py, as tools/gen_golden.py does.  The fixture holds DATA only: small low-resolution logits, targets, class weights and
what the reference produced for them.  The reference's models end in F.interpolate(out, size, mode='bilinear', align_corners=True); its criterion and meter see
the interpolated logits.  Here that interpolation is applied to the stored low-resolution logits before they enter the reference, and the recorded gradients are
with respect to the low-resolution logits -- what frostnet_amd.seg takes and returns.
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
import torch.nn.functional as F

import refshim

OUT = os.path.join(ROOT, "tests", "golden", "g18_seg.npz")
C, LOW, LOW2, SIZE = 19, (6, 7), (12, 15), (24, 30)
ZERO_WEIGHT_CLASS = 3


def up(x):
    return F.interpolate(x, SIZE, mode="bilinear", align_corners=True)


def targets(gen, n):
    t = torch.randint(0, C, (n,) + SIZE, generator=gen)
    t[:, 5] = 255                                         # two fully ignored rows
    t[:, 17] = 255
    t[torch.rand(t.shape, generator=gen) < 0.05] = 255   # and scattered ignored pixels
    return t


class Stub(torch.nn.Module):
    """Returns stored logits: the batch is a vector filled with the index of the stored entry."""

    def __init__(self, stored):
        super().__init__()
        self.stored = stored

    def forward(self, idx):
        return up(self.stored[int(idx[0])])


def main():
    SegmentationLoss, MIOU, val_seg = refshim.load_segmentation()
    torch.set_num_threads(8)
    gen = torch.Generator().manual_seed(18)
    wts = torch.rand(C, generator=gen) * 9.0 + 1.0       # Cityscapes-style: 1 .. 10, one class switched off
    wts[ZERO_WEIGHT_CLASS] = 0.0
    x = (torch.randn((2, C) + LOW, generator=gen) * 3.0).requires_grad_(True)
    x2 = (torch.randn((2, C) + LOW2, generator=gen) * 3.0).requires_grad_(True)
    t = targets(gen, 2)
    crit = SegmentationLoss(n_classes=C, loss_type="ce", device="cpu", ignore_idx=255, class_wts=wts)
    loss = crit(up(x), t)
    (gx,) = torch.autograd.grad(loss, x)
    loss_t = crit((up(x), up(x2)), t)
    gxt, gx2t = torch.autograd.grad(loss_t, (x, x2))
    crit_plain = SegmentationLoss(n_classes=C, loss_type="ce", device="cpu", ignore_idx=255)
    loss_p = crit_plain(up(x), t)
    (gxp,) = torch.autograd.grad(loss_p, x)
    inter, union = MIOU(num_classes=C).get_iou(up(x).detach(), t.clone())

    sizes = (2, 3, 1)
    stored = [torch.randn((n, C) + LOW, generator=gen) * 3.0 for n in sizes]
    vt = [targets(gen, n) for n in sizes]
    loader = [(torch.full((n,), i, dtype=torch.int64), vt[i]) for i, n in enumerate(sizes)]
    miou, vloss = val_seg(Stub(stored), loader, criterion=crit, num_classes=C, device="cpu")
    batch_iou = [MIOU(num_classes=C).get_iou(up(stored[i]), vt[i].clone()) for i in range(len(sizes))]

    arrs = dict(
        class_wts=wts.numpy(), x=x.detach().numpy(), x2=x2.detach().numpy(), target=t.numpy().astype(np.uint8),
        loss=np.float32(loss.item()), gx=gx.numpy(), loss_tuple=np.float32(loss_t.item()), gx_tuple=gxt.numpy(), gx2_tuple=gx2t.numpy(),
        loss_plain=np.float32(loss_p.item()), gx_plain=gxp.numpy(), inter=inter, union=union,
        val_miou=np.float64(miou), val_loss=np.float64(vloss),
        meta_torch_version=np.asarray(torch.__version__))
    for i in range(len(sizes)):
        arrs[f"val_x{i}"] = stored[i].numpy()
        arrs[f"val_t{i}"] = vt[i].numpy().astype(np.uint8)
        arrs[f"val_inter{i}"] = batch_iou[i][0]
        arrs[f"val_union{i}"] = batch_iou[i][1]
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; loss", loss.item(), "tuple", loss_t.item(), "val", float(miou), float(vloss))


if __name__ == "__main__":
    main()

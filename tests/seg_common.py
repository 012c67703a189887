"""Shared by tests/test_seg_cpu.py and tests/test_gpu_seg.py: the error rule, the input generator and the golden cases of the segmentation criterion."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 2e-6          # fp32 storage: max(FLOOR, 8 E32) norm-wise (the rule of tests/test_gpu_float_kernels.py)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def nrm(a, b):
    """Norm-wise relative error of a against b (fp64)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = float((a - b).norm())
    return d / max(float(b.norm()), 1e-300)


def bound(e32):
    return max(FLOOR, 8.0 * e32)


def hold(what, got, ref64, ref32, scale=1.0):
    """got against the fp64 reference within max(2e-6, 8 E32) * scale, E32 = the fp32 reference against fp64.  Prints observed / bound / E32."""
    e32 = nrm(ref32, ref64)
    obs, bnd = nrm(got, ref64), bound(e32) * scale
    print(f"[seg] {what}: observed {obs:.2e} bound {bnd:.2e} E32 {e32:.2e}")
    assert obs <= bnd, f"{what}: {obs:.3e} > {bnd:.3e} (E32 {e32:.3e})"
    return obs


def city_weights(c, gen):
    """Cityscapes-style class weights, 1 .. 10, with one class switched off."""
    w = torch.rand(c, generator=gen) * 9.0 + 1.0
    w[min(3, c - 1)] = 0.0
    return w


def make_case(n, c, hw, HW, seed, weights=False, integer_grid=False):
    """logits N(0, 3^2) (or a small integer grid: exact ties everywhere), targets with two fully ignored rows and, for n > 1, one image ignored entirely."""
    gen = torch.Generator().manual_seed(seed)
    if integer_grid:
        x = torch.randint(-2, 3, (n, c) + tuple(hw), generator=gen).float()
    else:
        x = torch.randn((n, c) + tuple(hw), generator=gen) * 3.0
    t = torch.randint(0, c, (n,) + tuple(HW), generator=gen)
    t[torch.rand(t.shape, generator=gen) < 0.03] = 255
    if HW[0] >= 4:
        t[:, 1] = 255
        t[:, HW[0] - 2] = 255
    if n > 1:
        t[n - 1] = 255
    return x, t, (city_weights(c, gen) if weights else None)


def torch_formulation(x, t, wt):
    """torch's own ops under autograd: F.interpolate -> F.cross_entropy with ignore_index = 255 -> (loss, gradient w.r.t. the low-resolution logits, upsampled logits)."""
    xr = x.detach().clone().requires_grad_(True)
    u = F.interpolate(xr, tuple(t.shape[1:]), mode="bilinear", align_corners=True) if tuple(t.shape[1:]) != tuple(x.shape[2:]) else xr
    loss = F.cross_entropy(u, t.long(), weight=None if wt is None else wt.to(x.dtype), ignore_index=255)
    (g,) = torch.autograd.grad(loss, xr)
    return loss.detach(), g, u.detach()


def direct_counts(u, t, c):
    """The three per-class pixel counts by a direct count."""
    pred = u.argmax(1)
    valid = t.long() < c
    inter = torch.stack([((pred == k) & (t == k) & valid).sum() for k in range(c)])
    ap = torch.stack([((pred == k) & valid).sum() for k in range(c)])
    am = torch.stack([((t == k) & valid).sum() for k in range(c)])
    return inter, ap, am


class StoredLogits(torch.nn.Module):
    """A module that returns stored low-resolution logits: its input is a vector filled with the index of the stored entry (the stub of tools/gen_golden_seg.py)."""

    def __init__(self, stored):
        super().__init__()
        self.stored = stored

    def forward(self, idx):
        return self.stored[int(idx[0])]


def golden_val(g, device):
    """(module, loader) of the golden validation run: three batches of 2, 3 and 1 images."""
    stored = [T(g[f"val_x{i}"]).to(device) for i in range(3)]
    loader = [(torch.full((stored[i].size(0),), i, dtype=torch.int64), T(g[f"val_t{i}"])) for i in range(3)]
    return StoredLogits(stored), loader

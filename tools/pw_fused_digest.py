"""One seeded pointwise layer, forward through the engine, then frost_pw_conv_bwd_fused called directly in three flavours on fixed inputs; dumps every result to an .npz.
Used by tests/test_gpu_pw_fused_spec.py to hold the shape-specialised fused-backward instances to the generic instance (FROST_PW_SPEC=0 in another process).
The reduce pass that fills the S1 / S2 coefficient rows sums with float atomics (its result differs from run to run in the last bits), so the process that runs second
takes the coefficient rows of the first (`coef_from`): both fused kernels then see identical bits.
usage: pw_fused_digest.py out.npz cin cout H B relu [coef_from.npz]"""
import os, sys, warnings
warnings.filterwarnings("ignore")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as ge
ge.build()
from frostnet_amd import engine as EN, _lib as L
from frostnet_amd._lib import call, ptr, stream
out = sys.argv[1]
cin, cout, H, B, relu = [int(v) for v in sys.argv[2:7]]
given = np.load(sys.argv[7]) if len(sys.argv) > 7 else None
dev = "cuda"
g = torch.Generator(device="cpu").manual_seed(4321)
res = {}


def layer(relu):
    E = EN.Engine(dev); qa = EN.QArena(8, dev)
    w = (torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cout) ** 0.5).to(dev).requires_grad_(True)
    gamma = (torch.rand(cout, generator=g) * 0.5 + 0.75).to(dev).requires_grad_(True)
    beta = (torch.rand(cout, generator=g) * 0.2 - 0.05).to(dev).requires_grad_(True)
    l = EN.ConvLayer("L", "pw", w, gamma, beta, torch.zeros(cout, device=dev), torch.ones(cout, device=dev), torch.zeros((), dtype=torch.int64, device=dev), None, 1, 1,
                     bool(relu), qa.alloc(), qa.alloc())
    E.add_layer(l)
    qx = qa.alloc(); qa.set_qparams(qx, 0.02, 3)
    x = E.new_act(B, H, H, cin, qx)
    x.buf[: x.numel] = torch.randint(-128, 128, (x.numel,), dtype=torch.int16, generator=g).to(torch.int8).to(dev)
    E.begin_step()
    y = E.conv(l, x)
    return E, l, x, y


for tag, rl, acc, want_dx in (("a", relu, 0, 1), ("b", 1 - relu, 1, 1), ("c", relu, 0, 0)):
    E, l, x, y = layer(rl)
    assert L.load_library().frost_pw_bwd_fused_ok(x.npix, x.c, l.cout), "shape outside the fused kernel"
    torch.cuda.synchronize()
    res[tag + "_y"] = y.buf[: y.numel].cpu().numpy(); res[tag + "_stats"] = l.stats.cpu().numpy().copy(); res[tag + "_qy"] = l.qy.cpu().numpy()
    gout = torch.cat([(torch.randn(y.numel, generator=g) * 1e-3).to(torch.bfloat16).view(torch.int16), torch.zeros(64, dtype=torch.int16)]).to(dev)
    args = (ptr(x.buf), ptr(x.q), ptr(l.wq_pack), ptr(l.wsum), ptr(l.wt_pack), ptr(l.qw), x.npix, x.c, l.cout)
    call("frost_pw_conv_bwd", *args, 0, ptr(l.coef), ptr(l.qy), int(l.relu), ptr(gout), None, None, 0, stream())          # reduce pass: S1 / S2 rows
    torch.cuda.synchronize()
    if given is not None:
        l.coef.copy_(torch.from_numpy(given[tag + "_coef"]).to(dev).view_as(l.coef))
    res[tag + "_coef"] = l.coef.cpu().numpy().copy()
    dwq = torch.zeros(E._dwq_elems(cout * cin), dtype=torch.float32, device=dev)
    dx = None
    if want_dx:
        dx = torch.zeros(x.numel + 64, dtype=torch.int16, device=dev)
        if acc:
            dx[: x.numel] = (torch.randn(x.numel, generator=g) * 1e-3).to(torch.bfloat16).view(torch.int16).to(dev)
    call("frost_pw_conv_bwd_fused", *args, ptr(l.coef), ptr(l.qy), int(l.relu), ptr(gout), None, ptr(dx), acc, ptr(dwq), stream())
    torch.cuda.synchronize()
    res[tag + "_coef_after"] = l.coef.cpu().numpy().copy()
    res[tag + "_dwq"] = dwq.cpu().numpy()
    if want_dx:
        res[tag + "_dx"] = dx.cpu().numpy()
np.savez(out, **res)

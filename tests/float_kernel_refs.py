"""Plain references for the float trainer's pointwise, BatchNorm and wiring kernels (csrc/frost_float.hip), no device.

Every function takes the operands the device sees (in bf16 mode: already rounded to bf16) and evaluates the kernel's definition in the
dtype it is given: torch.float64 is the reference, torch.float32 the yardstick (the same quantity in plain fp32 torch ops; its error
against fp64 is the E32 of tests/test_gpu_float_kernels.py).  tests/test_float_kernel_refs_cpu.py holds the fp64 form to torch's own
Conv2d -> BatchNorm2d -> activation under autograd.  The case lists of the GPU file live here so that both files see the same inputs."""
import numpy as np
import torch

BN_EPS, BN_MOM = 1e-5, 0.1
DEV_BN_EPS = float(np.float32(1e-5))          # the kernels' FROST_BN_EPS is the float literal 1e-5f: 2.5e-8 below 1e-5, which shows where the variance vanishes
ACT_NONE, ACT_RELU, ACT_HSWISH = 0, 1, 2
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_HSWISH: "hswish"}
F64, F32 = torch.float64, torch.float32
BF16_U = 2.0 ** -8          # unit roundoff of bf16: no correctly rounded element is further off
BAND_RTOL, BAND_SHARE = 1e-5, 1e-3


def round_up(v, m):
    return (v + m - 1) // m * m


def bf16_round(t):
    return t.float().bfloat16().float()


def seen(t, prec):
    """The value the device holds: rounded to bf16 by torch in bf16 mode."""
    return bf16_round(t) if prec == "bf16" else t.float()


# ------------------------------------------------------------------------------------------------ metric
def rel(a, ref):
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    err = float((a - ref).norm())
    return 0.0 if err == 0.0 else err / max(float(ref.norm()), 1e-300)


def rel_per_channel(a, ref):
    """Worst output channel (last dimension) of the norm-wise relative error: a wrong tile or tail is not averaged away."""
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    err, den = (a - ref).norm(dim=0), ref.norm(dim=0)
    r = torch.where(err == 0, torch.zeros_like(err), err / den.clamp_min(1e-300))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ pack layouts of k_f_prep
def pack_index(rows_pad, kpad, kq):
    """A-fragment layout [ct][kb][lane][ne]: element (ct, kb, lane, e) holds M[ct*16 + (lane & 15)][kb*kq + (lane >> 4)*ne + e];
    kq = 32, ne = 8 for bf16 and kq = 16, ne = 4 for fp32 (one 64-byte K step of a row either way)."""
    ne = kq // 4
    ct, kb, lane, e = np.meshgrid(np.arange(rows_pad // 16), np.arange(kpad // kq), np.arange(64), np.arange(ne), indexing="ij")
    row = ct * 16 + (lane & 15)
    k = kb * kq + (lane >> 4) * ne + e
    return torch.from_numpy(row.reshape(-1)), torch.from_numpy(k.reshape(-1))


def pack_matrix(m, rows_pad, kpad, kq):
    """m [rows][k] -> the flat pack, zeros in the padding."""
    mp = torch.zeros(rows_pad, kpad, dtype=m.dtype)
    mp[: m.shape[0], : m.shape[1]] = m
    row, k = pack_index(rows_pad, kpad, kq)
    return mp[row, k]


def unpack_matrix(flat, rows_pad, kpad, kq):
    row, k = pack_index(rows_pad, kpad, kq)
    out = torch.full((rows_pad, kpad), float("nan"), dtype=flat.dtype)
    out[row, k] = flat
    return out


def stem_matrix(w):
    """OIHW [cout][cin_g <= 4][kk] -> [cout][64] with k = tap*4 + c (taps 9..15 and channel 3 stay zero)."""
    cout, cg, kk = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    m = torch.zeros(cout, 16, 4, dtype=w.dtype)
    m[:, :kk, :cg] = w.reshape(cout, cg, kk).permute(0, 2, 1)
    return m.reshape(cout, 64)


def stem_unscatter(tmp, cout):
    """The permutation of frost_float_stem_wscatter: [co][tap*4 + c] -> [co][c][tap], 3 channels and 9 taps."""
    return tmp.reshape(cout, 16, 4)[:, :9, :3].permute(0, 2, 1).reshape(cout, 27)


def layer_packs(w, kind, prec):
    """(forward pack, transposed pack or None, kpad, kpad_t) of a pointwise (kind 0) or stem (kind 2) layer as flat fp32 tensors of the seen values."""
    kq = 32 if prec == "bf16" else 16
    cout = w.shape[0]
    cpad = round_up(cout, 16)
    ws = seen(w, prec)
    if kind == 2:
        return pack_matrix(stem_matrix(ws), cpad, 64, kq), None, 64, 0
    m = ws.reshape(cout, -1)
    cin = m.shape[1]
    kpad, kpad_t = round_up(cin, kq), round_up(cout, kq)
    return pack_matrix(m, cpad, kpad, kq), pack_matrix(m.t().contiguous(), round_up(cin, 16), kpad_t, kq), kpad, kpad_t


# ------------------------------------------------------------------------------------------------ the layer, stage by stage
def act_fwd(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_HSWISH:
        return z * torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
    return z


def act_grad(z, act):
    """d act / dz as autograd forms it: ReLU's mask z > 0; hard-swish (relu6(z + 3) + z * [0 < z + 3 < 6]) / 6 (hardtanh's open interval)."""
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_HSWISH:
        t = z + 3.0
        return (torch.clamp(t, 0.0, 6.0) + torch.where((t > 0) & (t < 6), z, torch.zeros_like(z))) / 6.0
    return torch.ones_like(z)


ACT_KINKS = {ACT_NONE: (), ACT_RELU: (0.0,), ACT_HSWISH: (-3.0, 0.0, 3.0)}


def band_mask(conv, scale, bias, act, rtol=BAND_RTOL):
    """Elements whose pre-activation z = conv*scale + bias lies within tau = rtol * (|conv*scale| + |bias|) of a kink of the activation's
    derivative (it jumps at 0 for ReLU and at -3 / +3 for hard-swish, whose slope also changes at 0).  A test zeroes the incoming gradient
    there: whichever way an fp32 comparison falls, S1, S2 and dc are the same."""
    cs = conv.double() * scale.double()
    z, tau = cs + bias.double(), rtol * (cs.abs() + bias.double().abs())
    m = torch.zeros_like(z, dtype=torch.bool)
    for k in ACT_KINKS[act]:
        m |= (z - k).abs() <= tau
    return m


def conv1x1(x, w, dtype=F64):
    return x.to(dtype) @ w.to(dtype).reshape(w.shape[0], -1).t()


def channel_sums(c):
    """sum, sum of squares, and the sums of the absolute terms (the scale of a summation error)."""
    return c.sum(0), (c * c).sum(0), c.abs().sum(0)


def bn_coefficients(s, q, count, gamma, beta, rmean, rvar, eps=BN_EPS):
    """k_f_bn_finalize in fp64 from the (double) sums: rows scale, bias, mean, inv, var and the running statistics after the update."""
    s, q, gamma, beta = s.double(), q.double(), gamma.double(), beta.double()
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    scale = gamma * inv
    unb = var * count / (count - 1.0) if count > 1 else var
    return dict(mean=mean, var=var, inv=inv, scale=scale, bias=beta - mean * scale, bias_mag=beta.abs() + (mean * scale).abs(),
                rmean=(1.0 - BN_MOM) * rmean.double() + BN_MOM * mean, rvar=(1.0 - BN_MOM) * rvar.double() + BN_MOM * unb,
                rmean_mag=(1.0 - BN_MOM) * rmean.double().abs() + BN_MOM * mean.abs())


def emit(c, scale, bias, act, dtype=F64):
    return act_fwd(c.to(dtype) * scale.to(dtype) + bias.to(dtype), act)


def masked_grad(c, g, scale, bias, act, dtype=F64):
    return g.to(dtype) * act_grad(c.to(dtype) * scale.to(dtype) + bias.to(dtype), act)


def bwd_sums(c, g, scale, bias, mean, inv, act, dtype=F64):
    """S1 = sum gm, S2 = sum gm * xhat, and the sums of the absolute terms: |gm|, and |gm| * (|c| + |mean|) * inv -- xhat = (c - mean) * inv
    is itself a difference, rounded relative to |c| + |mean|."""
    gm = masked_grad(c, g, scale, bias, act, dtype)
    c, mean, inv = c.to(dtype), mean.to(dtype), inv.to(dtype)
    xhat = (c - mean) * inv
    return gm.sum(0), (gm * xhat).sum(0), gm.abs().sum(0), (gm.abs() * (c.abs() + mean.abs()) * inv).sum(0)


def bwd_coefficients(S1, S2, count, gamma, inv, mean):
    """k_f_bwd_finalize in fp64: K1, a = S1/N, b = S2/N and the folded rows E, F of dc = g*K1 + conv*E + F (with the size of F's terms)."""
    S1, S2, gamma, inv, mean = S1.double(), S2.double(), gamma.double(), inv.double(), mean.double()
    K1, a, b = gamma * inv, S1 / count, S2 / count
    return dict(K1=K1, a=a, b=b, E=-K1 * b * inv, F=-K1 * a + K1 * b * mean * inv, F_mag=(K1 * a).abs() + (K1 * b * mean * inv).abs())


def dc_direct(c, g, scale, bias, mean, inv, K1, a, b, act, dtype=F64):
    """dc = K1 * ((gm - a) - xhat * b): the definition, and the order the fp32 mode evaluates."""
    gm = masked_grad(c, g, scale, bias, act, dtype)
    xhat = (c.to(dtype) - mean.to(dtype)) * inv.to(dtype)
    return K1.to(dtype) * ((gm - a.to(dtype)) - xhat * b.to(dtype))


def dc_folded(c, g, scale, bias, K1, E, F, act, dtype=F64):
    """dc = gm*K1 + conv*E + F: the form the bf16 mode evaluates from the rows K1, E, F."""
    gm = masked_grad(c, g, scale, bias, act, dtype)
    return gm * K1.to(dtype) + (c.to(dtype) * E.to(dtype) + F.to(dtype))


# ------------------------------------------------------------------------------------------------ the layer, whole (what the CPU test holds to torch)
def conv_bn_forward(x, w, gamma, beta, rmean, rvar, nbt, act, dtype=F64):
    """Conv2d(1x1, bias=False) -> BatchNorm2d(train) -> activation on x [npix][cin]."""
    c = conv1x1(x, w, dtype)
    s, q, _ = channel_sums(c)
    co = bn_coefficients(s, q, c.shape[0], gamma, beta, rmean, rvar)
    co = {k: v.to(dtype) for k, v in co.items()}
    co.update(conv=c, sum=s, sumsq=q, y=emit(c, co["scale"], co["bias"], act, dtype), nbt=nbt + 1)
    return co


def conv_bn_backward(fwd, x, w, g, gamma, act, dgamma, dbeta, dtype=F64):
    c, n = fwd["conv"], fwd["conv"].shape[0]
    S1, S2, _, _ = bwd_sums(c, g, fwd["scale"], fwd["bias"], fwd["mean"], fwd["inv"], act, dtype)
    bc = bwd_coefficients(S1, S2, n, gamma, fwd["inv"], fwd["mean"])
    dc = dc_direct(c, g, fwd["scale"], fwd["bias"], fwd["mean"], fwd["inv"], bc["K1"], bc["a"], bc["b"], act, dtype)
    wm = w.to(dtype).reshape(w.shape[0], -1)
    return dict(S1=S1, S2=S2, dc=dc, dgamma=dgamma.to(dtype) + S2, dbeta=dbeta.to(dtype) + S1, dW=dc.t() @ x.to(dtype), dx=dc @ wm, **bc)


# ------------------------------------------------------------------------------------------------ inputs (fixed seeds: the CPU and GPU files see the same)
def bn_params(c, g):
    """gamma in [0.6, 1.4], beta in +-0.1, running statistics away from their initial values (tests/test_gpu_float.py::_randomize_bn)."""
    return dict(gamma=torch.rand(c, generator=g) * 0.8 + 0.6, beta=torch.rand(c, generator=g) * 0.2 - 0.1,
                rmean=torch.randn(c, generator=g) * 0.1, rvar=torch.rand(c, generator=g) * 0.5 + 0.5)


def layer_inputs(npix, cin, cout, prec, seed):
    """randn activations with a per-channel offset that moves the conv means by up to 1.2 sigma (within +-2 sigma with the sample mean), weights randn * cin^-0.5,
    gradients randn * 0.1; x, gy as the device holds them, w the fp32 master (w_seen what the MFMA multiplies)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, generator=g) * cin ** -0.5
    off = torch.randn(cin, generator=g)
    x = torch.randn(npix, cin, generator=g)
    sd = (x @ w.t()).std(0, unbiased=False) if npix > 1 else w.norm(dim=1)          # an offset moves a channel's mean, not its variance
    x = x + off * (1.2 / float(((w @ off) / sd).abs().max()))
    gy = torch.randn(npix, cout, generator=g) * 0.1
    d = dict(w=w, w_seen=seen(w, prec), x=seen(x, prec), gy=seen(gy, prec), dgamma0=torch.randn(cout, generator=g) * 0.1,
             dbeta0=torch.randn(cout, generator=g) * 0.1, nbt0=3)
    d.update(bn_params(cout, g))
    return d


def kept_inputs(npix, c, prec, seed):
    """A kept conv output (unit variance, channel means within +-1.5) as the device holds it, its gradient, and the coefficient rows of ITS
    batch statistics as fp32 values -- the operands of the element-wise passes."""
    g = torch.Generator().manual_seed(seed)
    conv = seen(torch.randn(npix, c, generator=g) + (torch.rand(c, generator=g) * 3.0 - 1.5), prec)
    gy = seen(torch.randn(npix, c, generator=g) * 0.1, prec)
    d = dict(conv=conv, gy=gy)
    d.update(bn_params(c, g))
    s, q, _ = channel_sums(conv.double())
    co = bn_coefficients(s, q, npix, d["gamma"], d["beta"], d["rmean"], d["rvar"])
    d.update({k: co[k].float() for k in ("scale", "bias", "mean", "inv")})
    return d


def zero_band(gy, conv, scale, bias, act):
    """(gy with the marked elements zeroed, marked share)."""
    m = band_mask(conv, scale, bias, act)
    return torch.where(m, torch.zeros_like(gy), gy), float(m.double().mean())


def pw_seed(npix, cin, cout, act):
    return 100003 * act + 1009 * (npix % 9973) + 31 * cin + cout + PW_SEED_BUMP.get((npix, cin, cout, act), 0)


def ew_seed(npix, c, act):
    return 7 + 200003 * act + 1013 * (npix % 9973) + c + EW_SEED_BUMP.get((npix, c, act), 0)


# A single pixel is a zero-variance batch: z = beta +- round-off amplified by 1/sqrt(eps), so tau is a sizeable part of |beta|; the seed of
# such a case is moved until none of its 8 elements is marked (tests/test_float_kernel_refs_cpu.py checks the share of every case).
PW_SEED_BUMP = {}
EW_SEED_BUMP = {(1, 8, ACT_RELU): 17}

# (npix, cin, cout, act, strided) of the pointwise chain; why each is there: see test_pw_chain.
PW_SMALL = [(1, 8, 8, ACT_RELU, 0), (1, 8, 8, ACT_NONE, 0), (15, 8, 24, ACT_RELU, 0), (15, 8, 24, ACT_HSWISH, 0), (17, 24, 40, ACT_HSWISH, 0),
            (17, 24, 40, ACT_NONE, 0), (63, 40, 24, ACT_RELU, 0), (63, 40, 24, ACT_HSWISH, 1), (65, 32, 16, ACT_NONE, 0)]
PW_BOTH = [(98, 1728, 288, ACT_RELU, 0), (130, 64, 576, ACT_RELU, 1), (130, 64, 592, ACT_RELU, 0), (70000, 16, 80, ACT_RELU, 0)]
PW_CASES = {"bf16": PW_SMALL + [(200, 352, 80, ACT_RELU, 0), (200, 360, 80, ACT_RELU, 0)] + PW_BOTH,
            "fp32": PW_SMALL + [(200, 176, 80, ACT_RELU, 0), (200, 180, 80, ACT_RELU, 0)] + PW_BOTH}
# (npix, c, act, strided) of the element-wise passes
EW_BOTH = [(1, 8, ACT_RELU, 0), (5, 24, ACT_HSWISH, 1), (5, 24, ACT_NONE, 0), (50, 1728, ACT_RELU, 0), (9000, 64, ACT_HSWISH, 0), (9000, 64, ACT_RELU, 1)]
EW_CASES = {"bf16": EW_BOTH + [(131100, 128, ACT_RELU, 0)], "fp32": EW_BOTH}

"""Plain references for the bf16 inference kernels (csrc/frost_infer.hip, frost_iblock.hip, frost_iblockw.hip, frost_ihead.hip, frost_infer_pw,
frost_linear_f32), no device.  Activations are NCHW tensors here; every function evaluates the kernel's definition in the dtype it is given:
torch.float64 is the reference, torch.float32 the yardstick (E32 of tests/test_gpu_infer_kernels.py).

Two classes of data.  Class X (exact): small integers and an identity fold (FrostIDesc.gamma = NULL: W' = W, b' = beta) -- every product and partial
sum is an integer below 2^24, so fp32 accumulation in ANY order equals the fp64 value and its rounding to bf16 is one fixed bit pattern, which is
again an integer times a power of two: exactness carries through a composition.  Class T (tolerance): random data, real BatchNorm parameters.
tests/test_infer_kernel_refs_cpu.py holds these functions to torch's own modules and checks the conditions of class X for every case below.
The case tables of the GPU file live here so that both files see the same cases."""
import torch
import torch.nn.functional as TF

import float_kernel_refs as FR
from float_kernel_refs import ACT_HSWISH, ACT_NONE, ACT_RELU, BF16_U, DEV_BN_EPS, F32, F64, act_fwd, round_up  # noqa: F401

EXACT_LIMIT = 2 ** 24         # integers below it are exact in fp32
TIE_RTOL = 3e-7               # the device folds in fp32: add, sqrt, divide and the product round once each, 2^-24 apiece with the sqrt halving what it is given: < 2.2e-7


def rb(t):
    """One rounding to bf16 (round to nearest even), back in the dtype it came in.  Exact operands of class X are fp32-exact, so the way through
    float does not round twice there."""
    return t.float().bfloat16().to(t.dtype)


def bits(t):
    return t.float().bfloat16().view(torch.int16)


# ------------------------------------------------------------------------------------------------ fold and packs
def fold(w, gamma, beta, rmean, rvar, eps=DEV_BN_EPS):
    """(W', b') in fp64: W' = W * gamma / sqrt(rvar + eps), b' = beta - rmean * gamma / sqrt(rvar + eps); gamma None: W' = W, b' = beta or 0."""
    w = w.double()
    if gamma is None:
        return w, (beta.double() if beta is not None else torch.zeros(w.shape[0], dtype=F64))
    sf = gamma.double() / torch.sqrt(rvar.double() + eps)
    return w * sf.view(-1, *([1] * (w.dim() - 1))), beta.double() - rmean.double() * sf


def fold_terms(gamma, beta, rmean, rvar, eps=DEV_BN_EPS):
    """|beta| + |rmean * sf|: the size of the terms b' is made of."""
    if gamma is None:
        return beta.double().abs() if beta is not None else None
    sf = gamma.double() / torch.sqrt(rvar.double() + eps)
    return beta.double().abs() + (rmean.double() * sf).abs()


def bf16_weights(wf):
    """(bf16(W'), slack): the device rounds ITS fp32 fold, which lies within TIE_RTOL of W'; where a rounding tie lies that close, either
    neighbour is a correct result and slack holds their distance (zero everywhere else)."""
    lo, hi = rb(wf * (1.0 - TIE_RTOL)), rb(wf * (1.0 + TIE_RTOL))
    return rb(wf), (hi - lo).abs()


def pack0(m):
    """kind 0: [cout][cin_g] -> A fragments [ct][kb][lane][8] with (co = ct*16 + (lane&15), k = kb*32 + (lane>>4)*8 + e), zero padding."""
    return FR.pack_matrix(m, round_up(m.shape[0], 16), round_up(m.shape[1], 32), 32)


def unpack0(flat, cout, cin_g):
    return FR.unpack_matrix(flat, round_up(cout, 16), round_up(cin_g, 32), 32)[:cout, :cin_g]


def pack2(w):
    """kind 2, the stem: OIHW [cout][3][3][3] -> k = tap*4 + c, kpad = 64."""
    return FR.pack_matrix(FR.stem_matrix(w), round_up(w.shape[0], 16), 64, 32)


def unpack2(flat, cout):
    m = FR.unpack_matrix(flat, round_up(cout, 16), 64, 32)[:cout]
    return m.reshape(cout, 16, 4)[:, :9, :3].permute(0, 2, 1).reshape(cout, 3, 3, 3)


def pack1(w):
    """kind 1, depthwise: [c][1][k][k] -> fp32 [tap][cpad]."""
    c, kk = w.shape[0], w.shape[2] * w.shape[3]
    out = torch.zeros(kk, round_up(c, 16), dtype=w.dtype)
    out[:, :c] = w.reshape(c, kk).t()
    return out.reshape(-1)


def unpack1(flat, c, k):
    return flat.reshape(k * k, round_up(c, 16))[:, :c].t().reshape(c, 1, k, k)


# ------------------------------------------------------------------------------------------------ layers
def layer(x, w, b, k=1, stride=1, groups=1, act=ACT_NONE, dtype=F64):
    """act(conv(x, W') + b'), padding (k-1)/2, not rounded.  x NCHW, w OIHW (a [cout][cin] matrix is taken as 1x1)."""
    if w.dim() == 2:
        w = w.reshape(w.shape[0], w.shape[1], 1, 1)
    if k == 1 and stride == 1 and groups == 1:                                      # a matrix product: the same sums, and quick in double
        z = (x.to(dtype).permute(0, 2, 3, 1) @ w.to(dtype).reshape(w.shape[0], -1).t()).permute(0, 3, 1, 2)
        return act_fwd(z if b is None else z + b.to(dtype).view(1, -1, 1, 1), act)
    z = TF.conv2d(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), stride, (k - 1) // 2, 1, groups)
    return act_fwd(z, act)


def layer_terms(x, w, b, k=1, stride=1, groups=1, bterms=None):
    """sum of |x w| + the size of the bias terms: what a summation error is measured against."""
    bt = bterms if bterms is not None else (None if b is None else b.abs())
    return layer(x.abs(), w.abs(), bt, k, stride, groups, ACT_NONE, F64)


def stem(x, w, b, act=ACT_RELU, dtype=F64):
    """3x3 stride-2 pad-1 conv of the image as the kernels see it (rounded to bf16 once)."""
    return layer(rb(x.to(dtype)), w, b, 3, 2, 1, act, dtype)


def cat(a, b):
    return torch.cat([a, b], 1)


def add(a, b):
    """bf16(a + b): one fp32 addition of two bf16 values, rounded once."""
    return (a.float() + b.float()).bfloat16()


def avgpool(x, dtype=F64):
    return x.to(dtype).sum((2, 3)) / float(x.shape[2] * x.shape[3])


def avgpool_exact(x):
    """class X: float32(sum) / float32(hw), one correctly rounded division."""
    return x.double().sum((2, 3)).float() / torch.tensor(float(x.shape[2] * x.shape[3]), dtype=F32)


def linear(x, w, b, dtype=F64):
    return x.to(dtype) @ w.to(dtype).t() + b.to(dtype)


def bottleneck(x, sq, c1, dw, red, k, stride, residual, dtype=F64, trace=None):
    """[squeeze + ReLU -> cat([squeezed, x])] -> [conv1 + ReLU] -> depthwise k x k + ReLU -> reduce (linear) [-> bf16(bf16(out) + x)], every layer
    output rounded to bf16 once.  sq / c1 / dw / red: (W', b') or None.  trace: a list that receives (name, sum|term|, rounded output, relu)."""
    def run(name, a, wb, kk, st, groups, act):
        y = rb(layer(a, wb[0], wb[1], kk, st, groups, act, dtype))
        if trace is not None:
            trace.append((name, layer_terms(a, wb[0], wb[1], kk, st, groups), y, act == ACT_RELU))
        return y
    a = x.to(dtype)
    if c1 is not None:
        if sq is not None:
            a = cat(run("squeeze", a, sq, 1, 1, 1, ACT_RELU), a)
        a = run("conv1", a, c1, 1, 1, 1, ACT_RELU)
    a = run("conv2", a, dw, k, stride, a.shape[1], ACT_RELU)
    a = run("reduce", a, red, 1, 1, 1, ACT_NONE)
    return rb(a + x.to(dtype)) if residual else a


def sep_heads(x, dw_loc, pw_loc, dw_conf, pw_conf, dtype=F64, trace=None):
    """Both SepHeads of one source: depthwise 3x3 + ReLU (rounded to bf16) -> 1x1 (fp32 store, not rounded).  Returns (loc, conf) NCHW."""
    outs = []
    for name, dw, pw in (("loc", dw_loc, pw_loc), ("conf", dw_conf, pw_conf)):
        t = rb(layer(x, dw[0], dw[1], 3, 1, x.shape[1], ACT_RELU, dtype))
        y = layer(t, pw[0], pw[1], 1, 1, 1, ACT_NONE, dtype)
        if trace is not None:
            trace.append((name + ".dw", layer_terms(x, dw[0], dw[1], 3, 1, x.shape[1]), t, True))
            trace.append((name + ".pw", layer_terms(t, pw[0], pw[1]), y, False))
        outs.append(y)
    return outs


# ------------------------------------------------------------------------------------------------ class X operands
def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def int_conv(g, cout, cin_g, k=1):
    """(W in {-1, 0, 1}, b in [-3, 3])"""
    return ints(g, (cout, cin_g, k, k), -1, 1), ints(g, (cout,), -3, 3)


def trace_stats(trace):
    """per layer: (name, max sum|term|, share of nonzero outputs, distinct output values, relu)"""
    return [(nm, float(t.max()), float((y != 0).double().mean()), int(torch.unique(y).numel()), relu) for nm, t, y, relu in trace]


def int_case(seed, kind, **s):
    """Integer operands of one case: x in [-4, 4], weights in {-1, 0, 1}, biases in [-3, 3].  kind 'layer' (cin, cout, k, stride, groups, n, h, w, act),
    'block' (a BLOCK_CASES / BLOCKW_CASES geometry + n) or 'heads' (cin, cl, cc, n, h, w).  Returns (operands, reference output(s), trace_stats)."""
    g = torch.Generator().manual_seed(seed)
    tr = []
    if kind == "layer":
        x = ints(g, (s["n"], s["cin"], s["h"], s["w"]), -4, 4)
        w, b = int_conv(g, s["cout"], s["cin"] // s.get("groups", 1), s.get("k", 1))
        y = layer(x, w, b, s.get("k", 1), s.get("stride", 1), s.get("groups", 1), s.get("act", ACT_NONE))
        tr.append(("layer", layer_terms(x, w, b, s.get("k", 1), s.get("stride", 1), s.get("groups", 1)), rb(y), s.get("act") == ACT_RELU))
        return dict(x=x, w=w, b=b), y, trace_stats(tr)
    if kind == "block":
        x = ints(g, (s["n"], s["cin"], s["h"], s["w"]), -4, 4)
        conv1 = s["cexp"] != s["cin"] or s["r"] > 0
        sq = int_conv(g, s["r"], s["cin"]) if s["r"] else None
        c1 = int_conv(g, s["cexp"], s["r"] + s["cin"]) if conv1 else None
        dw = int_conv(g, s["cexp"], 1, s["k"])
        red = int_conv(g, s["cout"], s["cexp"])
        y = bottleneck(x, sq, c1, dw, red, s["k"], s["stride"], s["residual"], trace=tr)
        return dict(x=x, sq=sq, c1=c1, dw=dw, red=red), y, trace_stats(tr)
    if kind == "heads":
        x = ints(g, (s["n"], s["cin"], s["h"], s["w"]), -4, 4)
        ops = dict(x=x, dw_loc=int_conv(g, s["cin"], 1, 3), pw_loc=int_conv(g, s["cl"], s["cin"]), dw_conf=int_conv(g, s["cin"], 1, 3),
                   pw_conf=int_conv(g, s["cc"], s["cin"]))
        y = sep_heads(x, ops["dw_loc"], ops["pw_loc"], ops["dw_conf"], ops["pw_conf"], trace=tr)
        return ops, y, trace_stats(tr)
    raise ValueError(kind)


def bn_params(c, g):
    return FR.bn_params(c, g)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ================================================================================================ the case tables
# Thresholds re-read from the host functions; BP = 128 pixels per k_pw tile (frost_pw.hip:55).
# frost_infer_pw (frost_pw.hip:1100-1109): cin >= 129 and npix >= 256 -> frost_gemm_bf16_rows; everything else k_pw<M_DGRAD>.
#   set_tiling (:958-970): rowbytes = 2 cin; one chunk up to 512 B, 512-byte chunks above; the DMA-staged linear tile (gl) needs one chunk and
#   128 * rowbytes <= 32 KB, i.e. cin <= 128.  pw_wave_split (:974): CT <= 4 -> 8 pixel waves x 1, CT <= 8 -> 4 x 2, above 2 x 4.
#   launch_pw (:916-940): full 128-pixel tiles in one launch, the ragged tail in a second one.
# (npix, cin, cout)
PW_STAGED = [(1, 8, 8), (127, 8, 24), (128, 24, 72), (129, 40, 88), (300, 128, 136), (1, 128, 24), (127, 40, 136), (128, 128, 8), (129, 24, 88),
             (300, 8, 72), (300, 24, 24), (129, 128, 72), (127, 128, 88), (300, 40, 8),
             (8193, 24, 72)]      # 64 full tiles: launch_pw's LDS-resident weights (:921-923, res_mint = 64), the instance the networks run at B = 256, and a one-pixel tail
#   long rows: 136 -> 272 B, one chunk, tile past 32 KB (gl off); 256 -> the 512-byte chunk exactly; 264 -> two chunks, 16-byte tail; 512 -> two whole
#   chunks; 1280 -> five chunks.  cout 24 / 88 / 256: CT 2 / 6 / 16, the three wave splits.
PW_LONG = [(1, 136, 24), (8, 136, 88), (255, 136, 256), (8, 256, 24), (255, 264, 88), (1, 264, 256), (255, 512, 24), (8, 512, 256), (1, 1280, 88),
           (255, 1280, 256), (8, 1280, 24)]
#   wide GEMM (frost_wgrad.hip:575-582, launch_dgw :555-563): kp = round_up(cin, 16), KB = kp / 32 + (kp % 32 != 0): 136 -> kp 144, the last block
#   half filled and 8 columns of padding; 144 -> kp % 32 == 16; 160 -> whole blocks.  nch = ceil(ceil(cout / 16) / 8) channel groups; the 128-pixel
#   instance while ceil(npix / 256) * nch < 320, the 256-pixel one from there: cout = 136 (nch 2) at npix = 40961 (161 * 2 = 322).
PW_WIDE = [(256, 136, 8), (257, 144, 24), (383, 160, 136), (256, 160, 1728), (383, 136, 24), (257, 136, 136), (256, 144, 136), (40961, 136, 136)]
PW_CASES = PW_STAGED + PW_LONG + PW_WIDE

# frost_infer_dw (frost_infer.hip:227-238): one thread = 8 channels x IDW_WO = 4 output pixels of a row; cpad = round_up(c, 16) != c for 8, 24, 40.
# (k, stride, c, h, w): every (k, stride) on every map; wo % 4 takes 0..3 over the maps; 2x5 and below are smaller than the 5x5 window's padding;
# 8x6 with stride 2 pads one side only.
DW_MAPS = [(1, 1), (2, 2), (2, 5), (3, 5), (7, 7), (8, 6), (9, 11)]
DW_CASES = [(k, s, (8, 24, 40)[(i + k + s) % 3], h, w) for k in (3, 5) for s in (1, 2) for i, (h, w) in enumerate(DW_MAPS)]

# frost_infer_stem (frost_infer.hip:157-170): workgroup tile IS_TH = 4 rows x 128 columns, CT = ceil(cout / 16) in 1..4.
# (h, w, cout, layout): (9, 258) -> wo = 129 crosses the 128-column tile, ho = 5 is no multiple of 4; (5, 259) -> wo = 130.
STEM_IMAGES = [(1, 1), (2, 3), (7, 9), (8, 8), (9, 258), (5, 259)]
STEM_LAYOUTS = ["nchw", "nhwc", "crop"]
STEM_CASES = [(h, w, (8, 24, 32, 40, 64)[(3 * i + j) % 5], lay) for i, (h, w) in enumerate(STEM_IMAGES) for j, lay in enumerate(STEM_LAYOUTS)]

CAT_CASES = [(ca, cb, npix) for ca, cb in ((8, 8), (8, 24), (24, 40)) for npix in (1, 257)]
ADD_CASES = [8, 8 * 257]
POOL_CASES = [(n, hw, c) for n in (1, 3) for hw in (1, 49, 50) for c in (8, 24, 1280)]
# frost_linear_f32 -> launch_sgemm (frost_head.hip:144-164, max_split 2): two-way K split when tiles < 256 and K / 2 >= 64 (K >= 128); the 64-deep
# stage when K / ks >= 256 (K >= 512 with the split).  (n, k, o)
LIN_CASES = [(1, 127, 21), (65, 128, 64), (1, 511, 65), (65, 512, 1000), (1, 1280, 1000), (65, 1280, 21), (65, 127, 65), (1, 128, 1000)]

# frost_infer_block (frost_iblock.hip:279-351).  per_wave = ceil(ct3 * tpt / waves) selects MAXT 4 / 8 / 12 / 20; kb1 = round_up(r + cin, 32) / 32 <= 2
# selects the shallow conv1 instance, above it the 10-deep one; chunk 32 only with kb1 <= 2.  variants: (th, tw, waves, chunk); th = 0: the whole map.
def _blk(name, cin, r, cexp, cout, k, stride, h, w, residual, variants):
    return dict(name=name, cin=cin, r=r, cexp=cexp, cout=cout, k=k, stride=stride, h=h, w=w, residual=residual, variants=variants)


BLOCK_CASES = [
    _blk("sq24_72_k5", 24, 8, 72, 24, 5, 1, 7, 9, 1, [(0, 0, 4, 64), (4, 4, 4, 32)]),
    _blk("nosq16_96_k3s2", 16, 0, 96, 24, 3, 2, 9, 11, 0, [(4, 8, 4, 32), (4, 8, 4, 64)]),
    _blk("noconv1_32", 32, 0, 32, 16, 3, 1, 6, 6, 0, [(0, 0, 4, 64)]),
    _blk("sq40_240_k5s2", 40, 16, 240, 40, 5, 2, 8, 8, 0, [(4, 4, 4, 64), (3, 3, 4, 64)]),
    _blk("sq104_624_k5", 104, 24, 624, 104, 5, 1, 7, 7, 1, [(0, 0, 4, 64), (0, 0, 8, 64), (0, 0, 16, 64)]),
    _blk("kb1_10", 256, 64, 96, 24, 3, 1, 4, 4, 0, [(0, 0, 4, 64)]),
    _blk("acc_cout320", 40, 8, 64, 320, 3, 1, 7, 7, 0, [(4, 4, 8, 64), (4, 4, 4, 64), (0, 0, 8, 64), (0, 0, 4, 64), (4, 7, 4, 64)]),
]
# the fp32 emulation is checked on these four, and on every other case as well
EMULATED = ["sq24_72_k5", "sq40_240_k5s2", "sq104_624_k5", "sq240_1440_k5"]
EXTRA_CPU_BLOCKS = [_blk("sq240_1440_k5", 240, 40, 1440, 240, 5, 1, 4, 4, 1, [])]

# frost_infer_block_w (frost_iblockw.hip:215-242): no squeeze, tiles 4 x 4 / 4 x 8, (k3 s1 | k3 s2 | k5 s2) with conv1 (cin <= 32), k3 s1 without.
BLOCKW_CASES = []
for _i, (_k, _s, _c1) in enumerate([(3, 1, 1), (3, 2, 1), (5, 2, 1), (3, 1, 0)]):
    for _j, (_h, _w) in enumerate([(5, 7), (9, 6)]):
        _cexp = (32, 72)[(_i + _j) % 2]
        _cin = 24 if _c1 else _cexp
        _cout = 24 if (_s == 1 and _c1 and _j == 0) else (32 if (not _c1 and _cexp == 32) else (48, 24)[(_i + _j) % 2])      # 24 -> 24 and 32 -> 32: the residual
        BLOCKW_CASES.append(_blk("w_k%ds%d_c%d_%dx%d" % (_k, _s, _c1, _h, _w), _cin, 0, _cexp, _cout, _k, _s, _h, _w, int(_s == 1 and _cin == _cout),
                                 [(4, 4), (4, 8)]))

# frost_infer_head (frost_ihead.hip:160-189): IH_TP = 32 pixels per workgroup, IH_KC = 64 input channels per chunk (264 -> five chunks, the last one 8 wide),
# IH_CTMAX = 10 channel tiles over both heads.  (cin, h, w, anchors, offsets): stored widths 4 A and 21 A; the 1x1 layers carry round_up(., 8) channels.
HEAD_CLASSES = 21
HEAD_CASES = [(cin, h, w, (4, 6)[(i + j) % 2], ((0, 0), (6, 21))[(i + j // 2) % 2]) for i, cin in enumerate((8, 40, 96, 264))
              for j, (h, w) in enumerate(((1, 1), (2, 3), (5, 3)))]


# ------------------------------------------------------------------------------------------------ class X operands of the single-layer tables
def pw_seed(c):
    return 1000 + c[0] + c[1] + c[2]


def pw_ints(c, act=ACT_NONE):
    """(operands, reference, trace_stats) of a PW_CASES entry"""
    npix, cin, cout = c
    return int_case(pw_seed(c), "layer", n=1, h=1, w=npix, cin=cin, cout=cout, act=act)


# 16 outputs of one tap each: the seed of such a case is moved until the reference meets the conditions (tests/test_infer_kernel_refs_cpu.py checks every case)
DW_SEED_BUMP = {(5, 1, 8, 1, 1): 1}


def dw_seed(c):
    k, s, ch, h, w = c
    return 2000 + 97 * k + 31 * s + 7 * h + w + ch + DW_SEED_BUMP.get(tuple(c), 0)


def dw_ints(c, act=ACT_NONE, n=2):
    k, s, ch, h, w = c
    return int_case(dw_seed(c), "layer", n=n, h=h, w=w, cin=ch, cout=ch, k=k, stride=s, groups=ch, act=act)


def stem_seed(c):
    return 3000 + 13 * c[0] + c[1] + c[2]


def stem_ints(c, act=ACT_NONE, n=2):
    """the image holds integers, so its rounding to bf16 is the identity and the stem is a 3x3 stride-2 layer"""
    h, w, cout, _ = c
    return int_case(stem_seed(c), "layer", n=n, h=h, w=w, cin=3, cout=cout, k=3, stride=2, act=act)


def lin_ints(c):
    """a LIN_CASES entry as a 1x1 layer over n 'pixels': x [n][k], w [o][k], b [o], reference [n][o]"""
    n, k, o = c
    ops, y, st = int_case(4000 + n + k + o, "layer", n=1, h=1, w=n, cin=k, cout=o)
    return dict(x=ops["x"][0, :, 0, :].t().contiguous(), w=ops["w"].reshape(o, k), b=ops["b"]), y[0, :, 0, :].t().contiguous(), st


def pool_ints(c):
    """a POOL_CASES entry: x NCHW [n][c][1][hw]; the trace holds sum|x| (the division comes after the sum) and the fp32 means"""
    n, hw, ch = c
    x = ints(torch.Generator().manual_seed(5000 + n + hw + ch), (n, ch, 1, hw), -4, 4)
    y = avgpool_exact(x)
    return dict(x=x), y, trace_stats([("avgpool", x.abs().sum((2, 3)), y, False)])


def block_seed(c):
    return 7000 + sum(ord(ch) for ch in c["name"])


def head_seed(c):
    return 9000 + c[0] * 31 + c[1] * 7 + c[2] + c[3]

// Lite R-ASPP segmentation head of the float path (Semantic_Segmentation/model/layers/LRASPP.py _LRASPP + _Head, the three outer lines of
// model/mobilenetv3.py MobileNetV3Seg.forward), forward and backward, in the storage type of the float path (bf16 / fp32 NHWC, the *_f32 entries):
//     feat1 = ConvBNReLU(c4)                          existing float kernels (frost_float.hip)
//     g     = ConvBN(avgpool(c4))                     frost_seghead_pool here, then the existing float kernels
//     p     = W_proj (feat1 * up(hsig(g))) + b_proj   frost_seghead_gate_project          (c4's resolution)
//     out   = up(p) + W_aux c1 + b_aux                frost_seghead_logits                (c1's resolution)
// replaces: AvgPool2d, _Hsigmoid, two F.interpolate(align_corners=True), the FloatFunctional mul, two biased 1x1 Conv2d and the add, with their autograd backward.
// `project` is linear and bilinear weights sum to one, so project(up(z)) == up(project(z)): the 128-channel map at c1's resolution is never made, in either
// direction, and z itself is not stored (the backward recomputes it from feat1 and g).  up() follows seg_src (frost_common.h), horizontally first.
// Accumulation fp32; parameters and their gradients fp32.  The data gradients (dc1, dfeat1, dg, dp, the pool's dx) are gathers: every element is written once
// from sums in a fixed order.  The weight and bias gradients are per-workgroup register sums flushed with fp32 atomics: their last bits depend on the order.
#include "frost_common.h"

#define SH_CF_MAX 128      // feature channels of a 1x1 product here (the head's 128, c1's width)
#define SH_CP 32           // classes per chunk: above it the kernels work chunk by chunk (slow, correct)
#define SH_PT_GATE 16      // pixels per tile at c4's resolution
#define SH_PT 64           // pixels per tile at c1's resolution

template <typename T> struct SEl;
template <> struct SEl<uint16_t> {
  static __device__ __forceinline__ float ld(const uint16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(uint16_t* p, float v) { *p = f2bf(v); }
};
template <> struct SEl<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
__device__ __forceinline__ void sh_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void sh_st(uint16_t* p, float v) { *p = f2bf(v); }

// the reference's _Hsigmoid: relu6(v + 3) * (1 / 6); its gradient is hardtanh's open interval
__device__ __forceinline__ float sh_hsig(float v) { return fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) * (1.0f / 6.0f); }
__device__ __forceinline__ float sh_dhsig(float v) { const float t = v + 3.0f; return (t > 0.0f && t < 6.0f) ? (1.0f / 6.0f) : 0.0f; }
static inline float sh_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }
// seg_first with out == 1 allowed (scale == 0: every destination reads source 0)
__device__ __forceinline__ int sh_first(int c, float scale, int in, int out) {
  if (scale == 0.0f) return c <= 0 ? 0 : out;
  return seg_first(c, scale, in, out);
}
// weight of source index `src` in destination index d
__device__ __forceinline__ float sh_weight(int d, float scale, int in, int src) {
  int i0; float f;
  seg_src(d, scale, in, i0, f);
  const int i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  return (i0 == src ? 1.0f - f : 0.0f) + (i1 == src ? f : 0.0f);
}

// ------------------------------------------------------------------------------------------------ windowed average pool
// y[n][py][px][c] = mean of x[n][py*sh .. +kh)[px*sw .. +kw)[c] (no padding, floor mode: ph = (h - kh) / sh + 1); rows summed first, then the rows added up
template <typename ET>
__global__ __launch_bounds__(256) void k_sh_pool(const ET* __restrict__ x, int n, int h, int w, int c, int kh, int kw, int sh, int sw, int ph, int pw, ET* __restrict__ y) {
  const int64_t tot = (int64_t)n * ph * pw * c;
  const float div = (float)(kh * kw);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int ch = (int)(i % c); int64_t r = i / c;
    const int px = (int)(r % pw); r /= pw;
    const int py = (int)(r % ph); const int in = (int)(r / ph);
    const ET* base = x + (((int64_t)in * h + (int64_t)py * sh) * w + (int64_t)px * sw) * c + ch;
    float s = 0.0f;
    for (int dy = 0; dy < kh; ++dy) {
      float rs = 0.0f;
      for (int dx = 0; dx < kw; ++dx) rs += SEl<ET>::ld(base + ((int64_t)dy * w + dx) * c);
      s += rs;
    }
    SEl<ET>::st(y + i, s / div);
  }
}
// dx[n][y][x][c] = (sum of dy over the windows that contain (y, x)) / (kh kw) [+ addend]: a gather, pixels no window covers get the addend alone
template <typename ET>
__global__ __launch_bounds__(256) void k_sh_pool_bwd(const ET* __restrict__ dy, const ET* __restrict__ addend, int n, int h, int w, int c, int kh, int kw, int sh,
                                                      int sw, int ph, int pw, ET* __restrict__ dx) {
  const int64_t tot = (int64_t)n * h * w * c;
  const float div = (float)(kh * kw);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int ch = (int)(i % c); int64_t r = i / c;
    const int xx = (int)(r % w); r /= w;
    const int yy = (int)(r % h); const int in = (int)(r / h);
    const int py0 = yy >= kh ? (yy - kh) / sh + 1 : 0, py1 = min(yy / sh, ph - 1);
    const int px0 = xx >= kw ? (xx - kw) / sw + 1 : 0, px1 = min(xx / sw, pw - 1);
    float s = 0.0f;
    for (int py = py0; py <= py1; ++py)
      for (int px = px0; px <= px1; ++px) s += SEl<ET>::ld(dy + (((int64_t)in * ph + py) * pw + px) * c + ch);
    s = s / div;
    if (addend) s += SEl<ET>::ld(addend + i);
    SEl<ET>::st(dx + i, s);
  }
}

// ------------------------------------------------------------------------------------------------ gate + project
struct ShGate { int n, h4, w4, ph, pw, cf, nclass; float sy, sx; };

// up(hsig(g)) at pixel (y, x) of image `in`, channel c
template <typename ET>
__device__ __forceinline__ float sh_gate_at(const ShGate& g, const ET* __restrict__ gm, int in, int y, int x, int c) {
  int y0, x0; float fy, fx;
  seg_src(y, g.sy, g.ph, y0, fy);
  seg_src(x, g.sx, g.pw, x0, fx);
  const int y1 = y0 + 1 < g.ph ? y0 + 1 : g.ph - 1, x1 = x0 + 1 < g.pw ? x0 + 1 : g.pw - 1;
  const ET* b = gm + (int64_t)in * g.ph * g.pw * g.cf + c;
  const float a00 = sh_hsig(SEl<ET>::ld(b + ((int64_t)y0 * g.pw + x0) * g.cf)), a01 = sh_hsig(SEl<ET>::ld(b + ((int64_t)y0 * g.pw + x1) * g.cf));
  const float a10 = sh_hsig(SEl<ET>::ld(b + ((int64_t)y1 * g.pw + x0) * g.cf)), a11 = sh_hsig(SEl<ET>::ld(b + ((int64_t)y1 * g.pw + x1) * g.cf));
  const float top = (1.0f - fx) * a00 + fx * a01, bot = (1.0f - fx) * a10 + fx * a11;
  return (1.0f - fy) * top + fy * bot;
}

// p[pix][k] = sum_c W[k][c] feat1[pix][c] gate[pix][c] + b[k], fp32 [n][h4][w4][nclass]
template <typename ET>
__global__ __launch_bounds__(256) void k_sh_gate_project(const ShGate g, const ET* __restrict__ feat1, const ET* __restrict__ gm, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ p) {
  __shared__ float sz[SH_PT_GATE][SH_CF_MAX];
  __shared__ float sw[SH_CP][SH_CF_MAX + 1];
  const int tid = threadIdx.x, cf = g.cf;
  const int64_t npix = (int64_t)g.n * g.h4 * g.w4, tiles = (npix + SH_PT_GATE - 1) / SH_PT_GATE;
  const bool single = g.nclass <= SH_CP;
  bool loaded = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    for (int e = tid; e < SH_PT_GATE * cf; e += 256) {
      const int pl = e / cf, c = e - pl * cf;
      const int64_t pix = tile * SH_PT_GATE + pl;
      float z = 0.0f;
      if (pix < npix) {
        const int x = (int)(pix % g.w4); const int64_t r = pix / g.w4;
        z = SEl<ET>::ld(feat1 + pix * cf + c) * sh_gate_at(g, gm, (int)(r / g.h4), (int)(r % g.h4), x, c);
      }
      sz[pl][c] = z;
    }
    for (int k0 = 0; k0 < g.nclass; k0 += SH_CP) {
      const int kc = min(SH_CP, g.nclass - k0);
      if (!(single && loaded)) {
        __syncthreads();
        for (int e = tid; e < kc * cf; e += 256) { const int kl = e / cf, c = e - kl * cf; sw[kl][c] = W[(int64_t)(k0 + kl) * cf + c]; }
        loaded = true;
      }
      __syncthreads();
      for (int e = tid; e < SH_PT_GATE * SH_CP; e += 256) {
        const int kl = e % SH_CP, pl = e / SH_CP;
        const int64_t pix = tile * SH_PT_GATE + pl;
        if (kl < kc && pix < npix) {
          float s = 0.0f;
          for (int c = 0; c < cf; ++c) s += sw[kl][c] * sz[pl][c];
          p[pix * g.nclass + k0 + kl] = s + bias[k0 + kl];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward of a biased 1x1 product (project, auxlayer)
// d [pixel][k] (element strides) is the gradient of  sum_c W[k][c] v[pixel][c] + b[k]  with v = f (auxlayer: f = c1) or v = f * gate (project: f = feat1):
//   dW[k][c] += sum_pixels d v, db[k] += sum_pixels d           register sums over the workgroup's tiles, one atomic flush
//   dv = W^T d;  df = dv (auxlayer)  or  df = dv * gate, dgate = dv * f (fp32 scratch; its upsampling adjoint is k_sh_up_adjoint)
struct ShLin { int n, h, w, cf, nclass; int64_t dn, dc, dh, dw; };
template <typename ET, bool GATE, int PT>
__global__ __launch_bounds__(256) void k_sh_lin_bwd(const ShLin q, const ShGate g, const ET* __restrict__ f, const ET* __restrict__ gm, const float* __restrict__ d,
                                                     const float* __restrict__ W, float* __restrict__ dW, float* __restrict__ db, ET* __restrict__ df,
                                                     float* __restrict__ dgate) {
  __shared__ float sf[PT][SH_CF_MAX];
  __shared__ float sg[GATE ? PT : 1][GATE ? SH_CF_MAX : 1];
  __shared__ float sd[PT][SH_CP + 1];
  const int tid = threadIdx.x, cf = q.cf;
  const int64_t npix = (int64_t)q.n * q.h * q.w, tiles = (npix + PT - 1) / PT;
  for (int k0 = 0; k0 < q.nclass; k0 += SH_CP) {
    const int kc = min(SH_CP, q.nclass - k0);
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
    float accb = 0.0f;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      __syncthreads();
      for (int e = tid; e < PT * cf; e += 256) {
        const int pl = e / cf, c = e - pl * cf;
        const int64_t pix = tile * PT + pl;
        float v = 0.0f, gt = 0.0f;
        if (pix < npix) {
          v = SEl<ET>::ld(f + pix * cf + c);
          if (GATE) { const int x = (int)(pix % q.w); const int64_t r = pix / q.w; gt = sh_gate_at(g, gm, (int)(r / q.h), (int)(r % q.h), x, c); }
        }
        sf[pl][c] = v;
        if (GATE) sg[pl][c] = gt;
      }
      for (int e = tid; e < PT * kc; e += 256) {
        int pl, kl;
        if (q.dc == 1) { pl = e / kc; kl = e - pl * kc; } else { kl = e / PT; pl = e - kl * PT; }
        const int64_t pix = tile * PT + pl;
        float v = 0.0f;
        if (pix < npix) {
          const int x = (int)(pix % q.w); const int64_t r = pix / q.w;
          v = d[(r / q.h) * q.dn + (int64_t)(k0 + kl) * q.dc + (r % q.h) * q.dh + (int64_t)x * q.dw];
        }
        sd[pl][kl] = v;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int idx = tid + j * 256, kl = idx / cf, c = idx - kl * cf;
        if (kl < kc) {
          float s = 0.0f;
          for (int pl = 0; pl < PT; ++pl) s += sd[pl][kl] * (GATE ? sf[pl][c] * sg[pl][c] : sf[pl][c]);
          acc[j] += s;
        }
      }
      if (tid < kc) {
        float s = 0.0f;
        for (int pl = 0; pl < PT; ++pl) s += sd[pl][tid];
        accb += s;
      }
      if (k0 == 0) {
        for (int e = tid; e < PT * cf; e += 256) {
          const int pl = e / cf, c = e - pl * cf;
          const int64_t pix = tile * PT + pl;
          if (pix >= npix) continue;
          float dv = 0.0f;
          for (int k = 0; k < kc; ++k) dv += W[(int64_t)k * cf + c] * sd[pl][k];
          if (q.nclass > SH_CP) {          // the classes of the later chunks: read in place
            const int x = (int)(pix % q.w); const int64_t r = pix / q.w;
            const float* dr = d + (r / q.h) * q.dn + (r % q.h) * q.dh + (int64_t)x * q.dw;
            for (int k = SH_CP; k < q.nclass; ++k) dv += W[(int64_t)k * cf + c] * dr[(int64_t)k * q.dc];
          }
          if (GATE) { SEl<ET>::st(df + pix * cf + c, dv * sg[pl][c]); dgate[pix * cf + c] = dv * sf[pl][c]; }
          else SEl<ET>::st(df + pix * cf + c, dv);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = tid + j * 256, kl = idx / cf, c = idx - kl * cf;
      if (kl < kc) atomicAdd(dW + (int64_t)(k0 + kl) * cf + c, acc[j]);
    }
    if (tid < kc) atomicAdd(db + k0 + tid, accb);
  }
}

// ------------------------------------------------------------------------------------------------ adjoint of the upsampling, gather form
// dst[n][ys][xs][c] = sum over the destination pixels (Y, X) that read source (ys, xs) of wy wx src[n][Y][X][c], rows first; HS: times hsig'(gm) (dst is then dg)
struct ShUp { int n, hs, ws, hd, wd, c; int64_t sn, sc, sh, sw; float sy, sx; };
template <typename OT, typename GT, bool HS>
__global__ __launch_bounds__(256) void k_sh_up_adjoint(const ShUp u, const float* __restrict__ src, const GT* __restrict__ gm, OT* __restrict__ dst) {
  const int64_t tot = (int64_t)u.n * u.hs * u.ws * u.c;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int ch = (int)(i % u.c); int64_t r = i / u.c;
    const int xs = (int)(r % u.ws); r /= u.ws;
    const int ys = (int)(r % u.hs); const int in = (int)(r / u.hs);
    const int Y0 = sh_first(ys - 1, u.sy, u.hs, u.hd), Y1 = sh_first(ys + 1, u.sy, u.hs, u.hd);
    const int X0 = sh_first(xs - 1, u.sx, u.ws, u.wd), X1 = sh_first(xs + 1, u.sx, u.ws, u.wd);
    const float* b = src + (int64_t)in * u.sn + (int64_t)ch * u.sc;
    float s = 0.0f;
    for (int Y = Y0; Y < Y1; ++Y) {
      const float wy = sh_weight(Y, u.sy, u.hs, ys);
      if (wy == 0.0f) continue;
      float rs = 0.0f;
      for (int X = X0; X < X1; ++X) {
        const float wx = sh_weight(X, u.sx, u.ws, xs);
        if (wx != 0.0f) rs += wx * b[(int64_t)Y * u.sh + (int64_t)X * u.sw];
      }
      s += wy * rs;
    }
    if (HS) s *= sh_dhsig(SEl<GT>::ld(gm + i));
    sh_st(dst + i, s);
  }
}

// ------------------------------------------------------------------------------------------------ logits
// out[pix][k] = up(p)[pix][k] + (sum_c W[k][c] c1[pix][c] + b[k]), fp32 [n][h1][w1][nclass]; thread = (pixel, class group), up to 8 classes in registers
struct ShLog { int n, h1, w1, h4, w4, c1, nclass; float sy, sx; };
template <typename ET>
__global__ __launch_bounds__(256) void k_sh_logits(const ShLog g, const float* __restrict__ p, const ET* __restrict__ c1, const float* __restrict__ W,
                                                    const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float sc[SH_PT][SH_CF_MAX + 1];
  __shared__ float sw[SH_CP][SH_CF_MAX + 1];
  __shared__ float so[SH_PT][SH_CP + 1];
  const int tid = threadIdx.x, cc = g.c1;
  const int64_t npix = (int64_t)g.n * g.h1 * g.w1, tiles = (npix + SH_PT - 1) / SH_PT;
  const bool single = g.nclass <= SH_CP;
  bool loaded = false;
  const int pl = tid & (SH_PT - 1), q = tid / SH_PT;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    for (int e = tid; e < SH_PT * cc; e += 256) {
      const int l = e / cc, c = e - l * cc;
      const int64_t px = tile * SH_PT + l;
      sc[l][c] = px < npix ? SEl<ET>::ld(c1 + px * cc + c) : 0.0f;
    }
    const int64_t pix = tile * SH_PT + pl;
    int in = 0, y0 = 0, x0 = 0, y1 = 0, x1 = 0; float fy = 0.0f, fx = 0.0f;
    if (pix < npix) {
      const int x = (int)(pix % g.w1); const int64_t r = pix / g.w1;
      in = (int)(r / g.h1);
      seg_src((int)(r % g.h1), g.sy, g.h4, y0, fy);
      seg_src(x, g.sx, g.w4, x0, fx);
      y1 = y0 + 1 < g.h4 ? y0 + 1 : g.h4 - 1; x1 = x0 + 1 < g.w4 ? x0 + 1 : g.w4 - 1;
    }
    for (int k0 = 0; k0 < g.nclass; k0 += SH_CP) {
      const int kc = min(SH_CP, g.nclass - k0);
      if (!(single && loaded)) {
        __syncthreads();
        for (int e = tid; e < SH_CP * cc; e += 256) { const int kl = e / cc, c = e - kl * cc; sw[kl][c] = kl < kc ? W[(int64_t)(k0 + kl) * cc + c] : 0.0f; }
        loaded = true;
      }
      __syncthreads();
      float acc[SH_CP / 4];
#pragma unroll
      for (int j = 0; j < SH_CP / 4; ++j) acc[j] = 0.0f;
      for (int c = 0; c < cc; ++c) {
        const float v = sc[pl][c];
#pragma unroll
        for (int j = 0; j < SH_CP / 4; ++j) acc[j] += sw[q + 4 * j][c] * v;
      }
      if (pix < npix) {
        const float* pb = p + (int64_t)in * g.h4 * g.w4 * g.nclass;
#pragma unroll
        for (int j = 0; j < SH_CP / 4; ++j) {
          const int kl = q + 4 * j;
          if (kl < kc) {
            const int k = k0 + kl;
            const float a00 = pb[((int64_t)y0 * g.w4 + x0) * g.nclass + k], a01 = pb[((int64_t)y0 * g.w4 + x1) * g.nclass + k];
            const float a10 = pb[((int64_t)y1 * g.w4 + x0) * g.nclass + k], a11 = pb[((int64_t)y1 * g.w4 + x1) * g.nclass + k];
            const float top = (1.0f - fx) * a00 + fx * a01, bot = (1.0f - fx) * a10 + fx * a11;
            so[pl][kl] = ((1.0f - fy) * top + fy * bot) + (acc[j] + bias[k]);
          }
        }
      }
      __syncthreads();
      for (int e = tid; e < SH_PT * kc; e += 256) {
        const int l = e / kc, kl = e - l * kc;
        const int64_t px = tile * SH_PT + l;
        if (px < npix) out[px * g.nclass + k0 + kl] = so[l][kl];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ entries
static inline unsigned sh_grid(int64_t work, int per, int cap) {
  int64_t gsz = (work + per - 1) / per;
  if (gsz < 1) gsz = 1;
  return (unsigned)(gsz > cap ? cap : gsz);
}
static int sh_pool_check(int n, int h, int w, int c, int kh, int kw, int sh, int sw) {
  FROST_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0, "seghead_pool: sizes must be positive");
  FROST_REQUIRE(kh <= h && kw <= w, "seghead_pool: the window is larger than the map");
  return 0;
}
template <typename ET>
static int sh_pool(const ET* x, int n, int h, int w, int c, int kh, int kw, int sh, int sw, ET* y, void* stream) {
  if (sh_pool_check(n, h, w, c, kh, kw, sh, sw)) return 1;
  const int ph = (h - kh) / sh + 1, pw = (w - kw) / sw + 1;
  hipLaunchKernelGGL(k_sh_pool<ET>, dim3(sh_grid((int64_t)n * ph * pw * c, 256, 4096)), dim3(256), 0, as_stream(stream), x, n, h, w, c, kh, kw, sh, sw, ph, pw, y);
  return frost_check_launch("seghead_pool");
}
template <typename ET>
static int sh_pool_bwd(const ET* dy, const ET* addend, int n, int h, int w, int c, int kh, int kw, int sh, int sw, ET* dx, void* stream) {
  if (sh_pool_check(n, h, w, c, kh, kw, sh, sw)) return 1;
  const int ph = (h - kh) / sh + 1, pw = (w - kw) / sw + 1;
  hipLaunchKernelGGL(k_sh_pool_bwd<ET>, dim3(sh_grid((int64_t)n * h * w * c, 256, 8192)), dim3(256), 0, as_stream(stream), dy, addend, n, h, w, c, kh, kw, sh, sw, ph,
                     pw, dx);
  return frost_check_launch("seghead_pool_bwd");
}
static int sh_gate_geom(ShGate& g, int n, int h4, int w4, int ph, int pw, int cf, int nclass) {
  FROST_REQUIRE(n > 0 && h4 > 0 && w4 > 0 && ph > 0 && pw > 0, "seghead_gate_project: sizes must be positive");
  FROST_REQUIRE(cf >= 1 && cf <= SH_CF_MAX, "seghead_gate_project: 1 <= feature channels <= 128");
  FROST_REQUIRE(nclass >= 1 && nclass <= 255, "seghead_gate_project: 1 <= classes <= 255");
  g.n = n; g.h4 = h4; g.w4 = w4; g.ph = ph; g.pw = pw; g.cf = cf; g.nclass = nclass;
  g.sy = sh_scale(ph, h4); g.sx = sh_scale(pw, w4);
  return 0;
}
template <typename ET>
static int sh_gate_project(const ET* feat1, const ET* gm, const float* W, const float* b, int n, int h4, int w4, int ph, int pw, int cf, int nclass, float* p,
                           void* stream) {
  ShGate g;
  if (sh_gate_geom(g, n, h4, w4, ph, pw, cf, nclass)) return 1;
  hipLaunchKernelGGL(k_sh_gate_project<ET>, dim3(sh_grid((int64_t)n * h4 * w4, SH_PT_GATE, 2048)), dim3(256), 0, as_stream(stream), g, feat1, gm, W, b, p);
  return frost_check_launch("seghead_gate_project");
}
template <typename ET>
static int sh_gate_project_bwd(const ET* feat1, const ET* gm, const float* dp, const float* W, int n, int h4, int w4, int ph, int pw, int cf, int nclass, float* dW,
                               float* db, ET* dfeat1, ET* dg, float* scratch, void* stream) {
  ShGate g;
  if (sh_gate_geom(g, n, h4, w4, ph, pw, cf, nclass)) return 1;
  ShLin q; q.n = n; q.h = h4; q.w = w4; q.cf = cf; q.nclass = nclass;
  q.dn = (int64_t)h4 * w4 * nclass; q.dc = 1; q.dh = (int64_t)w4 * nclass; q.dw = nclass;
  hipLaunchKernelGGL((k_sh_lin_bwd<ET, true, SH_PT_GATE>), dim3(sh_grid((int64_t)n * h4 * w4, SH_PT_GATE, 128)), dim3(256), 0, as_stream(stream), q, g, feat1, gm, dp,
                     W, dW, db, dfeat1, scratch);
  if (frost_check_launch("seghead_gate_project_bwd")) return 1;
  ShUp u; u.n = n; u.hs = ph; u.ws = pw; u.hd = h4; u.wd = w4; u.c = cf;
  u.sn = (int64_t)h4 * w4 * cf; u.sc = 1; u.sh = (int64_t)w4 * cf; u.sw = cf; u.sy = g.sy; u.sx = g.sx;
  hipLaunchKernelGGL((k_sh_up_adjoint<ET, ET, true>), dim3(sh_grid((int64_t)n * ph * pw * cf, 256, 4096)), dim3(256), 0, as_stream(stream), u, (const float*)scratch,
                     gm, dg);
  return frost_check_launch("seghead_gate_project_bwd (dg)");
}
static int sh_log_geom(ShLog& g, int n, int h1, int w1, int h4, int w4, int c1, int nclass) {
  FROST_REQUIRE(n > 0 && h1 > 0 && w1 > 0 && h4 > 0 && w4 > 0, "seghead_logits: sizes must be positive");
  FROST_REQUIRE(c1 >= 1 && c1 <= SH_CF_MAX, "seghead_logits: 1 <= c1 channels <= 128");
  FROST_REQUIRE(nclass >= 1 && nclass <= 255, "seghead_logits: 1 <= classes <= 255");
  g.n = n; g.h1 = h1; g.w1 = w1; g.h4 = h4; g.w4 = w4; g.c1 = c1; g.nclass = nclass;
  g.sy = sh_scale(h4, h1); g.sx = sh_scale(w4, w1);
  return 0;
}
template <typename ET>
static int sh_logits(const float* p, const ET* c1, const float* W, const float* b, int n, int h1, int w1, int h4, int w4, int cc, int nclass, float* out, void* stream) {
  ShLog g;
  if (sh_log_geom(g, n, h1, w1, h4, w4, cc, nclass)) return 1;
  hipLaunchKernelGGL(k_sh_logits<ET>, dim3(sh_grid((int64_t)n * h1 * w1, SH_PT, 4096)), dim3(256), 0, as_stream(stream), g, p, c1, W, b, out);
  return frost_check_launch("seghead_logits");
}
template <typename ET>
static int sh_logits_bwd(const float* dout, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const ET* c1, const float* W, int n, int h1, int w1, int h4, int w4, int cc,
                         int nclass, ET* dc1, float* dW, float* db, float* dp, void* stream) {
  ShLog g;
  if (sh_log_geom(g, n, h1, w1, h4, w4, cc, nclass)) return 1;
  ShLin q; q.n = n; q.h = h1; q.w = w1; q.cf = cc; q.nclass = nclass; q.dn = sn; q.dc = sc; q.dh = sh; q.dw = sw;
  ShGate none = {};
  hipLaunchKernelGGL((k_sh_lin_bwd<ET, false, SH_PT>), dim3(sh_grid((int64_t)n * h1 * w1, SH_PT, 512)), dim3(256), 0, as_stream(stream), q, none, c1, (const ET*)nullptr,
                     dout, W, dW, db, dc1, (float*)nullptr);
  if (frost_check_launch("seghead_logits_bwd")) return 1;
  ShUp u; u.n = n; u.hs = h4; u.ws = w4; u.hd = h1; u.wd = w1; u.c = nclass; u.sn = sn; u.sc = sc; u.sh = sh; u.sw = sw; u.sy = g.sy; u.sx = g.sx;
  hipLaunchKernelGGL((k_sh_up_adjoint<float, float, false>), dim3(sh_grid((int64_t)n * h4 * w4 * nclass, 256, 8192)), dim3(256), 0, as_stream(stream), u, dout,
                     (const float*)nullptr, dp);
  return frost_check_launch("seghead_logits_bwd (dp)");
}

extern "C" int frost_seghead_pool(const uint16_t* x, int n, int h, int w, int c, int kh, int kw, int sh, int sw, uint16_t* y, void* stream) {
  return sh_pool<uint16_t>(x, n, h, w, c, kh, kw, sh, sw, y, stream);
}
extern "C" int frost_seghead_pool_f32(const float* x, int n, int h, int w, int c, int kh, int kw, int sh, int sw, float* y, void* stream) {
  return sh_pool<float>(x, n, h, w, c, kh, kw, sh, sw, y, stream);
}
extern "C" int frost_seghead_pool_bwd(const uint16_t* dy, const uint16_t* addend, int n, int h, int w, int c, int kh, int kw, int sh, int sw, uint16_t* dx, void* stream) {
  return sh_pool_bwd<uint16_t>(dy, addend, n, h, w, c, kh, kw, sh, sw, dx, stream);
}
extern "C" int frost_seghead_pool_bwd_f32(const float* dy, const float* addend, int n, int h, int w, int c, int kh, int kw, int sh, int sw, float* dx, void* stream) {
  return sh_pool_bwd<float>(dy, addend, n, h, w, c, kh, kw, sh, sw, dx, stream);
}
extern "C" int frost_seghead_gate_project(const uint16_t* feat1, const uint16_t* g, const float* w_proj, const float* b_proj, int n, int h4, int w4, int ph, int pw,
                                          int cf, int nclass, float* p, void* stream) {
  return sh_gate_project<uint16_t>(feat1, g, w_proj, b_proj, n, h4, w4, ph, pw, cf, nclass, p, stream);
}
extern "C" int frost_seghead_gate_project_f32(const float* feat1, const float* g, const float* w_proj, const float* b_proj, int n, int h4, int w4, int ph, int pw, int cf,
                                              int nclass, float* p, void* stream) {
  return sh_gate_project<float>(feat1, g, w_proj, b_proj, n, h4, w4, ph, pw, cf, nclass, p, stream);
}
extern "C" int frost_seghead_gate_project_bwd(const uint16_t* feat1, const uint16_t* g, const float* dp, const float* w_proj, int n, int h4, int w4, int ph, int pw,
                                              int cf, int nclass, float* dw_proj, float* db_proj, uint16_t* dfeat1, uint16_t* dg, float* scratch, void* stream) {
  return sh_gate_project_bwd<uint16_t>(feat1, g, dp, w_proj, n, h4, w4, ph, pw, cf, nclass, dw_proj, db_proj, dfeat1, dg, scratch, stream);
}
extern "C" int frost_seghead_gate_project_bwd_f32(const float* feat1, const float* g, const float* dp, const float* w_proj, int n, int h4, int w4, int ph, int pw, int cf,
                                                  int nclass, float* dw_proj, float* db_proj, float* dfeat1, float* dg, float* scratch, void* stream) {
  return sh_gate_project_bwd<float>(feat1, g, dp, w_proj, n, h4, w4, ph, pw, cf, nclass, dw_proj, db_proj, dfeat1, dg, scratch, stream);
}
extern "C" int frost_seghead_logits(const float* p, const uint16_t* c1, const float* w_aux, const float* b_aux, int n, int h1, int w1, int h4, int w4, int c1ch,
                                    int nclass, float* out, void* stream) {
  return sh_logits<uint16_t>(p, c1, w_aux, b_aux, n, h1, w1, h4, w4, c1ch, nclass, out, stream);
}
extern "C" int frost_seghead_logits_f32(const float* p, const float* c1, const float* w_aux, const float* b_aux, int n, int h1, int w1, int h4, int w4, int c1ch, int nclass,
                                        float* out, void* stream) {
  return sh_logits<float>(p, c1, w_aux, b_aux, n, h1, w1, h4, w4, c1ch, nclass, out, stream);
}
extern "C" int frost_seghead_logits_bwd(const float* dout, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const uint16_t* c1, const float* w_aux, int n, int h1, int w1,
                                        int h4, int w4, int c1ch, int nclass, uint16_t* dc1, float* dw_aux, float* db_aux, float* dp, void* stream) {
  return sh_logits_bwd<uint16_t>(dout, sn, sc, sh, sw, c1, w_aux, n, h1, w1, h4, w4, c1ch, nclass, dc1, dw_aux, db_aux, dp, stream);
}
extern "C" int frost_seghead_logits_bwd_f32(const float* dout, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const float* c1, const float* w_aux, int n, int h1, int w1,
                                            int h4, int w4, int c1ch, int nclass, float* dc1, float* dw_aux, float* db_aux, float* dp, void* stream) {
  return sh_logits_bwd<float>(dout, sn, sc, sh, sw, c1, w_aux, n, h1, w1, h4, w4, c1ch, nclass, dc1, dw_aux, db_aux, dp, stream);
}

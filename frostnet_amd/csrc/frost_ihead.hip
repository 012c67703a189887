// Fused SSDLite prediction heads of the bf16 INFERENCE path: both SepHeads of one source map (ssdlite.py SepHead: depthwise 3x3 + BN + ReLU -> 1x1 + BN, linear)
// as ONE launch that writes fp32 `loc` / `conf` straight in SSDLiteFrostNet._assemble's order.
//   per head: dw = bf16(relu(taps(x) + b_dw))  (fp32 FMA, bias first, taps in (ky, kx) order: k_inf_dw's order and rounding point)
//             out = sum_k dw[k] * W'[co][k] + b'[co]  (bf16 MFMA 16x16x32, K blocks in ascending order into ONE fp32 accumulator: frost_infer_pw's order)
// so bf16(out) equals frost_infer_dw + frost_infer_pw bit for bit, as the fused bottleneck kernels (frost_iblock.hip / frost_iblockw.hip) do against their layers.
//
// Work decomposition: a workgroup (4 waves) owns IH_TP = 32 consecutive pixels of the flattened [n][h][w] map (tiles cross image borders: the 2 x 2 and 1 x 1
// maps of a batch fill a tile instead of one workgroup per image) and walks the input channels in chunks of IH_KC = 64:
//   phase 1  thread (pixel, 8 channels): the nine 16-byte input taps are loaded ONCE and feed the depthwise convs of BOTH heads -> y2[head][pixel][chunk] in LDS
//   phase 2  wave (pixel tile of 16, every second channel tile of the concatenated [loc | conf] tile list): the chunk's two K blocks into its accumulators,
//            which stay in registers over the chunks (any Cin: K is chunked into the same accumulator)
// epilogue: + bias, fp32 stores at (off + pix * width + j) of the image's row for j < width -- the padded class channels (84 -> 88 -> 96) are computed and dropped.
// No bf16 head map, no gather pass, no atomics.  LDS: 18 KB per workgroup (y2 double-buffered: one barrier per chunk).
#include "frost_common.h"

typedef __bf16 v8bf_h __attribute__((ext_vector_type(8)));

#define IH_TP 32                 // pixels per workgroup (two MFMA pixel tiles)
#define IH_KC 64                 // input channels per chunk (two MFMA K blocks)
#define IH_YS (IH_KC + 8)        // y2 row stride in bf16 elements: 144 bytes (16-byte aligned rows, the 16 pixel rows of a tile spread over the banks)
#define IH_CTW 5                 // channel tiles (of 16) per wave
#define IH_CTMAX (2 * IH_CTW)    // ... per source: loc + conf

struct IHeadP {
  const uint16_t* x;
  const float* wdw0; const float* bdw0; const uint16_t* wpw0; const float* bpw0;      // head 0 = loc
  const float* wdw1; const float* bdw1; const uint16_t* wpw1; const float* bpw1;      // head 1 = conf
  float* out0; float* out1;
  long long stride0, stride1, off0, off1;        // floats per image row of loc / conf, offset of this source in the row
  long long npix;
  int width0, width1, vec0, vec1;                // stored channels per pixel; vec: every 4-channel group of a pixel is a 16-byte aligned store
  int ct0, ct1, h, w, cin, cpad_dw, kb, nchunk;
};

__device__ __forceinline__ void ih_unpack(const uint4 v, float (&f)[8]) {
  f[0] = bf2f(v.x & 0xffff); f[1] = bf2f(v.x >> 16); f[2] = bf2f(v.y & 0xffff); f[3] = bf2f(v.y >> 16);
  f[4] = bf2f(v.z & 0xffff); f[5] = bf2f(v.z >> 16); f[6] = bf2f(v.w & 0xffff); f[7] = bf2f(v.w >> 16);
}
__device__ __forceinline__ void ih_load8(const float* q, float (&f)[8]) {
  const float4 a = *(const float4*)q, b = *(const float4*)(q + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ uint4 ih_relu_pack(const float (&a)[8]) {
  uint4 o;
  o.x = cvt_pk_bf16(fmaxf(a[0], 0.f), fmaxf(a[1], 0.f)); o.y = cvt_pk_bf16(fmaxf(a[2], 0.f), fmaxf(a[3], 0.f));
  o.z = cvt_pk_bf16(fmaxf(a[4], 0.f), fmaxf(a[5], 0.f)); o.w = cvt_pk_bf16(fmaxf(a[6], 0.f), fmaxf(a[7], 0.f));
  return o;
}

__global__ __launch_bounds__(256) void k_ihead(const IHeadP p) {
  __shared__ __attribute__((aligned(16))) uint16_t y2[2][2][IH_TP * IH_YS];          // [chunk parity][head][pixel][channel of the chunk]
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const long long p0 = (long long)blockIdx.x * IH_TP;
  const int hw = p.h * p.w;
  // ---- depthwise role: pixel dp of the tile, channels [8 dc, 8 dc + 8) of the chunk
  const int dp = tid >> 3, dc = tid & 7;
  const long long gp = p0 + dp;
  const bool pok = gp < p.npix;
  int oy = 0, ox = 0; long long img = 0;
  if (pok) { img = gp / hw; const int rem = (int)(gp - img * hw); oy = rem / p.w; ox = rem - oy * p.w; }
  const uint16_t* ximg = p.x + img * hw * p.cin;
  // ---- GEMM role: pixel tile pt, channel tiles cw, cw + 2, ... of the list [loc tiles | conf tiles]
  const int pt = wv & 1, cw = wv >> 1;
  const int nct = p.ct0 + p.ct1;
  v4f acc[IH_CTW];
#pragma unroll
  for (int i = 0; i < IH_CTW; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < p.nchunk; ++c) {
    // ---- this chunk's A fragments (both K blocks of this wave's channel tiles), requested first: they travel with the depthwise operands
    uint4 af[IH_KC / 32][IH_CTW];
#pragma unroll
    for (int k2 = 0; k2 < IH_KC / 32; ++k2) {
      const int kb = c * (IH_KC / 32) + k2;
#pragma unroll
      for (int i = 0; i < IH_CTW; ++i) {
        const int t = cw + 2 * i;
        af[k2][i] = make_uint4(0, 0, 0, 0);
        if (t < nct && kb < p.kb) {
          const bool hd = t >= p.ct0;
          af[k2][i] = *(const uint4*)((hd ? p.wpw1 : p.wpw0) + (((size_t)(hd ? t - p.ct0 : t) * p.kb + kb) * 64 + lane) * 8);
        }
      }
    }
    const int ch = c * IH_KC + dc * 8;
    uint4 o0 = make_uint4(0, 0, 0, 0), o1 = make_uint4(0, 0, 0, 0);            // channels past Cin / pixels past the map: zeros (K padding of the GEMM)
    if (pok && ch < p.cin) {
      float a0[8], a1[8];
      ih_load8(p.bdw0 + ch, a0); ih_load8(p.bdw1 + ch, a1);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
        if (iy < 0 || iy >= p.h) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox - 1 + kx;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (ix >= 0 && ix < p.w) v = *(const uint4*)(ximg + ((long long)iy * p.w + ix) * p.cin + ch);
          float col[8], w0[8], w1[8];
          ih_unpack(v, col);
          ih_load8(p.wdw0 + (ky * 3 + kx) * p.cpad_dw + ch, w0);
          ih_load8(p.wdw1 + (ky * 3 + kx) * p.cpad_dw + ch, w1);
#pragma unroll
          for (int e = 0; e < 8; ++e) { a0[e] = fmaf(col[e], w0[e], a0[e]); a1[e] = fmaf(col[e], w1[e], a1[e]); }
        }
      }
      o0 = ih_relu_pack(a0); o1 = ih_relu_pack(a1);
    }
    // y2 is double-buffered over the chunks: ONE barrier per chunk (buffer c & 1 is rewritten by chunk c + 2, behind the barrier of chunk c + 1, which a wave
    // reaches only after its reads of chunk c)
    uint16_t* const yb0 = &y2[c & 1][0][0];
    uint16_t* const yb1 = &y2[c & 1][1][0];
    *(uint4*)(yb0 + dp * IH_YS + dc * 8) = o0;
    *(uint4*)(yb1 + dp * IH_YS + dc * 8) = o1;
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < IH_KC / 32; ++k2) {
      if (c * (IH_KC / 32) + k2 >= p.kb) break;
      const uint4 b0 = *(const uint4*)(yb0 + (pt * 16 + j) * IH_YS + k2 * 32 + g * 8);
      const uint4 b1 = *(const uint4*)(yb1 + (pt * 16 + j) * IH_YS + k2 * 32 + g * 8);
#pragma unroll
      for (int i = 0; i < IH_CTW; ++i) {
        const int t = cw + 2 * i;
        if (t >= nct) continue;
        const uint4 b = (t >= p.ct0) ? b1 : b0;
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf_h, af[k2][i]), __builtin_bit_cast(v8bf_h, b), acc[i], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: lane (j, g) holds pixel pt * 16 + j, channels ctl * 16 + 4 g .. + 3
  const long long ep = p0 + pt * 16 + j;
  if (ep >= p.npix) return;
  const long long eimg = ep / hw; const long long epix = ep - eimg * hw;
#pragma unroll
  for (int i = 0; i < IH_CTW; ++i) {
    const int t = cw + 2 * i;
    if (t >= nct) continue;
    const bool hd = t >= p.ct0;
    const int ctl = hd ? t - p.ct0 : t;
    const int ch = ctl * 16 + 4 * g;
    const int width = hd ? p.width1 : p.width0;
    if (ch >= width) continue;
    const float4 bb = *(const float4*)((hd ? p.bpw1 : p.bpw0) + ch);
    float* dst = (hd ? p.out1 : p.out0) + eimg * (hd ? p.stride1 : p.stride0) + (hd ? p.off1 : p.off0) + epix * width + ch;
    const float4 v = make_float4(acc[i][0] + bb.x, acc[i][1] + bb.y, acc[i][2] + bb.z, acc[i][3] + bb.w);
    if ((hd ? p.vec1 : p.vec0) && ch + 4 <= width) *(float4*)dst = v;
    else {
      dst[0] = v.x;
      if (ch + 1 < width) dst[1] = v.y;
      if (ch + 2 < width) dst[2] = v.z;
      if (ch + 3 < width) dst[3] = v.w;
    }
  }
}

// 1 if frost_infer_head takes a source map [h][w][cin] with cout_loc / cout_conf stored channels per pixel: Cin a multiple of 8 (any width: K is chunked),
// at most IH_CTMAX 16-channel tiles over the two heads.  Every source of SSDLite-FrostNet (4 or 6 anchors, 21 classes: 1 + 6 / 2 + 8 tiles) is taken.
extern "C" int frost_infer_head_ok(int h, int w, int cin, int cout_loc, int cout_conf) {
  if (h <= 0 || w <= 0 || cin < 8 || (cin & 7) || cout_loc <= 0 || cout_conf <= 0) return 0;
  return (round_up(cout_loc, 16) / 16 + round_up(cout_conf, 16) / 16 <= IH_CTMAX) ? 1 : 0;
}

/* Both SepHeads of one SSD source map, bf16 inference, one launch.  x: NHWC bf16 [n][h][w][cin].  wdw_* / bdw_*: fp32 taps [9][round_up(cin,16)] and folded bias of
 * the head's depthwise layer, wpw_* / bpw_*: bf16 A-fragment pack (kpad = round_up(cin,32)) and folded bias of its 1x1 layer (frost_infer_weight_prep).
 * Stores loc[img * loc_stride + loc_off + pix * cout_loc + j] (j < cout_loc) and conf[img * conf_stride + conf_off + pix * cout_conf + j] (j < cout_conf), fp32;
 * cout_conf counts the USED class channels (anchors * classes): the 1x1 layer's padding channels are not stored.  Nothing else of loc / conf is written. */
extern "C" int frost_infer_head(const uint16_t* x, const float* wdw_loc, const float* bdw_loc, const uint16_t* wpw_loc, const float* bpw_loc,
                                const float* wdw_conf, const float* bdw_conf, const uint16_t* wpw_conf, const float* bpw_conf, int n, int h, int w, int cin,
                                int cout_loc, int cout_conf, float* loc, int64_t loc_stride, int64_t loc_off, float* conf, int64_t conf_stride,
                                int64_t conf_off, void* stream) {
  FROST_REQUIRE(frost_infer_head_ok(h, w, cin, cout_loc, cout_conf), "infer_head: unsupported geometry");
  FROST_REQUIRE(x && wdw_loc && bdw_loc && wpw_loc && bpw_loc && wdw_conf && bdw_conf && wpw_conf && bpw_conf && loc && conf && n > 0, "infer_head: incomplete arguments");
  FROST_REQUIRE(loc_off >= 0 && conf_off >= 0 && loc_off + (int64_t)h * w * cout_loc <= loc_stride && conf_off + (int64_t)h * w * cout_conf <= conf_stride,
                "infer_head: the source does not fit its image row");
  IHeadP p = {};
  p.x = x; p.wdw0 = wdw_loc; p.bdw0 = bdw_loc; p.wpw0 = wpw_loc; p.bpw0 = bpw_loc; p.wdw1 = wdw_conf; p.bdw1 = bdw_conf; p.wpw1 = wpw_conf; p.bpw1 = bpw_conf;
  p.out0 = loc; p.out1 = conf; p.stride0 = loc_stride; p.stride1 = conf_stride; p.off0 = loc_off; p.off1 = conf_off;
  p.npix = (long long)n * h * w;
  p.width0 = cout_loc; p.width1 = cout_conf;
  p.vec0 = ((cout_loc & 3) == 0 && (loc_stride & 3) == 0 && (loc_off & 3) == 0 && ((uintptr_t)loc & 15) == 0) ? 1 : 0;
  p.vec1 = ((cout_conf & 3) == 0 && (conf_stride & 3) == 0 && (conf_off & 3) == 0 && ((uintptr_t)conf & 15) == 0) ? 1 : 0;
  p.ct0 = round_up(cout_loc, 16) / 16; p.ct1 = round_up(cout_conf, 16) / 16;
  p.h = h; p.w = w; p.cin = cin; p.cpad_dw = round_up(cin, 16); p.kb = round_up(cin, 32) / 32; p.nchunk = (cin + IH_KC - 1) / IH_KC;
  const long long grid = (p.npix + IH_TP - 1) / IH_TP;
  hipLaunchKernelGGL(k_ihead, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), p);
  return frost_check_launch("infer_head");
}

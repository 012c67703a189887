// Fused SSDLite prediction heads of the CONVERTED int8 detector: both SepHeads of one source map (ssdlite.py SepHead: quantized depthwise 3x3 + ReLU -> quantized
// 1x1, linear -> DeQuantStub) as ONE launch that writes fp32 `loc` / `conf` straight in SSDLiteFrostNet._assemble's order.
//   per head: d   = sum_taps w_dw * (q_x - zp_x)                      (int32; taps outside the map carry the input's zero point = real 0: frost_dw3.hip's zero-point fill)
//             q_d = requant_relu(d)  at the depthwise layer's record  (the emit expressions of frost_dw3.hip, cvt 1 / 2, term for term, `lowq` cap included)
//             a   = sum_k w_pw[co][k] * (q_d[k] - zp_d)               (int8 MFMA 16x16x64, int32 accumulators over the K chunks: integer sums are order-free)
//             q_o = requant(a)       at the head's record             (the linear emit expressions of frost_pw.hip, cvt 1 / 2)
//             out = (float)(q_o - zp_o) * s_o                         (k_dequant_act's expression)
// so `out` equals conv_converted x 2 + frost_dequant_act + _assemble's slice bit for bit.  The packs are the layers' own (depthwise [tap][cpad] int8 + wsum, pointwise
// A-fragment pack [ct][ks][lane][16 B] + wsum, coefficient rows A / B of frost_conv_finalize_converted(_fb)): nothing is repacked.  The pointwise pack holds zeros for
// k >= Cin and co >= Cout, so padded K lanes contribute nothing whatever the LDS bytes are (they are written as 0 anyway).
//
// Work decomposition (frost_ihead.hip's): a workgroup (4 waves) owns QH_TP = 32 consecutive pixels of the flattened [n][h][w] map (tiles cross image borders) and walks
// the input channels in chunks of QH_KC = 64 = one MFMA K block:
//   phase 1  thread (pixel, 8 channels): the nine 8-byte input taps are loaded ONCE and feed the depthwise convs of BOTH heads -> offset-binary indices in LDS only
//   phase 2  wave (pixel tile of 16, every second channel tile of the concatenated [loc | conf] tile list): one MFMA per tile and chunk, accumulators in registers
// epilogue: requantise, dequantise, fp32 stores at (off + pix * width + j) of the image's row for j < width -- the padded class channels (84 -> 88, 126 -> 128) are
// computed and dropped.  No int8 head map, no gather pass, no atomics.  LDS: 10 KB per workgroup (double-buffered over the chunks: one barrier per chunk).
//
// frost_cvt_place is the placement pass of the layer-launch form (geometries the fused kernel refuses, and the A/B switch): one int8 NHWC head map is dequantised
// and its used channels stored into the same row region -- no NCHW round trip, no cat.
#include "frost_common.h"

#define QH_TP 32                 // pixels per workgroup (two MFMA pixel tiles)
#define QH_KC 64                 // input channels per chunk (one MFMA K block)
#define QH_YS (QH_KC + 16)       // LDS row stride in bytes: 16-byte aligned rows, the 16 pixel rows of a tile spread over the banks
#define QH_CTW 5                 // channel tiles (of 16) per wave
#define QH_CTMAX (2 * QH_CTW)    // ... per source: loc + conf

struct CvtHeadP {
  const int8_t* x; const float* qx;
  const int8_t* wdw0; const int32_t* sdw0; const float* cdw0; const float* qdw0; const int8_t* wpw0; const int32_t* spw0; const float* cpw0; const float* qpw0;      // head 0 = loc
  const int8_t* wdw1; const int32_t* sdw1; const float* cdw1; const float* qdw1; const int8_t* wpw1; const int32_t* spw1; const float* cpw1; const float* qpw1;      // head 1 = conf
  float* out0; float* out1;
  long long stride0, stride1, off0, off1;        // floats per image row of loc / conf, offset of this source in the row
  long long npix;
  int width0, width1, vec0, vec1;                // stored channels per pixel; vec: every 4-channel group of a pixel is a 16-byte aligned store
  int ct0, ct1, cpad0, cpad1;                    // channel tiles / padded channels (coefficient row stride) of the two 1x1 layers
  int h, w, cin, cpad_dw, ks, cvt;               // cvt: 1 = QNNPACK form (integer bias bits in row B), 2 = FBGEMM form (float bias, per-channel multipliers)
};

// requantisation of one depthwise output with ReLU: frost_dw3.hip's emit expressions (D_EMIT, cvt 1 / 2), returned as the uint8 index
__device__ __forceinline__ uint32_t qh_dw_emit(int acc, float cA, float cB, int cvt, float zpf, bool lowq, float qcap) {
  float qv;
  if (cvt == 2) qv = rintf(fmaxf(((float)acc + cB) * cA, 0.0f)) + zpf;
  else { const float yv = fmaf(cA, (float)(acc + __float_as_int(cB)), 0.0f); qv = rintf(fmaxf(yv, 0.0f) * 1.0f) + zpf; }
  if (lowq) qv = fminf(qv, qcap);
  return __builtin_amdgcn_cvt_pk_u8_f32(qv, 0, 0u) & 255u;
}
// linear requantisation of one pointwise output: frost_pw.hip's emit expressions (M_EMIT, cvt 1 / 2)
__device__ __forceinline__ int qh_pw_emit(int acc, float cA, float cB, int cvt, float zpf, bool lowq, float qcap) {
  float qv;
  if (cvt == 2) qv = rintf(((float)acc + cB) * cA) + zpf;
  else { const float yv = fmaf(cA, (float)(acc + __float_as_int(cB)), 0.0f); qv = rintf(yv * 1.0f) + zpf; }
  if (lowq) qv = fminf(qv, qcap);
  return (int)(__builtin_amdgcn_cvt_pk_u8_f32(qv, 0, 0u) & 255u);
}
__device__ __forceinline__ void qh_sx8(const uint2 v, int (&o)[8]) {            // 8 signed bytes -> ints
  o[0] = (int)(v.x << 24) >> 24; o[1] = (int)(v.x << 16) >> 24; o[2] = (int)(v.x << 8) >> 24; o[3] = (int)v.x >> 24;
  o[4] = (int)(v.y << 24) >> 24; o[5] = (int)(v.y << 16) >> 24; o[6] = (int)(v.y << 8) >> 24; o[7] = (int)v.y >> 24;
}
__device__ __forceinline__ void qh_ld8i(const int32_t* q, int (&o)[8]) {
  const int4 a = *(const int4*)q, b = *(const int4*)(q + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void qh_ld8f(const float* q, float (&o)[8]) {
  const float4 a = *(const float4*)q, b = *(const float4*)(q + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

__global__ __launch_bounds__(256) void k_cvt_head(const CvtHeadP p) {
  __shared__ __attribute__((aligned(16))) uint8_t y2[2][2][QH_TP * QH_YS];          // [chunk parity][head][pixel][channel of the chunk], offset-binary indices
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const long long p0 = (long long)blockIdx.x * QH_TP;
  const int hw = p.h * p.w;
  // ---- depthwise role: pixel dp of the tile, channels [8 dc, 8 dc + 8) of the chunk
  const int dp = tid >> 3, dc = tid & 7;
  const long long gp = p0 + dp;
  const bool pok = gp < p.npix;
  int oy = 0, ox = 0; long long img = 0;
  if (pok) { img = gp / hw; const int rem = (int)(gp - img * hw); oy = rem / p.w; ox = rem - oy * p.w; }
  const int8_t* ximg = p.x + img * hw * p.cin;
  const int zpx = __float_as_int(p.qx[FROST_Q_ZP]);
  const uint32_t zfill = (uint32_t)((zpx - 128) & 255) * 0x01010101u;         // a tap outside the map: the input's zero point (real value 0)
  const float dzp0 = (float)__float_as_int(p.qdw0[FROST_Q_ZP]), dzp1 = (float)__float_as_int(p.qdw1[FROST_Q_ZP]);
  const float dcap0 = (float)q_hi(p.qdw0), dcap1 = (float)q_hi(p.qdw1);
  const bool dlow0 = dcap0 < 255.0f, dlow1 = dcap1 < 255.0f;                  // 7-bit records (reduce_range): the u8 conversion saturates at 255 only
  // ---- GEMM role: pixel tile pt, channel tiles cw, cw + 2, ... of the list [loc tiles | conf tiles]
  const int pt = wv & 1, cw = wv >> 1;
  const int nct = p.ct0 + p.ct1;
  v4i acc[QH_CTW];
  {
    // acc starts at -(zp_d - 128) * sum_k(w): the LDS bytes are q_d - 128, so acc = sum w * (q_d - zp_d) exactly (frost_pw.hip's initialisation)
    const int zd0 = __float_as_int(p.qdw0[FROST_Q_ZP]) - 128, zd1 = __float_as_int(p.qdw1[FROST_Q_ZP]) - 128;
#pragma unroll
    for (int i = 0; i < QH_CTW; ++i) {
      const int t = cw + 2 * i;
      acc[i] = (v4i){0, 0, 0, 0};
      if (t < nct) {
        const bool hd = t >= p.ct0;
        const int4 ws = *(const int4*)((hd ? p.spw1 : p.spw0) + (hd ? t - p.ct0 : t) * 16 + 4 * g);
        const int z = hd ? zd1 : zd0;
        acc[i] = (v4i){-z * ws.x, -z * ws.y, -z * ws.z, -z * ws.w};
      }
    }
  }

  for (int c = 0; c < p.ks; ++c) {
    // ---- this chunk's A fragments (the K block of this wave's channel tiles), requested first: they travel with the depthwise operands
    v4i af[QH_CTW];
#pragma unroll
    for (int i = 0; i < QH_CTW; ++i) {
      const int t = cw + 2 * i;
      af[i] = (v4i){0, 0, 0, 0};
      if (t < nct) {
        const bool hd = t >= p.ct0;
        af[i] = *(const v4i*)((hd ? p.wpw1 : p.wpw0) + (((size_t)(hd ? t - p.ct0 : t) * p.ks + c) * 64 + lane) * 16);
      }
    }
    const int ch = c * QH_KC + dc * 8;
    uint2 o0 = make_uint2(0u, 0u), o1 = make_uint2(0u, 0u);            // channels past Cin / pixels past the map: zeros (the pack's K padding is zero)
    if (pok && ch < p.cin) {
      int a0[8], a1[8];
      qh_ld8i(p.sdw0 + ch, a0); qh_ld8i(p.sdw1 + ch, a1);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a0[e] *= (128 - zpx); a1[e] *= (128 - zpx); }      // acc = sum w * (q - zp): frost_dw3.hip's acc0
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox - 1 + kx;
          uint2 v = make_uint2(zfill, zfill);
          if (iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) v = *(const uint2*)(ximg + ((long long)iy * p.w + ix) * p.cin + ch);
          int col[8], w0[8], w1[8];
          qh_sx8(v, col);
          qh_sx8(*(const uint2*)(p.wdw0 + (ky * 3 + kx) * p.cpad_dw + ch), w0);
          qh_sx8(*(const uint2*)(p.wdw1 + (ky * 3 + kx) * p.cpad_dw + ch), w1);
#pragma unroll
          for (int e = 0; e < 8; ++e) { a0[e] += col[e] * w0[e]; a1[e] += col[e] * w1[e]; }
        }
      }
      float A0[8], B0[8], A1[8], B1[8];
      qh_ld8f(p.cdw0 + FROST_COEF_A * p.cpad_dw + ch, A0); qh_ld8f(p.cdw0 + FROST_COEF_B * p.cpad_dw + ch, B0);
      qh_ld8f(p.cdw1 + FROST_COEF_A * p.cpad_dw + ch, A1); qh_ld8f(p.cdw1 + FROST_COEF_B * p.cpad_dw + ch, B1);
      uint32_t b0[8], b1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        b0[e] = qh_dw_emit(a0[e], A0[e], B0[e], p.cvt, dzp0, dlow0, dcap0) ^ 0x80u;
        b1[e] = qh_dw_emit(a1[e], A1[e], B1[e], p.cvt, dzp1, dlow1, dcap1) ^ 0x80u;
      }
      o0 = make_uint2(b0[0] | (b0[1] << 8) | (b0[2] << 16) | (b0[3] << 24), b0[4] | (b0[5] << 8) | (b0[6] << 16) | (b0[7] << 24));
      o1 = make_uint2(b1[0] | (b1[1] << 8) | (b1[2] << 16) | (b1[3] << 24), b1[4] | (b1[5] << 8) | (b1[6] << 16) | (b1[7] << 24));
    }
    // y2 is double-buffered over the chunks: ONE barrier per chunk (buffer c & 1 is rewritten by chunk c + 2, behind the barrier of chunk c + 1, which a wave
    // reaches only after its reads of chunk c)
    uint8_t* const yb0 = &y2[c & 1][0][0];
    uint8_t* const yb1 = &y2[c & 1][1][0];
    *(uint2*)(yb0 + dp * QH_YS + dc * 8) = o0;
    *(uint2*)(yb1 + dp * QH_YS + dc * 8) = o1;
    __syncthreads();
    const v4i bq0 = *(const v4i*)(yb0 + (pt * 16 + j) * QH_YS + g * 16);
    const v4i bq1 = *(const v4i*)(yb1 + (pt * 16 + j) * QH_YS + g * 16);
#pragma unroll
    for (int i = 0; i < QH_CTW; ++i) {
      const int t = cw + 2 * i;
      if (t >= nct) continue;
      acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], (t >= p.ct0) ? bq1 : bq0, acc[i], 0, 0, 0);
    }
  }

  // ---- epilogue: lane (j, g) holds pixel pt * 16 + j, channels ctl * 16 + 4 g .. + 3
  const long long ep = p0 + pt * 16 + j;
  if (ep >= p.npix) return;
  const long long eimg = ep / hw; const long long epix = ep - eimg * hw;
#pragma unroll
  for (int i = 0; i < QH_CTW; ++i) {
    const int t = cw + 2 * i;
    if (t >= nct) continue;
    const bool hd = t >= p.ct0;
    const int ctl = hd ? t - p.ct0 : t;
    const int ch = ctl * 16 + 4 * g;
    const int width = hd ? p.width1 : p.width0;
    if (ch >= width) continue;
    const float* coef = hd ? p.cpw1 : p.cpw0; const int cpad = hd ? p.cpad1 : p.cpad0;
    const float* qy = hd ? p.qpw1 : p.qpw0;
    const float4 a4 = *(const float4*)(coef + FROST_COEF_A * cpad + ch), b4 = *(const float4*)(coef + FROST_COEF_B * cpad + ch);
    const float A[4] = {a4.x, a4.y, a4.z, a4.w}, B[4] = {b4.x, b4.y, b4.z, b4.w};
    const int zpy = __float_as_int(qy[FROST_Q_ZP]); const float zpf = (float)zpy, scale = qy[FROST_Q_SCALE];
    const float qcap = (float)q_hi(qy); const bool lowq = qcap < 255.0f;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (float)(qh_pw_emit(acc[i][r], A[r], B[r], p.cvt, zpf, lowq, qcap) - zpy) * scale;       // k_dequant_act: (float)(idx - zp) * scale
    float* dst = (hd ? p.out1 : p.out0) + eimg * (hd ? p.stride1 : p.stride0) + (hd ? p.off1 : p.off0) + epix * width + ch;
    if ((hd ? p.vec1 : p.vec0) && ch + 4 <= width) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else {
      dst[0] = v[0];
      if (ch + 1 < width) dst[1] = v[1];
      if (ch + 2 < width) dst[2] = v[2];
      if (ch + 3 < width) dst[3] = v[3];
    }
  }
}

// 1 if frost_cvt_head takes a source map [h][w][cin] whose 1x1 layers have cout_loc / cout_conf channels (the LAYERS' widths, class padding included): Cin a multiple
// of 8 (any width: K is chunked), at most QH_CTMAX 16-channel tiles over the two heads.  Every source of SSDLite-FrostNet (16 + 88 / 24 + 128 channels) is taken.
extern "C" int frost_cvt_head_ok(int h, int w, int cin, int cout_loc, int cout_conf) {
  if (h <= 0 || w <= 0 || cin < 8 || (cin & 7) || cout_loc <= 0 || cout_conf <= 0) return 0;
  return (round_up(cout_loc, 16) / 16 + round_up(cout_conf, 16) / 16 <= QH_CTMAX) ? 1 : 0;
}

extern "C" int frost_cvt_head(const int8_t* x, const float* qrec_x, const FrostCvtHead* loc_head, const FrostCvtHead* conf_head, int n, int h, int w, int cin,
                              int width_loc, int width_conf, int mode, float* loc, int64_t loc_stride, int64_t loc_off, float* conf, int64_t conf_stride,
                              int64_t conf_off, void* stream) {
  FROST_REQUIRE(loc_head && conf_head, "cvt_head: incomplete arguments");
  const FrostCvtHead& a = *loc_head; const FrostCvtHead& b = *conf_head;
  FROST_REQUIRE(frost_cvt_head_ok(h, w, cin, a.cout, b.cout), "cvt_head: unsupported geometry");
  FROST_REQUIRE(mode == 2 || mode == 3, "cvt_head: mode 2 / 3 (converted QNNPACK / FBGEMM form, as frost_pw_conv_fwd)");
  FROST_REQUIRE(x && qrec_x && loc && conf && n > 0 && a.dw_wq && a.dw_wsum && a.dw_coef && a.dw_qy && a.pw_wq && a.pw_wsum && a.pw_coef && a.pw_qy &&
                b.dw_wq && b.dw_wsum && b.dw_coef && b.dw_qy && b.pw_wq && b.pw_wsum && b.pw_coef && b.pw_qy, "cvt_head: incomplete arguments");
  FROST_REQUIRE(width_loc > 0 && width_loc <= a.cout && width_conf > 0 && width_conf <= b.cout, "cvt_head: stored widths exceed the layers' channels");
  FROST_REQUIRE(loc_off >= 0 && conf_off >= 0 && loc_off + (int64_t)h * w * width_loc <= loc_stride && conf_off + (int64_t)h * w * width_conf <= conf_stride,
                "cvt_head: the source does not fit its image row");
  FROST_REQUIRE((((uintptr_t)x | (uintptr_t)a.dw_wq | (uintptr_t)b.dw_wq) & 7) == 0 &&
                (((uintptr_t)a.dw_wsum | (uintptr_t)b.dw_wsum | (uintptr_t)a.dw_coef | (uintptr_t)b.dw_coef | (uintptr_t)a.pw_wq | (uintptr_t)b.pw_wq |
                  (uintptr_t)a.pw_wsum | (uintptr_t)b.pw_wsum | (uintptr_t)a.pw_coef | (uintptr_t)b.pw_coef) & 15) == 0, "cvt_head: misaligned operands");
  CvtHeadP p = {};
  p.x = x; p.qx = qrec_x;
  p.wdw0 = a.dw_wq; p.sdw0 = a.dw_wsum; p.cdw0 = a.dw_coef; p.qdw0 = a.dw_qy; p.wpw0 = a.pw_wq; p.spw0 = a.pw_wsum; p.cpw0 = a.pw_coef; p.qpw0 = a.pw_qy;
  p.wdw1 = b.dw_wq; p.sdw1 = b.dw_wsum; p.cdw1 = b.dw_coef; p.qdw1 = b.dw_qy; p.wpw1 = b.pw_wq; p.spw1 = b.pw_wsum; p.cpw1 = b.pw_coef; p.qpw1 = b.pw_qy;
  p.out0 = loc; p.out1 = conf; p.stride0 = loc_stride; p.stride1 = conf_stride; p.off0 = loc_off; p.off1 = conf_off;
  p.npix = (long long)n * h * w;
  p.width0 = width_loc; p.width1 = width_conf;
  p.vec0 = ((width_loc & 3) == 0 && (loc_stride & 3) == 0 && (loc_off & 3) == 0 && ((uintptr_t)loc & 15) == 0) ? 1 : 0;
  p.vec1 = ((width_conf & 3) == 0 && (conf_stride & 3) == 0 && (conf_off & 3) == 0 && ((uintptr_t)conf & 15) == 0) ? 1 : 0;
  p.cpad0 = round_up(a.cout, 16); p.cpad1 = round_up(b.cout, 16); p.ct0 = p.cpad0 / 16; p.ct1 = p.cpad1 / 16;
  p.h = h; p.w = w; p.cin = cin; p.cpad_dw = round_up(cin, 16); p.ks = round_up(cin, 64) / 64; p.cvt = mode - 1;
  const long long grid = (p.npix + QH_TP - 1) / QH_TP;
  FROST_REQUIRE(grid <= 0x7fffffffLL, "cvt_head: too many pixels for one launch");
  hipLaunchKernelGGL(k_cvt_head, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), p);
  return frost_check_launch("cvt_head");
}

// ------------------------------------------------------------------------------------------------ placement of one int8 head map
// y: [n][hw][cout] offset-binary indices under qrec; out[img * stride + off + pix * width + j] = (float)(idx - zp) * scale for j < width (k_dequant_act's expression).
// One thread per group of 4 stored channels of a pixel; VEC: the group is one aligned 16-byte store (width, stride, off multiples of 4).
template <bool VEC>
__global__ __launch_bounds__(256) void k_cvt_place(const int8_t* __restrict__ y, const float* qrec, long long npix, int hw, int cout, int width, float* __restrict__ out,
                                                   long long stride, long long off) {
  const QP q = load_qp(qrec);
  const int ng = (width + 3) >> 2;
  const long long total = npix * ng;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long pix = i / ng; const int ch = (int)(i - pix * ng) * 4;
    const long long img = pix / hw, ip = pix - img * hw;
    const int8_t* src = y + pix * cout + ch;
    float* dst = out + img * stride + off + ip * width + ch;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (ch + r < width) ? (float)((int)src[r] + 128 - q.zp) * q.scale : 0.0f;
    if (VEC) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (ch + r < width) dst[r] = v[r];
    }
  }
}

extern "C" int frost_cvt_place(const int8_t* y, const float* qrec_y, int n, int hw, int cout, int width, float* out, int64_t out_stride, int64_t out_off, void* stream) {
  FROST_REQUIRE(y && qrec_y && out && n > 0 && hw > 0 && cout > 0, "cvt_place: incomplete arguments");
  FROST_REQUIRE(width > 0 && width <= cout, "cvt_place: the stored width exceeds the map's channels");
  FROST_REQUIRE(out_off >= 0 && out_off + (int64_t)hw * width <= out_stride, "cvt_place: the map does not fit its image row");
  const long long npix = (long long)n * hw;
  const long long total = npix * ((width + 3) >> 2);
  const bool vec = (width & 3) == 0 && (out_stride & 3) == 0 && (out_off & 3) == 0 && ((uintptr_t)out & 15) == 0;
  const long long nblk = (total + 255) / 256;
  const unsigned grid = (unsigned)(nblk < 4096 ? nblk : 4096);          // grid-stride loop
  if (vec) hipLaunchKernelGGL(k_cvt_place<true>, dim3(grid), dim3(256), 0, as_stream(stream), y, qrec_y, npix, hw, cout, width, out, (long long)out_stride, (long long)out_off);
  else hipLaunchKernelGGL(k_cvt_place<false>, dim3(grid), dim3(256), 0, as_stream(stream), y, qrec_y, npix, hw, cout, width, out, (long long)out_stride, (long long)out_off);
  return frost_check_launch("cvt_place");
}

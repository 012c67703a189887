// SSD training-time augmentation of a whole batch on the device: uint8 BGR images in, the detector's fp32 input and the padded MultiBoxLoss targets out, without
// host synchronisation (the reference augments one image at a time on the host with numpy + OpenCV).
//
// replaces: Object_Detection/utils/augmentations.py:400-417 (SSDAugmentation: ConvertFromInts, ToAbsoluteCoords, PhotometricDistort, Expand, RandomSampleCrop,
// RandomMirror, ToPercentCoords, Resize, SubtractMeans) and data/__init__.py:30-43 (BaseTransform), as restated by frostnet_amd/augment.py on CPU tensors (the
// definition and the parity yardstick: tests/test_gpu_augment.py expects plan words and pixels equal bit for bit, every value op here is one correctly rounded fp32
// operation in the definition's order -- the library builds with -ffp-contract=off).
//   * k_aug_plan, one wave per image: every lane draws the image's decisions redundantly from the same Philox4x32-10 counters (key = seed, counter = (image ordinal,
//     draw block, stream tag); draw k = word k & 3 of block k >> 2), in the reference's order; the box centres sit in LDS, the lanes stride over them for the crop's
//     centre test with a wave-wide any.  Loops are bounded at compile time: 64 mode rounds x 50 trials.  Writes the plan record, boxes_out, valid_out.
//   * k_aug_advance, one thread behind it on the stream: images seen += n (every wave of the plan launch has read the word by then).
//   * k_aug_apply, the hot path, output-centric: a thread owns four consecutive x of one output row (16-byte stores into the NCHW planes, 48 contiguous bytes
//     channels-last).  Per pixel four bilinear taps (OpenCV INTER_LINEAR, no antialiasing); a tap is mirrored, offset by the crop rect into the canvas, and inside
//     the pasted image reads the uint8 source pixel through the photometric chain, outside it takes the undistorted mean.  Adjacent pixels share source columns:
//     the two columns of the previous pixel stay in registers, and a row pair that collapses onto one source row is distorted once.  The plan record is read at
//     workgroup-uniform addresses (scalar registers); a workgroup never spans two images.  Any plan is memory-safe: a source pixel is read only after its
//     coordinates were checked against the image's size.
#include "frost_common.h"

#define AUG_T 256
#define AUG_TAG 0x53534441u          // "SSDA": keeps this Philox stream apart from the optimizer's and the dropout's

__device__ __forceinline__ void aug_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct AugRng { uint32_t k0, k1, o0, o1, n, blk, w0, w1, w2, w3; };
__device__ __forceinline__ uint32_t aug_word(AugRng& r) {
  const uint32_t b = r.n >> 2;
  if (b != r.blk) { uint32_t w[4]; aug_philox(r.o0, r.o1, b, AUG_TAG, r.k0, r.k1, w); r.w0 = w[0]; r.w1 = w[1]; r.w2 = w[2]; r.w3 = w[3]; r.blk = b; }
  const uint32_t i = r.n & 3u;
  ++r.n;
  return i == 0u ? r.w0 : i == 1u ? r.w1 : i == 2u ? r.w2 : r.w3;
}
__device__ __forceinline__ bool aug_coin(AugRng& r) { return (aug_word(r) >> 31) != 0u; }
__device__ __forceinline__ int aug_choice(AugRng& r, uint32_t k) { return (int)(((uint64_t)aug_word(r) * k) >> 32); }
__device__ __forceinline__ float aug_uniform(AugRng& r, float a, float b) {
  const float u = (float)(aug_word(r) >> 8) * 5.9604644775390625e-08f;          // 2^-24
  return a + (b - a) * u;
}

__global__ __launch_bounds__(64) void k_aug_plan(const int* __restrict__ sizes, const float* __restrict__ boxes, const uint8_t* __restrict__ valid, int G,
                                                 const int64_t* __restrict__ state, int* __restrict__ plan, float* __restrict__ boxes_out,
                                                 uint8_t* __restrict__ valid_out) {
  __shared__ float2 centre[FROST_AUG_MAX_G];          // (cx, cy) of every valid box on the canvas; NaN for a padding row: every comparison is false
  const int n = blockIdx.x, lane = threadIdx.x;
  const uint64_t seed = (uint64_t)state[0], ord = (uint64_t)state[1] + (uint64_t)n;
  AugRng rng = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)ord, (uint32_t)(ord >> 32), 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
  // ---- the photometric decisions, in the reference's order (augmentations.py:389-397)
  int flags = FROST_AUG_F_HSV;          // both orders of PhotometricDistort.pd convert to HSV and back, whatever the coins say
  float delta = 0.0f, alpha = 1.0f, sat = 1.0f, hue = 0.0f;
  if (aug_coin(rng)) { flags |= FROST_AUG_F_BRIGHT; delta = aug_uniform(rng, -32.0f, 32.0f); }
  if (aug_coin(rng)) {                  // randint(2) true = pd[:-1]: contrast before HSV
    flags |= FROST_AUG_F_CONTRAST_FIRST;
    if (aug_coin(rng)) { flags |= FROST_AUG_F_CONTRAST; alpha = aug_uniform(rng, 0.5f, 1.5f); }
  }
  if (aug_coin(rng)) { flags |= FROST_AUG_F_SAT; sat = aug_uniform(rng, 0.5f, 1.5f); }
  if (aug_coin(rng)) { flags |= FROST_AUG_F_HUE; hue = aug_uniform(rng, -18.0f, 18.0f); }
  if (!(flags & FROST_AUG_F_CONTRAST_FIRST) && aug_coin(rng)) { flags |= FROST_AUG_F_CONTRAST; alpha = aug_uniform(rng, 0.5f, 1.5f); }
  int perm = 0;
  if (aug_coin(rng)) { flags |= FROST_AUG_F_NOISE; perm = aug_choice(rng, 6u); }
  // ---- Expand (:312-337): randint(2) TRUE returns the image unchanged
  const int h0 = sizes[2 * n], w0 = sizes[2 * n + 1];
  const float wf = (float)w0, hf = (float)h0;
  int W = w0, H = h0, px = 0, py = 0;
  float ratio = 1.0f;
  if (!aug_coin(rng)) {
    flags |= FROST_AUG_F_EXPAND;
    ratio = aug_uniform(rng, 1.0f, 4.0f);
    const float left = aug_uniform(rng, 0.0f, wf * ratio - wf);
    const float top = aug_uniform(rng, 0.0f, hf * ratio - hf);
    W = (int)(wf * ratio); H = (int)(hf * ratio);
    px = (int)left; py = (int)top;
  }
  const float pxf = (float)px, pyf = (float)py;
  // ---- box centres on the canvas
  const float* brow = boxes + (int64_t)n * G * 5;
  const uint8_t* vrow = valid + (int64_t)n * G;
  bool mine = false;
  for (int g = lane; g < G; g += 64) {
    const bool v = vrow[g] != 0;
    const float bx1 = brow[g * 5] * wf + pxf, by1 = brow[g * 5 + 1] * hf + pyf, bx2 = brow[g * 5 + 2] * wf + pxf, by2 = brow[g * 5 + 3] * hf + pyf;
    centre[g] = v ? make_float2((bx1 + bx2) * 0.5f, (by1 + by2) * 0.5f) : make_float2(NAN, NAN);
    mine = mine || v;
  }
  __syncthreads();
  // ---- RandomSampleCrop (:208-309) as written.  Line 269's reject test `overlap.min() < min_iou and max_iou < overlap.max()` has max_iou = inf in all six options and
  // is never true: only the mode (uniform over six, 0 = the whole image) and the centre test matter, no IoU is computed.  `random.uniform(width - w)` is numpy's
  // uniform(low = width - w, high = 1.0), so int(left + w) can exceed W by one.  A trial that fails the aspect test consumes only its two size draws.  Added
  // definitions: no valid box -> mode 0 without draws; at most 64 mode rounds, then mode 0.
  int mode = 0, rounds = 0, x1 = 0, y1 = 0, x2 = W, y2 = H;
  float dw = 0.0f, dh = 0.0f;
  const float Wf = (float)W, Hf = (float)H;
  if (__ballot(mine) != 0ull) {
    bool done = false;
    for (int r = 0; r < FROST_AUG_MAX_ROUNDS && !done; ++r) {
      ++rounds;
      const int m = aug_choice(rng, 6u);
      if (m == 0) break;
      for (int t = 0; t < FROST_AUG_TRIALS; ++t) {
        const float w = aug_uniform(rng, 0.3f * Wf, Wf);
        const float h = aug_uniform(rng, 0.3f * Hf, Hf);
        const float q = h / w;
        if (q < 0.5f || q > 2.0f) continue;
        const float left = aug_uniform(rng, Wf - w, 1.0f);
        const float top = aug_uniform(rng, Hf - h, 1.0f);
        const int rx1 = (int)left, ry1 = (int)top, rx2 = (int)(left + w), ry2 = (int)(top + h);
        const float fx1 = (float)rx1, fy1 = (float)ry1, fx2 = (float)rx2, fy2 = (float)ry2;
        bool hit = false;
        for (int g = lane; g < G; g += 64) {
          const float2 c = centre[g];
          hit = hit || (fx1 < c.x && fy1 < c.y && fx2 > c.x && fy2 > c.y);          // strictly inside
        }
        if (__ballot(hit) != 0ull) { mode = m; x1 = rx1; y1 = ry1; x2 = rx2; y2 = ry2; dw = w; dh = h; done = true; break; }
      }
    }
  }
  const bool mirror = aug_coin(rng);          // RandomMirror (:340-347)
  if (mirror) flags |= FROST_AUG_F_MIRROR;
  // ---- boxes: clip to the UNCLIPPED rect, shift, mirror and divide by the CLIPPED crop's extent; survivors keep their rows
  const float rx1 = (float)x1, ry1 = (float)y1, rx2 = (float)x2, ry2 = (float)y2;
  const float cwf = (float)max(min(x2, W) - x1, 1), chf = (float)max(min(y2, H) - y1, 1);
  for (int g = lane; g < G; g += 64) {
    const float2 c = centre[g];
    const bool v = vrow[g] != 0;
    const bool keep = mode ? (rx1 < c.x && ry1 < c.y && rx2 > c.x && ry2 > c.y) : v;
    float bx1 = brow[g * 5] * wf + pxf, by1 = brow[g * 5 + 1] * hf + pyf, bx2 = brow[g * 5 + 2] * wf + pxf, by2 = brow[g * 5 + 3] * hf + pyf;
    if (mode) { bx1 = fmaxf(bx1, rx1); by1 = fmaxf(by1, ry1); bx2 = fminf(bx2, rx2); by2 = fminf(by2, ry2); }
    bx1 = bx1 - rx1; by1 = by1 - ry1; bx2 = bx2 - rx1; by2 = by2 - ry1;
    if (mirror) { const float a = cwf - bx2, b = cwf - bx1; bx1 = a; bx2 = b; }
    float* o = boxes_out + ((int64_t)n * G + g) * 5;
    o[0] = keep ? bx1 / cwf : 0.0f; o[1] = keep ? by1 / chf : 0.0f; o[2] = keep ? bx2 / cwf : 0.0f; o[3] = keep ? by2 / chf : 0.0f; o[4] = keep ? brow[g * 5 + 4] : 0.0f;
    valid_out[(int64_t)n * G + g] = keep ? 1 : 0;
  }
  if (lane == 0) {
    int* rec = plan + (int64_t)n * FROST_AUG_PLAN_WORDS;
    const bool cf = (flags & FROST_AUG_F_CONTRAST_FIRST) != 0;
    rec[FROST_AUG_FLAGS] = flags;
    rec[FROST_AUG_DELTA] = __float_as_int(delta);
    rec[FROST_AUG_ALPHA_PRE] = __float_as_int(cf ? alpha : 1.0f);
    rec[FROST_AUG_ALPHA_POST] = __float_as_int(cf ? 1.0f : alpha);
    rec[FROST_AUG_SAT] = __float_as_int(sat);
    rec[FROST_AUG_HUE] = __float_as_int(hue);
    rec[FROST_AUG_PERM] = perm;
    rec[FROST_AUG_RATIO] = __float_as_int(ratio);
    rec[FROST_AUG_PASTE_X] = px; rec[FROST_AUG_PASTE_Y] = py; rec[FROST_AUG_CANVAS_W] = W; rec[FROST_AUG_CANVAS_H] = H;
    rec[FROST_AUG_MODE] = mode; rec[FROST_AUG_ROUNDS] = rounds;
    rec[FROST_AUG_X1] = x1; rec[FROST_AUG_Y1] = y1; rec[FROST_AUG_X2] = x2; rec[FROST_AUG_Y2] = y2;
    rec[FROST_AUG_DRAWN_W] = __float_as_int(dw); rec[FROST_AUG_DRAWN_H] = __float_as_int(dh);
    for (int i = FROST_AUG_DRAWN_H + 1; i < FROST_AUG_PLAN_WORDS; ++i) rec[i] = 0;
  }
}

__global__ void k_aug_advance(int64_t* state, int n) { state[1] += n; }

// ---- the photometric chain on one BGR triple: nothing is clipped anywhere (the reference clips nothing) ------------------------------------------------------------
struct AugPhoto { float delta, a_pre, a_post, sat, hue; int hsv, p0, p1, p2; };
__device__ __forceinline__ float aug_sel3(float a, float b, float c, int i) { return i == 0 ? a : i == 1 ? b : c; }
// per hue sector 0 .. 5 the index into {v, v(1-s), v(1-sf), v(1-s(1-f))}, two bits each: b = 1,1,3,0,0,2  g = 3,0,0,2,1,1  r = 0,2,1,1,3,0
#define AUG_PACK6(a, b, c, d, e, f) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6) | ((e) << 8) | ((f) << 10))
__device__ __forceinline__ float aug_tab(float t0, float t1, float t2, float t3, int pack, int sector) {
  const int i = (pack >> (2 * sector)) & 3;
  return i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
}
__device__ __forceinline__ void aug_chain(const AugPhoto& p, float b, float g, float r, float (&o)[3]) {
  b = b + p.delta; g = g + p.delta; r = r + p.delta;
  b = b * p.a_pre; g = g * p.a_pre; r = r * p.a_pre;
  if (p.hsv) {                                                   // workgroup-uniform
    // OpenCV's float BGR -> HSV, H in degrees
    const float v = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    const float diff = v - mn;
    float s = diff / (fabsf(v) + FROST_F32_EPS);
    const float d = 60.0f / (diff + FROST_F32_EPS);
    float h = (v == r) ? (g - b) * d : (v == g) ? (b - r) * d + 120.0f : (r - g) * d + 240.0f;
    if (h < 0.0f) h = h + 360.0f;
    s = s * p.sat;                                               // RandomSaturation
    h = h + p.hue;                                               // RandomHue and its wrap
    if (h > 360.0f) h = h - 360.0f;
    if (h < 0.0f) h = h + 360.0f;
    // OpenCV's float HSV -> BGR
    h = h * (float)(1.0 / 60.0);
    if (h < 0.0f) h = h + 6.0f;
    if (h >= 6.0f) h = h - 6.0f;
    const float fl = floorf(h), f = h - fl;
    const int sector = min(max((int)fl, 0), 5);
    const float t1 = v * (1.0f - s), t2 = v * (1.0f - s * f), t3 = v * (1.0f - s * (1.0f - f));
    b = aug_tab(v, t1, t2, t3, AUG_PACK6(1, 1, 3, 0, 0, 2), sector);
    g = aug_tab(v, t1, t2, t3, AUG_PACK6(3, 0, 0, 2, 1, 1), sector);
    r = aug_tab(v, t1, t2, t3, AUG_PACK6(0, 2, 1, 1, 3, 0), sector);
  }
  b = b * p.a_post; g = g * p.a_post; r = r * p.a_post;
  o[0] = aug_sel3(b, g, r, p.p0); o[1] = aug_sel3(b, g, r, p.p1); o[2] = aug_sel3(b, g, r, p.p2);          // RandomLightingNoise: out[c] = in[perm[c]]
}

// one source column of a pixel's taps: the values of its upper and lower tap row
struct AugCol { int sx; float t[3], b[3]; };

// OpenCV INTER_LINEAR: src = (dst + 0.5) * scale - 0.5, i0 = floor, both taps clamped to [0, extent - 1]
__device__ __forceinline__ void aug_taps(int dst, float scale, int extent, int& i0, int& i1, float& frac) {
  const float src = ((float)dst + 0.5f) * scale - 0.5f;
  const float fl = floorf(src);
  frac = src - fl;
  const int i = (int)fl;
  i0 = min(max(i, 0), extent - 1);
  i1 = min(max(i + 1, 0), extent - 1);
}

template <bool CL, bool VEC>
__global__ __launch_bounds__(AUG_T) void k_aug_apply(const uint8_t* __restrict__ images, const int* __restrict__ sizes, const int* __restrict__ plan, int Hmax,
                                                     int Wmax, int S, int S4, float m0, float m1, float m2, float* __restrict__ x) {
  const int n = blockIdx.y;
  const int item = blockIdx.x * AUG_T + threadIdx.x;
  if (item >= S4 * S) return;
  const int y = item / S4, xq = (item - y * S4) * 4;
  const int* rec = plan + (int64_t)n * FROST_AUG_PLAN_WORDS;
  const int flags = rec[FROST_AUG_FLAGS];
  AugPhoto ph;
  ph.delta = __int_as_float(rec[FROST_AUG_DELTA]); ph.a_pre = __int_as_float(rec[FROST_AUG_ALPHA_PRE]); ph.a_post = __int_as_float(rec[FROST_AUG_ALPHA_POST]);
  ph.sat = __int_as_float(rec[FROST_AUG_SAT]); ph.hue = __int_as_float(rec[FROST_AUG_HUE]); ph.hsv = flags & FROST_AUG_F_HSV;
  {                                                              // permutation i of ((0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0))
    const int pi = min(max(rec[FROST_AUG_PERM], 0), 5);
    ph.p0 = pi >> 1;
    const int r0 = ph.p0 == 0 ? 1 : 0, r1 = ph.p0 == 2 ? 1 : 2;
    ph.p1 = (pi & 1) ? r1 : r0; ph.p2 = (pi & 1) ? r0 : r1;
  }
  const bool mirror = (flags & FROST_AUG_F_MIRROR) != 0;
  const int px = rec[FROST_AUG_PASTE_X], py = rec[FROST_AUG_PASTE_Y], x1 = rec[FROST_AUG_X1], y1 = rec[FROST_AUG_Y1];
  const int cw = max(min(rec[FROST_AUG_X2], rec[FROST_AUG_CANVAS_W]) - x1, 1), ch = max(min(rec[FROST_AUG_Y2], rec[FROST_AUG_CANVAS_H]) - y1, 1);   // the rect clipped to the canvas
  const int h = sizes[2 * n], w = sizes[2 * n + 1];
  const float scx = (float)cw / (float)S, scy = (float)ch / (float)S;
  const float mean[3] = {m0, m1, m2};
  const uint8_t* img = images + (int64_t)n * Hmax * Wmax * 3;

  int ty0, ty1; float fy;
  aug_taps(y, scy, ch, ty0, ty1, fy);
  const int syA = y1 + ty0 - py, syB = y1 + ty1 - py;            // source rows of the two taps (the crop is not mirrored vertically)
  const bool inA = syA >= 0 && syA < h, inB = syB >= 0 && syB < h;
  const uint8_t* rowA = img + (int64_t)(inA ? syA : 0) * Wmax * 3;
  const uint8_t* rowB = img + (int64_t)(inB ? syB : 0) * Wmax * 3;
  const float wy0 = 1.0f - fy;

  auto column = [&](int sx) {
    AugCol c;
    c.sx = sx;
    const bool inx = sx >= 0 && sx < w;
    if (inx && inA) { const uint8_t* p = rowA + sx * 3; aug_chain(ph, (float)p[0], (float)p[1], (float)p[2], c.t); }
    else { c.t[0] = m0; c.t[1] = m1; c.t[2] = m2; }              // outside the pasted image: the mean, undistorted (Expand runs after PhotometricDistort)
    if (syB == syA) { c.b[0] = c.t[0]; c.b[1] = c.t[1]; c.b[2] = c.t[2]; }
    else if (inx && inB) { const uint8_t* p = rowB + sx * 3; aug_chain(ph, (float)p[0], (float)p[1], (float)p[2], c.b); }
    else { c.b[0] = m0; c.b[1] = m1; c.b[2] = m2; }
    return c;
  };

  float out[3][4];
  AugCol c0, c1;
  bool have = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xx = min(xq + j, S - 1);                           // the tail of a row whose length is no multiple of four recomputes its last pixel; the store is masked
    int tx0, tx1; float fx;
    aug_taps(xx, scx, cw, tx0, tx1, fx);
    if (mirror) { tx0 = cw - 1 - tx0; tx1 = cw - 1 - tx1; }
    const int sx0 = x1 + tx0 - px, sx1 = x1 + tx1 - px;
    AugCol n0, n1;
    if (have && sx0 == c0.sx) n0 = c0; else if (have && sx0 == c1.sx) n0 = c1; else n0 = column(sx0);
    if (sx1 == n0.sx) n1 = n0; else if (have && sx1 == c0.sx) n1 = c0; else if (have && sx1 == c1.sx) n1 = c1; else n1 = column(sx1);
    c0 = n0; c1 = n1; have = true;
    const float wx0 = 1.0f - fx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = c0.t[c] * wx0 + c1.t[c] * fx, bot = c0.b[c] * wx0 + c1.b[c] * fx;
      out[c][j] = (top * wy0 + bot * fy) - mean[c];
    }
  }
  if (CL) {
    float* o = x + (((int64_t)n * S + y) * S + xq) * 3;
    if (VEC) {
      ((float4*)o)[0] = make_float4(out[0][0], out[1][0], out[2][0], out[0][1]);
      ((float4*)o)[1] = make_float4(out[1][1], out[2][1], out[0][2], out[1][2]);
      ((float4*)o)[2] = make_float4(out[2][2], out[0][3], out[1][3], out[2][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xq + j < S) { o[j * 3] = out[0][j]; o[j * 3 + 1] = out[1][j]; o[j * 3 + 2] = out[2][j]; }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = x + (((int64_t)n * 3 + c) * S + y) * S + xq;
      if (VEC) *(float4*)o = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (xq + j < S) o[j] = out[c][j];
      }
    }
  }
}

extern "C" int frost_aug_plan_words(void) { return FROST_AUG_PLAN_WORDS; }

extern "C" int frost_aug_plan(const int32_t* sizes, const float* boxes, const uint8_t* valid, int n, int g, int64_t* state, int32_t* plan, float* boxes_out,
                              uint8_t* valid_out, void* stream) {
  FROST_REQUIRE(sizes && boxes && valid && state && plan && boxes_out && valid_out, "aug_plan: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "aug_plan: n outside 1 .. 65535");
  FROST_REQUIRE(g >= 1 && g <= FROST_AUG_MAX_G, "aug_plan: G outside 1 .. 1024");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_aug_plan, dim3(n), dim3(64), 0, s, sizes, boxes, valid, g, (const int64_t*)state, plan, boxes_out, valid_out);
  hipLaunchKernelGGL(k_aug_advance, dim3(1), dim3(1), 0, s, state, n);
  return frost_check_launch("aug_plan");
}

extern "C" int frost_aug_apply(const uint8_t* images, const int32_t* sizes, const int32_t* plan, int n, int hmax, int wmax, int size, float mean_b, float mean_g,
                               float mean_r, int channels_last, float* x, void* stream) {
  FROST_REQUIRE(images && sizes && plan && x, "aug_apply: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "aug_apply: n outside 1 .. 65535");
  FROST_REQUIRE(size >= 1 && size <= FROST_AUG_MAX_SIZE, "aug_apply: size outside 1 .. 4096");
  FROST_REQUIRE(hmax >= 1 && wmax >= 1 && (int64_t)hmax * wmax * 3 <= INT32_MAX, "aug_apply: Hmax / Wmax below 1, or a slot above 2^31 bytes");
  const int s4 = (size + 3) / 4;
  const dim3 grid((s4 * size + AUG_T - 1) / AUG_T, n), block(AUG_T);
  const bool vec = size % 4 == 0 && ((uintptr_t)x & 15u) == 0;          // 16-byte stores need rows of whole float4s
  hipStream_t s = as_stream(stream);
#define AUG_LAUNCH(CL, VEC) hipLaunchKernelGGL((k_aug_apply<CL, VEC>), grid, block, 0, s, images, sizes, plan, hmax, wmax, size, s4, mean_b, mean_g, mean_r, x)
  if (channels_last) { if (vec) AUG_LAUNCH(true, true); else AUG_LAUNCH(true, false); }
  else { if (vec) AUG_LAUNCH(false, true); else AUG_LAUNCH(false, false); }
#undef AUG_LAUNCH
  return frost_check_launch("aug_apply");
}

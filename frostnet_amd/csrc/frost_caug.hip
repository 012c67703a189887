// The classifier's input pipeline on a whole batch on the device: uint8 images in, the network's normalised fp32 input out, without host synchronisation (the
// reference runs torchvision on PIL images, one image at a time on the host).
//
// replaces: Classification/utils/data_functions.py:23-42 (RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize; Resize -> CenterCrop -> ToTensor ->
// Normalize), as restated by frostnet_amd/cls_augment.py on CPU tensors (the definition and the parity yardstick: tests/test_gpu_cls_augment.py expects plan words and
// pixels equal bit for bit).  The resize is Pillow's antialiased two-pass triangle resampler: fp64 weights in Pillow's written order (the library builds with
// -ffp-contract=off), 22-bit fixed-point coefficients, a uint8 intermediate between the horizontal and the vertical pass.
//   * k_caug_plan, one lane per image: RandomResizedCrop.get_params (ten trials in fp64, exp as the definition's Horner polynomial, then the central fallback) and the
//     mirror coin, from Philox4x32-10 counters (key = seed, counter = (image ordinal, draw block, stream tag)).  k_caug_advance, one thread behind it: images seen += n.
//   * k_caug_eval_plan, one lane per image: Resize + CenterCrop as a plan record (integer arithmetic only).
//   * k_caug_apply, the hot path.  A workgroup owns (image, band of CAUG_BR output rows, chunk of up to CAUG_TW output columns).  It writes the coefficients of its
//     columns and rows into LDS once (fp64, one division per tap), runs the horizontal pass of the source rows its band needs into an LDS uint8 tile -- the
//     definition's uint8 intermediate IS that tile; the taps of an output pixel are consecutive source bytes and are read as aligned dwords shifted into place
//     (caug_hrow) -- and then the vertical pass out of LDS: a thread owns four consecutive output pixels, reads 12 contiguous tile
//     bytes per tap row, looks the three channels up in the 3 x 256 normalisation table (LDS) and stores 16 bytes per plane (48 contiguous bytes channels-last).
//     The mirror is folded into the horizontal pass: tile column j holds window column size - 1 - j.  That path needs at most FROST_CAUG_MAX_TAPS taps per axis
//     (ceil(scale) <= 4) and at most CAUG_ROWS source rows per band; any other crop takes the general path of the same kernel, one thread per output pixel with
//     the coefficients recomputed tap by tap (slow, and correct for every crop the slot allows).  Any plan is memory-safe: rect and grid are clamped into the slot.
#include "frost_common.h"

#define CAUG_T 256
#define CAUG_TAG 0x43524F50u          // "CROP": keeps this Philox stream apart from the detector's augmentation, the optimizer's and the dropout's
#define CAUG_BR 8                     // output rows of a band
#define CAUG_TW 256                   // output columns of a chunk (a multiple of 4)
#define CAUG_K FROST_CAUG_MAX_TAPS
#define CAUG_ROWS 40                  // source rows of a band on the LDS path: (CAUG_BR - 1) * 4 + 2 * 4 + 2 = 38 at the cap
#define CAUG_BITS 22                  // Pillow's PRECISION_BITS for 8-bit channels

__device__ __forceinline__ void caug_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct CaugRng { uint32_t k0, k1, o0, o1, n, blk, w0, w1, w2, w3; };
__device__ __forceinline__ uint32_t caug_word(CaugRng& r) {
  const uint32_t b = r.n >> 2;
  if (b != r.blk) { uint32_t w[4]; caug_philox(r.o0, r.o1, b, CAUG_TAG, r.k0, r.k1, w); r.w0 = w[0]; r.w1 = w[1]; r.w2 = w[2]; r.w3 = w[3]; r.blk = b; }
  const uint32_t i = r.n & 3u;
  ++r.n;
  return i == 0u ? r.w0 : i == 1u ? r.w1 : i == 2u ? r.w2 : r.w3;
}
__device__ __forceinline__ int caug_choice(CaugRng& r, uint32_t k) { return (int)(((uint64_t)caug_word(r) * k) >> 32); }
__device__ __forceinline__ double caug_unit(CaugRng& r) { return (double)(caug_word(r) >> 8) * 5.9604644775390625e-08; }          // 2^-24

// exp(t), |t| <= log 2: the definition's Horner sequence over 1 / k!, k = 13 .. 0 (cls_augment.exp_poly) -- 13 multiplies and 13 adds, no libm on either side
__device__ __forceinline__ double caug_exp(double t) {
  double r = 1.0 / 6227020800.0;
  r = r * t + 1.0 / 479001600.0; r = r * t + 1.0 / 39916800.0; r = r * t + 1.0 / 3628800.0; r = r * t + 1.0 / 362880.0; r = r * t + 1.0 / 40320.0;
  r = r * t + 1.0 / 5040.0; r = r * t + 1.0 / 720.0; r = r * t + 1.0 / 120.0; r = r * t + 1.0 / 24.0; r = r * t + 1.0 / 6.0; r = r * t + 1.0 / 2.0;
  r = r * t + 1.0; r = r * t + 1.0;
  return r;
}

__global__ __launch_bounds__(64) void k_caug_plan(const int* __restrict__ sizes, int n, int size, double s0, double s1, double l0, double l1, double r0, double r1,
                                                  const int64_t* __restrict__ state, int* __restrict__ plan) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint64_t seed = (uint64_t)state[0], ord = (uint64_t)state[1] + (uint64_t)i;
  CaugRng rng = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)ord, (uint32_t)(ord >> 32), 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
  const int h0 = sizes[2 * i], w0 = sizes[2 * i + 1];
  const double area = (double)((int64_t)h0 * (int64_t)w0);
  int flags = 0, tries = 0, x0 = 0, y0 = 0, w = 0, h = 0;
  bool found = false;
  for (int t = 0; t < FROST_CAUG_TRIALS && !found; ++t) {          // RandomResizedCrop.get_params
    ++tries;
    const double target = area * (s0 + (s1 - s0) * caug_unit(rng));
    const double aspect = caug_exp(l0 + (l1 - l0) * caug_unit(rng));
    const double wd = rint(sqrt(target * aspect)), hd = rint(sqrt(target / aspect));          // rint: half to even, as Python's round
    if (wd > 0.0 && wd <= (double)w0 && hd > 0.0 && hd <= (double)h0) {
      w = (int)wd; h = (int)hd;
      y0 = caug_choice(rng, (uint32_t)(h0 - h + 1));
      x0 = caug_choice(rng, (uint32_t)(w0 - w + 1));
      found = true;
    }
  }
  if (!found) {                                                     // the central fallback
    flags |= FROST_CAUG_F_FALLBACK;
    const double in_ratio = (double)w0 / (double)h0;
    if (in_ratio < r0) { w = w0; h = (int)fmin(fmax(rint((double)w0 / r0), 1.0), (double)h0); }
    else if (in_ratio > r1) { h = h0; w = (int)fmin(fmax(rint((double)h0 * r1), 1.0), (double)w0); }
    else { w = w0; h = h0; }
    x0 = (w0 - w) / 2; y0 = (h0 - h) / 2;
  }
  if ((caug_word(rng) >> 31) != 0u) flags |= FROST_CAUG_F_MIRROR;  // RandomHorizontalFlip
  int* rec = plan + (int64_t)i * FROST_CAUG_PLAN_WORDS;
  rec[FROST_CAUG_FLAGS] = flags; rec[FROST_CAUG_X0] = x0; rec[FROST_CAUG_Y0] = y0; rec[FROST_CAUG_W] = w; rec[FROST_CAUG_H] = h;
  rec[FROST_CAUG_RW] = size; rec[FROST_CAUG_RH] = size; rec[FROST_CAUG_OX] = 0; rec[FROST_CAUG_OY] = 0; rec[FROST_CAUG_TRIES] = tries;
  for (int k = FROST_CAUG_TRIES + 1; k < FROST_CAUG_PLAN_WORDS; ++k) rec[k] = 0;
}

__global__ void k_caug_advance(int64_t* state, int n) { state[1] += n; }

__device__ __forceinline__ int caug_half_even(int d) { return (d + ((d >> 1) & 1)) >> 1; }          // round(d / 2), half to even, d >= 0

__global__ __launch_bounds__(64) void k_caug_eval_plan(const int* __restrict__ sizes, int n, int size, int resize, int* __restrict__ plan) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int h0 = sizes[2 * i], w0 = sizes[2 * i + 1];
  // Resize(resize): the shorter side -> resize, the longer -> int(resize * long / short)
  const int64_t lng = (int64_t)resize * (int64_t)max(h0, w0) / (int64_t)max(min(h0, w0), 1);
  const int g = (int)min(lng, (int64_t)1 << 30);
  const int rw = w0 <= h0 ? resize : g, rh = w0 <= h0 ? g : resize;
  int* rec = plan + (int64_t)i * FROST_CAUG_PLAN_WORDS;
  rec[FROST_CAUG_FLAGS] = 0; rec[FROST_CAUG_X0] = 0; rec[FROST_CAUG_Y0] = 0; rec[FROST_CAUG_W] = w0; rec[FROST_CAUG_H] = h0;
  rec[FROST_CAUG_RW] = rw; rec[FROST_CAUG_RH] = rh; rec[FROST_CAUG_OX] = caug_half_even(max(rw - size, 0)); rec[FROST_CAUG_OY] = caug_half_even(max(rh - size, 0));
  for (int k = FROST_CAUG_OY + 1; k < FROST_CAUG_PLAN_WORDS; ++k) rec[k] = 0;
}

// ---- Pillow's precompute_coeffs for the triangle filter, one axis ---------------------------------------------------------------------------------------------------
struct CaugAxis { double scale, support, ss; int in, taps; };
__device__ __forceinline__ CaugAxis caug_axis(int in, int out) {
  CaugAxis a;
  a.in = in;
  a.scale = (double)in / (double)out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = fs; a.ss = 1.0 / fs;
  a.taps = (int)fmin(ceil(fs), 1.0e6) * 2 + 1;
  return a;
}
// output index xx: the first source index, the number of taps, the centre
__device__ __forceinline__ void caug_bounds(const CaugAxis& a, int xx, int& xmin, int& cnt, double& center) {
  center = ((double)xx + 0.5) * a.scale;
  xmin = (int)fmin(center - a.support + 0.5, (double)a.in);          // the C cast: towards zero (a valid index never reaches the fmin)
  if (xmin < 0) xmin = 0;
  int xmax = (int)fmin(center + a.support + 0.5, (double)a.in);
  if (xmax > a.in) xmax = a.in;
  cnt = max(xmax - xmin, 0);
}
__device__ __forceinline__ double caug_weight(const CaugAxis& a, int x, int xmin, double center) {
  const double v = fabs(((double)(x + xmin) - center + 0.5) * a.ss);
  return v < 1.0 ? 1.0 - v : 0.0;
}
__device__ __forceinline__ double caug_wsum(const CaugAxis& a, int xmin, int cnt, double center) {
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww = ww + caug_weight(a, x, xmin, center);          // ascending x, as Pillow sums
  return ww;
}
__device__ __forceinline__ int caug_coef(double w, double ww) {
  if (ww != 0.0) w = w / ww;
  return (int)(0.5 + w * 4194304.0);          // normalize_coeffs_8bpc: 2^22
}
__device__ __forceinline__ int caug_clip8(int acc) { return min(max(acc >> CAUG_BITS, 0), 255); }

// NT consecutive source pixels (3 NT bytes from byte `goff` of the batch) times their coefficients, read as ALIGNED dwords: the (3 NT + 3) / 4 + 1 dwords from
// goff & ~3 on, shifted into place by v_alignbyte, instead of 3 NT byte loads (the byte loads were what bound the kernel).  The caller guarantees that `base` is
// 4-byte aligned and that goff + 32 does not pass the end of the batch.  coef: this column's coefficients, twp words apart; taps behind the last one are zero.
template <int NT>
__device__ __forceinline__ void caug_hrow(const uint8_t* __restrict__ base, int64_t goff, const int* coef, int twp, int& a0, int& a1, int& a2) {
  constexpr int ND = (NT * 3 + 3) / 4;
  const uint32_t* p = (const uint32_t*)(base + (goff & ~(int64_t)3));
  const uint32_t sh = (uint32_t)goff & 3u;
  uint32_t d[ND + 1], w[ND];
#pragma unroll
  for (int k = 0; k <= ND; ++k) d[k] = p[k];
#pragma unroll
  for (int k = 0; k < ND; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);          // bytes 4 k + sh .. 4 k + sh + 3 of the dwords = bytes 4 k .. of the pixels
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = coef[t * twp];
    a0 += (int)((w[(3 * t) >> 2] >> (8 * ((3 * t) & 3))) & 255u) * c;
    a1 += (int)((w[(3 * t + 1) >> 2] >> (8 * ((3 * t + 1) & 3))) & 255u) * c;
    a2 += (int)((w[(3 * t + 2) >> 2] >> (8 * ((3 * t + 2) & 3))) & 255u) * c;
  }
}

template <bool CL, bool VEC>
__global__ __launch_bounds__(CAUG_T) void k_caug_apply(const uint8_t* __restrict__ images, const int* __restrict__ sizes, const int* __restrict__ plan, int Hmax,
                                                       int Wmax, int S, int nchunk, float m0, float m1, float m2, float d0, float d1, float d2, float* __restrict__ x) {
  // LDS, sized by the host for the chunk width twp = min(round_up(S, 4), CAUG_TW): at S = 224 that is 39 232 bytes, four workgroups per CU
  extern __shared__ __attribute__((aligned(16))) uint8_t caug_lds[];
  const int twp = min((S + 3) & ~3, CAUG_TW);
  uint8_t* tile = caug_lds;                                         // [CAUG_ROWS][twp][3]: a multiple of 16 bytes
  float* lut = (float*)(tile + CAUG_ROWS * twp * 3);                // [3][256]
  int* hmin = (int*)(lut + 3 * 256);                                // [twp]
  int* hco = hmin + twp;                                            // [CAUG_K][twp], tap-major: the lanes of a wave read consecutive words
  int* vmin = hco + CAUG_K * twp;                                   // [CAUG_BR]
  int* vco = vmin + CAUG_BR;                                        // [CAUG_BR][CAUG_K]
  const int n = blockIdx.y, tid = threadIdx.x;
  const int band = blockIdx.x / nchunk, chunk = blockIdx.x - band * nchunk;
  const int y0 = band * CAUG_BR, nr = min(CAUG_BR, S - y0), c0 = chunk * CAUG_TW, tw = min(CAUG_TW, S - c0);
  const int* rec = plan + (int64_t)n * FROST_CAUG_PLAN_WORDS;
  // the record, clamped into the slot: any plan is memory-safe (a valid plan passes unchanged)
  const int h = min(max(sizes[2 * n], 1), Hmax), w = min(max(sizes[2 * n + 1], 1), Wmax);
  const int W = min(max(rec[FROST_CAUG_W], 1), w), H = min(max(rec[FROST_CAUG_H], 1), h);
  const int X0 = min(max(rec[FROST_CAUG_X0], 0), w - W), Y0 = min(max(rec[FROST_CAUG_Y0], 0), h - H);
  const int RW = min(max(rec[FROST_CAUG_RW], 1), 1 << 30), RH = min(max(rec[FROST_CAUG_RH], 1), 1 << 30);
  const int OX = min(max(rec[FROST_CAUG_OX], 0), 1 << 30), OY = min(max(rec[FROST_CAUG_OY], 0), 1 << 30);
  const bool mirror = (rec[FROST_CAUG_FLAGS] & FROST_CAUG_F_MIRROR) != 0;
  const int64_t slot_bytes = (int64_t)Hmax * Wmax * 3, crop0 = (int64_t)n * slot_bytes + ((int64_t)Y0 * Wmax + X0) * 3;
  const uint8_t* img = images + crop0;                               // the crop's first pixel; rows are Wmax * 3 bytes apart
  const int pitch = Wmax * 3;
  const int64_t dword_end = ((uintptr_t)images & 3u) == 0 ? (int64_t)gridDim.y * slot_bytes - 32 : -1;          // the last byte offset caug_hrow may start at

  for (int i = tid; i < 3 * 256; i += CAUG_T) {                     // ToTensor + Normalize of every byte value: ((v / 255) - mean) / std, each rounded to fp32
    const int c = i >> 8;
    const float m = c == 0 ? m0 : c == 1 ? m1 : m2, d = c == 0 ? d0 : c == 1 ? d1 : d2;
    lut[i] = ((float)(i & 255) / 255.0f - m) / d;
  }
  const CaugAxis ax = caug_axis(W, RW), ay = caug_axis(H, RH);
  int rlo, nrows;
  {
    int a, b, cnt; double ctr;
    caug_bounds(ay, OY + y0, a, cnt, ctr);
    caug_bounds(ay, OY + y0 + nr - 1, b, cnt, ctr);
    rlo = a; nrows = b + cnt - a;                                   // the bounds grow with the index: the band reads source rows rlo .. rlo + nrows - 1
  }
  const bool lds_path = ax.taps <= CAUG_K && ay.taps <= CAUG_K && nrows >= 1 && nrows <= CAUG_ROWS;          // workgroup-uniform

  if (lds_path) {
    // ---- coefficients, once per workgroup
    for (int j = tid; j < tw; j += CAUG_T) {
      const int wc = mirror ? S - 1 - (c0 + j) : c0 + j;            // the window column that output column c0 + j shows
      int xmin, cnt; double ctr;
      caug_bounds(ax, OX + wc, xmin, cnt, ctr);
      const double ww = caug_wsum(ax, xmin, cnt, ctr);
      hmin[j] = xmin;
      for (int t = 0; t < CAUG_K; ++t) {                            // (t < taps is uniform: an up-scale divides three times, not nine)
        int c = 0;
        if (t < ax.taps && t < cnt) c = caug_coef(caug_weight(ax, t, xmin, ctr), ww);
        hco[t * twp + j] = c;
      }
    }
    {
      const int i = CAUG_T - 1 - tid;                               // the last lanes: the first ones may still be busy with a column
      if (i < nr) {
        int ymin, cnt; double ctr;
        caug_bounds(ay, OY + y0 + i, ymin, cnt, ctr);
        const double ww = caug_wsum(ay, ymin, cnt, ctr);
        vmin[i] = ymin - rlo;
        for (int t = 0; t < CAUG_K; ++t) {
          int c = 0;
          if (t < ay.taps && t < cnt) c = caug_coef(caug_weight(ay, t, ymin, ctr), ww);
          vco[i * CAUG_K + t] = c;
        }
      }
    }
    __syncthreads();
    // ---- horizontal pass: source rows rlo .. of the crop -> the uint8 tile
    const int kx = ax.taps, ky = ay.taps;
    for (int item = tid; item < nrows * tw; item += CAUG_T) {
      const int r = item / tw, j = item - r * tw;
      const int64_t roff = (int64_t)min(rlo + r, H - 1) * pitch;
      const uint8_t* row = img + roff;
      const int xm = hmin[j];
      int a0 = 1 << (CAUG_BITS - 1), a1 = a0, a2 = a0;
      const int64_t goff = crop0 + roff + xm * 3;
      if (goff <= dword_end) {                                       // all but the last few pixels of the batch
        if (kx <= 3) caug_hrow<3>(images, goff, hco + j, twp, a0, a1, a2);
        else if (kx <= 5) caug_hrow<6>(images, goff, hco + j, twp, a0, a1, a2);
        else caug_hrow<9>(images, goff, hco + j, twp, a0, a1, a2);
      } else for (int t0 = 0; t0 < kx; t0 += 3) {                          // taps in groups of three (3, 5, 7 or 9 of them): nine byte loads in flight, not three
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int c = hco[(t0 + u) * twp + j];
          const uint8_t* p = row + min(xm + t0 + u, W - 1) * 3;     // a tap behind the last one has coefficient 0: its (clamped) pixel does not count
          a0 += (int)p[0] * c; a1 += (int)p[1] * c; a2 += (int)p[2] * c;
        }
      }
      uint8_t* o = tile + (r * twp + j) * 3;
      o[0] = (uint8_t)caug_clip8(a0); o[1] = (uint8_t)caug_clip8(a1); o[2] = (uint8_t)caug_clip8(a2);
    }
    __syncthreads();
    // ---- vertical pass out of the tile, the table, the stores: four output pixels of one row per thread
    const int nq = (tw + 3) >> 2;
    for (int item = tid; item < nr * nq; item += CAUG_T) {
      const int i = item / nq, q = item - i * nq;
      int acc[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) acc[k] = 1 << (CAUG_BITS - 1);
      const int r0 = vmin[i];
      for (int t0 = 0; t0 < ky; t0 += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int c = vco[i * CAUG_K + t0 + u];
          const uint32_t* p = (const uint32_t*)(tile + (min(r0 + t0 + u, nrows - 1) * twp + 4 * q) * 3);          // 12 bytes at a multiple of 12
          const uint32_t u0 = p[0], u1 = p[1], u2 = p[2];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] += (int)((u0 >> (8 * k)) & 255u) * c; acc[4 + k] += (int)((u1 >> (8 * k)) & 255u) * c; acc[8 + k] += (int)((u2 >> (8 * k)) & 255u) * c;
          }
        }
      }
      float out[12];                                                // byte k of the 12: pixel k / 3, channel k % 3
#pragma unroll
      for (int k = 0; k < 12; ++k) out[k] = lut[(k % 3) * 256 + caug_clip8(acc[k])];
      const int yy = y0 + i, xq = c0 + 4 * q;
      if (CL) {
        float* o = x + (((int64_t)n * S + yy) * S + xq) * 3;
        if (VEC) {
          ((float4*)o)[0] = make_float4(out[0], out[1], out[2], out[3]);
          ((float4*)o)[1] = make_float4(out[4], out[5], out[6], out[7]);
          ((float4*)o)[2] = make_float4(out[8], out[9], out[10], out[11]);
        } else {
#pragma unroll
          for (int k = 0; k < 12; ++k) if (xq + k / 3 < S) o[k] = out[k];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float* o = x + (((int64_t)n * 3 + c) * S + yy) * S + xq;
          if (VEC) *(float4*)o = make_float4(out[c], out[3 + c], out[6 + c], out[9 + c]);
          else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (xq + k < S) o[k] = out[3 * k + c];
          }
        }
      }
    }
    return;
  }

  // ---- the general path: any scale.  One thread per output pixel, every coefficient recomputed where it is used.
  __syncthreads();          // the table
  for (int item = tid; item < nr * tw; item += CAUG_T) {
    const int i = item / tw, j = item - i * tw;
    const int wc = mirror ? S - 1 - (c0 + j) : c0 + j;
    int xmin, xcnt, ymin, ycnt; double xc, yc;
    caug_bounds(ax, OX + wc, xmin, xcnt, xc);
    caug_bounds(ay, OY + y0 + i, ymin, ycnt, yc);
    const double xww = caug_wsum(ax, xmin, xcnt, xc), yww = caug_wsum(ay, ymin, ycnt, yc);
    int v0 = 1 << (CAUG_BITS - 1), v1 = v0, v2 = v0;
    for (int ty = 0; ty < ycnt; ++ty) {
      const int cy = caug_coef(caug_weight(ay, ty, ymin, yc), yww);
      const uint8_t* row = img + (int64_t)min(ymin + ty, H - 1) * pitch;
      int a0 = 1 << (CAUG_BITS - 1), a1 = a0, a2 = a0;
      for (int tx = 0; tx < xcnt; ++tx) {
        const int cx = caug_coef(caug_weight(ax, tx, xmin, xc), xww);
        const uint8_t* p = row + min(xmin + tx, W - 1) * 3;
        a0 += (int)p[0] * cx; a1 += (int)p[1] * cx; a2 += (int)p[2] * cx;
      }
      v0 += caug_clip8(a0) * cy; v1 += caug_clip8(a1) * cy; v2 += caug_clip8(a2) * cy;          // the uint8 intermediate
    }
    const float o0 = lut[caug_clip8(v0)], o1 = lut[256 + caug_clip8(v1)], o2 = lut[512 + caug_clip8(v2)];
    const int yy = y0 + i, xx = c0 + j;
    if (CL) {
      float* o = x + (((int64_t)n * S + yy) * S + xx) * 3;
      o[0] = o0; o[1] = o1; o[2] = o2;
    } else {
      float* o = x + ((int64_t)n * 3 * S + yy) * S + xx;
      o[0] = o0; o[(int64_t)S * S] = o1; o[(int64_t)2 * S * S] = o2;
    }
  }
}

extern "C" int frost_caug_plan_words(void) { return FROST_CAUG_PLAN_WORDS; }

extern "C" int frost_caug_plan(const int32_t* sizes, int n, int size, double scale_lo, double scale_hi, double log_ratio_lo, double log_ratio_hi, double ratio_lo,
                               double ratio_hi, int64_t* state, int32_t* plan, void* stream) {
  FROST_REQUIRE(sizes && state && plan, "caug_plan: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "caug_plan: n outside 1 .. 65535");
  FROST_REQUIRE(size >= 1 && size <= FROST_AUG_MAX_SIZE, "caug_plan: size outside 1 .. 4096");
  FROST_REQUIRE(scale_lo > 0.0 && scale_lo <= scale_hi && ratio_lo >= 0.5 && ratio_lo <= ratio_hi && ratio_hi <= 2.0, "caug_plan: scale or ratio bounds out of order or range");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_caug_plan, dim3((n + 63) / 64), dim3(64), 0, s, sizes, n, size, scale_lo, scale_hi, log_ratio_lo, log_ratio_hi, ratio_lo, ratio_hi,
                     (const int64_t*)state, plan);
  hipLaunchKernelGGL(k_caug_advance, dim3(1), dim3(1), 0, s, state, n);
  return frost_check_launch("caug_plan");
}

extern "C" int frost_caug_eval_plan(const int32_t* sizes, int n, int size, int resize, int32_t* plan, void* stream) {
  FROST_REQUIRE(sizes && plan, "caug_eval_plan: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "caug_eval_plan: n outside 1 .. 65535");
  FROST_REQUIRE(size >= 1 && size <= resize && resize <= FROST_AUG_MAX_SIZE, "caug_eval_plan: 1 <= size <= resize <= 4096 expected");
  hipLaunchKernelGGL(k_caug_eval_plan, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), sizes, n, size, resize, plan);
  return frost_check_launch("caug_eval_plan");
}

extern "C" int frost_caug_apply(const uint8_t* images, const int32_t* sizes, const int32_t* plan, int n, int hmax, int wmax, int size, float mean0, float mean1,
                                float mean2, float std0, float std1, float std2, int channels_last, float* x, void* stream) {
  FROST_REQUIRE(images && sizes && plan && x, "caug_apply: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "caug_apply: n outside 1 .. 65535");
  FROST_REQUIRE(size >= 1 && size <= FROST_AUG_MAX_SIZE, "caug_apply: size outside 1 .. 4096");
  FROST_REQUIRE(hmax >= 1 && wmax >= 1 && (int64_t)hmax * wmax * 3 <= INT32_MAX, "caug_apply: Hmax / Wmax below 1, or a slot above 2^31 bytes");
  FROST_REQUIRE(std0 != 0.0f && std1 != 0.0f && std2 != 0.0f, "caug_apply: a std of zero");
  const int nchunk = (size + CAUG_TW - 1) / CAUG_TW, nband = (size + CAUG_BR - 1) / CAUG_BR;
  const dim3 grid(nband * nchunk, n), block(CAUG_T);
  const int twp = size + 3 < CAUG_TW ? (size + 3) & ~3 : CAUG_TW;
  const size_t lds = (size_t)CAUG_ROWS * twp * 3 + 3 * 256 * 4 + (size_t)(1 + CAUG_K) * twp * 4 + CAUG_BR * (1 + CAUG_K) * 4;
  const bool vec = size % 4 == 0 && ((uintptr_t)x & 15u) == 0;          // 16-byte stores need rows of whole float4s
  hipStream_t s = as_stream(stream);
#define CAUG_LAUNCH(CL, VEC) \
  hipLaunchKernelGGL((k_caug_apply<CL, VEC>), grid, block, lds, s, images, sizes, plan, hmax, wmax, size, nchunk, mean0, mean1, mean2, std0, std1, std2, x)
  if (channels_last) { if (vec) CAUG_LAUNCH(true, true); else CAUG_LAUNCH(true, false); }
  else { if (vec) CAUG_LAUNCH(false, true); else CAUG_LAUNCH(false, false); }
#undef CAUG_LAUNCH
  return frost_check_launch("caug_apply");
}

// The segmentation input pipeline on a whole batch on the device: uint8 pictures and uint8 label maps in, the network's normalised fp32 input and the criterion's
// target out, without host synchronisation (the reference runs Pillow on PIL images, one pair at a time on the host).
//
// replaces: Semantic_Segmentation/utilities/data_transforms.py (RandomFlip, RandomScale, RandomCrop, Resize, Normalize) as composed by data_loader/segmentation/voc.py
// and cityscapes.py, as restated by frostnet_amd/seg_augment.py on CPU tensors (the definition and the parity yardstick: tests/test_gpu_seg_augment.py expects plan
// words, pixels and labels equal bit for bit).  The picture's resize is Pillow's antialiased two-pass resampler with the Lanczos filter (training) or the triangle
// filter (validation): fp64 weights in Pillow's written order (the library builds with -ffp-contract=off), sin as the definition's fixed fp64 sequence, 22-bit
// fixed-point coefficients with negative weights rounded away from zero, a uint8 intermediate between the horizontal and the vertical pass.  The label's resize is
// Pillow's nearest-neighbour index table, filled by repeated fp64 addition.
//   * k_saug_plan, one lane per image: one Philox4x32-10 block = (scale unit, row offset, column offset, coin).  k_saug_advance, one thread behind it: images seen += n.
//   * k_saug_eval_plan, one lane per image: the validation records.
//   * k_saug_tables, one wave per (image, axis): the serial accumulation of Pillow's index table from index 0 up to the window's last entry (at most
//     FROST_SAUG_MAX_GRID dependent additions in one lane; the waves of a batch run side by side), written as "source column of output column j" / "source row of
//     output row i" with both mirrors folded in and -1 for padding.
//   * k_saug_apply, the hot path, designed from k_caug_apply.  A workgroup owns (image, band of SAUG_BR output rows, chunk of up to SAUG_TW output columns).  It
//     writes the signed coefficients of its columns and rows into LDS once, runs the horizontal pass of the source rows its band needs into an LDS uint8 tile (the
//     definition's uint8 intermediate; the taps are consecutive source bytes read as aligned dwords, saug_hrow), and then the vertical pass out of LDS: four output
//     pixels per thread through the 3 x 256 normalisation table, 16-byte stores.  A window column or row outside the grid has all-zero coefficients and never
//     touches the source: a zero byte IS the picture's padding.  The Cityscapes-order mirror is folded into the column order of the tile, the PASCAL-VOC-order mirror
//     into the tap order (the taps of the mirrored source, read from the unmirrored one, are the same bytes with the coefficients reversed).  Only the crop window
//     of the grid is ever computed.  That path needs at most FROST_SAUG_MAX_TAPS taps per axis and SAUG_ROWS source rows per band (Lanczos down to half size); any
//     other record takes the general path of the same kernel, one thread per output pixel.
//   * k_saug_labels: target[y][x] = labels[row table[y]][column table[x]], or ignore_idx, as int64 or uint8.
// Any plan is memory-safe: every word is clamped.
#include "frost_common.h"

#define SAUG_T 256
#define SAUG_TAG 0x53454741u          // "SEGA": keeps this Philox stream apart from the classifier's and the detector's augmentation, the optimizer's and the dropout's
#define SAUG_BR 8                     // output rows of a band
#define SAUG_TW 256                   // output columns of a chunk (a multiple of 4)
#define SAUG_K FROST_SAUG_MAX_TAPS
#define SAUG_ROWS 28                  // source rows of a band on the LDS path: (SAUG_BR - 1) * 2 + 1 + 13 at the cap
#define SAUG_BITS 22                  // Pillow's PRECISION_BITS for 8-bit channels
#define SAUG_PI 0x1.921fb54442d18p+1

__device__ __forceinline__ void saug_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// exp(t), |t| <= log 2: cls_augment.exp_poly, the Horner sequence over 1 / k!, k = 13 .. 0
__device__ __forceinline__ double saug_exp(double t) {
  double r = 1.0 / 6227020800.0;
  r = r * t + 1.0 / 479001600.0; r = r * t + 1.0 / 39916800.0; r = r * t + 1.0 / 3628800.0; r = r * t + 1.0 / 362880.0; r = r * t + 1.0 / 40320.0;
  r = r * t + 1.0 / 5040.0; r = r * t + 1.0 / 720.0; r = r * t + 1.0 / 120.0; r = r * t + 1.0 / 24.0; r = r * t + 1.0 / 6.0; r = r * t + 1.0 / 2.0;
  r = r * t + 1.0; r = r * t + 1.0;
  return r;
}

// sin(pi x), |x| < 2^30: seg_augment.sin_pi -- x = n + r, t = pi r, Horner over (-1)^k / (2k + 1)!, k = 11 .. 0, in t^2, times t, negated for odd n
__device__ __forceinline__ double saug_sinpi(double x) {
  const double n = rint(x);
  const double t = SAUG_PI * (x - n), t2 = t * t;
  double p = -0x1.761b413163819p-75;
  p = p * t2 + 0x1.71b8ef6dcf572p-66; p = p * t2 + -0x1.2f49b46814157p-57; p = p * t2 + 0x1.952c77030ad4ap-49; p = p * t2 + -0x1.ae7f3e733b81fp-41;
  p = p * t2 + 0x1.6124613a86d09p-33; p = p * t2 + -0x1.ae64567f544e4p-26; p = p * t2 + 0x1.71de3a556c734p-19; p = p * t2 + -0x1.a01a01a01a01ap-13;
  p = p * t2 + 0x1.1111111111111p-7; p = p * t2 + -0x1.5555555555555p-3; p = p * t2 + 1.0;
  const double s = p * t;
  return ((int)n & 1) ? -s : s;
}
__device__ __forceinline__ double saug_sinc(double v) { return v == 0.0 ? 1.0 : saug_sinpi(v) / (v * SAUG_PI); }

__device__ __forceinline__ int saug_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int saug_pad(int crop, int side) { return max(0, (1 + crop - side) >> 1); }          // RandomCrop: max(0, int((1 + crop - side) / 2))

__global__ __launch_bounds__(64) void k_saug_plan(const int* __restrict__ sizes, int n, int cw, int ch, double l0, double l1, int flip_first,
                                                  const int64_t* __restrict__ state, int* __restrict__ plan) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint64_t seed = (uint64_t)state[0], ord = (uint64_t)state[1] + (uint64_t)i;
  uint32_t w[4];
  saug_philox((uint32_t)ord, (uint32_t)(ord >> 32), 0u, SAUG_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const int h0 = sizes[2 * i], w0 = sizes[2 * i + 1];
  const double u = (double)(w[0] >> 8) * 5.9604644775390625e-08;          // 2^-24
  const double s = saug_exp(l0 + u * (l1 - l0));                           // RandomScale
  const int rw = (int)fmin(fmax(rint((double)w0 * s), 1.0), (double)FROST_SAUG_MAX_GRID);          // rint: half to even, as Python's round
  const int rh = (int)fmin(fmax(rint((double)h0 * s), 1.0), (double)FROST_SAUG_MAX_GRID);
  const int pw = saug_pad(cw, rw), ph = saug_pad(ch, rh);                 // RandomCrop: pad, then a uniform window of the padded grid
  const int oy = (int)(((uint64_t)w[1] * (uint32_t)(rh + 2 * ph - ch + 1)) >> 32) - ph;
  const int ox = (int)(((uint64_t)w[2] * (uint32_t)(rw + 2 * pw - cw + 1)) >> 32) - pw;
  const int flags = FROST_SAUG_F_LANCZOS | (flip_first ? FROST_SAUG_F_FLIP_FIRST : 0) | ((w[3] >> 31) != 0u ? FROST_SAUG_F_MIRROR : 0);          // RandomFlip
  int* rec = plan + (int64_t)i * FROST_SAUG_PLAN_WORDS;
  rec[FROST_SAUG_FLAGS] = flags; rec[FROST_SAUG_RW] = rw; rec[FROST_SAUG_RH] = rh; rec[FROST_SAUG_OX] = ox; rec[FROST_SAUG_OY] = oy;
  rec[FROST_SAUG_PADW] = pw; rec[FROST_SAUG_PADH] = ph; rec[7] = 0;
}

__global__ void k_saug_advance(int64_t* state, int n) { state[1] += n; }

__global__ __launch_bounds__(64) void k_saug_eval_plan(const int* __restrict__ sizes, int n, int cw, int ch, int* __restrict__ plan) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int* rec = plan + (int64_t)i * FROST_SAUG_PLAN_WORDS;
  rec[FROST_SAUG_FLAGS] = cw > 0 ? FROST_SAUG_F_TRIANGLE : 0;
  rec[FROST_SAUG_RW] = cw > 0 ? cw : sizes[2 * i + 1];
  rec[FROST_SAUG_RH] = cw > 0 ? ch : sizes[2 * i];
  for (int k = FROST_SAUG_OX; k < FROST_SAUG_PLAN_WORDS; ++k) rec[k] = 0;
}

// ---- a plan record, clamped: any plan is memory-safe (a valid plan passes unchanged) ---------------------------------------------------------------------------------
struct SaugRec { int h, w, RW, RH, OX, OY, filt; bool mirror, first; };          // filt: 0 none, 1 Lanczos, 2 triangle
__device__ __forceinline__ SaugRec saug_rec(const int* __restrict__ sizes, const int* __restrict__ plan, int n, int Hmax, int Wmax) {
  const int* rec = plan + (int64_t)n * FROST_SAUG_PLAN_WORDS;
  const int flags = rec[FROST_SAUG_FLAGS];
  SaugRec r;
  r.h = saug_clampi(sizes[2 * n], 1, Hmax); r.w = saug_clampi(sizes[2 * n + 1], 1, Wmax);
  r.filt = (flags & FROST_SAUG_F_TRIANGLE) ? 2 : (flags & FROST_SAUG_F_LANCZOS) ? 1 : 0;
  r.RW = r.filt ? saug_clampi(rec[FROST_SAUG_RW], 1, FROST_SAUG_MAX_GRID) : r.w;
  r.RH = r.filt ? saug_clampi(rec[FROST_SAUG_RH], 1, FROST_SAUG_MAX_GRID) : r.h;
  r.OX = saug_clampi(rec[FROST_SAUG_OX], -FROST_SAUG_MAX_GRID, FROST_SAUG_MAX_GRID);
  r.OY = saug_clampi(rec[FROST_SAUG_OY], -FROST_SAUG_MAX_GRID, FROST_SAUG_MAX_GRID);
  r.mirror = (flags & FROST_SAUG_F_MIRROR) != 0; r.first = (flags & FROST_SAUG_F_FLIP_FIRST) != 0;
  return r;
}

// ---- Pillow's nearest-neighbour index table (ImagingScaleAffine): xo = a / 2; idx[x] = (int) xo; xo += a -- accumulated, NOT (int)((x + 0.5) a) ------------------------
// One workgroup of one wave per (image, axis).  Lane 0 runs the serial accumulation: the entries in front of the window are additions alone (unrolled by eight, the
// chain's latency is what they cost), the window's entries go into LDS; all lanes fill the padding in front of it and write the table out behind it, coalesced.
// (One lane per (image, axis) inside ONE wave, each storing into its own table in global memory, took 256 us at the Cityscapes grid: 64 cache lines per store.)
__global__ __launch_bounds__(64) void k_saug_tables(const int* __restrict__ sizes, const int* __restrict__ plan, int Hmax, int Wmax, int cw, int ch,
                                                    int* __restrict__ tables) {
  __shared__ int tab[FROST_AUG_MAX_SIZE];
  const int img = blockIdx.x >> 1, axis = blockIdx.x & 1, tid = threadIdx.x;          // axis 0: columns, 1: rows
  const SaugRec r = saug_rec(sizes, plan, img, Hmax, Wmax);
  const int n_in = axis ? r.h : r.w, n_out = axis ? r.RH : r.RW, off = axis ? r.OY : r.OX, c = axis ? ch : cw;
  int* out = tables + (int64_t)img * (cw + ch) + (axis ? cw : 0);
  const bool rev_out = !axis && r.mirror && !r.first, rev_src = !axis && r.mirror && r.first;
  for (int j = tid; j < c; j += 64) tab[j] = -1;                     // the window's entries outside the grid stay padding
  __syncthreads();
  if (tid == 0) {
    const double a = (double)n_in / (double)n_out;
    double xo = 0.5 * a;
    const int last = min(n_out, off + c), skip = min(max(off, 0), max(last, 0));
    int g = 0;
    for (; g + 8 <= skip; g += 8) { xo = xo + a; xo = xo + a; xo = xo + a; xo = xo + a; xo = xo + a; xo = xo + a; xo = xo + a; xo = xo + a; }
    for (; g < skip; ++g) xo = xo + a;
    for (; g < last; ++g) {
      const int v = min((int)xo, n_in - 1), j = g - off;
      tab[rev_out ? c - 1 - j : j] = rev_src ? n_in - 1 - v : v;
      xo = xo + a;
    }
  }
  __syncthreads();
  for (int j = tid; j < c; j += 64) out[j] = tab[j];
}

// ---- Pillow's precompute_coeffs, one axis ----------------------------------------------------------------------------------------------------------------------------
struct SaugAxis { double scale, support, ss; int in, taps; bool lanczos; };
__device__ __forceinline__ SaugAxis saug_axis(int in, int out, int filt) {
  SaugAxis a;
  a.in = in; a.lanczos = filt == 1;
  a.scale = (double)in / (double)out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = a.lanczos ? 3.0 * fs : fs; a.ss = 1.0 / fs;
  a.taps = (int)fmin(ceil(a.support), 1.0e6) * 2 + 1;
  return a;
}
// output index xx: the first source index, the number of taps, the centre
__device__ __forceinline__ void saug_bounds(const SaugAxis& a, int xx, int& xmin, int& cnt, double& center) {
  center = ((double)xx + 0.5) * a.scale;
  xmin = (int)fmin(center - a.support + 0.5, (double)a.in);          // the C cast: towards zero (a valid index never reaches the fmin)
  if (xmin < 0) xmin = 0;
  int xmax = (int)fmin(center + a.support + 0.5, (double)a.in);
  if (xmax > a.in) xmax = a.in;
  cnt = max(xmax - xmin, 0);
}
__device__ __forceinline__ double saug_weight(const SaugAxis& a, int x, int xmin, double center) {
  const double v = ((double)(x + xmin) - center + 0.5) * a.ss;
  if (a.lanczos) return (v >= -3.0 && v < 3.0) ? saug_sinc(v) * saug_sinc(v / 3.0) : 0.0;
  const double t = fabs(v);
  return t < 1.0 ? 1.0 - t : 0.0;
}
__device__ __forceinline__ double saug_wsum(const SaugAxis& a, int xmin, int cnt, double center) {
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww = ww + saug_weight(a, x, xmin, center);          // ascending x, as Pillow sums
  return ww;
}
__device__ __forceinline__ int saug_coef(double w, double ww) {
  if (ww != 0.0) w = w / ww;
  return w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);          // normalize_coeffs_8bpc: 2^22, a negative weight rounds away from zero too
}
__device__ __forceinline__ int saug_clip8(int acc) { return min(max(acc >> SAUG_BITS, 0), 255); }

// The SAUG_K coefficients of one output index into LDS at stride `stride`, zeros behind the last tap; `rev`: in reverse tap order (the mirrored source).
__device__ __forceinline__ void saug_coefs_to_lds(const SaugAxis& a, int xmin, int cnt, double center, bool rev, int* dst, int stride) {
  double wt[SAUG_K], ww = 0.0;
#pragma unroll
  for (int t = 0; t < SAUG_K; ++t) {
    wt[t] = t < cnt ? saug_weight(a, t, xmin, center) : 0.0;
    ww = ww + wt[t];                                                 // (a zero behind the last tap changes nothing)
  }
#pragma unroll
  for (int t = 0; t < SAUG_K; ++t) {
    if (t < cnt) dst[(rev ? cnt - 1 - t : t) * stride] = saug_coef(wt[t], ww);
    else dst[t * stride] = 0;
  }
}

// NT consecutive source pixels (3 NT bytes from byte `goff` of the batch) times their coefficients, read as ALIGNED dwords shifted into place by v_alignbyte.  The
// caller guarantees that `base` is 4-byte aligned and that goff + 48 does not pass the end of the batch.  coef: this column's coefficients, twp words apart.
template <int NT>
__device__ __forceinline__ void saug_hrow(const uint8_t* __restrict__ base, int64_t goff, const int* coef, int twp, int& a0, int& a1, int& a2) {
  constexpr int ND = (NT * 3 + 3) / 4;
  const uint32_t* p = (const uint32_t*)(base + (goff & ~(int64_t)3));
  const uint32_t sh = (uint32_t)goff & 3u;
  uint32_t d[ND + 1], w[ND];
#pragma unroll
  for (int k = 0; k <= ND; ++k) d[k] = p[k];
#pragma unroll
  for (int k = 0; k < ND; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = coef[t * twp];
    a0 += (int)((w[(3 * t) >> 2] >> (8 * ((3 * t) & 3))) & 255u) * c;
    a1 += (int)((w[(3 * t + 1) >> 2] >> (8 * ((3 * t + 1) & 3))) & 255u) * c;
    a2 += (int)((w[(3 * t + 2) >> 2] >> (8 * ((3 * t + 2) & 3))) & 255u) * c;
  }
}

template <bool CL, bool VEC>
__device__ __forceinline__ void saug_store4(float* __restrict__ x, int n, int yy, int xq, int cw, int ch, const float* out) {          // out[k]: pixel k / 3, channel k % 3
  if (CL) {
    float* o = x + (((int64_t)n * ch + yy) * cw + xq) * 3;
    if (VEC) {
      ((float4*)o)[0] = make_float4(out[0], out[1], out[2], out[3]);
      ((float4*)o)[1] = make_float4(out[4], out[5], out[6], out[7]);
      ((float4*)o)[2] = make_float4(out[8], out[9], out[10], out[11]);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) if (xq + k / 3 < cw) o[k] = out[k];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = x + (((int64_t)n * 3 + c) * ch + yy) * cw + xq;
      if (VEC) *(float4*)o = make_float4(out[c], out[3 + c], out[6 + c], out[9 + c]);
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (xq + k < cw) o[k] = out[3 * k + c];
      }
    }
  }
}

template <bool CL, bool VEC>
__global__ __launch_bounds__(SAUG_T) void k_saug_apply(const uint8_t* __restrict__ images, const int* __restrict__ sizes, const int* __restrict__ plan, int N, int Hmax,
                                                       int Wmax, int cw, int ch, int nchunk, float m0, float m1, float m2, float d0, float d1, float d2,
                                                       float* __restrict__ x) {
  // LDS, sized by the host for the chunk width twp = min(round_up(cw, 4), SAUG_TW): at 256 columns 39 712 bytes, four workgroups per CU
  extern __shared__ __attribute__((aligned(16))) uint8_t saug_lds[];
  const int twp = min((cw + 3) & ~3, SAUG_TW);
  uint8_t* tile = saug_lds;                                         // [SAUG_ROWS][twp][3]: a multiple of 16 bytes
  float* lut = (float*)(tile + SAUG_ROWS * twp * 3);                // [3][256]
  int* hmin = (int*)(lut + 3 * 256);                                // [twp]: the first source column of the taps, -1 = padding
  int* hco = hmin + twp;                                            // [SAUG_K][twp], tap-major: the lanes of a wave read consecutive words
  int* vmin = hco + SAUG_K * twp;                                   // [SAUG_BR]: the first tile row of the taps, -1 = padding
  int* vco = vmin + SAUG_BR;                                        // [SAUG_BR][SAUG_K]
  const int n = blockIdx.y, tid = threadIdx.x;
  const int band = blockIdx.x / nchunk, chunk = blockIdx.x - band * nchunk;
  const int y0 = band * SAUG_BR, nr = min(SAUG_BR, ch - y0), c0 = chunk * SAUG_TW, tw = min(SAUG_TW, cw - c0);
  const SaugRec R = saug_rec(sizes, plan, n, Hmax, Wmax);
  const int W = R.w, H = R.h;
  const bool rev_out = R.mirror && !R.first, rev_src = R.mirror && R.first;
  const int64_t slot_bytes = (int64_t)Hmax * Wmax * 3, img0 = (int64_t)n * slot_bytes;
  const uint8_t* img = images + img0;
  const int pitch = Wmax * 3;
  const int64_t dword_end = ((uintptr_t)images & 3u) == 0 ? (int64_t)N * slot_bytes - 48 : -1;          // the last byte offset saug_hrow may start at

  for (int i = tid; i < 3 * 256; i += SAUG_T) {                     // ToTensor + Normalize of every byte value: ((v / 255) - mean) / std, each rounded to fp32
    const int c = i >> 8;
    const float m = c == 0 ? m0 : c == 1 ? m1 : m2, d = c == 0 ? d0 : c == 1 ? d1 : d2;
    lut[i] = ((float)(i & 255) / 255.0f - m) / d;
  }
  const SaugAxis ax = saug_axis(W, R.RW, R.filt), ay = saug_axis(H, R.RH, R.filt);
  const int gya = max(R.OY + y0, 0), gyb = min(R.OY + y0 + nr - 1, R.RH - 1);          // the band's rows inside the grid
  int rlo = 0, nrows = 0;
  if (gya <= gyb) {
    int a, b, cnt; double ctr;
    saug_bounds(ay, gya, a, cnt, ctr);
    saug_bounds(ay, gyb, b, cnt, ctr);
    rlo = a; nrows = b + cnt - a;                                   // the bounds grow with the index: the band reads source rows rlo .. rlo + nrows - 1
  }
  const bool lds_path = gya > gyb || (ax.taps <= SAUG_K && ay.taps <= SAUG_K && nrows >= 1 && nrows <= SAUG_ROWS);          // workgroup-uniform

  if (lds_path) {
    // ---- coefficients, once per workgroup
    for (int j = tid; j < tw; j += SAUG_T) {
      const int gx = R.OX + (rev_out ? cw - 1 - (c0 + j) : c0 + j);          // the grid column that output column c0 + j shows
      if (gx < 0 || gx >= R.RW || gya > gyb) hmin[j] = -1;
      else {
        int xmin, cnt; double ctr;
        saug_bounds(ax, gx, xmin, cnt, ctr);
        hmin[j] = rev_src ? W - xmin - cnt : xmin;                  // the taps of the mirrored source are columns W - 1 - xmin down to W - xmin - cnt of the source
        saug_coefs_to_lds(ax, xmin, cnt, ctr, rev_src, hco + j, twp);
      }
    }
    {
      const int i = SAUG_T - 1 - tid;                               // the last lanes: the first ones may still be busy with a column
      if (i < nr) {
        const int gy = R.OY + y0 + i;
        if (gy < 0 || gy >= R.RH) vmin[i] = -1;
        else {
          int ymin, cnt; double ctr;
          saug_bounds(ay, gy, ymin, cnt, ctr);
          vmin[i] = ymin - rlo;
          saug_coefs_to_lds(ay, ymin, cnt, ctr, false, vco + i * SAUG_K, 1);
        }
      }
    }
    __syncthreads();
    // ---- horizontal pass: source rows rlo .. -> the uint8 tile
    const int kx = ax.taps, ky = ay.taps;
    for (int item = tid; item < nrows * tw; item += SAUG_T) {
      const int r = item / tw, j = item - r * tw;
      const int xm = hmin[j];
      uint8_t* o = tile + (r * twp + j) * 3;
      if (xm < 0) { o[0] = 0; o[1] = 0; o[2] = 0; continue; }       // padding: the source is not touched
      const int64_t roff = (int64_t)min(rlo + r, H - 1) * pitch;
      const uint8_t* row = img + roff;
      int a0 = 1 << (SAUG_BITS - 1), a1 = a0, a2 = a0;
      const int64_t goff = img0 + roff + xm * 3;
      if (goff <= dword_end) {                                       // all but the last few pixels of the batch
        if (kx <= 7) saug_hrow<7>(images, goff, hco + j, twp, a0, a1, a2);
        else saug_hrow<SAUG_K>(images, goff, hco + j, twp, a0, a1, a2);
      } else for (int t = 0; t < kx; ++t) {
        const int c = hco[t * twp + j];
        const uint8_t* p = row + min(xm + t, W - 1) * 3;             // a tap behind the last one has coefficient 0: its (clamped) pixel does not count
        a0 += (int)p[0] * c; a1 += (int)p[1] * c; a2 += (int)p[2] * c;
      }
      o[0] = (uint8_t)saug_clip8(a0); o[1] = (uint8_t)saug_clip8(a1); o[2] = (uint8_t)saug_clip8(a2);
    }
    __syncthreads();
    // ---- vertical pass out of the tile, the table, the stores: four output pixels of one row per thread
    const int nq = (tw + 3) >> 2;
    for (int item = tid; item < nr * nq; item += SAUG_T) {
      const int i = item / nq, q = item - i * nq;
      const int r0 = vmin[i];
      float out[12];                                                // byte k of the 12: pixel k / 3, channel k % 3
      if (r0 < 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = lut[(k % 3) * 256];   // a padded row
      } else {
        int acc[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] = 1 << (SAUG_BITS - 1);
        for (int t = 0; t < ky; ++t) {
          const int c = vco[i * SAUG_K + t];
          const uint32_t* p = (const uint32_t*)(tile + (min(r0 + t, nrows - 1) * twp + 4 * q) * 3);          // 12 bytes at a multiple of 12
          const uint32_t u0 = p[0], u1 = p[1], u2 = p[2];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] += (int)((u0 >> (8 * k)) & 255u) * c; acc[4 + k] += (int)((u1 >> (8 * k)) & 255u) * c; acc[8 + k] += (int)((u2 >> (8 * k)) & 255u) * c;
          }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = lut[(k % 3) * 256 + saug_clip8(acc[k])];
      }
      saug_store4<CL, VEC>(x, n, y0 + i, c0 + 4 * q, cw, ch, out);
    }
    return;
  }

  // ---- the general path: any scale.  One thread per output pixel, every coefficient recomputed where it is used.
  __syncthreads();          // the table
  for (int item = tid; item < nr * tw; item += SAUG_T) {
    const int i = item / tw, j = item - i * tw;
    const int gx = R.OX + (rev_out ? cw - 1 - (c0 + j) : c0 + j), gy = R.OY + y0 + i;
    int v0 = 0, v1 = 0, v2 = 0;                                      // padding
    if (gx >= 0 && gx < R.RW && gy >= 0 && gy < R.RH) {
      int xmin, xcnt, ymin, ycnt; double xc, yc;
      saug_bounds(ax, gx, xmin, xcnt, xc);
      saug_bounds(ay, gy, ymin, ycnt, yc);
      const double xww = saug_wsum(ax, xmin, xcnt, xc), yww = saug_wsum(ay, ymin, ycnt, yc);
      v0 = v1 = v2 = 1 << (SAUG_BITS - 1);
      for (int ty = 0; ty < ycnt; ++ty) {
        const int cy = saug_coef(saug_weight(ay, ty, ymin, yc), yww);
        const uint8_t* row = img + (int64_t)min(ymin + ty, H - 1) * pitch;
        int a0 = 1 << (SAUG_BITS - 1), a1 = a0, a2 = a0;
        for (int tx = 0; tx < xcnt; ++tx) {
          const int cx = saug_coef(saug_weight(ax, tx, xmin, xc), xww);
          const int sx = min(xmin + tx, W - 1);
          const uint8_t* p = row + (rev_src ? W - 1 - sx : sx) * 3;
          a0 += (int)p[0] * cx; a1 += (int)p[1] * cx; a2 += (int)p[2] * cx;
        }
        v0 += saug_clip8(a0) * cy; v1 += saug_clip8(a1) * cy; v2 += saug_clip8(a2) * cy;          // the uint8 intermediate
      }
      v0 = saug_clip8(v0); v1 = saug_clip8(v1); v2 = saug_clip8(v2);
    }
    const float o0 = lut[v0], o1 = lut[256 + v1], o2 = lut[512 + v2];
    const int yy = y0 + i, xx = c0 + j;
    if (CL) {
      float* o = x + (((int64_t)n * ch + yy) * cw + xx) * 3;
      o[0] = o0; o[1] = o1; o[2] = o2;
    } else {
      float* o = x + ((int64_t)n * 3 * ch + yy) * cw + xx;
      o[0] = o0; o[(int64_t)ch * cw] = o1; o[(int64_t)2 * ch * cw] = o2;
    }
  }
}

// ---- the label map: a gather through the two index tables, four output pixels of one row per thread --------------------------------------------------------------------
template <bool I64, bool VEC>
__global__ __launch_bounds__(SAUG_T) void k_saug_labels(const uint8_t* __restrict__ labels, const int* __restrict__ tables, int Hmax, int Wmax, int cw, int ch, int ignore,
                                                        void* __restrict__ target) {
  const int n = blockIdx.y, nq = (cw + 3) >> 2;
  const int item = blockIdx.x * SAUG_T + threadIdx.x;
  if (item >= ch * nq) return;
  const int y = item / nq, xq = (item - y * nq) * 4;
  const int* xt = tables + (int64_t)n * (cw + ch);
  const int ty = min(xt[cw + y], Hmax - 1);
  const uint8_t* row = labels + ((int64_t)n * Hmax + max(ty, 0)) * Wmax;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int tx = xq + k < cw ? min(xt[xq + k], Wmax - 1) : -1;
    v[k] = (ty < 0 || tx < 0) ? ignore : (int)row[tx];
  }
  const int64_t o = ((int64_t)n * ch + y) * cw + xq;
  if (I64) {
    int64_t* t = (int64_t*)target + o;
    if (VEC) { ((longlong2*)t)[0] = make_longlong2(v[0], v[1]); ((longlong2*)t)[1] = make_longlong2(v[2], v[3]); }
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (xq + k < cw) t[k] = v[k];
    }
  } else {
    uint8_t* t = (uint8_t*)target + o;
    if (VEC) *(uint32_t*)t = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (xq + k < cw) t[k] = (uint8_t)v[k];
    }
  }
}

extern "C" int frost_saug_plan_words(void) { return FROST_SAUG_PLAN_WORDS; }

extern "C" int frost_saug_plan(const int32_t* sizes, int n, int crop_w, int crop_h, double log_scale_lo, double log_scale_hi, int flip_first, int64_t* state,
                               int32_t* plan, void* stream) {
  FROST_REQUIRE(sizes && state && plan, "saug_plan: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "saug_plan: n outside 1 .. 65535");
  FROST_REQUIRE(crop_w >= 1 && crop_w <= FROST_AUG_MAX_SIZE && crop_h >= 1 && crop_h <= FROST_AUG_MAX_SIZE, "saug_plan: crop side outside 1 .. 4096");
  FROST_REQUIRE(log_scale_lo >= -0.6931471805599454 && log_scale_lo <= log_scale_hi && log_scale_hi <= 0.6931471805599454, "saug_plan: scale bounds out of order or outside 1/2 .. 2");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_saug_plan, dim3((n + 63) / 64), dim3(64), 0, s, sizes, n, crop_w, crop_h, log_scale_lo, log_scale_hi, flip_first, (const int64_t*)state, plan);
  hipLaunchKernelGGL(k_saug_advance, dim3(1), dim3(1), 0, s, state, n);
  return frost_check_launch("saug_plan");
}

extern "C" int frost_saug_eval_plan(const int32_t* sizes, int n, int crop_w, int crop_h, int32_t* plan, void* stream) {
  FROST_REQUIRE(sizes && plan, "saug_eval_plan: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "saug_eval_plan: n outside 1 .. 65535");
  FROST_REQUIRE((crop_w == 0 && crop_h == 0) || (crop_w >= 1 && crop_w <= FROST_AUG_MAX_SIZE && crop_h >= 1 && crop_h <= FROST_AUG_MAX_SIZE),
                "saug_eval_plan: size is 0 x 0 (none) or each side in 1 .. 4096");
  hipLaunchKernelGGL(k_saug_eval_plan, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), sizes, n, crop_w, crop_h, plan);
  return frost_check_launch("saug_eval_plan");
}

extern "C" int frost_saug_apply(const uint8_t* images, const uint8_t* labels, const int32_t* sizes, const int32_t* plan, int n, int hmax, int wmax, int crop_w,
                                int crop_h, float mean0, float mean1, float mean2, float std0, float std1, float std2, int ignore_idx, int channels_last,
                                int target_int64, int parts, int32_t* tables, float* x, void* target, void* stream) {
  FROST_REQUIRE(sizes && plan && parts >= 1 && parts <= 7, "saug_apply: incomplete arguments, or parts outside 1 .. 7");
  FROST_REQUIRE((!(parts & 5) || tables) && (!(parts & 2) || (images && x)) && (!(parts & 4) || (labels && target)), "saug_apply: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535, "saug_apply: n outside 1 .. 65535");
  FROST_REQUIRE(crop_w >= 1 && crop_w <= FROST_AUG_MAX_SIZE && crop_h >= 1 && crop_h <= FROST_AUG_MAX_SIZE, "saug_apply: crop side outside 1 .. 4096");
  FROST_REQUIRE(hmax >= 1 && wmax >= 1 && (int64_t)hmax * wmax * 3 <= INT32_MAX, "saug_apply: Hmax / Wmax below 1, or a slot above 2^31 bytes");
  FROST_REQUIRE(std0 != 0.0f && std1 != 0.0f && std2 != 0.0f, "saug_apply: a std of zero");
  FROST_REQUIRE(ignore_idx >= 0 && ignore_idx <= 255, "saug_apply: ignore_idx outside 0 .. 255");
  hipStream_t s = as_stream(stream);
  if (parts & 1) hipLaunchKernelGGL(k_saug_tables, dim3(2 * n), dim3(64), 0, s, sizes, plan, hmax, wmax, crop_w, crop_h, tables);
  if (parts & 2) {
    const int nchunk = (crop_w + SAUG_TW - 1) / SAUG_TW, nband = (crop_h + SAUG_BR - 1) / SAUG_BR;
    const dim3 grid(nband * nchunk, n), block(SAUG_T);
    const int twp = crop_w + 3 < SAUG_TW ? (crop_w + 3) & ~3 : SAUG_TW;
    const size_t lds = (size_t)SAUG_ROWS * twp * 3 + 3 * 256 * 4 + (size_t)(1 + SAUG_K) * twp * 4 + SAUG_BR * (1 + SAUG_K) * 4;
    const bool vec = crop_w % 4 == 0 && ((uintptr_t)x & 15u) == 0;          // 16-byte stores need rows of whole float4s
#define SAUG_LAUNCH(CL, VEC) \
    hipLaunchKernelGGL((k_saug_apply<CL, VEC>), grid, block, lds, s, images, sizes, plan, n, hmax, wmax, crop_w, crop_h, nchunk, mean0, mean1, mean2, std0, std1, std2, x)
    if (channels_last) { if (vec) SAUG_LAUNCH(true, true); else SAUG_LAUNCH(true, false); }
    else { if (vec) SAUG_LAUNCH(false, true); else SAUG_LAUNCH(false, false); }
#undef SAUG_LAUNCH
  }
  if (parts & 4) {
    const int items = crop_h * ((crop_w + 3) / 4);
    const dim3 grid((items + SAUG_T - 1) / SAUG_T, n), block(SAUG_T);
    const bool vec = crop_w % 4 == 0 && ((uintptr_t)target & (target_int64 ? 15u : 3u)) == 0;
#define SAUG_LABELS(I64, VEC) hipLaunchKernelGGL((k_saug_labels<I64, VEC>), grid, block, 0, s, labels, (const int*)tables, hmax, wmax, crop_w, crop_h, ignore_idx, target)
    if (target_int64) { if (vec) SAUG_LABELS(true, true); else SAUG_LABELS(true, false); }
    else { if (vec) SAUG_LABELS(false, true); else SAUG_LABELS(false, false); }
#undef SAUG_LABELS
  }
  return frost_check_launch("saug_apply");
}

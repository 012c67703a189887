// SSD Detect layer on the device: softmax, box decoding, per-class top-k selection and greedy NMS -- two kernels, no host synchronisation, no data-dependent
// launch shape (the torch form gathers by boolean mask once per image and class: N * (C - 1) synchronisations per batch, not capturable).
//
// replaces: Object_Detection/ssd_qmv2.py:290-292,320-327 (nn.Softmax + Detect in the test phase), Object_Detection/layers/functions/detection.py:14-66 (Detect)
// with layers/box_utils.py:140-158 (decode) and the IoU rule of torchvision.ops.nms, as restated batched by frostnet_amd/ssdlite.py::Detect.forward_torch (the
// CPU definition and the parity yardstick: tests/test_gpu_detect_post.py).  Per image n and class c != bkg:
//   * s_p = softmax(conf[n, p, :])[c] (max-shifted, fp32); box_p = decode(loc[n, p], prior_p): cxcy = p.cxcy + l.xy * v0 * p.wh, wh = p.wh * exp(l.wh * v1),
//     x1y1 = cxcy - wh / 2, x2y2 = wh + x1y1;
//   * candidates: s_p > conf_thresh (a NaN score never is one); ordered by score descending, equal scores by the LOWER prior index first; the first top_k stay;
//   * greedy NMS in that order on box * min_dim: a candidate is kept iff IoU <= nms_thresh against every earlier kept box, IoU = inter / (area_a + area_b - inter)
//     with the intersection's width / height clamped at 0;
//   * out[n, c, r] = (score, x1, y1, x2, y2) of the r-th kept candidate (unscaled box), every other row 0; counts[n, c] = number of kept rows.
// detection.py:68-71 (a cross-class rank filter written into a temporary) has no effect in the reference and is not reproduced.
#include "frost_common.h"
#include <math.h>

#define DET_TP 256            // priors per workgroup of the score / decode pass (one lane per prior)
#define DET_T 512             // threads of the select + NMS workgroup
#define DET_MAXK 512          // top_k cap: one thread per candidate, 8 ballot words per suppression row
#define DET_MAXW (DET_MAXK / 64)

// ---- pass 1: softmax + decode.  conf rows (C floats: not a power of two) are staged through LDS so the global reads are unit-stride; scores are written
// class-major [N][C][P] so the selection reads them unit-stride; the decoded box once per prior
__global__ __launch_bounds__(DET_TP) void k_det_score(const float* __restrict__ loc, const float* __restrict__ conf, const float* __restrict__ priors, int P, int C,
                                                      int bkg, float var0, float var1, int staged, float* __restrict__ scores, float* __restrict__ boxes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* tile = (float*)smem;                                        // [DET_TP][C | 1] (odd row stride: lanes hit distinct banks)
  const int n = blockIdx.y, p0 = blockIdx.x * DET_TP, tid = threadIdx.x, p = p0 + tid;
  const int np = min(DET_TP, P - p0), cs = C | 1;
  const float* src = conf + ((int64_t)n * P + p0) * C;
  if (staged) {
    for (int i = tid; i < np * C; i += DET_TP) tile[(i / C) * cs + (i % C)] = src[i];
    __syncthreads();
  }
  if (p >= P) return;
  const float* row = staged ? (tile + tid * cs) : (src + (int64_t)tid * C);
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
  float s = 0.0f;
  for (int c = 0; c < C; ++c) s += expf(row[c] - m);
  float* sc = scores + (int64_t)n * C * P + p;
  for (int c = 0; c < C; ++c) if (c != bkg) sc[(int64_t)c * P] = expf(row[c] - m) / s;
  const float4 l = *(const float4*)(loc + ((int64_t)n * P + p) * 4), pr = *(const float4*)(priors + (int64_t)p * 4);
  const float cx = pr.x + l.x * var0 * pr.z, cy = pr.y + l.y * var0 * pr.w;
  const float w = pr.z * expf(l.z * var1), h = pr.w * expf(l.w * var1);
  const float x1 = cx - w / 2, y1 = cy - h / 2;
  *(float4*)(boxes + ((int64_t)n * P + p) * 4) = make_float4(x1, y1, w + x1, h + y1);
}

// The order key of a prior: (score bits + 1) << 32 | ~index for a candidate, 0 otherwise.  Scores are >= 0, so their bit patterns order like their values; every key
// of an (image, class) is distinct, and a larger key means "earlier in the detection order" (higher score, then lower prior index)
__device__ __forceinline__ unsigned long long det_key(float s, float thresh, int p) {
  return s > thresh ? (((unsigned long long)(__float_as_uint(s) + 1u)) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p) : 0ull;
}

// wave 0: the bin (from the top) in which the running count reaches `rem`.  ctl[2] = bin, ctl[3] = what is left to take inside it, ctl[4] = total count
__device__ __forceinline__ void det_find_bin(const unsigned* hist, unsigned rem, unsigned* ctl) {
  const int lane = threadIdx.x & 63, b0 = 255 - 4 * lane;
  const unsigned h0 = hist[b0], h1 = hist[b0 - 1], h2 = hist[b0 - 2], h3 = hist[b0 - 3];
  unsigned incl = h0 + h1 + h2 + h3;
  for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  const unsigned long long reach = __ballot(incl >= rem);
  if (lane == 63) ctl[4] = incl;
  if (reach != 0ull && lane == __ffsll((long long)reach) - 1) {
    unsigned r = rem - (incl - (h0 + h1 + h2 + h3));                 // still to take when this lane's four bins begin
    int b = b0;
    if (h0 < r) { r -= h0; b = b0 - 1; if (h1 < r) { r -= h1; b = b0 - 2; if (h2 < r) { r -= h2; b = b0 - 3; } } }
    ctl[2] = (unsigned)b; ctl[3] = r;
  }
}

// ---- pass 2: one workgroup per (image, class): exact top-k by radix select on the 64-bit order keys, rank sort in LDS, suppression matrix as ballot words, greedy
// scan in one wave, kept rows + count.  out rows past the count (and the whole background plane) are written as zeros here: the caller need not clear `out`
__global__ __launch_bounds__(DET_T) void k_det_select_nms(const float* __restrict__ scores, const float* __restrict__ boxes, int P, int C, int bkg, int top_k,
                                                          float conf_thresh, float nms_thresh, float min_dim, float* __restrict__ out, int* __restrict__ counts) {
  __shared__ unsigned long long ckey[DET_MAXK];                      // compacted keys, then reused as nothing else
  __shared__ unsigned long long skey[DET_MAXK];                      // sorted (descending)
  __shared__ float4 sbox[DET_MAXK];                                  // boxes * min_dim in detection order
  __shared__ unsigned long long supp[DET_MAXK * DET_MAXW];           // supp[i][w]: candidates j > i (bit j - 64 w) that candidate i suppresses
  __shared__ unsigned long long gone[DET_MAXW];                      // result of the scan: suppressed candidates
  __shared__ unsigned hist[256];
  __shared__ unsigned ctl[8];                                        // {slot counter, -, bin, left in bin, total}
  const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* o = out + ((int64_t)n * C + c) * top_k * 5;
  int kept_n = 0, K = 0;
  if (c != bkg) {
    const float* sc = scores + ((int64_t)n * C + c) * P;
    // -- exact threshold key: 8-bit digits from the top; ends as soon as a digit's bin is taken whole
    unsigned long long prefix = 0ull, himask = 0ull;
    unsigned rem = 0u;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      for (int i = tid; i < 256; i += DET_T) hist[i] = 0u;
      __syncthreads();
      for (int p = tid; p < P; p += DET_T) {
        const unsigned long long k = det_key(sc[p], conf_thresh, p);
        if (k != 0ull && (k & himask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (pass == 0) {                                               // number of candidates -> K
        if (wave == 0) det_find_bin(hist, 0xffffffffu, ctl);
        __syncthreads();
        K = min((unsigned)top_k, ctl[4]);
        rem = (unsigned)K;
        __syncthreads();
        if (K == 0) break;
      }
      if (wave == 0) det_find_bin(hist, rem, ctl);
      __syncthreads();
      const unsigned b = ctl[2], left = ctl[3], inbin = hist[b];
      prefix |= (unsigned long long)b << shift;
      himask |= 255ull << shift;
      rem = left;
      __syncthreads();
      if (inbin == left) break;                                      // the whole bin belongs to the top K: every key >= prefix is selected
    }
    if (K > 0) {
      // -- compact the K selected keys (any order: the sort below fixes it), then rank sort: distinct keys, rank = number of larger keys
      if (tid == 0) ctl[0] = 0u;
      __syncthreads();
      for (int p = tid; p < P; p += DET_T) {
        const unsigned long long k = det_key(sc[p], conf_thresh, p);
        if (k != 0ull && k >= prefix) { const unsigned s = atomicAdd(&ctl[0], 1u); if (s < (unsigned)K) ckey[s] = k; }
      }
      __syncthreads();
      if (tid < K) {
        const unsigned long long mine = ckey[tid];
        int r = 0;
        for (int j = 0; j < K; ++j) r += ckey[j] > mine ? 1 : 0;
        skey[r] = mine;
      }
      __syncthreads();
      float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
      float score = 0.0f;
      if (tid < K) {
        const unsigned long long k = skey[tid];
        const unsigned p = 0xffffffffu - (unsigned)(k & 0xffffffffull);
        score = __uint_as_float((unsigned)(k >> 32) - 1u);
        bx = *(const float4*)(boxes + ((int64_t)n * P + p) * 4);
        sbox[tid] = make_float4(bx.x * min_dim, bx.y * min_dim, bx.z * min_dim, bx.w * min_dim);
      }
      __syncthreads();
      // -- suppression words: one ballot per (row i, word w); lane = candidate j of the word
      const int nw = (K + 63) >> 6;
      for (int q = wave; q < K * nw; q += DET_T / 64) {
        const int i = q / nw, w = q - i * nw, j = w * 64 + lane;
        bool s = false;
        if (j > i && j < K) {
          const float4 a = sbox[i], b = sbox[j];
          const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f), ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
          const float inter = iw * ih;
          const float iou = inter / ((a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y) - inter);
          s = !(iou <= nms_thresh);
        }
        const unsigned long long word = __ballot(s);
        if (lane == 0) supp[i * DET_MAXW + w] = word;
      }
      __syncthreads();
      // -- greedy scan, one wave: lane w holds word w of the suppressed set; K dependent steps, the row loads do not depend on them
      if (wave == 0) {
        unsigned long long g = 0ull;
        for (int i = 0; i < K; ++i) {
          const unsigned long long row = lane < nw ? supp[i * DET_MAXW + lane] : 0ull;
          const unsigned long long gw = __shfl(g, i >> 6);
          if (!((gw >> (i & 63)) & 1ull)) g |= row;
        }
        if (lane < nw) gone[lane] = g;
      }
      __syncthreads();
      for (int w = 0; w < nw; ++w) {
        const int nb = min(64, K - w * 64);
        const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
        kept_n += __popcll(~gone[w] & valid);
      }
      if (tid < K && !((gone[tid >> 6] >> (tid & 63)) & 1ull)) {
        int r = __popcll(~gone[tid >> 6] & ((1ull << (tid & 63)) - 1ull));
        for (int w = 0; w < (tid >> 6); ++w) r += __popcll(~gone[w]);
        float* d = o + r * 5;
        d[0] = score; d[1] = bx.x; d[2] = bx.y; d[3] = bx.z; d[4] = bx.w;
      }
    }
  }
  for (int e = kept_n * 5 + tid; e < top_k * 5; e += DET_T) o[e] = 0.0f;
  if (tid == 0) counts[n * C + c] = kept_n;
}

extern "C" int frost_detect_max_top_k(void) { return DET_MAXK; }
// scores [n][c][p] and boxes [n][p][4]: work buffers of the caller (contents undefined on entry; the background plane of scores is never written or read)
extern "C" int frost_detect_forward(const float* loc, const float* conf, const float* priors, int n, int p, int c, int bkg_label, int top_k, float conf_thresh,
                                    float nms_thresh, float var0, float var1, float min_dim, float* scores, float* boxes, float* out, int32_t* counts, void* stream) {
  FROST_REQUIRE(loc && conf && priors && scores && boxes && out && counts, "detect_forward: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535 && p >= 1 && c >= 2 && c <= 65535 && (int64_t)n * c * p < (int64_t)1 << 40, "detect_forward: bad sizes");
  FROST_REQUIRE(top_k >= 1 && top_k <= DET_MAXK, "detect_forward: top_k outside 1 .. 512");
  FROST_REQUIRE(nms_thresh > 0.0f, "detect_forward: nms_thresh must be positive");
  hipStream_t s = as_stream(stream);
  const size_t lds = (size_t)DET_TP * (size_t)(c | 1) * 4;
  const int staged = lds <= 160 * 1024 ? 1 : 0;                      // wider class rows are read from global memory directly
  static bool set = false;
  if (!set) { (void)hipFuncSetAttribute((const void*)k_det_score, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); set = true; }
  hipLaunchKernelGGL(k_det_score, dim3((p + DET_TP - 1) / DET_TP, n), dim3(DET_TP), staged ? lds : 0, s, loc, conf, priors, p, c, bkg_label, var0, var1, staged, scores, boxes);
  hipLaunchKernelGGL(k_det_select_nms, dim3(c, n), dim3(DET_T), 0, s, scores, boxes, p, c, bkg_label, top_k, conf_thresh, nms_thresh, min_dim, out, counts);
  return frost_check_launch("detect_forward");
}

// PASCAL VOC average precision on the device: the scoring phase of the detection recipe, with the evaluator state in device memory -- no host synchronisation, no
// data-dependent launch shape (the reference copies one masked gather per image and class to the host, writes one text file per class and walks every detection in Python).
//
// replaces: Object_Detection/qeval_convert.py:348-396 (test_net's per-class gather), :211-345 (voc_eval) and :177-208 (voc_ap), as restated by
// frostnet_amd/voc_eval.py::VOCEvaluator on CPU tensors (the definition and the parity yardstick: tests/test_gpu_voc_eval.py).
//   * k_voc_update, one workgroup per (class, image): the image's ground truth of the class compacted into LDS in index order; one thread per detection row (score > 0)
//     scales its box, takes jmax = the first index of the largest fp32 IoU, and is FP (no box, or not IoU > ovthresh), ignored (jmax difficult), or a claimant of jmax;
//     the claim is an LDS atomicMax of the 64-bit record, so the claimant that ranks first in the final order is the TP and the rest are FP.  One global atomicAdd per
//     workgroup reserves the slots of the class row; the records land in arrival order (they are distinct, the sort decides).  The same launch adds npos.
//   * k_voc_advance, one thread behind it on the stream: images seen += n (every workgroup of the update has read the counter by then).
//   * k_voc_ap, one workgroup per class over its row sorted descending: block scan of the TP / FP flags with a carry between chunks, rec / prec in fp64; the 07 metric
//     keeps eleven running maxima and adds them up in order in one thread; the area metric walks back from the end with the suffix maximum of prec.
// record = score bits << 32 | (~ordinal & 0x3FFFFFFF) << 2 | flag (0 ignored, 1 TP, 2 FP), ordinal = image ordinal * top_k + row; an empty slot is 0.
#include "frost_common.h"

#define VOC_T 256             // threads of both kernels
#define VOC_MAXK 1024         // detection rows of one (image, class)
#define VOC_MAXG 1024         // ground-truth rows of one image
#define VOC_ORD_MASK 0x3FFFFFFFull
#define VOC_CURSOR_STOP (1 << 30)   // capacity <= 2^30; a class cursor at or past this is no longer advanced, so it cannot wrap however long updates go on after an overflow

// ctr: int32 words {cursor [C], npos [C], images seen, overflow}
__global__ __launch_bounds__(VOC_T) void k_voc_update(const float* __restrict__ det, const float* __restrict__ gt, const uint8_t* __restrict__ difficult,
                                                      const uint8_t* __restrict__ valid, const float* __restrict__ sizes, int C, int K, int G, int bkg, float ovthresh,
                                                      float offset, int top_k, int max_images, int64_t capacity, unsigned long long* __restrict__ records,
                                                      int* __restrict__ ctr) {
  __shared__ float4 sbox[VOC_MAXG];                                  // the class's boxes of this image, index order
  __shared__ uint8_t sdiff[VOC_MAXG];
  __shared__ unsigned long long claim[VOC_MAXG];                     // per box: the largest record that points at it
  __shared__ int res[VOC_MAXK];                                      // per row: -2 no detection, -1 FP, -3 ignored, j >= 0 claimant of box j
  __shared__ unsigned sh[4];                                         // {boxes of the class, detections, slot base, next slot}
  const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  if (c == bkg) return;
  const int img = ctr[2 * C] + n;
  if (img >= max_images) {                                           // the ordinal field would overflow: drop the image, flag it
    if (tid == 0) atomicOr(&ctr[2 * C + 1], 1);
    return;
  }
  if (tid < 4) sh[tid] = 0u;
  // -- wave 0: compaction in index order, npos
  if (tid < 64) {
    int base = 0, npos = 0;
    for (int g0 = 0; g0 < G; g0 += 64) {
      const int g = g0 + lane;
      bool mine = false, diff = false;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g < G && valid[(int64_t)n * G + g]) {
        const float* row = gt + ((int64_t)n * G + g) * 5;
        const int label = (int)row[4];
        if ((label < bkg ? label : label + 1) == c) { mine = true; diff = difficult[(int64_t)n * G + g] != 0; b = make_float4(row[0], row[1], row[2], row[3]); }
      }
      const unsigned long long m = __ballot(mine);
      if (mine) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        sbox[pos] = b; sdiff[pos] = diff ? 1 : 0; claim[pos] = 0ull;
      }
      base += __popcll(m);
      npos += __popcll(__ballot(mine && !diff));
    }
    if (lane == 0) { sh[0] = (unsigned)base; if (npos) atomicAdd(&ctr[C + c], npos); }
  }
  __syncthreads();
  const int ng = (int)sh[0];
  const float w = sizes ? sizes[2 * n] : 1.0f, h = sizes ? sizes[2 * n + 1] : 1.0f;
  const float* drow = det + ((int64_t)n * C + c) * K * 5;
  // -- one thread per row: jmax, verdict or claim
  int cnt = 0;
  for (int r = tid; r < K; r += VOC_T) {
    const float s = drow[r * 5];
    int v = -2;
    if (s > 0.0f) {
      ++cnt;
      v = -1;
      const float bx1 = drow[r * 5 + 1] * w + offset, by1 = drow[r * 5 + 2] * h + offset, bx2 = drow[r * 5 + 3] * w + offset, by2 = drow[r * 5 + 4] * h + offset;
      const float barea = (bx2 - bx1) * (by2 - by1);
      float best = -INFINITY;
      int jmax = 0;
      for (int j = 0; j < ng; ++j) {
        const float4 g = sbox[j];
        const float iw = fmaxf(fminf(g.z, bx2) - fmaxf(g.x, bx1), 0.0f), ih = fmaxf(fminf(g.w, by2) - fmaxf(g.y, by1), 0.0f);
        const float inter = iw * ih;
        const float iou = inter / (barea + (g.z - g.x) * (g.w - g.y) - inter);
        if (iou > best) { best = iou; jmax = j; }                   // strict: the lowest index wins ties, a NaN never wins
      }
      if (ng > 0 && best > ovthresh) {
        if (sdiff[jmax]) v = -3;
        else {
          v = jmax;
          const unsigned ord = (unsigned)img * (unsigned)top_k + (unsigned)r;
          atomicMax(&claim[jmax], ((unsigned long long)__float_as_uint(s) << 32) | ((~(unsigned long long)ord & VOC_ORD_MASK) << 2));
        }
      }
    }
    res[r] = v;
  }
  if (cnt) atomicAdd(&sh[1], (unsigned)cnt);
  __syncthreads();
  if (tid == 0 && sh[1]) sh[2] = __atomic_load_n(&ctr[c], __ATOMIC_RELAXED) >= VOC_CURSOR_STOP ? (unsigned)VOC_CURSOR_STOP : (unsigned)atomicAdd(&ctr[c], (int)sh[1]);
  __syncthreads();
  const int64_t base = (int64_t)sh[2];
  bool over = false;
  for (int r = tid; r < K; r += VOC_T) {
    const int v = res[r];
    if (v == -2) continue;
    const unsigned ord = (unsigned)img * (unsigned)top_k + (unsigned)r;
    const unsigned long long key = ((unsigned long long)__float_as_uint(drow[r * 5]) << 32) | ((~(unsigned long long)ord & VOC_ORD_MASK) << 2);
    const unsigned long long flag = v == -3 ? 0ull : (v >= 0 && claim[v] == key) ? 1ull : 2ull;
    const int64_t slot = base + (int64_t)atomicAdd(&sh[3], 1u);
    if (slot >= 0 && slot < capacity) records[(int64_t)c * capacity + slot] = key | flag;
    else over = true;
  }
  if (over) atomicOr(&ctr[2 * C + 1], 1);
}

__global__ void k_voc_advance(int* ctr, int C, int n) { ctr[2 * C] += n; }

// inclusive block scan of two counts and one running maximum over VOC_T threads, in thread order
__device__ __forceinline__ void voc_scan(int& a, int& b, double& m, int* wa, int* wb, double* wm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int ta = __shfl_up(a, o), tb = __shfl_up(b, o);
    const double tm = __shfl_up(m, o);
    if (lane >= o) { a += ta; b += tb; m = fmax(m, tm); }
  }
  __syncthreads();                                                   // the previous chunk's readers of wa / wb / wm are done
  if (lane == 63) { wa[wave] = a; wb[wave] = b; wm[wave] = m; }
  __syncthreads();
  for (int i = 0; i < wave; ++i) { a += wa[i]; b += wb[i]; m = fmax(m, wm[i]); }
}

// sorted: [C][capacity] records, descending (empty slots last).  counts: [5][C] int64 {npos, ndet, tp, fp, ignored}
__global__ __launch_bounds__(VOC_T) void k_voc_ap(const unsigned long long* __restrict__ sorted, const int* __restrict__ ctr, int C, int64_t capacity, int bkg,
                                                  int use07, double* __restrict__ ap, int64_t* __restrict__ counts) {
  __shared__ int wa[VOC_T / 64], wb[VOC_T / 64];
  __shared__ double wm[VOC_T / 64];
  __shared__ double red[VOC_T / 64][11];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (c == bkg) {
    if (tid == 0) { ap[c] = __longlong_as_double(0x7ff8000000000000ll); for (int i = 0; i < 5; ++i) counts[(int64_t)i * C + c] = 0; }
    return;
  }
  const unsigned long long* row = sorted + (int64_t)c * capacity;
  const int64_t nd = min((int64_t)ctr[c], capacity);
  const int npos_i = ctr[C + c];
  const double npos = (double)npos_i;
  // -- forward: cumulative tp / fp, rec / prec, the eleven maxima of the 07 metric
  double mx[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) mx[i] = 0.0;
  int ctp = 0, cfp = 0;                                              // carry: counts before this chunk
  for (int64_t r0 = 0; r0 < nd; r0 += VOC_T) {
    const int64_t r = r0 + tid;
    const unsigned flag = r < nd ? (unsigned)(row[r] & 3ull) : 0u;
    int a = (r < nd && flag == 1u) ? 1 : 0, b = (r < nd && flag == 2u) ? 1 : 0;
    double unused = 0.0;
    voc_scan(a, b, unused, wa, wb, wm);
    if (r < nd && use07) {
      const double tp = (double)(ctp + a), fp = (double)(cfp + b);
      const double rec = tp / npos, prec = tp / fmax(tp + fp, 2.220446049250313e-16);
#pragma unroll
      for (int i = 0; i < 11; ++i) if (rec >= (double)i * 0.1) mx[i] = fmax(mx[i], prec);
    }
    int ta = 0, tb = 0;
    for (int i = 0; i < VOC_T / 64; ++i) { ta += wa[i]; tb += wb[i]; }
    ctp += ta; cfp += tb;
  }
  const int ttp = ctp, tfp = cfp;
  double result = -1.0;
  if (nd > 0 && use07) {
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      double v = mx[i];
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
      if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int i = 0; i < 11; ++i) {
        double p = red[0][i];
        for (int k = 1; k < VOC_T / 64; ++k) p = fmax(p, red[k][i]);
        acc = acc + p / 11.0;
      }
      result = acc;
    }
  } else if (nd > 0) {
    // -- backward: thread order = descending rank, so the scan's running maximum is the suffix maximum of prec and its counts are those of the ranks >= r
    double sum = 0.0, cmax = 0.0;
    int sa = 0, sb = 0;                                              // carry: tp / fp flags at ranks behind this chunk
    for (int64_t q0 = 0; q0 < nd; q0 += VOC_T) {
      const int64_t q = q0 + tid, r = nd - 1 - q;
      const unsigned flag = q < nd ? (unsigned)(row[r] & 3ull) : 0u;
      const int own_a = (q < nd && flag == 1u) ? 1 : 0, own_b = (q < nd && flag == 2u) ? 1 : 0;
      int ea = own_a, eb = own_b;                                    // inclusive counts at rank r = the totals minus the flags strictly behind it
      double dummy = 0.0;
      voc_scan(ea, eb, dummy, wa, wb, wm);
      const double tp = (double)(ttp - (sa + ea - own_a)), fp = (double)(tfp - (sb + eb - own_b));
      double m = q < nd ? tp / fmax(tp + fp, 2.220446049250313e-16) : 0.0;
      int ta = 0, tb = 0;
      for (int i = 0; i < VOC_T / 64; ++i) { ta += wa[i]; tb += wb[i]; }
      int za = 0, zb = 0;
      voc_scan(za, zb, m, wa, wb, wm);                               // m: maximum of prec over this chunk's ranks >= r
      m = fmax(m, cmax);
      if (own_a) sum += (tp / npos - (tp - 1.0) / npos) * m;
      double cm = wm[0];
      for (int i = 1; i < VOC_T / 64; ++i) cm = fmax(cm, wm[i]);
      cmax = fmax(cmax, cm);
      sa += ta; sb += tb;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();
    if (lane == 0) red[wave][0] = sum;
    __syncthreads();
    if (tid == 0) {
      double acc = red[0][0];
      for (int k = 1; k < VOC_T / 64; ++k) acc += red[k][0];
      result = npos_i == 0 ? __longlong_as_double(0x7ff8000000000000ll) : acc;          // rec = 0 / 0 everywhere: the reference's sum is NaN
    }
  }
  if (tid == 0) {
    ap[c] = result;
    counts[c] = npos_i; counts[(int64_t)C + c] = nd; counts[(int64_t)2 * C + c] = ttp; counts[(int64_t)3 * C + c] = tfp;
    counts[(int64_t)4 * C + c] = nd - ttp - tfp;
  }
}

extern "C" int frost_voc_update(const float* detections, const float* gt, const uint8_t* difficult, const uint8_t* valid, const float* sizes, int n, int c, int k,
                                int g, int bkg_label, float ovthresh, float det_offset, int top_k, int max_images, int64_t capacity, uint64_t* records, int32_t* ctr,
                                void* stream) {
  FROST_REQUIRE(detections && gt && difficult && valid && records && ctr, "voc_update: incomplete arguments");
  FROST_REQUIRE(n >= 1 && n <= 65535 && c >= 2 && c <= 65535 && bkg_label >= 0 && bkg_label < c, "voc_update: bad sizes");
  FROST_REQUIRE(top_k >= 1 && top_k <= VOC_MAXK && k >= 1 && k <= top_k, "voc_update: K outside 1 .. top_k, or top_k outside 1 .. 1024");
  FROST_REQUIRE(g >= 1 && g <= VOC_MAXG, "voc_update: G outside 1 .. 1024");
  FROST_REQUIRE(max_images >= 1 && (int64_t)max_images * top_k <= (int64_t)1 << 30 && capacity >= 1 && capacity <= VOC_CURSOR_STOP,
                "voc_update: max_images * top_k above 2^30, or capacity outside 1 .. 2^30");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_voc_update, dim3(c, n), dim3(VOC_T), 0, s, detections, gt, difficult, valid, sizes, c, k, g, bkg_label, ovthresh, det_offset, top_k, max_images,
                     capacity, (unsigned long long*)records, ctr);
  hipLaunchKernelGGL(k_voc_advance, dim3(1), dim3(1), 0, s, ctr, c, n);
  return frost_check_launch("voc_update");
}

extern "C" int frost_voc_ap(const uint64_t* sorted_records, const int32_t* ctr, int c, int64_t capacity, int bkg_label, int use_07_metric, double* ap, int64_t* counts,
                            void* stream) {
  FROST_REQUIRE(sorted_records && ctr && ap && counts, "voc_ap: incomplete arguments");
  FROST_REQUIRE(c >= 2 && c <= 65535 && bkg_label >= 0 && bkg_label < c && capacity >= 1, "voc_ap: bad sizes");
  hipLaunchKernelGGL(k_voc_ap, dim3(c), dim3(VOC_T), 0, as_stream(stream), (const unsigned long long*)sorted_records, ctr, c, capacity, bkg_label, use_07_metric, ap, counts);
  return frost_check_launch("voc_ap");
}

extern "C" int frost_voc_reset(uint64_t* records, int32_t* ctr, int c, int64_t capacity, void* stream) {
  FROST_REQUIRE(records && ctr && c >= 2 && capacity >= 1, "voc_reset: bad arguments");
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(records, 0, (size_t)c * (size_t)capacity * 8, s) != hipSuccess) { frost_set_error("voc_reset: memset failed"); return 1; }
  if (hipMemsetAsync(ctr, 0, (size_t)(2 * c + 2) * 4, s) != hipSuccess) { frost_set_error("voc_reset: memset failed"); return 1; }
  return 0;
}

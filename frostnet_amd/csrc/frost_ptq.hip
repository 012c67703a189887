// Post-training quantisation: the activation observer of the default PTQ qconfigs on the device.
// replaces: torch.ao.quantization.HistogramObserver.forward (2048 bins, upsample rate 16) -- torch.aminmax, torch.histc, _combine_histograms /
// _upscale_histogram (repeat_interleave, two linspaces, bucketize, bincount) -- restated in fp32 in frostnet_amd/ptq.py (hist_update), which
// tests/test_cpu_ptq.py holds bit-equal to stock torch.  The search for the clipping range (calculate_qparams) stays stock torch on the host: it runs once.
//
// Three launches per site and batch, all state in the site record (include/frost_hip.h):
//   k_ptq_range    batch min / max (wave + workgroup reduction, two ordered float atomics per workgroup), non-finite values counted
//   k_ptq_count    2048-bin counts against the range the state and the batch decide: per-workgroup LDS histogram with integer atomics; a wave first
//                  merges the lanes that share a bin with a ballot (a post-ReLU tensor puts about half of its elements into one bin: 64 lanes adding to
//                  one LDS address serialise), then flushes its non-zero bins with integer global atomics
//   k_ptq_combine  one workgroup: the branch decision of HistogramObserver.forward, the old histogram held in LDS, one thread per destination bin walking
//                  its contiguous run of fine bins in ascending order (the summation order of torch.bincount), new state stored, scratch re-armed
#include "frost_common.h"

#define PTQ_BINS FROST_PTQ_BINS
#define PTQ_FINE (FROST_PTQ_BINS * 16)
// workgroups per launch: the count pass wants every SIMD full (8 workgroups of 4 waves per CU; its flush is at most 2048 integer atomics per workgroup), the range pass
// ends in two same-address float atomics per workgroup, which serialise at the memory side
#define PTQ_RANGE_WG 1024
#define PTQ_COUNT_WG 2048

struct PtqDense {
  const float* x;
  __device__ __forceinline__ float at(int64_t i) const { return x[i]; }
};
struct PtqStrided {          // logical (n, c, h, w) with element strides; decoded channel-fastest when sc == 1 (channels_last) for coalescing: the update is order-free
  const float* x; int c, h, w; int64_t sn, sc, sh, sw;
  __device__ __forceinline__ float at(int64_t i) const {
    int64_t t = i;
    if (sc == 1) { const int ch = (int)(t % c); t /= c; const int xw = (int)(t % w); t /= w; const int yh = (int)(t % h); const int64_t in = t / h;
      return x[in * sn + ch * sc + yh * sh + xw * sw]; }
    const int xw = (int)(t % w); t /= w; const int yh = (int)(t % h); t /= h; const int ch = (int)(t % c); const int64_t in = t / c;
    return x[in * sn + ch * sc + yh * sh + xw * sw];
  }
};

// ------------------------------------------------------------------------------------------------ batch range
template <class S> __global__ __launch_bounds__(256) void k_ptq_range(S src, int64_t n, int64_t n4, float* site, int32_t* nonfinite) {
  __shared__ float sh[8]; __shared__ int sbad[4];
  float lo = INFINITY, hi = -INFINITY; int bad = 0;
  const int tid = threadIdx.x;
  if (n4 > 0) {          // dense and 16-byte aligned: four elements per load
    const float4* x4 = (const float4*)src.x;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 v = x4[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { if (isfinite(e[k])) { lo = fminf(lo, e[k]); hi = fmaxf(hi, e[k]); } else ++bad; }
    }
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = src.at(i);
    if (isfinite(v)) { lo = fminf(lo, v); hi = fmaxf(hi, v); } else ++bad;
  }
  lo = wave_min(lo); hi = wave_max(hi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0) { sh[tid >> 6] = lo; sh[4 + (tid >> 6)] = hi; sbad[tid >> 6] = bad; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i) { lo = fminf(lo, sh[i]); hi = fmaxf(hi, sh[4 + i]); bad += sbad[i]; }
    if (lo <= hi) { atomic_min_f32(site + 2, lo); atomic_max_f32(site + 3, hi); }
    if (bad) atomicAdd(nonfinite, bad);
  }
}

// the range of this call's histogram: HistogramObserver.forward's (new_min, new_max), widened like torch.histc when it is a single value
__device__ __forceinline__ bool ptq_call_range(const float* site, float& lo, float& hi) {
  const float mn = site[0], mx = site[1], xmin = site[2], xmax = site[3];
  if (!(xmin <= xmax)) return false;                       // the batch held no finite value: nothing to count
  const bool fresh = (mn == INFINITY) || (mx == -INFINITY);
  lo = fresh ? xmin : fminf(mn, xmin); hi = fresh ? xmax : fmaxf(mx, xmax);
  if (lo == hi) { lo = lo - 1.0f; hi = hi + 1.0f; }
  return true;
}
__device__ __forceinline__ int ptq_bin(float v, float lo, float hi) {          // aten histc: (int64)((x - lo) / (hi - lo) * bins), the right edge into the last bin
  int pos = (int)(((v - lo) / (hi - lo)) * (float)PTQ_BINS);
  return min(max(pos, 0), PTQ_BINS - 1);
}

// One element per lane into the workgroup's LDS histogram.  Called by whole waves (pos < 0: nothing to add).  Two merging rounds: the lanes in the bin of a
// leader are counted with a ballot and added once; the first leader is a lane whose neighbour shares its bin (the crowded bin of a post-ReLU tensor, if there
// is one), the second the first lane left.  What remains adds one by one.
__device__ __forceinline__ void ptq_lds_add(unsigned* hist, int pos) {
  const int lane = threadIdx.x & 63;
  bool live = pos >= 0;
  unsigned long long act = __ballot(live);
  if (act == 0ull) return;
  const int nb = __builtin_amdgcn_update_dpp(-2, pos, 0x111, 0xf, 0xf, false);          // row_shr:1 -- the left neighbour inside a row of 16 lanes (-2 at a row's first lane)
  const unsigned long long pairs = __ballot(live && nb == pos);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long cand = (r == 0 && pairs != 0ull) ? pairs : act;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)cand) - 1);
    const int lb = __builtin_amdgcn_readlane(pos, leader);
    const unsigned long long same = __ballot(live && pos == lb);
    if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
    live = live && pos != lb;
    act = __ballot(live);
    if (act == 0ull) return;
  }
  if (live) atomicAdd(&hist[pos], 1u);
}

template <class S> __global__ __launch_bounds__(256) void k_ptq_count(S src, int64_t n, int64_t n4, const float* site, int32_t* counts) {
  __shared__ unsigned hist[PTQ_BINS];
  const int tid = threadIdx.x;
  float lo, hi;
  if (!ptq_call_range(site, lo, hi)) return;               // (uniform: every thread reads the same record)
  for (int i = tid; i < PTQ_BINS; i += 256) hist[i] = 0u;
  __syncthreads();
  if (n4 > 0) {
    const float4* x4 = (const float4*)src.x;
    for (int64_t b = (int64_t)blockIdx.x * 256; b < n4; b += (int64_t)gridDim.x * 256) {      // b is uniform: whole waves reach ptq_lds_add
      const int64_t i = b + tid;
      float4 v = make_float4(NAN, NAN, NAN, NAN);
      if (i < n4) v = x4[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) ptq_lds_add(hist, (e[k] >= lo && e[k] <= hi) ? ptq_bin(e[k], lo, hi) : -1);
    }
  }
  for (int64_t b = n4 * 4 + (int64_t)blockIdx.x * 256; b < n; b += (int64_t)gridDim.x * 256) {
    const int64_t i = b + tid;
    const float v = (i < n) ? src.at(i) : NAN;
    ptq_lds_add(hist, (v >= lo && v <= hi) ? ptq_bin(v, lo, hi) : -1);
  }
  __syncthreads();
  for (int i = tid; i < PTQ_BINS; i += 256) { const unsigned v = hist[i]; if (v) atomicAdd(&counts[i], (int)v); }
}

// ------------------------------------------------------------------------------------------------ combine
// torch.linspace(a, b, n) in fp32: one fused multiply-add per element from the nearer end (the library is built with -ffp-contract=off: fmaf is explicit)
__device__ __forceinline__ float ptq_linspace(float a, float b, float step, int n, int i) { return (i < n / 2) ? fmaf(step, (float)i, a) : fmaf(-step, (float)(n - 1 - i), b); }

__global__ __launch_bounds__(1024) void k_ptq_combine(float* site) {
  __shared__ float old[PTQ_BINS]; __shared__ float part[16];
  const int tid = threadIdx.x;
  const float mn = site[0], mx = site[1], xmin = site[2], xmax = site[3];
  float* hist = site + FROST_PTQ_HDR;
  int32_t* counts = (int32_t*)(site + FROST_PTQ_HDR + PTQ_BINS);
  if (!(xmin <= xmax)) return;                             // no finite value in the batch: the state stays (the counts were never touched)
  const bool fresh = (mn == INFINITY) || (mx == -INFINITY);
  const float nmin = fresh ? xmin : fminf(mn, xmin), nmax = fresh ? xmax : fmaxf(mx, xmax);
  float u[2], h[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) { const int j = tid + k * 1024; u[k] = (float)counts[j]; h[k] = hist[j]; old[j] = h[k]; }
  __syncthreads();                                         // every thread holds the old record; the old histogram is in LDS
  float out[2];
  if (fresh) { out[0] = u[0]; out[1] = u[1]; }
  else if (nmin == mn && nmax == mx) { out[0] = h[0] + u[0]; out[1] = h[1] + u[1]; }
  else if (mn == mx) {
    // a constant history: histc([mn]) over the new range times the old total (a single non-zero bin: the sum is exact in any order)
    float s = wave_sum(h[0] + h[1]);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    float total = 0.0f;
    for (int i = 0; i < 16; ++i) total += part[i];
    const int pos = ptq_bin(mn, nmin, nmax);               // (nmin < nmax here: an equal pair would have been the same-range branch)
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int j = tid + k * 1024; out[k] = ((j == pos) ? 1.0f : 0.0f) * total + u[k]; }
  } else {
    const float step = (mx - mn) / (float)PTQ_FINE;        // linspace step of the fine mid-points == the fine bin size (the same expression)
    const float half = 0.5f * step;
    const float bstep = (nmax - nmin) / (float)PTQ_BINS;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int j = tid + k * 1024;
      // fine bin i goes to bin (number of boundaries <= mid_i) - 1, clipped: bin j owns [first i with mid_i >= boundary_j, first i with mid_i >= boundary_{j+1})
      int ends[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int jb = j + s;
        if (jb == 0) { ends[s] = 0; continue; }
        if (jb == PTQ_BINS) { ends[s] = PTQ_FINE; continue; }
        const float bound = ptq_linspace(nmin, nmax, bstep, PTQ_BINS + 1, jb);
        int a = 0, b = PTQ_FINE;                           // smallest i in [0, PTQ_FINE] with mid_i >= bound
        while (a < b) {
          const int m = (a + b) >> 1;
          const float mid = ptq_linspace(mn, mx, step, PTQ_FINE + 1, m) + half;
          if (mid >= bound) b = m; else a = m + 1;
        }
        ends[s] = a;
      }
      float acc = 0.0f;
      for (int i = ends[0]; i < ends[1]; ++i) acc += old[i >> 4] / 16.0f;
      out[k] = u[k] + acc;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) { const int j = tid + k * 1024; hist[j] = out[k]; counts[j] = 0; }
  if (tid == 0) { site[0] = nmin; site[1] = nmax; site[2] = INFINITY; site[3] = -INFINITY; }
}

static int ptq_grid(int64_t n, int cap) {
  const int64_t g = (n + 256 * 16 - 1) / (256 * 16);
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" int frost_ptq_site_words(void) { return FROST_PTQ_SITE_WORDS; }

extern "C" int frost_ptq_observe(const float* x, int64_t n, float* site, int32_t* nonfinite, void* stream) {
  FROST_REQUIRE(x != nullptr && site != nullptr && nonfinite != nullptr && n > 0, "ptq_observe: null pointer or empty tensor");
  const int64_t n4 = (((uintptr_t)x & 15) == 0) ? n / 4 : 0;
  const PtqDense src{x};
  hipLaunchKernelGGL(k_ptq_range<PtqDense>, dim3(ptq_grid(n, PTQ_RANGE_WG)), dim3(256), 0, as_stream(stream), src, n, n4, site, nonfinite);
  hipLaunchKernelGGL(k_ptq_count<PtqDense>, dim3(ptq_grid(n, PTQ_COUNT_WG)), dim3(256), 0, as_stream(stream), src, n, n4, (const float*)site, (int32_t*)(site + FROST_PTQ_HDR + PTQ_BINS));
  hipLaunchKernelGGL(k_ptq_combine, dim3(1), dim3(1024), 0, as_stream(stream), site);
  return frost_check_launch("ptq_observe");
}

extern "C" int frost_ptq_observe_strided(const float* x, int n, int c, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* site,
                                         int32_t* nonfinite, void* stream) {
  FROST_REQUIRE(x != nullptr && site != nullptr && nonfinite != nullptr && n > 0 && c > 0 && h > 0 && w > 0, "ptq_observe_strided: null pointer or empty tensor");
  FROST_REQUIRE(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ptq_observe_strided: negative strides are not supported");
  const int64_t tot = (int64_t)n * c * h * w;
  const bool nchw = (sw == 1 && sh == w && sc == (int64_t)h * w && sn == (int64_t)c * h * w);
  const bool nhwc = (sc == 1 && sw == c && sh == (int64_t)w * c && sn == (int64_t)h * w * c);
  if (nchw || nhwc) return frost_ptq_observe(x, tot, site, nonfinite, stream);          // dense in memory: the update does not depend on the element order
  const PtqStrided src{x, c, h, w, sn, sc, sh, sw};
  hipLaunchKernelGGL(k_ptq_range<PtqStrided>, dim3(ptq_grid(tot, PTQ_RANGE_WG)), dim3(256), 0, as_stream(stream), src, tot, (int64_t)0, site, nonfinite);
  hipLaunchKernelGGL(k_ptq_count<PtqStrided>, dim3(ptq_grid(tot, PTQ_COUNT_WG)), dim3(256), 0, as_stream(stream), src, tot, (int64_t)0, (const float*)site, (int32_t*)(site + FROST_PTQ_HDR + PTQ_BINS));
  hipLaunchKernelGGL(k_ptq_combine, dim3(1), dim3(1024), 0, as_stream(stream), site);
  return frost_check_launch("ptq_observe_strided");
}

// ------------------------------------------------------------------------------------------------ fused float layers on the float kernels
__global__ __launch_bounds__(256) void k_ptq_coef(const FrostFDesc* descs) {
  const FrostFDesc d = descs[blockIdx.y];
  for (int c = blockIdx.x * 256 + threadIdx.x; c < d.cpad; c += gridDim.x * 256) {
    d.coef[0 * d.cpad + c] = 1.0f;                                       // scale row
    d.coef[1 * d.cpad + c] = (c < d.cout && d.beta) ? d.beta[c] : 0.0f;  // bias row
  }
}
extern "C" int frost_ptq_coef(const FrostFDesc* descs, int nlayers, void* stream) {
  if (nlayers <= 0) return 0;
  hipLaunchKernelGGL(k_ptq_coef, dim3(2, nlayers), dim3(256), 0, as_stream(stream), descs);
  return frost_check_launch("ptq_coef");
}

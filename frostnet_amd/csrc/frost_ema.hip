// Weight EMA (timm ModelEmaV3 semantics) of a whole module tree as ONE multi-tensor launch.
// replaces: the stock loop over state_dict() -- ~1 000 small lerp_ and ~600 scalar copy_ launches for a QAT FrostNet-Large, behind ~1 000 clones of
// the buffers a bound model aliases onto its qrecord arena.  A state dict is mostly single words, so the grid is NOT (chunks, entries): the host
// precomputes a flat workgroup map (include/frost_hip.h): one workgroup per FROST_EMA_CHUNK-unit chunk of a large entry, many small entries per workgroup.
// No atomics, no dependence between workgroups: every destination unit is written by exactly one lane, once.
#include "frost_common.h"

// dst = lerp(dst, src, w) on the bit patterns of one fp32 word; explicit fma (bit-equal to CPU torch lerp_ for |w| < 0.5), the subtraction is never
// contracted into it (-ffp-contract=off).  A source that is not finite is copied: an observer that never saw data holds min_val = +inf / max_val = -inf for good.
__device__ __forceinline__ uint32_t ema_word(uint32_t s, uint32_t d, float w, bool lerp) {
  if (!lerp) return s;
  const float sf = __uint_as_float(s), df = __uint_as_float(d);
  if (!(fabsf(sf) <= 3.402823466e+38f)) return s;
  return __float_as_uint(__builtin_fmaf(w, sf - df, df));
}

__global__ __launch_bounds__(256) void k_ema_update(const FrostEmaEntry* __restrict__ table, int nentries, const int4* __restrict__ wgmap,
                                                    const float* __restrict__ weight) {
  __shared__ int s_pref[FROST_EMA_SMALL_ROWS];
  __shared__ int s_n[FROST_EMA_SMALL_ROWS];
  __shared__ int s_kind[FROST_EMA_SMALL_ROWS];
  __shared__ const char* s_src[FROST_EMA_SMALL_ROWS];
  __shared__ char* s_dst[FROST_EMA_SMALL_ROWS];
  const int4 m = wgmap[blockIdx.x];
  const float w = *weight;
  const int tid = threadIdx.x;
  if (m.x == 0) {                                                                // one chunk of a large entry: {0, entry, chunk, 0}
    if ((unsigned)m.y >= (unsigned)nentries) return;
    const FrostEmaEntry e = table[m.y];
    const int64_t units = e.kind == FROST_EMA_COPY8 ? 2 * e.n : e.n;               // 8-byte elements travel as two words
    const int64_t first = (int64_t)m.z * FROST_EMA_CHUNK;
    if (m.z < 0 || first >= units) return;
    const int len = units - first < FROST_EMA_CHUNK ? (int)(units - first) : FROST_EMA_CHUNK;
    if (e.kind == FROST_EMA_COPY1) {
      const uint8_t* s = (const uint8_t*)e.src + first;
      uint8_t* d = (uint8_t*)e.dst + first;
      for (int i = tid; i < len; i += 256) d[i] = s[i];
      return;
    }
    const bool lerp = e.kind == FROST_EMA_LERP;
    const uint32_t* s = (const uint32_t*)e.src + first;
    uint32_t* d = (uint32_t*)e.dst + first;
    const uintptr_t sa = (uintptr_t)s, da = (uintptr_t)d;
    if (((sa ^ da) & 15) != 0) {                                                   // the two sides are never 16-byte aligned together: word by word
      for (int i = tid; i < len; i += 256) d[i] = ema_word(s[i], d[i], w, lerp);
      return;
    }
    int head = (int)(((16 - (sa & 15)) & 15) >> 2);                                // words in front of the first 16-byte boundary (arenas hand out 4-byte offsets)
    if (head > len) head = len;
    const int nv = (len - head) >> 2;
    if (tid < head) d[tid] = ema_word(s[tid], d[tid], w, lerp);
    const uint4* s4 = (const uint4*)(s + head);
    uint4* d4 = (uint4*)(d + head);
    for (int i = tid; i < nv; i += 256) {
      const uint4 a = s4[i];
      uint4 b = d4[i];
      b.x = ema_word(a.x, b.x, w, lerp); b.y = ema_word(a.y, b.y, w, lerp); b.z = ema_word(a.z, b.z, w, lerp); b.w = ema_word(a.w, b.w, w, lerp);
      d4[i] = b;
    }
    const int t = head + 4 * nv + tid;                                             // at most three words behind the last full vector
    if (t < len) d[t] = ema_word(s[t], d[t], w, lerp);
    return;
  }
  // small entries packed into one workgroup: {1, first row, rows, units}; row = {entry, first unit of the entry within this workgroup's slice, 0, 0}
  const int nrows = m.z < FROST_EMA_SMALL_ROWS ? m.z : FROST_EMA_SMALL_ROWS;
  if (tid < nrows) {
    const int4 r = wgmap[m.y + tid];
    const bool ok = (unsigned)r.x < (unsigned)nentries;
    FrostEmaEntry e;
    if (ok) e = table[r.x];
    s_pref[tid] = r.y;
    s_kind[tid] = ok ? e.kind : FROST_EMA_COPY4;
    s_n[tid] = ok ? (int)(e.kind == FROST_EMA_COPY8 ? 2 * e.n : e.n) : 0;
    s_src[tid] = ok ? (const char*)e.src : nullptr;
    s_dst[tid] = ok ? (char*)e.dst : nullptr;
  }
  __syncthreads();
  if (nrows <= 0) return;
  for (int u = tid; u < m.w; u += 256) {
    int lo = 0, hi = nrows - 1;                                                    // the row whose slice holds unit u: the last one that starts at or before it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_pref[mid] <= u) lo = mid; else hi = mid - 1;
    }
    const int i = u - s_pref[lo];
    if (i < 0 || i >= s_n[lo]) continue;
    const int kind = s_kind[lo];
    if (kind == FROST_EMA_COPY1) {
      ((uint8_t*)s_dst[lo])[i] = ((const uint8_t*)s_src[lo])[i];
    } else {
      uint32_t* d = (uint32_t*)s_dst[lo] + i;
      *d = ema_word(((const uint32_t*)s_src[lo])[i], *d, w, kind == FROST_EMA_LERP);
    }
  }
}

extern "C" int frost_ema_entry_bytes(void) { return (int)sizeof(FrostEmaEntry); }

extern "C" int frost_ema_update(const FrostEmaEntry* table, int nentries, const int32_t* wgmap, int nwg, const float* weight, void* stream) {
  if (nwg <= 0 || nentries <= 0) return 0;
  hipLaunchKernelGGL(k_ema_update, dim3((unsigned)nwg), dim3(256), 0, as_stream(stream), table, nentries, (const int4*)wgmap, weight);
  return frost_check_launch("ema_update");
}

// Segmentation criterion and mean-IoU counts with the bilinear upsampling (align_corners=True) fused in: weighted 2-D cross entropy with ignore = 255, its
// gradient with respect to the LOW-resolution logits, argmax and the three per-class pixel counts, from one C-ABI call (include/frost_hip.h, frostnet_amd/seg.py).
// replaces: F.interpolate -> F.cross_entropy forward + backward -> argmax -> three histc calls on the host, i.e. five passes over N*C*H*W fp32 values that
// this file never materialises: an upsampled logit lives in registers only.
//
// Shape of the upsampling kernel.  A workgroup owns a tile of th x tw low-resolution cells.  An output pixel (Y, X) reads the cells (y0, x0), (y0, x1), (y1, x0),
// (y1, x1); it BELONGS to cell (y0, x0).  All pixels with the same y0 = r form band r, all columns with the same x0 a column group.  Per band, thread = one output
// column: the four taps are constant down the column inside a band, so the thread interpolates them horizontally once (top[c], bot[c]) and then walks the band's
// rows with u[c] = (1 - fy) top[c] + fy bot[c] in registers -- torch's own association.  While walking it sums (1 - fy) g and fy g (g = wt (softmax - onehot) /
// W_sum) per class in registers: the vertical half of the transposed interpolation.  The column sums go to LDS, then threads indexed by (cell, class) gather their
// columns in ascending X with the horizontal weights: the other half.  Row cy of dx is band cy's top sum plus band cy - 1's bottom sum, carried in LDS from one
// band to the next.  Every dx element is written once, by one thread, from sums taken in a fixed order: no floating-point atomics, bit-identical from run to run.
// The gradient of a tile needs band cy0 - 1 and column group cx0 - 1 as well (the halo): those pixels are recomputed, their loss and counts are left to the
// neighbour that owns them.  Loss: fp64 per thread, one partial per workgroup, summed in index order by the last workgroup (ticket).  Counts: run-length
// compressed per thread, staged in LDS with 32-bit integer atomics, flushed with one 64-bit atomic per non-zero class.
// Equal sizes take k_seg_id: one read per logit, no taps.
#include "frost_common.h"

#define SEG_IGNORE 255
#define SEG_TW_MAX 31
#define SEG_MAX_GRID FROST_SEG_MAX_PARTIALS
#define SEG_WSUM_GRID 1024

struct SegGeom {
  int n, c, h, w, H, W;
  int64_t sn, sc, sh, sw;          // element strides of logits and dx
  float scale_y, scale_x;
  int th, tw, tiles_y, tiles_x, ntiles;
  int tbytes;                      // 8: int64 targets, 1: uint8
};

// (the index and weight rule of the upsampling, seg_src / seg_first, is in frost_common.h: the segmentation head's kernels follow the same one)
// a target as 0 .. 256: 256 stands for every int64 value outside 0 .. 255 (outside the contract, never an index)
__device__ __forceinline__ int seg_target(const void* t, int tbytes, int64_t idx) {
  if (tbytes == 1) return (int)((const uint8_t*)t)[idx];
  const int64_t v = ((const int64_t*)t)[idx];
  return (v < 0 || v > 255) ? 256 : (int)v;
}
__device__ __forceinline__ void seg_part_store(double* p, double v) {
  __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double seg_part_load(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Sum of one double per thread over the launch, in a fixed order: wave tree, waves in index order, workgroups in index order by the last one to arrive.
// Returns true in thread 0 of that last workgroup with the total in `total`.  sh: 8 doubles, sflag: one int of LDS.
__device__ inline bool seg_grid_sum(double v, double* part, uint32_t* ticket, double* sh, int* sflag, double& total) {
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  v = wave_sum_d(v);
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double s = sh[0];
    for (int i = 1; i < nw; ++i) s += sh[i];
    seg_part_store(part + blockIdx.x, s);
  }
  if (!last_block_done2(ticket, gridDim.x, sflag)) return false;
  double s = 0.0;
  for (int i = tid; i < (int)gridDim.x; i += blockDim.x) s += seg_part_load(part + i);
  s = wave_sum_d(s);
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  if (tid != 0) return false;
  total = sh[0];
  for (int i = 1; i < nw; ++i) total += sh[i];
  return true;
}

// W_sum = sum of wt[t] over the valid targets (fp64: a sum of fp32 weights, exact for any realistic pixel count)
__global__ __launch_bounds__(256) void k_seg_wsum(const void* __restrict__ tgt, int tbytes, int64_t total, int C, const float* __restrict__ wt,
                                                   double* __restrict__ part, uint32_t* __restrict__ ticket, double* __restrict__ wsum) {
  __shared__ double sh[8];
  __shared__ int sflag;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = seg_target(tgt, tbytes, i);
    if (t < C) acc += (double)(wt ? wt[t] : 1.0f);
  }
  double tot;
  if (seg_grid_sum(acc, part, ticket, sh, &sflag, tot)) *wsum = tot;
}

// run-length compressed counts of one thread, staged in the workgroup's LDS histogram [inter | pred | mask] x C
struct SegRuns {
  int cur_t, cur_p; uint32_t n_mask, n_inter, n_pred;
  __device__ __forceinline__ void init() { cur_t = -1; cur_p = -1; n_mask = n_inter = n_pred = 0; }
  __device__ __forceinline__ void flush(uint32_t* hist, int C) {
    if (n_mask) atomicAdd(&hist[2 * C + cur_t], n_mask);
    if (n_inter) atomicAdd(&hist[cur_t], n_inter);
    if (n_pred) atomicAdd(&hist[C + cur_p], n_pred);
    n_mask = n_inter = n_pred = 0;
  }
  __device__ __forceinline__ void add(uint32_t* hist, int C, int t, int p) {
    if (t != cur_t || p != cur_p) { flush(hist, C); cur_t = t; cur_p = p; }
    ++n_mask; ++n_pred; n_inter += (t == p) ? 1u : 0u;
  }
};

// tail shared by both kernels: counts to the state, the loss through the ordered sum
__device__ inline void seg_finish(double loss_acc, uint32_t bad, uint32_t* hist, int C, unsigned long long* state, double* part, uint32_t* ticket,
                                  const double* wsum, float* loss_out, double* sh, int* sflag) {
  __syncthreads();
  if (state) {
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) { const uint32_t v = hist[i]; if (v) atomicAdd(state + i, (unsigned long long)v); }
    if (bad) atomicAdd(state + 3 * C + 1, (unsigned long long)bad);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(state + 3 * C, 1ull);
  }
  if (loss_out) {
    double tot;
    if (seg_grid_sum(loss_acc, part, ticket, sh, sflag, tot)) *loss_out = (float)(tot / *wsum);          // 0 / 0 = NaN when nothing is valid, as torch
  }
}

// ---- the upsampling kernel ---------------------------------------------------------------------------------------------------
// CP: classes held in registers at once.  GEN = false: c <= CP, one chunk, u[] in registers.  GEN = true: any c, the gradient in chunks of CP classes, the
// softmax statistics of a pixel recomputed per chunk by streaming its taps (slow, correct).
template <int CP, int NT, bool GEN>
__global__ __launch_bounds__(NT) void k_seg_up(const SegGeom g, const float* __restrict__ x, const void* __restrict__ tgt, const float* __restrict__ wt,
                                                const double* __restrict__ wsum, float* __restrict__ dx, unsigned long long* __restrict__ state,
                                                double* __restrict__ part, uint32_t* __restrict__ ticket, float* __restrict__ loss_out) {
  constexpr int CS = CP + 1;                     // odd-ish pitch of a class row in LDS: column threads write pitch apart, (cell, class) threads read along it
  extern __shared__ float smem[];
  float* colT = smem;                            // [NT][CS] column sums weighted (1 - fy)
  float* colB = colT + NT * CS;                  // ... weighted fy
  float* accT = colB + NT * CS;                  // [tw][CS] the band's gathered sums
  float* accB = accT + SEG_TW_MAX * CS;
  float* carry = accB + SEG_TW_MAX * CS;         // the previous band's bottom sums
  float* s_fx = carry + SEG_TW_MAX * CS;         // [NT] horizontal weight of the chunk's columns
  int* s_first = (int*)(s_fx + NT);              // [tw + 3] first column of the groups cx0 - 1 .. cx0 + tw + 1
  uint32_t* hist = (uint32_t*)(s_first + SEG_TW_MAX + 3);   // [3 c]
  __shared__ double sh[8];
  __shared__ int sflag;
  const int tid = threadIdx.x, C = g.c;
  const bool want_dx = dx != nullptr, want_sm = want_dx || loss_out != nullptr;
  const int hb = g.h >= 2 ? g.h - 1 : 1;                               // bands
  for (int i = tid; i < 3 * C; i += NT) hist[i] = 0;
  float inv_wsum = 0.0f;
  if (want_dx) { const double ws = *wsum; inv_wsum = ws > 0.0 ? (float)(1.0 / ws) : 0.0f; }
  double loss_acc = 0.0;
  uint32_t bad = 0;
  SegRuns runs; runs.init();

  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y, n = tile / (g.tiles_x * g.tiles_y);
    const int cy0 = ty * g.th, cx0 = tx * g.tw;
    const int twl = min(g.tw, g.w - cx0);
    __syncthreads();
    if (tid < twl + 3) s_first[tid] = seg_first(cx0 - 1 + tid, g.scale_x, g.w, g.W);
    __syncthreads();
    const int Xown = s_first[1], Xhi = s_first[twl + 1], Xlo = want_dx ? s_first[0] : Xown;
    const int rlo = want_dx ? cy0 - 1 : cy0, rhi = min(cy0 + g.th - 1, g.h - 1);
    const float* xn = x + (int64_t)n * g.sn;
    const int64_t tbase = (int64_t)n * g.H * g.W;

    for (int c0 = 0; c0 < C; c0 += CP) {
      if (c0 > 0 && !want_dx) break;                                   // loss and counts are taken in the first chunk
      const int cw = min(CP, C - c0);                                  // classes of this chunk
      const int items = twl * cw;                                      // (cell, class) pairs: item -> thread is the same map in every phase below
      if (want_dx) __syncthreads();                                    // ... of this chunk: the map changes with cw, the previous chunk's owners are done
      for (int it = tid; it < items; it += NT) carry[(it / cw) * CS + it % cw] = 0.0f;
      for (int r = rlo; r <= rhi; ++r) {
        for (int it = tid; it < items; it += NT) { const int a = (it / cw) * CS + it % cw; accT[a] = 0.0f; accB[a] = 0.0f; }
        if (r >= 0 && r < hb) {
          const int Ylo = seg_first(r, g.scale_y, g.h, g.H), Yhi = seg_first(r + 1, g.scale_y, g.h, g.H);
          const int r1 = min(r + 1, g.h - 1);
          const bool own_band = r >= cy0 && c0 == 0;
          for (int Xc = Xlo; Xc < Xhi; Xc += NT) {
            const int X = Xc + tid;
            if (X < Xhi) {
              int x0; float fx;
              seg_src(X, g.scale_x, g.w, x0, fx);
              const int x1 = min(x0 + 1, g.w - 1);
              const float l0x = 1.0f - fx;
              s_fx[tid] = fx;
              const bool own = own_band && X >= Xown;
              const float* p00 = xn + (int64_t)r * g.sh + (int64_t)x0 * g.sw;
              const float* p01 = xn + (int64_t)r * g.sh + (int64_t)x1 * g.sw;
              const float* p10 = xn + (int64_t)r1 * g.sh + (int64_t)x0 * g.sw;
              const float* p11 = xn + (int64_t)r1 * g.sh + (int64_t)x1 * g.sw;
              float top[CP], bot[CP], aT[CP], aB[CP];
#pragma unroll
              for (int c = 0; c < CP; ++c) {
                aT[c] = 0.0f; aB[c] = 0.0f; top[c] = 0.0f; bot[c] = 0.0f;
                if (c < cw) {
                  const int64_t o = (int64_t)(c0 + c) * g.sc;
                  top[c] = l0x * p00[o] + fx * p01[o];
                  bot[c] = l0x * p10[o] + fx * p11[o];
                }
              }
              for (int Y = Ylo; Y < Yhi; ++Y) {
                int y0; float fy;
                seg_src(Y, g.scale_y, g.h, y0, fy);
                const float l0y = 1.0f - fy;
                const int t = seg_target(tgt, g.tbytes, tbase + (int64_t)Y * g.W + X);
                const bool valid = t < C;
                if (own && !valid && t != SEG_IGNORE) ++bad;
                const float wgt = valid ? (wt ? wt[t] : 1.0f) : 0.0f;
                const float coef = wgt * inv_wsum;
                const bool need_stats = own && valid;                  // loss and counts
                if (!need_stats && coef == 0.0f) continue;             // an ignored pixel, or a halo pixel of weight zero: contributes nothing anywhere
                float e[CP];
                float m = -INFINITY, ut = 0.0f, s = 0.0f;
                int arg = 0;
                if (!GEN) {
#pragma unroll
                  for (int c = 0; c < CP; ++c) {
                    e[c] = l0y * top[c] + fy * bot[c];
                    if (c < cw && e[c] > m) { m = e[c]; arg = c; }
                  }
                  if (want_sm) {
#pragma unroll
                    for (int c = 0; c < CP; ++c) {
                      if (c < cw) {
                        ut = (c == t) ? e[c] : ut;
                        e[c] = expf(e[c] - m);
                        s += e[c];
                      }
                    }
                  }
                } else {
                  for (int c = 0; c < C; ++c) {
                    const int64_t o = (int64_t)c * g.sc;
                    const float u = l0y * (l0x * p00[o] + fx * p01[o]) + fy * (l0x * p10[o] + fx * p11[o]);
                    if (u > m) { m = u; arg = c; }
                  }
                  if (want_sm) {
                    for (int c = 0; c < C; ++c) {
                      const int64_t o = (int64_t)c * g.sc;
                      const float u = l0y * (l0x * p00[o] + fx * p01[o]) + fy * (l0x * p10[o] + fx * p11[o]);
                      ut = (c == t) ? u : ut;
                      s += expf(u - m);
                    }
#pragma unroll
                    for (int c = 0; c < CP; ++c) e[c] = (c < cw) ? expf((l0y * top[c] + fy * bot[c]) - m) : 0.0f;
                  }
                }
                if (need_stats) {
                  if (loss_out) loss_acc += (double)(wgt * ((m + logf(s)) - ut));
                  if (state) runs.add(hist, C, t, arg);
                }
                if (want_dx && coef != 0.0f) {
                  const float inv_s = 1.0f / s;
                  const int tl = t - c0;
#pragma unroll
                  for (int c = 0; c < CP; ++c) {
                    if (c < cw) {
                      const float gc = coef * (e[c] * inv_s - ((c == tl) ? 1.0f : 0.0f));
                      aT[c] += l0y * gc; aB[c] += fy * gc;
                    }
                  }
                }
              }
              if (own && state) runs.flush(hist, C);
              if (want_dx) {
#pragma unroll
                for (int c = 0; c < CP; ++c) { if (c < cw) { colT[tid * CS + c] = aT[c]; colB[tid * CS + c] = aB[c]; } }
              }
            }
            if (want_dx) {
              __syncthreads();
              const int Xe = min(Xc + NT, Xhi);
              for (int it = tid; it < items; it += NT) {
                const int cxl = it / cw, c = it % cw, a = cxl * CS + c;
                float sT = accT[a], sB = accB[a];
                int k0 = max(s_first[cxl], Xc), k1 = min(s_first[cxl + 1], Xe);          // group x0 = cx - 1: this cell is its right tap
                for (int k = k0; k < k1; ++k) { const float f = s_fx[k - Xc]; sT += f * colT[(k - Xc) * CS + c]; sB += f * colB[(k - Xc) * CS + c]; }
                k0 = max(s_first[cxl + 1], Xc); k1 = min(s_first[cxl + 2], Xe);              // group x0 = cx: the left tap
                for (int k = k0; k < k1; ++k) { const float f = 1.0f - s_fx[k - Xc]; sT += f * colT[(k - Xc) * CS + c]; sB += f * colB[(k - Xc) * CS + c]; }
                accT[a] = sT; accB[a] = sB;
              }
              __syncthreads();
            }
          }
        }
        if (want_dx) {
          for (int it = tid; it < items; it += NT) {
            const int cxl = it / cw, c = it % cw, a = cxl * CS + c;
            if (r >= cy0) dx[(int64_t)n * g.sn + (int64_t)(c0 + c) * g.sc + (int64_t)r * g.sh + (int64_t)(cx0 + cxl) * g.sw] = carry[a] + accT[a];
            carry[a] = accB[a];
          }
        }
      }
    }
  }
  seg_finish(loss_acc, bad, hist, C, state, part, ticket, wsum, loss_out, sh, &sflag);
}

// ---- equal sizes: one read per logit ---------------------------------------------------------------------------------------
template <int CP, bool GEN>
__global__ __launch_bounds__(256) void k_seg_id(const SegGeom g, const float* __restrict__ x, const void* __restrict__ tgt, const float* __restrict__ wt,
                                                 const double* __restrict__ wsum, float* __restrict__ dx, unsigned long long* __restrict__ state,
                                                 double* __restrict__ part, uint32_t* __restrict__ ticket, float* __restrict__ loss_out) {
  extern __shared__ float smem[];
  uint32_t* hist = (uint32_t*)smem;
  __shared__ double sh[8];
  __shared__ int sflag;
  const int tid = threadIdx.x, C = g.c;
  const bool want_dx = dx != nullptr, want_sm = want_dx || loss_out != nullptr;
  for (int i = tid; i < 3 * C; i += 256) hist[i] = 0;
  __syncthreads();
  float inv_wsum = 0.0f;
  if (want_dx) { const double ws = *wsum; inv_wsum = ws > 0.0 ? (float)(1.0 / ws) : 0.0f; }
  double loss_acc = 0.0;
  uint32_t bad = 0;
  const int64_t hw = (int64_t)g.H * g.W, total = hw * g.n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / hw); const int64_t rem = i - (int64_t)n * hw;
    const int Y = (int)(rem / g.W), X = (int)(rem - (int64_t)Y * g.W);
    const int64_t base = (int64_t)n * g.sn + (int64_t)Y * g.sh + (int64_t)X * g.sw;
    const float* p = x + base;
    const int t = seg_target(tgt, g.tbytes, i);
    const bool valid = t < C;
    if (!valid && t != SEG_IGNORE) ++bad;
    const float wgt = valid ? (wt ? wt[t] : 1.0f) : 0.0f;
    const float coef = wgt * inv_wsum;
    if (!valid) {                                                                     // ignored: its gradient is zero, it is in no count
      if (want_dx) for (int c = 0; c < C; ++c) dx[base + (int64_t)c * g.sc] = 0.0f;
      continue;
    }
    float e[CP];
    float m = -INFINITY, ut = 0.0f, s = 0.0f;
    int arg = 0;
    if (!GEN) {
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        e[c] = (c < C) ? p[(int64_t)c * g.sc] : 0.0f;
        if (c < C && e[c] > m) { m = e[c]; arg = c; }
      }
      if (want_sm) {
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          if (c < C) { ut = (c == t) ? e[c] : ut; e[c] = expf(e[c] - m); s += e[c]; }
        }
      }
    } else {
      for (int c = 0; c < C; ++c) { const float u = p[(int64_t)c * g.sc]; if (u > m) { m = u; arg = c; } }
      if (want_sm) for (int c = 0; c < C; ++c) { const float u = p[(int64_t)c * g.sc]; ut = (c == t) ? u : ut; s += expf(u - m); }
    }
    if (loss_out) loss_acc += (double)(wgt * ((m + logf(s)) - ut));
    if (state) { atomicAdd(&hist[2 * C + t], 1u); atomicAdd(&hist[C + arg], 1u); if (arg == t) atomicAdd(&hist[t], 1u); }
    if (want_dx) {
      const float inv_s = 1.0f / s;
      if (!GEN) {
#pragma unroll
        for (int c = 0; c < CP; ++c) { if (c < C) dx[base + (int64_t)c * g.sc] = coef * (e[c] * inv_s - ((c == t) ? 1.0f : 0.0f)); }
      } else {
        for (int c = 0; c < C; ++c) dx[base + (int64_t)c * g.sc] = coef * (expf(p[(int64_t)c * g.sc] - m) * inv_s - ((c == t) ? 1.0f : 0.0f));
      }
    }
  }
  seg_finish(loss_acc, bad, hist, C, state, part, ticket, wsum, loss_out, sh, &sflag);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// workspace: two ticket blocks, W_sum, the partials of the W_sum pass and of the main pass
#define SEG_WS_TICKET_A 0
#define SEG_WS_TICKET_B 256
#define SEG_WS_WSUM 512
#define SEG_WS_PART_A 1024
#define SEG_WS_PART_B (SEG_WS_PART_A + SEG_WSUM_GRID * 8)
#define SEG_WS_BYTES (SEG_WS_PART_B + SEG_MAX_GRID * 8)

extern "C" int frost_seg_workspace_bytes(void) { return SEG_WS_BYTES; }
extern "C" int frost_seg_state_words(int c) { return 3 * c + 2; }

template <int CP, int NT, bool GEN>
static int seg_launch_up(SegGeom g, const float* x, const void* tgt, const float* wt, const double* wsum, float* dx, unsigned long long* state, double* part,
                         uint32_t* ticket, float* loss, hipStream_t st) {
  // columns of one group: ceil((W - 1) / (w - 1)) (+ 1 where the rounding of scale * X moves a boundary); a tile of tw cells walks tw + 1 groups per band
  const int per = g.w > 1 ? (g.W - 1 + g.w - 2) / (g.w - 1) : g.W;
  int tw = NT / (per > 0 ? per : 1) - 1;
  tw = tw < 1 ? 1 : (tw > SEG_TW_MAX ? SEG_TW_MAX : tw);
  const int ntx = (g.w + tw - 1) / tw;
  tw = (g.w + ntx - 1) / ntx;                                          // equal tiles
  int th = 8;
  while (th > 2 && (int64_t)g.n * ((g.h + th - 1) / th) * ntx < 1024) th >>= 1;
  g.th = th; g.tw = tw; g.tiles_y = (g.h + th - 1) / th; g.tiles_x = (g.w + tw - 1) / tw;
  const int64_t nt = (int64_t)g.n * g.tiles_y * g.tiles_x;
  FROST_REQUIRE(nt < (int64_t)1 << 30, "frost_seg_forward: too many tiles");
  g.ntiles = (int)nt;
  constexpr int CS = CP + 1;
  const size_t lds = (size_t)(2 * NT * CS + 3 * SEG_TW_MAX * CS + NT + SEG_TW_MAX + 3 + 3 * g.c) * 4;
  FROST_REQUIRE(lds <= 65536 - 128, "frost_seg_forward: LDS budget");
  const unsigned grid = (unsigned)(nt < SEG_MAX_GRID ? nt : SEG_MAX_GRID);
  hipLaunchKernelGGL((k_seg_up<CP, NT, GEN>), dim3(grid), dim3(NT), lds, st, g, x, tgt, wt, wsum, dx, state, part, ticket, loss);
  return frost_check_launch("seg_up");
}

template <int CP, bool GEN>
static int seg_launch_id(SegGeom g, const float* x, const void* tgt, const float* wt, const double* wsum, float* dx, unsigned long long* state, double* part,
                         uint32_t* ticket, float* loss, hipStream_t st) {
  const int64_t total = (int64_t)g.n * g.H * g.W;
  int64_t blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < SEG_MAX_GRID ? blocks : SEG_MAX_GRID);
  hipLaunchKernelGGL((k_seg_id<CP, GEN>), dim3(grid), dim3(256), (size_t)(3 * g.c) * 4, st, g, x, tgt, wt, wsum, dx, state, part, ticket, loss);
  return frost_check_launch("seg_id");
}

extern "C" int frost_seg_forward(const float* logits, int n, int c, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const void* target,
                                 int target_bytes, int H, int W, const float* class_wts, float* loss, float* dx, int64_t* state, void* workspace, void* stream) {
  FROST_REQUIRE(logits && target && workspace, "frost_seg_forward: null logits, target or workspace");
  FROST_REQUIRE(n >= 1 && h >= 1 && w >= 1, "frost_seg_forward: empty logits");
  FROST_REQUIRE(c >= 2 && c <= 255, "frost_seg_forward: 2 <= classes <= 255 (255 is the ignore label)");
  FROST_REQUIRE(H >= h && W >= w, "frost_seg_forward: the target is smaller than the logits");
  FROST_REQUIRE(target_bytes == 8 || target_bytes == 1, "frost_seg_forward: targets are int64 or uint8");
  FROST_REQUIRE(sn >= 0 && sc >= 1 && sh >= 0 && sw >= 0, "frost_seg_forward: strides");
  FROST_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && (int64_t)n * H * W < ((int64_t)1 << 40), "frost_seg_forward: target too large");
  if (!loss && !dx && !state) return 0;
  hipStream_t st = as_stream(stream);
  uint8_t* ws = (uint8_t*)workspace;
  double* wsum = (double*)(ws + SEG_WS_WSUM);
  if (loss || dx) {
    const int64_t total = (int64_t)n * H * W;
    const int64_t blocks = (total + 2047) / 2048;
    const unsigned grid = (unsigned)(blocks < SEG_WSUM_GRID ? (blocks < 1 ? 1 : blocks) : SEG_WSUM_GRID);
    hipLaunchKernelGGL(k_seg_wsum, dim3(grid), dim3(256), 0, st, target, target_bytes, total, c, class_wts, (double*)(ws + SEG_WS_PART_A),
                       (uint32_t*)(ws + SEG_WS_TICKET_A), wsum);
    if (frost_check_launch("seg_wsum")) return 1;
  }
  SegGeom g = {};
  g.n = n; g.c = c; g.h = h; g.w = w; g.H = H; g.W = W; g.sn = sn; g.sc = sc; g.sh = sh; g.sw = sw; g.tbytes = target_bytes;
  g.scale_y = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f;
  g.scale_x = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
  unsigned long long* stp = (unsigned long long*)state;
  double* part = (double*)(ws + SEG_WS_PART_B);
  uint32_t* ticket = (uint32_t*)(ws + SEG_WS_TICKET_B);
  if (H == h && W == w) {
    if (c <= 8) return seg_launch_id<8, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
    if (c <= 24) return seg_launch_id<24, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
    if (c <= 32) return seg_launch_id<32, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
    return seg_launch_id<1, true>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
  }
  if (c <= 8) return seg_launch_up<8, 256, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
  if (c <= 24) return seg_launch_up<24, 256, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
  if (c <= 32) return seg_launch_up<32, 128, false>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
  return seg_launch_up<32, 128, true>(g, logits, target, class_wts, wsum, dx, stp, part, ticket, loss, st);
}

// stats_weighted.hip -- the item pass of the ML statistics accumulation (stats_accum.hip) with a weight per entry:
// Mixture::accumulate and DiagonalStatisticsAccumulator::accumulate (aku/Distributions.cc:249-260, 2134-2161) with the
// gamma that a Baum-Welch segmentation gives a (frame, pdf) pair, operation by operation: the component's posterior is
// gamma * weight * lik / total, mixture_ll gets gamma * safe_log(total) also where total is 0, the counts go up by one
// per entry with a positive total, aux gamma is fabs.
//
// k_stats_items_w is k_stats_items with that weight: the same dimension instances, LDS layout, slab layout and launch
// shape (stats.h, stats_launch_shape), so the pdf and Gaussian passes of stats_accum.hip reduce its slabs unchanged, and
// with every weight 1.0 it writes the bytes of the plain kernel (1.0 * x is x).  The row list and the weights are device
// arrays; the weight is read from global memory by the lane that owns the frame.
#include <hip/hip_runtime.h>

#include "common.h"
#include "stats.h"

namespace aasr {

// LDS of an item workgroup, as in stats_accum.hip: [records (if staged)][posteriors: block x max_comps]
// [gamma safe_log(total): block][row: block][total > 0: block]
static size_t stats_w_lds_bytes(const StatsParams &p) {
  return (size_t)((p.lds_recs ? p.max_comps * p.rec : 0) + p.block * p.max_comps + p.block) * sizeof(double) +
         (size_t)2 * p.block * sizeof(int32_t);
}

template <int DIMP>
__global__ __launch_bounds__(STATS_THREADS) void k_stats_items_w(StatsParams p, const double *__restrict__ weights, int64_t n_frames) {
  extern __shared__ double lds[];
  const StatsItem it = p.items[blockIdx.x];
  const int D = p.dim, REC = p.rec, B = p.block;
  const int r0 = p.state_off[it.pdf], M = p.state_off[it.pdf + 1] - r0;
  double *lrec = lds;
  double *lg = lds + (p.lds_recs ? p.max_comps * REC : 0);
  double *llt = lg + B * p.max_comps;
  int32_t *lrow = (int32_t *)(llt + B);
  int32_t *lok = lrow + B;
  const double *R = p.recs + (size_t)r0 * REC;
  if (p.lds_recs) {
    for (int i = threadIdx.x; i < M * REC; i += STATS_THREADS) lrec[i] = R[i];
    R = lrec;
    __syncthreads();
  }
  double *slab = p.slab + it.slab;
  const int W = 2 + 2 * D;
  const int NT = M * D + M + 1;  // sums of gamma x and gamma x^2 per (dimension, component), gamma per component, counts
  for (int base = 0; base < it.n; base += B) {
    const int nb = min(B, it.n - base);
    const int t = threadIdx.x;
    if (t < nb) {
      // posteriors, one lane per frame
      const int row = p.rows[it.row_begin + base + t];
      const double w = weights[it.row_begin + base + t];
      const bool in_range = row >= 0 && row < n_frames;
      double x[DIMP];
#pragma unroll
      for (int d = 0; d < DIMP; d++) x[d] = d < D && in_range ? p.x[(size_t)row * D + d] : 0.0;
      double total = 0;
      for (int k = 0; k < M; k++) {
        const double *rec = R + (size_t)k * REC;
        double ll = 0;
#pragma unroll
        for (int d = 0; d < DIMP; d++) {  // padded dimensions: mean 0, precision 0, frame 0 -- they add +0
          const double df = x[d] - rec[d];
          ll += df * df * rec[DIMP + d];
        }
        ll *= -0.5;
        ll += rec[2 * DIMP];
        const double lik = exp(ll);
        lg[t * M + k] = lik;
        total += rec[2 * DIMP + 1] * lik;
      }
      const int ok = total > 0 && in_range;
      if (ok)
        for (int k = 0; k < M; k++) lg[t * M + k] = w * R[(size_t)k * REC + 2 * DIMP + 1] * lg[t * M + k] / total;
      const double sl = total < 1e-50 ? log(1e-50) : log(total);  // util::safe_log
      llt[t] = in_range ? w * sl : 0.0;  // gamma * safe_log(total), the product rounded before it is added
      lrow[t] = row;
      lok[t] = ok;
    }
    __syncthreads();
    // sums over the sub-block's frames in frame order, one thread per output value, carried in the slab
    for (int j = t; j < NT; j += STATS_THREADS) {
      if (j < M * D) {
        const int d = j / M, k = j - d * M;
        double *sx = slab + (size_t)k * W + 2 + d, *sxx = sx + D;
        double ax = base ? *sx : 0.0, axx = base ? *sxx : 0.0;
        for (int f = 0; f < nb; f++) {
          if (!lok[f]) continue;
          const double xv = p.x[(size_t)lrow[f] * D + d];
          const double gx = lg[f * M + k] * xv;
          ax += gx;
          axx += gx * xv;
        }
        *sx = ax;
        *sxx = axx;
      } else if (j < M * D + M) {
        const int k = j - M * D;
        double *s = slab + (size_t)k * W;
        double ag = base ? s[0] : 0.0, aa = base ? s[1] : 0.0;
        for (int f = 0; f < nb; f++) {
          if (!lok[f]) continue;
          const double g = lg[f * M + k];
          ag += g;
          aa += fabs(g);
        }
        s[0] = ag;
        s[1] = aa;
      } else {
        double *s = slab + (size_t)M * W;
        double cnt = base ? s[0] : 0.0, mll = base ? s[1] : 0.0;
        for (int f = 0; f < nb; f++) {
          cnt += lok[f] ? 1.0 : 0.0;
          mll += llt[f];  // gamma * safe_log(total), also where total is 0
        }
        s[0] = cnt;
        s[1] = mll;
      }
    }
    __syncthreads();
  }
}

void stats_items_w_launch(const StatsParams &p, const double *weights, int64_t n_frames, int dimp, int n_items,
                          hipStream_t stream) {
  if (n_items <= 0) return;
  const size_t lds = stats_w_lds_bytes(p);
#define AASR_CASE(N)                                                                                          \
  case N:                                                                                                     \
    hipLaunchKernelGGL(k_stats_items_w<N>, dim3((unsigned)n_items), dim3(STATS_THREADS), lds, stream, p, weights, \
                       n_frames);                                                                             \
    break;
  switch (dimp) {
    AASR_CASE(8)
    AASR_CASE(16)
    AASR_CASE(24)
    AASR_CASE(32)
    AASR_CASE(40)
    AASR_CASE(48)
    AASR_CASE(64)
    AASR_CASE(96)
    AASR_CASE(128)
    AASR_CASE(192)
    default:
      raise(AASR_ERR_UNSUPPORTED, "stats: no weighted accumulation kernel for padded dimension %d", dimp);
  }
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

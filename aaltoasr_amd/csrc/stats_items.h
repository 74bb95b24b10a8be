// stats_items.h -- the item pass of the ML statistics accumulation, once for its two kernels: k_stats_items
// (stats_accum.hip: every frame of the row list with gamma 1) and k_stats_items_w (stats_weighted.hip: a weight per
// entry of the row list).  Device code only; the layout is stats.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_loglik.h"
#include "stats.h"

namespace aasr {

// LDS of an item workgroup: [records (if staged)][posteriors: block x max_comps][gamma safe_log(total): block]
// [row: block][total > 0: block]
inline size_t stats_items_lds_bytes(const StatsParams &p) {
  return (size_t)((p.lds_recs ? p.max_comps * p.rec : 0) + p.block * p.max_comps + p.block) * sizeof(double) +
         (size_t)2 * p.block * sizeof(int32_t);
}

// One workgroup per work item.  WEIGHTED: entry e of the row list has gamma weights[e] and may name a row outside
// 0 .. n_frames, for which no frame is read and nothing is added; p.frame_ll is not written.  Otherwise gamma is 1.0
// (1.0 * x is x: with every weight 1.0 the weighted kernel writes the plain kernel's bytes), every row is in range and
// weights and n_frames are not looked at.  p comes by value, as the kernels get it: through a reference the <192>
// instance, the one that spills, spills four more registers (tests/test_kernel_notes.py holds it where it is).
template <int DIMP, bool WEIGHTED>
__device__ __forceinline__ void stats_items_body(StatsParams p, const double *__restrict__ weights, int64_t n_frames) {
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
      double w = 1.0;
      if (WEIGHTED) w = weights[it.row_begin + base + t];
      const bool in_range = !WEIGHTED || (row >= 0 && row < n_frames);
      double x[DIMP];
#pragma unroll
      for (int d = 0; d < DIMP; d++) x[d] = d < D && in_range ? p.x[(size_t)row * D + d] : 0.0;
      double total = 0;
      for (int k = 0; k < M; k++) {
        const double *rec = R + (size_t)k * REC;
        const double lik = exp(diag_loglik<DIMP>(x, rec, DIMP, DIMP));
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
      if (!WEIGHTED && p.frame_ll) p.frame_ll[row] = sl;
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

}  // namespace aasr

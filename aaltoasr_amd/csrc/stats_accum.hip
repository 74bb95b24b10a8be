// stats_accum.hip -- ML statistics accumulation on the device: Mixture::accumulate and
// DiagonalStatisticsAccumulator::accumulate (aku/Distributions.cc:249-260, 2134-2161) over many
// frames at once, with the likelihoods of DiagonalGaussian::compute_log_likelihood and
// Mixture::compute_likelihood (Distributions.cc:1040-1062, 2079-2086) in double, operation by operation.
//
// Three passes (stats.h): one workgroup per work item (a pdf and up to STATS_CHUNK of its frames) sums
// its frames into a slab; one workgroup per pdf adds its slabs in item order into the record
// accumulators; at fetch time one workgroup per pool Gaussian adds the records that share it.  Within an
// item every sum runs over the frames in frame order, one thread per output value.
#include <hip/hip_runtime.h>

#include "common.h"
#include "stats.h"

namespace aasr {

// LDS of an item workgroup: [records (if staged)][posteriors: block x max_comps][safe_log(total): block]
// [row: block][total > 0: block]
static size_t stats_lds_bytes(const StatsParams &p) {
  return (size_t)((p.lds_recs ? p.max_comps * p.rec : 0) + p.block * p.max_comps + p.block) * sizeof(double) +
         (size_t)2 * p.block * sizeof(int32_t);
}

template <int DIMP>
__global__ __launch_bounds__(STATS_THREADS) void k_stats_items(StatsParams p) {
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
      double x[DIMP];
#pragma unroll
      for (int d = 0; d < DIMP; d++) x[d] = d < D ? p.x[(size_t)row * D + d] : 0.0;
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
      const int ok = total > 0;
      if (ok)
        for (int k = 0; k < M; k++) lg[t * M + k] = 1.0 * R[(size_t)k * REC + 2 * DIMP + 1] * lg[t * M + k] / total;
      const double sl = total < 1e-50 ? log(1e-50) : log(total);  // util::safe_log
      llt[t] = sl;
      lrow[t] = row;
      lok[t] = ok;
      if (p.frame_ll) p.frame_ll[row] = sl;
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
          mll += 1.0 * llt[f];  // gamma * safe_log(total) with gamma = 1, also where total is 0
        }
        s[0] = cnt;
        s[1] = mll;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(STATS_THREADS) void k_stats_pdf_reduce(const int32_t *__restrict__ pdfs,
                                                                    const int32_t *__restrict__ item_begin,
                                                                    const StatsItem *__restrict__ items,
                                                                    const double *__restrict__ slab,
                                                                    const int32_t *__restrict__ state_off, int D,
                                                                    double *__restrict__ racc, double *__restrict__ pacc) {
  const int q = blockIdx.x, pdf = pdfs[q];
  const int r0 = state_off[pdf], M = state_off[pdf + 1] - r0;
  const int W = 2 + 2 * D, n = M * W + 2;
  const int i0 = item_begin[q], i1 = item_begin[q + 1];
  for (int j = threadIdx.x; j < n; j += STATS_THREADS) {
    double *dst = j < M * W ? racc + (size_t)r0 * W + j : pacc + 2 * (size_t)pdf + (j - M * W);
    double a = *dst;
    for (int i = i0; i < i1; i++) a += slab[items[i].slab + j];
    *dst = a;
  }
}

__global__ __launch_bounds__(128) void k_stats_gauss_reduce(const double *__restrict__ racc,
                                                            const double *__restrict__ pacc,
                                                            const int32_t *__restrict__ g_off,
                                                            const int32_t *__restrict__ g_rec,
                                                            const int32_t *__restrict__ rec_pdf, int D,
                                                            double *__restrict__ gacc) {
  const int g = blockIdx.x;
  const int W = 2 + 2 * D;
  const int a0 = g_off[g], a1 = g_off[g + 1];
  for (int j = threadIdx.x; j < W + 1; j += 128) {
    double a = 0;
    for (int i = a0; i < a1; i++) {
      const int r = g_rec[i];
      a += j == 0 ? pacc[2 * (size_t)rec_pdf[r]] : racc[(size_t)r * W + j - 1];
    }
    gacc[(size_t)g * (W + 1) + j] = a;
  }
}

void stats_items_launch(const StatsParams &p, int dimp, int n_items, hipStream_t stream) {
  if (n_items <= 0) return;
  const size_t lds = stats_lds_bytes(p);
#define AASR_CASE(N)                                                                                        \
  case N:                                                                                                   \
    hipLaunchKernelGGL(k_stats_items<N>, dim3((unsigned)n_items), dim3(STATS_THREADS), lds, stream, p); \
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
      raise(AASR_ERR_UNSUPPORTED, "stats: no accumulation kernel for padded dimension %d", dimp);
  }
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
}

void stats_pdf_reduce_launch(const int32_t *pdfs, const int32_t *item_begin, int n_pdfs, const StatsItem *items,
                             const double *slab, const int32_t *state_off, int dim, double *racc, double *pacc,
                             hipStream_t stream) {
  if (n_pdfs <= 0) return;
  hipLaunchKernelGGL(k_stats_pdf_reduce, dim3((unsigned)n_pdfs), dim3(STATS_THREADS), 0, stream, pdfs, item_begin,
                     items, slab, state_off, dim, racc, pacc);
  AASR_HIP(hipGetLastError());
}

void stats_gauss_reduce_launch(const double *racc, const double *pacc, const int32_t *g_off, const int32_t *g_rec,
                               const int32_t *rec_pdf, int n_gauss, int dim, double *gacc, hipStream_t stream) {
  if (n_gauss <= 0) return;
  hipLaunchKernelGGL(k_stats_gauss_reduce, dim3((unsigned)n_gauss), dim3(128), 0, stream, racc, pacc, g_off, g_rec,
                     rec_pdf, dim, gacc);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

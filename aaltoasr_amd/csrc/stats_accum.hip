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
#include "stats_items.h"

namespace aasr {

template <int DIMP>
__global__ __launch_bounds__(STATS_THREADS) void k_stats_items(StatsParams p) {
  stats_items_body<DIMP, false>(p, nullptr, 0);
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
  const bool launched = dispatch_dimp(dimp, [&](auto n) {
    hipLaunchKernelGGL(k_stats_items<n()>, dim3((unsigned)n_items), dim3(STATS_THREADS), stats_items_lds_bytes(p), stream, p);
  });
  if (!launched) raise(AASR_ERR_UNSUPPORTED, "stats: no accumulation kernel for padded dimension %d", dimp);
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

// stats_weighted.hip -- the item pass of the ML statistics accumulation (stats_accum.hip) with a weight per entry:
// Mixture::accumulate and DiagonalStatisticsAccumulator::accumulate (aku/Distributions.cc:249-260, 2134-2161) with the
// gamma that a Baum-Welch segmentation gives a (frame, pdf) pair, operation by operation: the component's posterior is
// gamma * weight * lik / total, mixture_ll gets gamma * safe_log(total) also where total is 0, the counts go up by one
// per entry with a positive total, aux gamma is fabs.
//
//
// k_stats_items_w and k_stats_items are one body (stats_items.h): the same dimension instances, LDS layout, slab layout
// and launch shape (stats.h, stats_launch_shape), so the pdf and Gaussian passes of stats_accum.hip reduce its slabs
// unchanged, and with every weight 1.0 it writes the bytes of the plain kernel.  The row list and the weights are device
// arrays; the weight is read from global memory by the lane that owns the frame.
#include <hip/hip_runtime.h>

#include "common.h"
#include "stats.h"
#include "stats_items.h"

namespace aasr {

template <int DIMP>
__global__ __launch_bounds__(STATS_THREADS) void k_stats_items_w(StatsParams p, const double *__restrict__ weights, int64_t n_frames) {
  stats_items_body<DIMP, true>(p, weights, n_frames);
}

void stats_items_w_launch(const StatsParams &p, const double *weights, int64_t n_frames, int dimp, int n_items,
                          hipStream_t stream) {
  if (n_items <= 0) return;
  const bool launched = dispatch_dimp(dimp, [&](auto n) {
    hipLaunchKernelGGL(k_stats_items_w<n()>, dim3((unsigned)n_items), dim3(STATS_THREADS), stats_items_lds_bytes(p), stream, p,
                       weights, n_frames);
  });
  if (!launched) raise(AASR_ERR_UNSUPPORTED, "stats: no weighted accumulation kernel for padded dimension %d", dimp);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

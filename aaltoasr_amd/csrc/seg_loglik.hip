// seg_loglik.hip -- per frame the log-likelihood of the pdf its segmentation gives it (seg_loglik.h): the
// likelihoods of DiagonalGaussian::compute_log_likelihood and Mixture::compute_likelihood
// (aku/Distributions.cc:1040-1062, 2079-2086) in double and util::safe_log of the total, operation by operation
// as k_stats_items (stats_accum.hip) states them -- its frame_ll, byte for byte, without the accumulation.
//
// One workgroup per work item, one lane per row.  A sub-block of the item's rows is staged in LDS (a wave per row, the
// lanes along the row: whole contiguous rows from global memory), then every lane walks all the mixture's components
// over its own row, SEGLL_KB of them per pass.  The records' address is the same for every lane, so the compiler
// fetches them with scalar loads (the code object holds s_load_dwordx* in the component loop and no vector load of a
// record).  A component's sum runs over the dimensions in order and the total over the components in order, whatever
// the pass width: the passes only share the row operand.
#include <hip/hip_runtime.h>

#include "common.h"
#include "seg_loglik.h"

namespace aasr {

__global__ __launch_bounds__(SEGLL_ITEM) void k_segll_items(const double *__restrict__ x,
                                                            const int32_t *__restrict__ rows,
                                                            const SegllItem *__restrict__ items,
                                                            const double *__restrict__ recs,
                                                            const int32_t *__restrict__ state_off,
                                                            double *__restrict__ frame_ll, int D, int DIMP, int stride,
                                                            int sub) {
  extern __shared__ double lx[];
  const SegllItem it = items[blockIdx.x];
  const int REC = 2 * DIMP + 2;
  const int r0 = state_off[it.pdf], M = state_off[it.pdf + 1] - r0;
  const double *R = recs + (size_t)r0 * REC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int base = 0; base < it.n; base += sub) {
    const int nb = min(sub, it.n - base);
    if (base) __syncthreads();  // the previous sub-block's rows are still being read
    for (int r = wave; r < nb; r += SEGLL_ITEM / 64) {
      const double *src = x + (size_t)rows[it.row_begin + base + r] * D;
      for (int d = lane; d < D; d += 64) lx[r * stride + d] = src[d];
    }
    __syncthreads();
    if (t < nb) {
      const double *xr = lx + t * stride;
      double total = 0;
      for (int k = 0; k < M; k += SEGLL_KB) {
        // (a pass past the mixture's end reads its last record again and adds nothing)
        const int kb = min(SEGLL_KB, M - k);
        const double *a0 = R + (size_t)k * REC, *a1 = R + (size_t)min(k + 1, M - 1) * REC;
        const double *a2 = R + (size_t)min(k + 2, M - 1) * REC, *a3 = R + (size_t)min(k + 3, M - 1) * REC;
        double l0 = 0, l1 = 0, l2 = 0, l3 = 0;
        for (int d = 0; d < D; d++) {
          const double xv = xr[d];
          const double d0 = xv - a0[d], d1 = xv - a1[d], d2 = xv - a2[d], d3 = xv - a3[d];
          l0 += d0 * d0 * a0[DIMP + d];
          l1 += d1 * d1 * a1[DIMP + d];
          l2 += d2 * d2 * a2[DIMP + d];
          l3 += d3 * d3 * a3[DIMP + d];
        }
#pragma unroll 1
        for (int j = 0; j < kb; j++) {  // in component order; one copy of exp in the code
          const double *a = a0 + (size_t)j * REC;
          double ll = j == 0 ? l0 : j == 1 ? l1 : j == 2 ? l2 : l3;
          ll *= -0.5;
          ll += a[2 * DIMP];
          total += a[2 * DIMP + 1] * exp(ll);
        }
      }
      frame_ll[rows[it.row_begin + base + t]] = total < 1e-50 ? log(1e-50) : log(total);  // util::safe_log
    }
  }
}

void segll_items_launch(const SegllParams &p, int n_items, hipStream_t stream) {
  if (n_items <= 0) return;
  const size_t lds = (size_t)p.sub * p.stride * sizeof(double);
  hipLaunchKernelGGL(k_segll_items, dim3((unsigned)n_items), dim3(SEGLL_ITEM), lds, stream, p.x, p.rows, p.items, p.recs,
                     p.state_off, p.frame_ll, p.dim, p.dimp, p.stride, p.sub);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

// diag_loglik.h -- the log-likelihood of DiagonalGaussian::compute_log_likelihood (aku/Distributions.cc:1040-1062) in
// double, operation by operation, for the device kernels that evaluate an AASR_PREC_F64 record
// ([mean x dimp][precision x dimp][constant, weight]) against a frame: the statistics item kernels (stats_items.h),
// k_full_lik (stats_full_accum.hip) and pass 1 of the CMLLR statistics (mllr_pass1.h).
#pragma once
#include <hip/hip_runtime.h>

namespace aasr {

// The sum of df * df * precision over the first n dimensions in order, * -0.5, + constant.  prec_off: the record's
// padded dimension.  Padded dimensions (mean 0, precision 0, frame 0) add +0 to a sum that is never -0, so a caller
// may run over them or stop at the model's dimension: the bits are the same.  N > 0: n is N, and the loop is unrolled
// whole, which a caller that holds its frame in registers needs; otherwise the loop is left to the compiler.
template <int N = 0>
__device__ __forceinline__ double diag_loglik(const double *x, const double *rec, int n, int prec_off) {
  double ll = 0;
  auto add = [&](int d) {
    const double df = x[d] - rec[d];
    ll += df * df * rec[prec_off + d];
  };
  if constexpr (N > 0) {
#pragma unroll
    for (int d = 0; d < N; d++) add(d);
  } else {
    for (int d = 0; d < n; d++) add(d);
  }
  ll *= -0.5;
  ll += rec[2 * prec_off];
  return ll;
}

}  // namespace aasr

// mllr_pass1.h -- the posterior step that the two pass-1 kernels of the CMLLR statistics share: k_mllr_weights
// (mllr_accum.hip, one pdf of probability 1 per frame) and k_mllr_entry_pass1 (mllr_entries.hip, a list of
// (pdf, probability) per frame).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_loglik.h"
#include "mllr.h"

namespace aasr {

// A frame lane evaluates the M records from r0 on against its frame x into lg[0 ... M): the likelihoods of
// DiagonalGaussian::compute_log_likelihood, then the posteriors prior * lik / sum, which ignore the mixture weights
// (MllrTrainer.cc:40-49).  A component whose value is not > 0 adds nothing (MllrTrainer.cc:153), so a pdf whose sum is 0
// or not finite adds nothing at all.  -> beta with the posteriors added to it in component order.
__device__ __forceinline__ double mllr_posteriors(const MllrParams &p, const double *x, int r0, int M, double prior,
                                                  double *lg, double beta) {
  double sum = 0;
  for (int k = 0; k < M; k++) {
    const double lik = exp(diag_loglik(x, p.recs + (size_t)(r0 + k) * p.rec, p.dim, p.dimp));
    lg[k] = lik;
    sum += lik;
  }
  for (int k = 0; k < M; k++) {
    double pr = prior * lg[k] / sum;
    if (!(pr > 0)) pr = 0;
    lg[k] = pr;
    beta += pr;
  }
  return beta;
}

}  // namespace aasr

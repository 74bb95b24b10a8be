// mllr_entries.hip -- pass 1 of the CMLLR statistics (mllr.h) from weighted entries: MllrTrainer::collect_data
// (aku/MllrTrainer.cc:22-60, 147-163) called once per (pdf, probability) of a frame, as train_mllr calls it over
// Segmentator::pdf_probs (aku/mllr.cc:136-141).  k_mllr_weights (mllr_accum.hip) is the case of one pdf of probability 1
// per frame; here a frame has a list, of any length, so the workgroup goes round by round: in round r the frame lanes
// evaluate their r-th entry into the LDS posterior area of k_mllr_weights, operation by operation as that kernel does,
// and the (frame, dimension) threads add the round to the w and u they keep in registers.  The sums of a frame continue
// across its entries in list order; with one entry of weight 1.0 they are k_mllr_weights' sums, byte for byte.  Lanes of
// frames with few entries idle while the workgroup's longest list finishes.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.h"
#include "mllr.h"
#include "mllr_pass1.h"

namespace aasr {

// (frame, dimension) values a thread keeps: thread tid has dimension tid % 64 of the frames tid / 64 + 4 s
constexpr int MLLR_E_SLOTS = MLLR_P1_FRAMES * 64 / MLLR_THREADS;
static_assert(MLLR_MAX_DIM < 64 && MLLR_P1_FRAMES * 64 % MLLR_THREADS == 0, "the (frame, dimension) map of pass 1");

size_t mllr_entry_weights_lds_bytes(int dim, int max_comps) {
  return mllr_weights_lds_bytes(dim, max_comps) + (size_t)MLLR_P1_FRAMES * sizeof(int32_t);
}

// LDS: k_mllr_weights' [frames][posteriors][beta share: unused][first record][components], then [entries: 64]
__global__ __launch_bounds__(MLLR_THREADS) void k_mllr_entry_pass1(MllrEntryParams q) {
  extern __shared__ double lds[];
  const MllrParams &p = q.p;
  const int D = p.dim, XS = D | 1, MC = p.max_comps, B = MLLR_P1_FRAMES;
  double *xs = lds;
  double *lg = xs + B * XS;
  double *lbeta = lg + B * MC;
  int32_t *lr0 = (int32_t *)(lbeta + B);
  int32_t *lm = lr0 + B;
  int32_t *lcnt = lm + B;
  const int f0 = blockIdx.x * B, nb = min(B, p.n - f0);
  const int tid = threadIdx.x;
  for (int j = tid; j < nb * D; j += MLLR_THREADS) {
    const int t = j / D, d = j - t * D;
    xs[t * XS + d] = p.x[(size_t)(f0 + t) * D + d];
  }
  // the frame lanes: their list, and the workgroup's rounds
  int64_t e0 = 0, e1 = 0;
  if (tid < B) {
    if (tid < nb) {
      e0 = q.off[f0 + tid];
      e1 = q.off[f0 + tid + 1];
      if (e0 < 0 || e1 < e0 || e1 > q.n_entries) e1 = e0;  // (offsets that do not describe the arrays: no entries)
    }
    lcnt[tid] = e1 - e0 > (int64_t)INT_MAX ? INT_MAX : (int32_t)(e1 - e0);
  }
  __syncthreads();
  int rounds = 0;
  for (int t = 0; t < B; t++) rounds = max(rounds, lcnt[t]);
  const int i = tid & 63, tq = tid >> 6;
  double w[MLLR_E_SLOTS], u[MLLR_E_SLOTS];
#pragma unroll
  for (int s = 0; s < MLLR_E_SLOTS; s++) w[s] = u[s] = 0;
  double beta = 0;
  for (int r = 0; r < rounds; r++) {
    if (tid < nb) {
      const int t = tid;
      int r0 = 0, M = 0;
      double pw = 0;
      if (r < e1 - e0) {
        const int pdf = q.pdf[e0 + r];
        pw = q.weight[e0 + r];
        if (pdf >= 0 && pdf < q.n_states) {
          r0 = p.state_off[pdf];
          M = p.state_off[pdf + 1] - r0;
        }
      }
      // the entry's probability as the prior
      beta = mllr_posteriors(p, xs + t * XS, r0, M, pw, lg + t * MC, beta);
      lr0[t] = r0;
      lm[t] = M;
    }
    __syncthreads();
    if (i < D) {
#pragma unroll
      for (int s = 0; s < MLLR_E_SLOTS; s++) {
        const int t = tq + (MLLR_THREADS / 64) * s;
        if (t >= nb) continue;
        const int r0 = lr0[t], M = lm[t];
        double ws = w[s], us = u[s];
        for (int g = 0; g < M; g++) {
          const double pr = lg[t * MC + g];
          if (!(pr > 0)) continue;
          ws += p.inv_var[(size_t)(r0 + g) * D + i] * pr;   // 1 / covar(i) * prob
          us += p.mean_var[(size_t)(r0 + g) * D + i] * pr;  // mean(i) / covar(i) * prob
        }
        w[s] = ws;
        u[s] = us;
      }
    }
    __syncthreads();
  }
  const int DU = D + 1;
  if (tid < nb) {
    p.u[(size_t)(f0 + tid) * DU + D] = beta;
    p.ok[f0 + tid] = beta > 0 ? 1 : 0;
  }
  if (i < D) {
#pragma unroll
    for (int s = 0; s < MLLR_E_SLOTS; s++) {
      const int t = tq + (MLLR_THREADS / 64) * s;
      if (t >= nb) continue;
      p.w[(size_t)(f0 + t) * D + i] = w[s];
      p.u[(size_t)(f0 + t) * DU + i] = u[s];
    }
  }
}

void mllr_entry_weights_launch(const MllrEntryParams &q, hipStream_t stream) {
  if (q.p.n <= 0) return;
  const unsigned blocks = (unsigned)((q.p.n + MLLR_P1_FRAMES - 1) / MLLR_P1_FRAMES);
  hipLaunchKernelGGL(k_mllr_entry_pass1, dim3(blocks), dim3(MLLR_THREADS),
                     mllr_entry_weights_lds_bytes(q.p.dim, q.p.max_comps), stream, q);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

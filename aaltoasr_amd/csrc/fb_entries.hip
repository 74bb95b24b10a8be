// fb_entries.hip -- per-frame pdf occupancies of the forward-backward pass (hmmnet_fb.hip) into the weighted entries of
// the statistics accumulation, on the device: the per-frame sum and division of HmmNetBaumWelch::next_frame
// (aku/HmmNetBaumWelch.cc:714-789) in dense form.  Layout and order: fb_entries.h.  Every value has one lane and one
// fixed order of operations; nothing is added across lanes.
#include <hip/hip_runtime.h>

#include "common.h"
#include "fb_entries.h"

namespace aasr {

__global__ __launch_bounds__(FBE_THREADS) void k_fb_frame_sums(const FbEntryUtt *__restrict__ utt,
                                                               const double *__restrict__ occ,
                                                               double *__restrict__ sums) {
  const FbEntryUtt u = utt[blockIdx.y];
  const int t = blockIdx.x * FBE_THREADS + threadIdx.x;
  if (t >= u.T) return;
  const double *o = occ + u.occ + (int64_t)t * u.n_pdf;
  double s = 0;
  for (int j = 0; j < u.n_pdf; j++) s += o[j];
  sums[u.sums + t] = s;
}

__global__ __launch_bounds__(FBE_THREADS) void k_fb_entry_counts(const FbEntryUtt *__restrict__ utt,
                                                                 const FbEntryPair *__restrict__ pairs, int n_pairs,
                                                                 const double *__restrict__ occ,
                                                                 int32_t *__restrict__ counts) {
  const int q = blockIdx.x * FBE_THREADS + threadIdx.x;
  if (q >= n_pairs) return;
  const FbEntryPair p = pairs[q];
  const FbEntryUtt u = utt[p.utt];
  const double *o = occ + u.occ + p.slot;
  int32_t n = 0;
  for (int t = 0; t < u.T; t++) n += o[(int64_t)t * u.n_pdf] > 0 ? 1 : 0;
  counts[q] = n;
}

__global__ __launch_bounds__(FBE_THREADS) void k_fb_entry_fill(const FbEntryUtt *__restrict__ utt,
                                                               const FbEntryPair *__restrict__ pairs, int n_pairs,
                                                               const double *__restrict__ occ,
                                                               const double *__restrict__ sums,
                                                               const int64_t *__restrict__ out,
                                                               int32_t *__restrict__ rows, double *__restrict__ weights) {
  const int q = blockIdx.x * FBE_THREADS + threadIdx.x;
  if (q >= n_pairs) return;
  const FbEntryPair p = pairs[q];
  const FbEntryUtt u = utt[p.utt];
  const double *o = occ + u.occ + p.slot;
  const double *s = sums + u.sums;
  int64_t at = out[q];
  const int64_t end = out[q + 1];  // the count pass found as many entries: nothing is written past them
  for (int t = 0; t < u.T && at < end; t++) {
    const double g = o[(int64_t)t * u.n_pdf];
    if (!(g > 0)) continue;
    rows[at] = (int32_t)(u.row0 + t);
    weights[at] = g / s[t];
    at++;
  }
}

void fb_frame_sums_launch(const FbEntryUtt *utt, int32_t n_utt, int32_t max_T, const double *occ, double *sums,
                          hipStream_t stream) {
  if (n_utt <= 0 || max_T <= 0) return;
  hipLaunchKernelGGL(k_fb_frame_sums, dim3((unsigned)((max_T + FBE_THREADS - 1) / FBE_THREADS), (unsigned)n_utt),
                     dim3(FBE_THREADS), 0, stream, utt, occ, sums);
  AASR_HIP(hipGetLastError());
}

void fb_entry_counts_launch(const FbEntryUtt *utt, const FbEntryPair *pairs, int32_t n_pairs, const double *occ,
                            int32_t *counts, hipStream_t stream) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL(k_fb_entry_counts, dim3((unsigned)((n_pairs + FBE_THREADS - 1) / FBE_THREADS)), dim3(FBE_THREADS), 0,
                     stream, utt, pairs, n_pairs, occ, counts);
  AASR_HIP(hipGetLastError());
}

void fb_entry_fill_launch(const FbEntryUtt *utt, const FbEntryPair *pairs, int32_t n_pairs, const double *occ,
                          const double *sums, const int64_t *out, int32_t *rows, double *weights, hipStream_t stream) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL(k_fb_entry_fill, dim3((unsigned)((n_pairs + FBE_THREADS - 1) / FBE_THREADS)), dim3(FBE_THREADS), 0,
                     stream, utt, pairs, n_pairs, occ, sums, out, rows, weights);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

// fst_conf.hip -- the device passes of the FST decoder's confidence: the best acoustic value of every frame and its
// per-utterance sum, and the best different hypothesis among a search's surviving tokens (layout: fst_conf.h; the row
// sweep and the record's body: fst_conf_frame.h, shared with k_fst_conf_chunk).
#include "fst_conf_frame.h"

namespace aasr {

template <int BYTES>
__global__ __launch_bounds__(FSTC_THREADS) void k_fst_frame_best(const FstFrameBestParams p, const int64_t total) {
  const int lane = threadIdx.x & 63, lpr = p.lanes_per_row, sub = lane & (lpr - 1);
  int64_t f = ((int64_t)blockIdx.x * (FSTC_THREADS / 64) + (threadIdx.x >> 6)) * (64 / lpr) + lane / lpr;
  const bool live = f < total;
  if (!live) f = total - 1;  // (the lanes past the last row sweep it once more and write nothing: every lane shuffles)
  int32_t lo = 0, hi = p.n_utt - 1;  // the last utterance whose first frame is <= f: the one that holds f
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (p.frame_off[mid] <= f)
      lo = mid;
    else
      hi = mid - 1;
  }
  const size_t row_bytes = (size_t)p.n_models * BYTES;
  const uintptr_t s = (uintptr_t)p.lna + (size_t)(p.row0[lo] + (f - p.frame_off[lo])) * row_bytes, e = s + row_bytes;
  const float best = fst_row_best<BYTES>(s, e, sub, lpr, p.decode);
  if (live && sub == 0) p.frame_best[f] = best;
}

// one wave per utterance: 64 maxima per coalesced load, then the reference's chain over them, the same in every lane
__global__ __launch_bounds__(FSTC_THREADS) void k_fst_frame_sum(const FstFrameBestParams p) {
  const int lane = threadIdx.x & 63;
  const int32_t u = (int32_t)(blockIdx.x * (FSTC_THREADS / 64) + (threadIdx.x >> 6));
  if (u >= p.n_utt) return;  // (the whole wave)
  const int64_t end = p.frame_off[u + 1];
  float sum = 0.0f;  // FstConfidenceWithPhoneLoop::run: m_best_acu_score = 0, += per frame
  for (int64_t base = p.frame_off[u]; base < end; base += 64) {
    const float v = base + lane < end ? p.frame_best[base + lane] : 0.0f;
    const int n = end - base < 64 ? (int)(end - base) : 64;
    for (int j = 0; j < n; j++) sum = __fadd_rn(sum, __shfl(v, j, 64));
  }
  if (lane == 0) p.sum[u] = sum;
}

__global__ __launch_bounds__(FSTC_THREADS) void k_fst_conf_tokens(const FstParams p, FstConfRecord *rec) {
  __shared__ FstConfLds s;
  fst_conf_record(p, (int32_t)blockIdx.x, s, rec);
}

void fst_frame_best_launch(const FstFrameBestParams &p, int64_t total_frames, hipStream_t st) {
  if (p.n_utt <= 0) return;
  if (total_frames > 0) {
    FstFrameBestParams q = p;
    q.lanes_per_row = fst_lanes_per_row(p.n_models, p.lnabytes);
    const int64_t rows_per_group = (int64_t)(FSTC_THREADS / 64) * (64 / q.lanes_per_row);
    const dim3 grid((unsigned)((total_frames + rows_per_group - 1) / rows_per_group)), block(FSTC_THREADS);
    if (p.lnabytes == 4)
      hipLaunchKernelGGL(k_fst_frame_best<4>, grid, block, 0, st, q, total_frames);
    else if (p.lnabytes == 2)
      hipLaunchKernelGGL(k_fst_frame_best<2>, grid, block, 0, st, q, total_frames);
    else
      hipLaunchKernelGGL(k_fst_frame_best<1>, grid, block, 0, st, q, total_frames);
  }
  hipLaunchKernelGGL(k_fst_frame_sum, dim3((unsigned)((p.n_utt + FSTC_THREADS / 64 - 1) / (FSTC_THREADS / 64))), dim3(FSTC_THREADS), 0, st, p);
}

void fst_conf_tokens_launch(const FstParams &p, FstConfRecord *rec, int32_t n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_fst_conf_tokens, dim3((unsigned)n_launch), dim3(FSTC_THREADS), 0, st, p, rec);
}

}  // namespace aasr

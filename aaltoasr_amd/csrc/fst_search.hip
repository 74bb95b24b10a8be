// fst_search.hip -- the FST decoder's token pass: one workgroup per utterance, the frame loop inside (layout, phases
// and the reference's line numbers: fst_search.h; the body of a frame and the result block: fst_frame.h, shared with
// the resumable entry of fst_stream.hip).
#include "fst_frame.h"

namespace aasr {

__global__ __launch_bounds__(FST_THREADS) void k_fst_search(const FstParams p) {
  __shared__ FstLds s;

  const int32_t u = (int32_t)blockIdx.x;
  const int32_t T = p.n_frames[u];
  const FstUtt m = fst_utt(p, u);

  fst_start(p, m, s);
  int32_t n_act = 1, status = FST_OK;
  for (int32_t t = 0; t < T; t++) {
    const uint8_t *row = p.lna + (size_t)(p.row0[u] + t) * (size_t)p.n_models * (size_t)p.lnabytes;
    status = fst_frame(p, m, s, row, n_act);
    if (status != FST_OK) break;
  }
  fst_result(p, m, s, u, status, n_act);
}

void fst_search_launch(const FstParams &p, int32_t n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_fst_search, dim3((unsigned)n_launch), dim3(FST_THREADS), 0, st, p);
}

}  // namespace aasr

// fst_stream.hip -- the resumable entry of the FST token pass: one workgroup per session, the frames of one feed
// (layout and rules: fst_stream.h; the feed's body: fst_chunk.h, shared with k_fst_conf_chunk; the frame body and the
// result block: fst_frame.h, shared with k_fst_search).
#include "fst_chunk.h"

namespace aasr {

__global__ __launch_bounds__(FST_THREADS) void k_fst_search_chunk(const FstParams p, const FstStreamParams q) {
  __shared__ FstLds s;
  fst_chunk(p, q, s, (int32_t)blockIdx.x);
}

void fst_stream_launch(const FstParams &p, const FstStreamParams &q, int32_t n_sessions, hipStream_t st) {
  if (n_sessions <= 0) return;
  hipLaunchKernelGGL(k_fst_search_chunk, dim3((unsigned)n_sessions), dim3(FST_THREADS), 0, st, p, q);
}

}  // namespace aasr

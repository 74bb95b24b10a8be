// fst_conf_stream.hip -- the confidence's resumable entry: per feed one launch that runs a session's grammar search, its
// phone-loop search and its best-acoustics carry as sibling workgroups (layout and rules: fst_conf_stream.h; the bodies:
// fst_chunk.h, fst_conf_frame.h, shared with k_fst_search_chunk, k_fst_conf_tokens and k_fst_frame_best).
#include "fst_chunk.h"
#include "fst_conf_frame.h"
#include "fst_conf_stream.h"

namespace aasr {

namespace {

struct FstConfChunkLds {
  FstLds search;
  FstConfLds record;
};

// roles 0 and 1: the feed's frames, then the record over the tokens they left
__device__ __forceinline__ void search_role(const FstParams &p, const FstStreamParams &q, FstConfChunkLds &s, int32_t u, FstConfRecord *rec) {
  if (!fst_chunk(p, q, s.search, u)) return;  // (the whole workgroup) the record stays as it is
  __threadfence();
  __syncthreads();  // result[u] was written by one lane
  fst_conf_record(p, u, s.record, rec);
}

// role 2: 256 / lpr rows per pass; their best values go through LDS to the chain, which every lane runs alike
template <int BYTES>
__device__ __forceinline__ void acu_role(const FstParams &p, const FstFeed f, const FstConfStreamParams &c, unsigned *s_val, int32_t u) {
  const int tid = threadIdx.x, lpr = c.lanes_per_row, sub = tid & (lpr - 1), r = tid / lpr, rows = FST_THREADS / lpr;
  if (!f.fresh && f.n_new <= 0) return;  // (the whole workgroup)
  float sum = f.fresh ? 0.0f : c.sum[u];  // FstConfidenceWithPhoneLoop::run: m_best_acu_score = 0, += per frame
  const int32_t before = f.fresh ? 0 : c.sum_frames[u];
  const size_t row_bytes = (size_t)p.n_models * BYTES;
  for (int32_t base = 0; base < f.n_new; base += rows) {
    const bool live = base + r < f.n_new;
    const int32_t i = live ? base + r : f.n_new - 1;  // (the lanes past the last row sweep it once more: every lane shuffles)
    const uintptr_t a = (uintptr_t)p.lna + (size_t)(f.row0 + i) * row_bytes;
    const float best = fst_row_best<BYTES>(a, a + row_bytes, sub, lpr, p.decode);
    if (live && sub == 0) s_val[r] = __float_as_uint(best);
    __syncthreads();
    const int n = f.n_new - base < rows ? f.n_new - base : rows;
    for (int j = 0; j < n; j++) sum = __fadd_rn(sum, __uint_as_float(s_val[j]));
    __syncthreads();  // (the next pass overwrites the values)
  }
  if (tid == 0) {
    c.sum[u] = sum;
    c.sum_frames[u] = before + (f.n_new > 0 ? f.n_new : 0);
  }
}

}  // namespace

__global__ __launch_bounds__(FST_THREADS) void k_fst_conf_chunk(const FstParams pg, const FstStreamParams qg, const FstParams pp,
                                                               const FstStreamParams qp, const FstConfStreamParams c) {
  __shared__ FstConfChunkLds s;
  const int32_t u = (int32_t)blockIdx.x;
  const unsigned role = blockIdx.y;  // (the same for every lane of the workgroup)
  if (role == 0) {
    search_role(pg, qg, s, u, c.rec[0]);
  } else if (role == 1) {
    search_role(pp, qp, s, u, c.rec[1]);
  } else {
    const FstFeed f = qg.feed[u];
    if (pg.lnabytes == 4)
      acu_role<4>(pg, f, c, s.search.hist, u);
    else if (pg.lnabytes == 2)
      acu_role<2>(pg, f, c, s.search.hist, u);
    else
      acu_role<1>(pg, f, c, s.search.hist, u);
  }
}

void fst_conf_stream_launch(const FstParams &pg, const FstStreamParams &qg, const FstParams &pp, const FstStreamParams &qp,
                            const FstConfStreamParams &c, int32_t n_sessions, bool phone_loop, hipStream_t st) {
  if (n_sessions <= 0) return;
  FstConfStreamParams cc = c;
  cc.lanes_per_row = fst_lanes_per_row(pg.n_models, pg.lnabytes);
  hipLaunchKernelGGL(k_fst_conf_chunk, dim3((unsigned)n_sessions, phone_loop ? 3u : 1u), dim3(FST_THREADS), 0, st, pg, qg, pp, qp, cc);
}

}  // namespace aasr

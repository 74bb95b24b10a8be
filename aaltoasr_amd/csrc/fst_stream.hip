// fst_stream.hip -- the resumable entry of the FST token pass: one workgroup per session, the frames of one feed
// (layout and rules: fst_stream.h; the frame body and the result block: fst_frame.h, shared with k_fst_search).
#include "fst_frame.h"
#include "fst_stream.h"

namespace aasr {

__global__ __launch_bounds__(FST_THREADS) void k_fst_search_chunk(const FstParams p, const FstStreamParams q) {
  __shared__ FstLds s;

  const int tid = threadIdx.x;
  const int32_t u = (int32_t)blockIdx.x;
  const FstFeed f = q.feed[u];
  const FstSessionState old = q.state[u];
  const bool fresh = f.fresh || old.fresh;
  if (!fresh && (f.n_new <= 0 || old.status != FST_OK)) return;  // (the same for every lane) nothing to do, or sticky
  const FstUtt m = fst_utt(p, u);

  int32_t n_act = 1, status = FST_OK, done = 0;
  if (fresh) {
    fst_start(p, m, s);
  } else {
    if (tid == 0) {
      s.flag = 0;
      s.nhist = old.n_hist;
    }
    n_act = old.n_act;
    done = old.frames_done;
    __syncthreads();
  }
  // (the handle refuses a feed past the duration table's last column D before it is queued; the bound here only keeps
  // a miscounted feed inside the table)
  const int32_t n_new = f.n_new < p.D - done ? f.n_new : p.D - done;
  for (int32_t i = 0; i < n_new; i++) {
    const uint8_t *row = p.lna + (size_t)(f.row0 + i) * (size_t)p.n_models * (size_t)p.lnabytes;
    status = fst_frame(p, m, s, row, n_act);
    done++;  // the frame that ends the search counts as consumed
    if (status != FST_OK) break;
  }
  fst_result(p, m, s, u, status, n_act);
  if (tid == 0) {
    FstSessionState st;
    st.n_act = n_act;
    st.status = status;
    st.n_hist = s.nhist;
    st.frames_done = done;
    st.fresh = 0;
    st.n_partial = 0;
    if (s.best)  // the token behind best_lp: the highest log-probability, the earlier token among equals
      st.n_partial = fst_history_words(p, m, m.t_hist[(int32_t)~(uint32_t)s.best], q.part_words + (size_t)u * p.cap_words, p.cap_words);
    q.state[u] = st;
  }
}

void fst_stream_launch(const FstParams &p, const FstStreamParams &q, int32_t n_sessions, hipStream_t st) {
  if (n_sessions <= 0) return;
  hipLaunchKernelGGL(k_fst_search_chunk, dim3((unsigned)n_sessions), dim3(FST_THREADS), 0, st, p, q);
}

}  // namespace aasr

// fst_chunk.h -- the device body of a session's feed, shared by the two resumable entries of the FST token pass:
// k_fst_search_chunk (fst_stream.hip, one search per session) and k_fst_conf_chunk (fst_conf_stream.hip, the grammar and
// the phone-loop search of a session as sibling workgroups).  One copy: restore the record or start, the frames of the
// feed with fst_frame.h's frame body, the result block, the record and the partial words.  Rules: fst_stream.h.
// Included by device code only.
#pragma once
#include "fst_frame.h"
#include "fst_stream.h"

namespace aasr {

namespace {

// Session u's feed.  Every lane calls it and every lane gets the same answer: false when the session was left untouched
// (nothing to do, or a sticky status), true when result[u], the record and the partial words were written -- by lane 0,
// with no barrier behind the writes.
__device__ __forceinline__ bool fst_chunk(const FstParams &p, const FstStreamParams &q, FstLds &s, int32_t u) {
  const int tid = threadIdx.x;
  const FstFeed f = q.feed[u];
  const FstSessionState old = q.state[u];
  const bool fresh = f.fresh || old.fresh;
  if (!fresh && (f.n_new <= 0 || old.status != FST_OK)) return false;  // (the same for every lane) nothing to do, or sticky
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
  return true;
}

}  // namespace

}  // namespace aasr

// fst_stream.h -- layout of the FST decoder's streaming sessions (fst_stream.hip, the handle in fst_stream.cc).
//
// A session is one utterance of a batch whose search is cut at feed boundaries.  Everything the search holds per
// utterance lives in global memory already (fst_search.h: the tokens t_*, the history table h_key, the recombination
// table, which every frame leaves empty); what a launch of k_fst_search keeps in registers and LDS is the record below.
// k_fst_search_chunk, one workgroup of FST_THREADS per session, restores it, runs the frames of one feed with the batch
// kernel's own frame body (fst_frame.h) and saves it again.  That body of a feed is fst_chunk.h's fst_chunk, which
// k_fst_conf_chunk (fst_conf_stream.h) runs too, once per network of a confidence.
//
//   fresh (the feed's flag, or the record's after creation)   the start of k_fst_search: both tables cleared, one
//                 token at the initial node with 0.0f, dur 0 and no words, frames_done = 0
//   otherwise     n_act, status and the history count are restored; nothing is cleared
//   frames        frames_done .. frames_done + n_new - 1 read rows row0 .. row0 + n_new - 1 of the feed's buffer
//   at the end    the record, the FstResult of the frames so far (the batch kernel's result block) and the partial
//                 hypothesis: the words of the best token over all nodes (the token behind best_lp), in part_words
//
// A session with n_new == 0 that is not fresh is left untouched.  A status other than FST_OK is sticky: the session
// skips its frames and keeps status, frames_done and record until it is reset.  frames_done counts the frames consumed,
// the one that ended the search included, so that it does not depend on where the feeds were cut.
// No grid-wide synchronisation, vector atomics only, no scratch; LDS as k_fst_search (1 072 bytes).
#pragma once
#include "fst_search.h"

namespace aasr {

struct FstSessionState {
  int32_t n_act, status, n_hist, frames_done, fresh;
  int32_t n_partial;  // words of the partial hypothesis in part_words (-1: they did not fit, never)
};

struct FstFeed {  // one feed's orders for a session
  int64_t row0;
  int32_t n_new, fresh;
};

struct FstStreamParams {
  FstSessionState *state;
  const FstFeed *feed;
  int32_t *part_words;  // [sessions][cap_words]
};

// p: the sessions' FstParams with lna, decode, lnabytes and n_models of this feed (row0 and n_frames are not read)
void fst_stream_launch(const FstParams &p, const FstStreamParams &q, int32_t n_sessions, hipStream_t st);

}  // namespace aasr

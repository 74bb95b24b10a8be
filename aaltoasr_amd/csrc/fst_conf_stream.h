// fst_conf_stream.h -- layout of the confidence on streaming sessions (fst_conf_stream.hip, the handle in
// fst_conf_stream.cc): what a confidence carries across feed boundaries, and one launch per feed.
//
// k_fst_conf_chunk, grid (sessions, roles), FST_THREADS lanes per workgroup; blockIdx.y is the role, the same for a
// whole workgroup.  Without a phone loop there is one role, with one there are three:
//   role 0   the grammar search of the feed: the body of k_fst_search_chunk (fst_chunk.h) on the grammar's FstParams and
//            FstStreamParams, then -- behind a barrier, the record reads the result block one lane wrote -- the session's
//            FstConfRecord with the body of k_fst_conf_tokens (fst_conf_frame.h)
//   role 1   the same on the phone-loop network's own FstParams and FstStreamParams
//   role 2   the best-acoustics carry: the best value of each of the feed's rows with k_fst_frame_best's row sweep
//            (fst_conf_frame.h; 256 / lanes_per_row rows per pass, their values through LDS), then the session's
//            __fadd_rn chain continued from the sum the last feed left (0.0f when fresh), in frame order, whatever the
//            feed's size -- never a tree.  It runs for every fed frame, whatever became of the two searches: the
//            reference's run() adds a frame's best value whatever became of the tokens.
// The three workgroups of a session share nothing but the feed's orders and the acoustic rows, which they only read: no
// ordering between them is needed, and none between sessions.
//
// A search workgroup that leaves its session untouched (no new frame and not fresh, or a sticky status) leaves the record
// untouched too.  The carried sum and its frame count live in global memory, one pair per session.
// No grid-wide synchronisation, vector atomics only, no scratch.  LDS: k_fst_search's 1 072 bytes plus the record's 48
// (role 2 keeps its pass of row values in the search's histogram words).
#pragma once
#include "fst_conf.h"
#include "fst_stream.h"

namespace aasr {

struct FstConfStreamParams {
  FstConfRecord *rec[2];  // [sessions] each: grammar, phone loop
  float *sum;             // [sessions] the carried sum of the frames' best values
  int32_t *sum_frames;    // [sessions] the frames it covers
  int32_t lanes_per_row;  // 8, 16, 32 or 64: set by fst_conf_stream_launch
};

// pg, qg: the grammar search's params with lna, decode, lnabytes and n_models of this feed; pp, qp: the phone loop's
// (read only with phone_loop).  qg.feed and qp.feed are the same orders.
void fst_conf_stream_launch(const FstParams &pg, const FstStreamParams &qg, const FstParams &pp, const FstStreamParams &qp,
                            const FstConfStreamParams &c, int32_t n_sessions, bool phone_loop, hipStream_t st);

}  // namespace aasr

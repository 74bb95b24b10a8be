// fst_conf.h -- layout of the confidence passes beside the FST token pass (fst_conf.hip, the handle in fst_conf.cc).
//
// k_fst_frame_best   8, 16, 32 or 64 neighbouring lanes per frame row (the power of two that covers the row's 16-byte chunks:
//                    a short row does not idle most of a wave), four waves per workgroup: the row's best acoustic value.  The
//                    row is swept in 16-byte chunks on the 16-byte grid of the address space (a row of an odd model count does
//                    not start on it): a chunk that lies inside the row is one 16-byte load per lane, the two ragged ends are
//                    read element by element.  Nothing outside the row is read.  4-byte rows: the reference's loop (start
//                    -999999999.9f, replaced on strict >) keeps the FIRST of the values that compare equal; the lanes carry
//                    (value, column) and the earlier column wins among equals, so +0 / -0 come out as the loop leaves them.
//                    2- and 1-byte rows: the decode tables fall strictly, so the smallest code decodes to the best value.
//                    No LDS, no atomics.
// k_fst_frame_sum    one wave per utterance: the float sum of its frames' best values in frame order (__fadd_rn chain from
//                    0.0f), the reference's `m_best_acu_score += ...` -- 64 values per coalesced load, then the chain over
//                    them by lane broadcast, the same in every lane (a lane of its own would wait for every value in turn).
// k_fst_conf_tokens  one workgroup per utterance over the tokens k_fst_search left (t_node, t_lp, t_hist, result[u].n_tokens,
//                    candidate order): the best end-node token by that kernel's rule (highest log-probability, the earlier
//                    token among equals), its history id, and the best log-probability among the tokens of any other history
//                    id -- equal ids are equal word sequences (fst_search.h).  LDS: 48 bytes of wave results.  No atomics.
// The row sweep of k_fst_frame_best and the body of k_fst_conf_tokens are device functions in fst_conf_frame.h, shared with
// the streaming entry k_fst_conf_chunk (fst_conf_stream.h), which carries a confidence across the feeds of a live session.
#pragma once
#include <string>
#include <vector>

#include "../../include/aasr.h"
#include "fst_search.h"

struct aasr_fst_batch;

namespace aasr {

constexpr int FSTC_THREADS = 256;
constexpr float FSTC_NONE = -9999999.9f;        // no other hypothesis / no end-node token (FstConfidence.cc)
constexpr float FSTC_ACU_START = -999999999.9f;  // get_best_frame_acu_prob's start value

struct FstConfRecord {
  int32_t best_final_hist, best_final_n_words, has_final, has_different;
  float best_final_lp, best_different_lp;
};

struct FstFrameBestParams {
  const uint8_t *lna;
  const float *decode;
  int32_t lnabytes, n_models, n_utt;
  int32_t lanes_per_row;     // 8, 16, 32 or 64: set by fst_frame_best_launch
  const int64_t *row0;       // [n_utt]
  const int64_t *frame_off;  // [n_utt + 1] exclusive scan of the utterances' frame counts
  float *frame_best;         // [frame_off[n_utt]]
  float *sum;                // [n_utt]
};

void fst_frame_best_launch(const FstFrameBestParams &p, int64_t total_frames, hipStream_t st);
void fst_conf_tokens_launch(const FstParams &p, FstConfRecord *rec, int32_t n_launch, hipStream_t st);

// fst_search.cc: the device pointers of a batch (lna and decode unset) and the LNA decode table of a code width
const FstParams &fst_batch_params(const aasr_fst_batch *b);
void fst_decode_table(int32_t lnabytes, std::vector<float> &table);


// fst_conf.cc, shared with the streaming handle (fst_conf_stream.cc).  The option checks of one search, with the calling
// function's name; the phone loop's derived history capacity for a longest utterance; and one utterance's result from
// what a sync fetched: r holds frames and is otherwise zero, status and logprob are the two searches' (phone: FST_OK and
// -1.0f without a phone loop), g the grammar's record, sum the frames' best values.  -> true when a search overflowed
// (r keeps the statuses, valid 0); raises when the record's best end-node token is not the search's.
void fst_conf_check_options(const aasr_fst_options &o, const char *who, const char *which);
int32_t fst_conf_phone_history(const aasr_fst_options &phone, int64_t longest);
bool fst_conf_finish(aasr_fst_conf_result &r, const int32_t status[2], const float logprob[2], const FstConfRecord &g, bool phone_loop,
                     float sum, const std::string &grammar, const std::string &ploop, const char *who, int32_t u);

}  // namespace aasr

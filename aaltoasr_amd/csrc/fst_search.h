// fst_search.h -- layout of the FST token pass on the device (fst_search.hip, the handle in fst_search.cc).
//
// One workgroup of FST_THREADS = 256 lanes per utterance, a batch of utterances per launch, the frame loop inside the
// kernel; no grid-wide synchronisation.  LDS: FST_LDS_BYTES = 1280 at the most (a 256-bin histogram of the radix select,
// four wave totals of the scans, the frame's best key and a few words of flags).  No scratch memory, no private arrays.
//
// Per utterance, in global memory (every utterance of a batch has the batch's capacities):
//   tokens      t_node, t_lp, t_dur, t_hist [cap_tok = token_limit + 1], t_off [cap_tok + 1]: the active tokens and
//               the exclusive scan of their nodes' out-degrees -- candidate c of a frame is arc c - t_off[i] of token i
//               (i found by bisection), which IS the reference's propagation order (FstSearch_tmpl.hh:62, :184)
//   candidates  c_lp, c_tok, c_node, c_dur, c_hist, c_slot, w_key [cap_cand]
//   recombination  r_key, r_val [cap_recomb, a power of two]: open addressing on (node << 32 | history id), the value a
//               64-bit atomicMax of (order-preserving image of the float) << 32 | ~candidate index -- the winner of a
//               (node, history) is its best log-probability, the earliest candidate among equals, whatever the arrival
//               order.  The slots a frame used are cleared at its end by the candidates that used them.
//   histories   h_key [cap_hist, a power of two]: open addressing on (parent id << 32 | word id), inserted with
//               compare-and-swap; the id of a history is its slot + 1, the root (no words) is 0.  Equal ids are equal
//               word sequences by induction, so recombination compares sequences, never hash values.  Which slot a key
//               lands in depends on arrival order; nothing that leaves the kernel depends on the id's value.
//   result      res_words [cap_words = longest utterance + 1]: the word ids of the best end-node token
//
// Per frame: (1) scan of out-degrees; (2) every candidate's log-probability in the reference's operation order with
// __fmul_rn / __fadd_rn, and the frame's best; (3) the candidates with lp > best - beam (float subtraction; the best
// itself always) intern their history and enter the recombination table -- the reference's in-flight pruning
// (:226) drops only what its exact cut (:106-111) drops too; (4) the winners' keys, compacted; (5) when there are more
// than token_limit + 1 (:101-102 keeps one more than the limit), a radix select over the 64-bit keys, eight passes of
// eight bits with an LDS histogram; (6) the selected winners become the active tokens, in candidate order.  The reference
// holds its tokens sorted by log-probability; here their order is candidate order, which changes which of two EQUAL
// candidates is "earlier" in the next frame and nothing else (tools/fst_restate.py reports every such tie).
//
// A capacity exceeded ends the utterance with FST_OVERFLOW_*; nothing is truncated silently.
//
// The start, the frame's six phases and the result block are device functions in fst_frame.h, shared with the resumable
// entry k_fst_search_chunk (fst_stream.h), which runs the frames of one feed of a live session from saved state.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int FST_THREADS = 256;
constexpr int FST_LDS_BYTES = 1280;

enum : int32_t { FST_OK = 0, FST_NO_TOKENS = 1, FST_OVERFLOW_CANDIDATES = 2, FST_OVERFLOW_RECOMB = 3, FST_OVERFLOW_HISTORY = 4 };

struct FstResult {
  int32_t status, n_tokens, n_words;
  float logprob, best_lp, best_final_lp;
};

struct FstParams {
  // network (CSR)
  const int32_t *arc_begin, *arc_tgt, *arc_word, *node_pdf, *node_end;
  const float *arc_lp;
  int32_t initial;
  // acoustics: rows of n_models values of lnabytes bytes; decode: 65536 (2-byte) or 256 (1-byte) floats built on the host
  const uint8_t *lna;
  const float *decode;
  int32_t lnabytes, n_models;
  const int64_t *row0;
  const int32_t *n_frames;
  // durations: dur_slot[pdf] the pdf's row in dur_table (rows of D + 1 floats), -1 none; dur_slot NULL: no model
  const int32_t *dur_slot;
  const float *dur_table;
  int32_t D;
  float beam, duration_scale, transition_scale;
  int32_t token_limit;
  int32_t cap_tok, cap_cand, cap_recomb, cap_hist, cap_words;
  int32_t *t_node, *t_dur, *t_hist, *t_off;
  float *t_lp;
  float *c_lp;
  int32_t *c_tok, *c_node, *c_dur, *c_hist, *c_slot;
  unsigned long long *w_key, *r_key, *r_val, *h_key;
  int32_t *res_words;
  FstResult *result;
};

void fst_search_launch(const FstParams &p, int32_t n_launch, hipStream_t st);

// the n tokens utterance u holds, by descending log-probability (the earlier first among equals), with their words read
// back through the history table; synchronises st.  who: the calling function's name for the messages (fst_search.cc)
void fst_tokens_read(const char *who, const FstParams &p, int32_t u, int32_t n, hipStream_t st, int32_t *node, float *logprob,
                     int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words);

}  // namespace aasr

// fb_entries.h -- device layout of the step from the forward-backward pass's per-frame pdf occupancies to the weighted
// entries of the statistics accumulation (fb_entries.hip), shared with the handle code in hmmnet_fb.cc.
//
// HmmNetBaumWelch::next_frame (aku/HmmNetBaumWelch.cc:714-789) sums a frame's arc posteriors per pdf and divides every
// one by their sum.  Dense: s_t = sum_j occ[t][j] in the order of the network's pdf list, and the entry (t, j) exists
// where occ[t][j] > 0, with weight occ[t][j] / s_t.  A pair is one (utterance, pdf of its network); the host orders the
// pairs by global pdf, then by utterance, so that the entries of a pair follow each other in the output and a pair's
// lane writes its frames in ascending order: the order of rows_by_pdf (stats.h).  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

enum { FBE_THREADS = 256 };

struct FbEntryUtt {
  int64_t occ;   // T x n_pdf doubles in the occupancy buffer
  int64_t sums;  // T doubles in the frame-sum buffer
  int64_t row0;  // frame row of the utterance's first frame
  int32_t T, n_pdf;
};

struct FbEntryPair {
  int32_t utt;   // index into the covered utterances
  int32_t slot;  // position of the pdf in its network's pdf list
};

// s_t per frame: one lane per frame, pdf-list order.  grid: (ceil(max T / FBE_THREADS), utterances)
void fb_frame_sums_launch(const FbEntryUtt *utt, int32_t n_utt, int32_t max_T, const double *occ, double *sums,
                          hipStream_t stream);
// entries per pair: one lane per pair
void fb_entry_counts_launch(const FbEntryUtt *utt, const FbEntryPair *pairs, int32_t n_pairs, const double *occ,
                            int32_t *counts, hipStream_t stream);
// one lane per pair walks its frames in order and writes row0 + t and occ / s_t from out[pair] on
void fb_entry_fill_launch(const FbEntryUtt *utt, const FbEntryPair *pairs, int32_t n_pairs, const double *occ,
                          const double *sums, const int64_t *out, int32_t *rows, double *weights, hipStream_t stream);

}  // namespace aasr

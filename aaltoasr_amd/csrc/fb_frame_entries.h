// fb_frame_entries.h -- the forward-backward pass's per-frame pdf occupancies as weighted entries grouped by FRAME
// (fb_frame_entries.hip), shared with the handle code in hmmnet_fb.cc.  fb_entries.h groups the same entries by pdf for
// the statistics accumulation; the CMLLR accumulation (mllr_entries.hip) walks a frame's (pdf, weight) list, so it takes
// them frame-major: off[r] .. off[r + 1] are the entries of frame row r of the caller's frame buffer, in the order of the
// utterance's network's pdf list -- the order in which s_t is summed (k_fb_frame_sums, which this file reuses: a weight
// here is occ[t][j] / s_t with the bytes of the pdf-major entry).  A row no covered utterance owns has no entries.
//
// Three steps, every value with one lane and a fixed order, no atomics: the count of a frame (one lane per frame over
// its contiguous occupancy row) into a zeroed per-row array; the exclusive prefix sums of the rows on the device
// (blocks of FBF_SCAN_ROWS rows, the blocks' totals by one workgroup, the add); the fill, one lane per frame again.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fb_entries.h"

namespace aasr {

enum { FBF_THREADS = 256, FBF_SCAN_ITEMS = 4, FBF_SCAN_ROWS = FBF_THREADS * FBF_SCAN_ITEMS };

inline int64_t fb_frame_scan_blocks(int64_t n_rows) { return (n_rows + 1 + FBF_SCAN_ROWS - 1) / FBF_SCAN_ROWS; }

// counts[row0 + t] = the entries of frame t of every utterance; counts zeroed by the caller, the utterances' rows
// disjoint.  grid: (ceil(max T / FBF_THREADS), utterances)
void fb_frame_counts_launch(const FbEntryUtt *utt, int32_t n_utt, int32_t max_T, const double *occ, int32_t *counts,
                            hipStream_t stream);
// off[r] = sum of counts[0 .. r) for r = 0 .. n_rows (n_rows + 1 values); block_sums: fb_frame_scan_blocks(n_rows) + 1
void fb_frame_offsets_launch(const int32_t *counts, int64_t n_rows, int64_t *block_sums, int64_t *off, hipStream_t stream);
// one lane per frame writes its entries from off[row0 + t] on: the global pdf pdfs[pdf_at[u] + j] and occ / s_t
void fb_frame_fill_launch(const FbEntryUtt *utt, const int64_t *pdf_at, const int32_t *pdfs, int32_t n_utt, int32_t max_T,
                          const double *occ, const double *sums, const int64_t *off, int32_t *pdf, double *weight,
                          hipStream_t stream);

}  // namespace aasr

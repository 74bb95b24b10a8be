// seg_loglik.h -- device layout of the per-frame log-likelihood of a state segmentation (seg_loglik.hip), shared
// with its handle (seg_loglik.cc).
//
// Every frame has one pdf; what comes back is safe_log(Mixture::compute_likelihood(frame)) of that pdf, the frame_ll
// of the statistics accumulation (stats_accum.hip) without its sums.  The host groups the frames by pdf (the row list
// of stats.h) and cuts the list into work items of one pdf and at most SEGLL_ITEM rows.  One workgroup runs one item,
// one lane per row: the item's rows go through LDS in sub-blocks of `sub` rows of `stride` doubles (the dimension made
// odd, so that the lanes of a wave read a column from different banks), every lane reads its row from there once per
// SEGLL_KB components, and the mixture's records -- one address for the whole workgroup -- come through the scalar
// cache.  The loops run over the dimension and the mixture size from memory: any dimension, any number of components.
// No atomics, one store per row: the same input gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int SEGLL_ITEM = 256;              // rows per work item at most, and the workgroup's lanes
constexpr int SEGLL_KB = 4;                  // components evaluated per pass over a lane's row
constexpr int SEGLL_LDS_BYTES = 64 * 1024;   // a sub-block's rows stay within this at any dimension

struct SegllItem {
  int64_t row_begin;  // first entry of the item's rows in the row list
  int32_t pdf, n;
};

struct SegllParams {
  const double *x;           // frame rows [n_frames x dim]
  const int32_t *rows;       // row list grouped by pdf, frame order within a pdf
  const SegllItem *items;
  const double *recs;        // AASR_PREC_F64 records: [mean x dimp][precision x dimp][constant, weight]
  const int32_t *state_off;  // first record of every pdf
  double *frame_ll;          // per frame safe_log(total)
  int32_t dim, dimp;
  int32_t stride;            // doubles between two rows in LDS (odd, >= dim)
  int32_t sub;               // rows per sub-block: 1 ... SEGLL_ITEM, sub x stride doubles within SEGLL_LDS_BYTES
};

// the LDS layout of a dimension: stride and rows per sub-block
inline void segll_shape(int dim, int32_t *stride, int32_t *sub) {
  *stride = dim | 1;
  const int64_t fit = SEGLL_LDS_BYTES / ((int64_t)*stride * (int64_t)sizeof(double));
  *sub = (int32_t)(fit < 1 ? 0 : fit > SEGLL_ITEM ? SEGLL_ITEM : fit);  // 0: not even one row (dimension > 8190)
}

void segll_items_launch(const SegllParams &p, int n_items, hipStream_t stream);

}  // namespace aasr

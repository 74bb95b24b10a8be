// moments.h -- device layout of the blocked feature moments (moments_accum.hip), shared with its host driver
// (feanorm.cc).
//
// aku/feanorm.cc sums x and x^2 (and, with --cov or -P, x x^T) over blocks of -b consecutive frames of one utterance
// before it adds a block to the global sums.  Here a block is a SEGMENT: a contiguous run of rows of the frame buffer,
// (first row, length, utterance).  Nothing is gathered and there is no row list.
//
// The host cuts every segment into ITEMS of at most MOMENTS_RUN rows, counted from the segment's first row, so the
// cut depends on the segment alone.  An item kernel writes the item's partial sums to its slab; k_moments_seg_add
// adds a segment's slabs in run order into the segment's sums.  No atomics: the same segment gives the same bytes,
// whatever calls and launches the segments around it fall into.
//
// Diagonal mode (k_moments_diag): a segment's sums are 2 d + 1 doubles -- the count, sum x [d], sum x^2 [d] -- on the
// vector pipe in double.
// Full mode (k_moments_full<PB>): G = sum xi xi^T with xi = [1, x] on v_mfma_f64_16x16x4_f64, in scatter.h's tile
// layout: d + 1 padded to PB blocks of 16 (PB = 1 ... 8, d <= 127), the tiles (R, C) with R >= C, tile
// R (R + 1) / 2 + C, each [row][col] of 256 doubles.  Entry (0, 0) is the count, column 0 sum x, the rest sum x x^T.
//
// Slab memory of a launch: at most MOMENTS_SLAB_BYTES of item slabs and never more than MOMENTS_MAX_SEGMENTS
// segments (the adding pass has a segment per block row); launches are cut between segments, and a single segment
// always fits (its slabs are allocated whatever the bound says).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "scatter.h"

namespace aasr {

constexpr int MOMENTS_RUN = 256;  // rows per item: one workgroup pass
constexpr int MOMENTS_MAX_DIM = SCATTER_MAX_DIM;
constexpr int64_t MOMENTS_SLAB_BYTES = (int64_t)64 << 20;
constexpr int MOMENTS_MAX_SEGMENTS = 32768;
constexpr int MOMENTS_DIAG_THREADS = 256;

// doubles of one item's slab and of one segment's sums
inline int64_t moments_doubles(int dim, bool full) { return full ? scatter_class_doubles(dim) : 2 * (int64_t)dim + 1; }

struct MomentsItem {
  int32_t first;  // first row of the frame buffer
  int32_t len;    // 1 ... MOMENTS_RUN
};

// the items of one segment within one launch: consecutive slabs
struct MomentsGroup {
  int32_t first;  // slab index within the launch
  int32_t count;
  int32_t out;    // the segment's place in the call's output
  int32_t pad;
};

// the slabs of items [item0, item0 + n_items) of x [rows x dim], then out[g.out] = the slabs of every group added in
// item order
void moments_launch(const double *x, int dim, bool full, const MomentsItem *items, int item0, int n_items,
                    const MomentsGroup *groups, int n_groups, double *slab, double *out, hipStream_t stream);

}  // namespace aasr

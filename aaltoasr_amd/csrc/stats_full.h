// stats_full.h -- device layout of the full second moments of ML statistics (stats_full_accum.hip), shared with its
// host driver (stats.cc): PDF_ML_STATS | PDF_ML_FULL_STATS, what FullStatisticsAccumulator::accumulate
// (aku/Distributions.cc:133-141) adds for every component of a frame's mixture.
//
// Per pool Gaussian g the accumulator holds S_g = sum_t gamma_{t,k} xi_t xi_t^T with xi = [1, x] over the frames of
// every mixture that holds g, in scatter.h's tile layout: d + 1 padded to PB blocks of 16 (PB = 1 ... 8,
// d <= SCATTER_MAX_DIM), the tiles (R, C) with R >= C, tile R (R + 1) / 2 + C, each [row][col] of 256 doubles.
//
// Two passes over the row list that the mode-1 accumulation already builds (the frames of every pdf in frame order):
//   - a work item is one pdf and at most SCATTER_ITEM (256) of its rows, a unit one (item, component).  k_full_lik
//     (a workgroup per unit) and k_full_norm (a workgroup per item): the posteriors of the item's rows,
//     [component][row of the item], exactly as k_stats_items forms them.
//   - k_full_units, a workgroup per unit: the weighted outer products of the item's rows on the f64 matrix pipe as
//     k_scatter_items does them (a wave per tile row, sub-blocks of SCATTER_SB rows through LDS, the weight on the A
//     side), the weight of a row its posterior for the unit's component; the unit's tiles go to its slab.
//   - k_full_slab_add, per pool Gaussian of the launch: acc += the slabs of its units, one after the other.
//
// Order of summation.  Within a unit: the rows in frame order, four rows a matrix instruction.  Per pool Gaussian:
// pdfs ascending, the items of a pdf in item order, the components of an item in record order (a mixture may hold a
// Gaussian twice) -- the order of the units themselves.  No atomics.  A call's launches take consecutive items, so
// a Gaussian meets its units in that same order whatever the slab bound cuts the call into: the same input gives the
// same bytes.  (Across pdfs this is not the record order of the mode-1 Gaussian pass, which first sums a record over
// all calls; the two agree to rounding.)
//
// Memory of a launch.  A unit's slab is NT 256 doubles = PB (PB + 1) / 2 x 2 KiB: 12 KiB at 39 dimensions (PB 3),
// 72 KiB at 127 (PB 8).  A launch holds whole items and at most STATS_FULL_SLAB_BYTES = 64 MiB of slabs (one item
// at least): 5 461 units at 39 dimensions, that is 341 items of 16 components (87 000 rows) or 46 items of 118, and
// 910 units at 127 dimensions.  The largest single item, 118 components at 127 dimensions, is 8.3 MiB.  The
// posteriors of a launch are 8 bytes per (row, component) with at most 256 rows a unit: never more than the slab
// bytes / NT.  A call with more is cut into launches that follow each other on the stream and reuse both buffers.
// The accumulator itself is NT 2 KiB per pool Gaussian: 600 MB for 50 000 Gaussians at 39 dimensions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "scatter.h"

namespace aasr {

constexpr int64_t STATS_FULL_SLAB_BYTES = (int64_t)64 << 20;

struct FullItem {
  int32_t start;  // first entry of the row list
  int32_t len;    // 1 ... SCATTER_ITEM
  int32_t pdf;
  int32_t pad;
  int64_t gam;    // first double of its posteriors [components x len] in the launch's posterior buffer
};

struct FullUnit {
  int32_t item;  // index into the call's items
  int32_t comp;  // component of the item's mixture
};

// the units of one pool Gaussian within one launch: entries [first, first + count) of the entry list, each a unit
// (= slab) index within the launch
struct FullGroup {
  int32_t g;
  int32_t first;
  int32_t count;
  int32_t pad;
};

struct FullParams {
  const double *x;           // frame rows [n x dim]
  int32_t dim;
  const int32_t *rows;       // the row list grouped by pdf, frame order within a pdf
  const FullItem *items;     // the call's items
  const FullUnit *units;     // the call's units, item after item
  const double *recs;        // AASR_PREC_F64 records: [mean x dimp][precision x dimp][constant, weight]
  int32_t rec;               // doubles per record (2 dimp + 2)
  const int32_t *state_off;  // first record of every pdf
  double *gam;               // the launch's posteriors
  double *slab;              // the launch's slabs, [unit][NT x 256]
};

// one launch (n_items, n_units > 0): the posteriors of items [item0, item0 + n_items), the slabs of units
// [unit0, unit0 + n_units), then acc += the slabs of every group's entries in entry order
void stats_full_launch(const FullParams &p, int item0, int n_items, int unit0, int n_units, const FullGroup *groups,
                       int n_groups, const int32_t *entries, double *acc, hipStream_t stream);
// packed [n_gauss x dim (dim + 1) / 2] = the lower triangles (row-major, j <= i) of sum gamma x x^T from the accumulator
void stats_full_pack_launch(const double *acc, int n_gauss, int dim, double *packed, hipStream_t stream);

}  // namespace aasr

// scatter.h -- device layout of the class-scatter accumulation (scatter_accum.hip), shared with its host driver
// (lda.cc).
//
// FullStatisticsAccumulator::accumulate (aku/Distributions.cc:133-141) adds gamma x to the mean sum and gamma x x^T to
// the second moment of the frame's class.  With xi = [1, x] that is one symmetric matrix per class,
//   G_c = sum_t gamma_t xi_t xi_t^T:  entry (0, 0) gamma, column 0 sum gamma x, the rest sum gamma x x^T.
// The host groups a call's rows by class (a compressed row list, frame order within a class) and cuts every class
// into work items of at most SCATTER_ITEM rows.  k_scatter_items: a workgroup per item, a wave per tile row, the
// item's rows gathered through LDS in sub-blocks of SCATTER_SB, rank-4 updates on the f64 matrix pipe, the tiles
// written to the item's slab.  k_scatter_slab_add: per class, acc += its items' slabs in item order.  No atomics:
// the same input gives the same bytes, whatever the slab bound cuts the call into.
//
// Tiles: d + 1 is padded to PB blocks of 16 (PB = 1 ... 8, d <= 127); a class keeps the tiles (R, C) with R >= C,
// tile R (R + 1) / 2 + C, each [row][col] of 256 doubles.
//
// Slab memory of a launch: an item's slab is NT 256 doubles = PB (PB + 1) / 2 x 2 KiB -- 12 KiB at 39 dimensions
// (PB 3), 72 KiB at 127 (PB 8).  A launch holds at most SCATTER_SLAB_BYTES = 64 MiB of slabs, that is
// 64 MiB / 12 KiB = 5 461 items (1.4 million rows in full items) at 39 dimensions and 910 items (233 000 rows) at
// 127, and never more than SCATTER_MAX_ITEMS = 32 768 items (the slab pass's grid has a class group per block row,
// and PB 1 would allow exactly that many).  A call with more items is cut into launches that follow each other on
// the stream and reuse the slab.  64 MiB: enough items to fill the device's 1 024 SIMDs several times at every PB
// (910 items x 8 waves at PB 8), small next to the accumulator of a real model (5 000 classes x 12 KiB = 59 MiB).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int SCATTER_ITEM = 256;  // rows per work item (1 024-frame chunks left SIMDs without a second wave)
constexpr int SCATTER_SB = 32;     // rows per LDS sub-block
constexpr int SCATTER_MAX_DIM = 127;
constexpr int64_t SCATTER_SLAB_BYTES = (int64_t)64 << 20;
constexpr int SCATTER_MAX_ITEMS = 32768;

inline int scatter_pb(int dim) { return (dim + 1 + 15) / 16; }
inline int scatter_tiles(int pb) { return pb * (pb + 1) / 2; }
// doubles of one item's slab and of one class's accumulator
inline int64_t scatter_class_doubles(int dim) { return (int64_t)scatter_tiles(scatter_pb(dim)) * 256; }

struct ScatterItem {
  int32_t start;  // first entry of the row list
  int32_t len;    // 1 ... SCATTER_ITEM
  int32_t cls;
  int32_t pad;
};

// the items of one class within one launch: consecutive slabs
struct ScatterGroup {
  int32_t cls;
  int32_t first;  // slab index within the launch
  int32_t count;
  int32_t pad;
};

struct ScatterParams {
  const double *x;       // frame rows [n x dim]
  const double *weight;  // [n] or nullptr: 1
  const int32_t *rows;   // the compressed row list
  const ScatterItem *items;
  int32_t dim;
};

// the slabs of items [item0, item0 + n_items), then acc += the slabs of every group in item order
void scatter_launch(const ScatterParams &p, int item0, int n_items, const ScatterGroup *groups, int n_groups, double *slab,
                    double *acc, hipStream_t stream);
// the second half of scatter_launch alone: acc += the slabs of every group in item order
void scatter_slab_add_launch(int dim, const ScatterGroup *groups, int n_groups, const double *slab, double *acc,
                             hipStream_t stream);
// scatter_launch over weighted entries (scatter_entries.hip): p.rows are the entries' frame rows, class run after class
// run, p.weight the entries' weights (indexed as p.rows is, never null); an entry of weight 0 does not read its row
void scatter_entries_launch(const ScatterParams &p, int item0, int n_items, const ScatterGroup *groups, int n_groups,
                            double *slab, double *acc, hipStream_t stream);

}  // namespace aasr

struct aasr_scatter;
namespace aasr {
// a handle's accumulator on the device, [classes x scatter_class_doubles(dim)] in the tile layout above (lda.cc), for
// a driver that goes on working with the sums where they are (tie.cc)
const double *scatter_device_accumulator(const aasr_scatter *h);
}  // namespace aasr

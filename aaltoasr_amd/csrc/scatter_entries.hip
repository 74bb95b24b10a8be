// scatter_entries.hip -- the per-class scatter sums of scatter_accum.hip from weighted entries: a pdf-major entry list
// (aasr_fb_batch_entries_dev's layout: per class a run of frame rows, each with a weight of its own), so that a frame
// may stand under several classes (layout and slab arithmetic: scatter.h).
//
// k_scatter_entries<PB>: a workgroup of PB waves per work item (one class, at most SCATTER_ITEM consecutive entries of
// the class's run), wave R owning tile row R; the gather through LDS and the matrix-pipe loop are tri_scatter_item's
// (tri_scatter.h) with the weight of the entry: an entry of weight 0 does not read its frame row.  The slabs are added
// by scatter_accum.hip's k_scatter_slab_add, in item order.
#include <hip/hip_runtime.h>

#include "common.h"
#include "scatter.h"
#include "tri_scatter.h"

namespace aasr {

// p.rows: the entries' frame rows; p.weight: the entries' weights, indexed as p.rows is
template <int PB>
__global__ __launch_bounds__(64 * PB) void k_scatter_entries(ScatterParams p, int item0, double *__restrict__ slab) {
  const ScatterItem it = p.items[item0 + blockIdx.x];
  tile_f64x4 acc[PB];
  const int R = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  tri_scatter_item<PB, WeightOfEntry>(p.x, p.dim, p.rows, it.start, it.len, p.weight + it.start, R, acc);
  tri_tiles_store(slab + ((size_t)blockIdx.x * (PB * (PB + 1) / 2) + (size_t)R * (R + 1) / 2) * 256, acc, R);
}

void scatter_entries_launch(const ScatterParams &p, int item0, int n_items, const ScatterGroup *groups, int n_groups,
                            double *slab, double *acc, hipStream_t stream) {
  if (n_items <= 0) return;
  const bool launched = dispatch_pb(scatter_pb(p.dim), [&](auto n) {
    hipLaunchKernelGGL(k_scatter_entries<n()>, dim3((unsigned)n_items), dim3(64 * n()), 0, stream, p, item0, slab);
  });
  if (!launched) raise(AASR_ERR_UNSUPPORTED, "scatter: no accumulation kernel for dimension %d", p.dim);
  AASR_HIP(hipGetLastError());
  scatter_slab_add_launch(p.dim, groups, n_groups, slab, acc, stream);
}

}  // namespace aasr

// scatter_accum.hip -- per-class scatter sums on the device: FullStatisticsAccumulator::accumulate
// (aku/Distributions.cc:133-141) over many frames at once, G_c = sum_t gamma_t xi_t xi_t^T with xi = [1, x]
// (layout and slab arithmetic: scatter.h).
//
// k_scatter_items<PB>: a workgroup of PB waves per work item (one class, at most SCATTER_ITEM rows of the row list),
// wave R owning tile row R; the gather through LDS and the matrix-pipe loop are tri_scatter_item's (tri_scatter.h) with
// the weight of the frame row.
#include <hip/hip_runtime.h>

#include "common.h"
#include "scatter.h"
#include "tri_scatter.h"

namespace aasr {

template <int PB>
__global__ __launch_bounds__(64 * PB) void k_scatter_items(ScatterParams p, int item0, double *__restrict__ slab) {
  const ScatterItem it = p.items[item0 + blockIdx.x];
  tile_f64x4 acc[PB];
  const int R = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  tri_scatter_item<PB, WeightOfRow>(p.x, p.dim, p.rows, it.start, it.len, p.weight, R, acc);
  tri_tiles_store(slab + ((size_t)blockIdx.x * (PB * (PB + 1) / 2) + (size_t)R * (R + 1) / 2) * 256, acc, R);
}

// a thread per value of a class's accumulator; block row g: the items of one class in this launch
__global__ __launch_bounds__(256) void k_scatter_slab_add(const double *__restrict__ slab, const ScatterGroup *__restrict__ groups,
                                                          int64_t TS, double *__restrict__ acc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= TS) return;
  const ScatterGroup g = groups[blockIdx.y];
  double a = acc[(size_t)g.cls * TS + e];
  for (int i = 0; i < g.count; i++) a += slab[(size_t)(g.first + i) * TS + e];
  acc[(size_t)g.cls * TS + e] = a;
}

void scatter_launch(const ScatterParams &p, int item0, int n_items, const ScatterGroup *groups, int n_groups, double *slab,
                    double *acc, hipStream_t stream) {
  if (n_items <= 0) return;
  const bool launched = dispatch_pb(scatter_pb(p.dim), [&](auto n) {
    hipLaunchKernelGGL(k_scatter_items<n()>, dim3((unsigned)n_items), dim3(64 * n()), 0, stream, p, item0, slab);
  });
  if (!launched) raise(AASR_ERR_UNSUPPORTED, "scatter: no accumulation kernel for dimension %d", p.dim);
  AASR_HIP(hipGetLastError());
  scatter_slab_add_launch(p.dim, groups, n_groups, slab, acc, stream);
}

void scatter_slab_add_launch(int dim, const ScatterGroup *groups, int n_groups, const double *slab, double *acc,
                             hipStream_t stream) {
  if (n_groups <= 0) return;
  const int64_t TS = scatter_class_doubles(dim);
  hipLaunchKernelGGL(k_scatter_slab_add, dim3((unsigned)((TS + 255) / 256), (unsigned)n_groups), dim3(256), 0, stream, slab,
                     groups, TS, acc);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

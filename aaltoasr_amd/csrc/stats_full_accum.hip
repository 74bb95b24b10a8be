// stats_full_accum.hip -- full second moments of ML statistics on the device: per pool Gaussian
// S_g = sum_t gamma_{t,k} xi_t xi_t^T with xi = [1, x], FullStatisticsAccumulator::accumulate
// (aku/Distributions.cc:133-141) under Mixture::accumulate (:2134-2161) over many frames at once (layout, order of
// summation and slab arithmetic: stats_full.h).
//
// k_full_lik, a workgroup per (work item, component), a thread per row, then k_full_norm, a workgroup per work item, a
// thread per row.  The posteriors are k_stats_items' (stats_items.h) bit for bit: per component diag_loglik
// (diag_loglik.h) and exp (k_full_lik); the total in component order; 1.0 * w * lik / total on frames with total > 0, 0
// on the others, whose rows k_full_units stages as zeros (k_full_norm).  There a lane holds its frame in registers per
// dimension instance and walks the components; here a thread takes one (component, row) from memory and the component
// is the workgroup's, so that one kernel serves every dimension, a record is read through the scalar cache and a
// launch of a few hundred items still fills the device (items x components workgroups).
//
// k_full_units<PB>: a workgroup of PB waves per unit, wave R owning the tiles (R, 0 ... R): tri_scatter_item
// (tri_scatter.h), as in k_scatter_items, with the row's weight read from the unit's posteriors.  A row of weight 0 (a
// frame whose total is not positive, which the mode-1 kernel skips, or a component of weight 0) is not read, so a frame
// holding NaN or Inf (total NaN, weight 0) leaves the sums clean as it does in mode 1.  A wave never holds more than
// its tile row: the components are separate workgroups.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diag_loglik.h"
#include "stats_full.h"
#include "tri_scatter.h"

namespace aasr {

// the likelihood of the rows of unit (item, component) into the unit's place in the posterior buffer
__global__ __launch_bounds__(SCATTER_ITEM) void k_full_lik(FullParams p, int unit0) {
  const FullUnit u = p.units[unit0 + blockIdx.x];
  const FullItem it = p.items[u.item];
  const int t = threadIdx.x;
  if (t >= it.len) return;
  const int D = p.dim, REC = p.rec, DP = (REC - 2) / 2;
  const double *rec = p.recs + (size_t)(p.state_off[it.pdf] + u.comp) * REC;
  const double *x = p.x + (size_t)p.rows[it.start + t] * D;
  p.gam[it.gam + (size_t)u.comp * it.len + t] = exp(diag_loglik(x, rec, D, DP));
}

// likelihoods -> posteriors, in place
__global__ __launch_bounds__(SCATTER_ITEM) void k_full_norm(FullParams p, int item0) {
  const FullItem it = p.items[item0 + blockIdx.x];
  const int t = threadIdx.x;
  if (t >= it.len) return;
  const int REC = p.rec, DP = (REC - 2) / 2;
  const int r0 = p.state_off[it.pdf], M = p.state_off[it.pdf + 1] - r0;
  const double *R = p.recs + (size_t)r0 * REC;
  double *gam = p.gam + it.gam;
  double total = 0;
  for (int k = 0; k < M; k++) total += R[(size_t)k * REC + 2 * DP + 1] * gam[k * it.len + t];
  const bool ok = total > 0;
  for (int k = 0; k < M; k++)
    gam[k * it.len + t] = ok ? 1.0 * R[(size_t)k * REC + 2 * DP + 1] * gam[k * it.len + t] / total : 0.0;
}

template <int PB>
__global__ __launch_bounds__(64 * PB) void k_full_units(FullParams p, int unit0) {
  const FullUnit u = p.units[unit0 + blockIdx.x];
  const FullItem it = p.items[u.item];
  const double *wgt = p.gam + it.gam + (size_t)u.comp * it.len;  // the unit's posteriors, one per row of the item
  tile_f64x4 acc[PB];
  const int R = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  tri_scatter_item<PB, WeightOfEntry>(p.x, p.dim, p.rows, it.start, it.len, wgt, R, acc);
  tri_tiles_store(p.slab + ((size_t)blockIdx.x * (PB * (PB + 1) / 2) + (size_t)R * (R + 1) / 2) * 256, acc, R);
}

// a thread per value of a Gaussian's accumulator; block row q: the units of one pool Gaussian in this launch
__global__ __launch_bounds__(256) void k_full_slab_add(const double *__restrict__ slab, const FullGroup *__restrict__ groups,
                                                       const int32_t *__restrict__ entries, int64_t TS,
                                                       double *__restrict__ acc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= TS) return;
  const FullGroup g = groups[blockIdx.y];
  double a = acc[(size_t)g.g * TS + e];
  for (int i = 0; i < g.count; i++) a += slab[(size_t)entries[g.first + i] * TS + e];
  acc[(size_t)g.g * TS + e] = a;
}

// a workgroup per pool Gaussian, a thread per packed entry e = i (i + 1) / 2 + j: entry (i + 1, j + 1), j <= i, of its tiles
__global__ __launch_bounds__(256) void k_full_pack(const double *__restrict__ acc, int64_t TS, int D, double *__restrict__ packed) {
  const int tri = D * (D + 1) / 2;
  const double *a = acc + (size_t)blockIdx.x * TS;
  double *o = packed + (size_t)blockIdx.x * tri;
  for (int e = threadIdx.x; e < tri; e += 256) {
    int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);  // (the float root may be one off either way)
    while (i * (i + 1) / 2 > e) i--;
    while ((i + 1) * (i + 2) / 2 <= e) i++;
    const int r = i + 1, q = e - i * (i + 1) / 2 + 1;
    o[e] = a[((size_t)(r / 16) * (r / 16 + 1) / 2 + q / 16) * 256 + (r % 16) * 16 + q % 16];
  }
}

void stats_full_launch(const FullParams &p, int item0, int n_items, int unit0, int n_units, const FullGroup *groups,
                       int n_groups, const int32_t *entries, double *acc, hipStream_t stream) {
  if (n_items <= 0 || n_units <= 0) return;
  hipLaunchKernelGGL(k_full_lik, dim3((unsigned)n_units), dim3(SCATTER_ITEM), 0, stream, p, unit0);
  AASR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_full_norm, dim3((unsigned)n_items), dim3(SCATTER_ITEM), 0, stream, p, item0);
  AASR_HIP(hipGetLastError());
  const bool launched = dispatch_pb(scatter_pb(p.dim), [&](auto n) {
    hipLaunchKernelGGL(k_full_units<n()>, dim3((unsigned)n_units), dim3(64 * n()), 0, stream, p, unit0);
  });
  if (!launched)
    raise(AASR_ERR_UNSUPPORTED, "stats: no full-statistics kernel for dimension %d (1 ... %d)", p.dim, SCATTER_MAX_DIM);
  AASR_HIP(hipGetLastError());
  const int64_t TS = scatter_class_doubles(p.dim);
  hipLaunchKernelGGL(k_full_slab_add, dim3((unsigned)((TS + 255) / 256), (unsigned)n_groups), dim3(256), 0, stream, p.slab,
                     groups, entries, TS, acc);
  AASR_HIP(hipGetLastError());
}

void stats_full_pack_launch(const double *acc, int n_gauss, int dim, double *packed, hipStream_t stream) {
  if (n_gauss <= 0) return;
  hipLaunchKernelGGL(k_full_pack, dim3((unsigned)n_gauss), dim3(256), 0, stream, acc, scatter_class_doubles(dim), dim,
                     packed);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

// stats_full_accum.hip -- full second moments of ML statistics on the device: per pool Gaussian
// S_g = sum_t gamma_{t,k} xi_t xi_t^T with xi = [1, x], FullStatisticsAccumulator::accumulate
// (aku/Distributions.cc:133-141) under Mixture::accumulate (:2134-2161) over many frames at once (layout, order of
// summation and slab arithmetic: stats_full.h).
//
// k_full_lik, a workgroup per (work item, component), a thread per row, then k_full_norm, a workgroup per work item, a
// thread per row.  The posteriors are k_stats_items' (stats_accum.hip), operation by operation: per component the sum
// of df * df * precision over the dimensions in order, * -0.5, + constant, exp (k_full_lik); the total in component
// order; 1.0 * w * lik / total on frames with total > 0, 0 on the others, whose rows k_full_units stages as zeros (k_full_norm).  The
// arithmetic is a copy, not a shared function: there a lane holds its frame in registers per dimension instance and
// walks the components, here a thread takes one (component, row) from memory and the component is the workgroup's, so
// that one kernel serves every dimension, a record is read through the scalar cache and a launch of a few hundred
// items still fills the device (items x components workgroups).  The padded dimensions that k_stats_items runs over
// add +0 to a sum that is never -0, so stopping at the model's dimension gives the same bits.
//
// k_full_units<PB>: k_scatter_items (scatter_accum.hip) with the row's weight read from the unit's posteriors: a
// workgroup of PB waves per unit, wave R owns the tiles (R, 0 ... R), the rows gathered through LDS in sub-blocks of
// SCATTER_SB as xi, rank-4 updates by v_mfma_f64_16x16x4_f64 with the weight on the A side, the accumulators in
// registers until the unit's end.  A wave never holds more than its tile row: the components are separate workgroups.
#include <hip/hip_runtime.h>

#include "common.h"
#include "stats_full.h"

namespace aasr {

typedef double full_f64x4 __attribute__((ext_vector_type(4)));

// the likelihood of the rows of unit (item, component) into the unit's place in the posterior buffer
__global__ __launch_bounds__(SCATTER_ITEM) void k_full_lik(FullParams p, int unit0) {
  const FullUnit u = p.units[unit0 + blockIdx.x];
  const FullItem it = p.items[u.item];
  const int t = threadIdx.x;
  if (t >= it.len) return;
  const int D = p.dim, REC = p.rec, DP = (REC - 2) / 2;
  const double *rec = p.recs + (size_t)(p.state_off[it.pdf] + u.comp) * REC;
  const double *x = p.x + (size_t)p.rows[it.start + t] * D;
  double ll = 0;
  for (int d = 0; d < D; d++) {
    const double df = x[d] - rec[d];
    ll += df * df * rec[DP + d];
  }
  ll *= -0.5;
  ll += rec[2 * DP];
  p.gam[it.gam + (size_t)u.comp * it.len + t] = exp(ll);
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

// f64 16x16x4: lane l holds A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; result register r of lane l is
// D[row l / 16 + 4 r][col l % 16] (mllr_accum.hip).
template <int PB>
__global__ __launch_bounds__(64 * PB) void k_full_units(FullParams p, int unit0) {
  constexpr int NT = PB * (PB + 1) / 2;
  constexpr int W = 16 * PB;         // values of a padded row
  constexpr int XS = 16 * (PB | 1);  // LDS row stride: an odd number of 128-byte lines (scatter_accum.hip)
  constexpr int SB = SCATTER_SB, PER = SB / 4;  // a pass of the 64 PB threads covers 4 rows
  __shared__ double xs[SB * XS];
  __shared__ double ws[SB];
  __shared__ int32_t ridx[SCATTER_ITEM];
  const FullUnit u = p.units[unit0 + blockIdx.x];
  const FullItem it = p.items[u.item];
  const double *wgt = p.gam + it.gam + (size_t)u.comp * it.len;  // the unit's posteriors, one per row of the item
  const int D = p.dim;
  const int tid = threadIdx.x;
  const int lane = tid & 63, R = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  for (int j = tid; j < it.len; j += 64 * PB) ridx[j] = p.rows[it.start + j];
  __syncthreads();
  const int srow = tid / W, scol = tid - srow * W;  // the thread's place in a pass of the gather
  // the thread's PER values of sub-block s; column 0 carries the row's weight to ws and is 1 in xs.  A row of weight 0
  // (a frame whose total is not positive, which the mode-1 kernel skips, or a component of weight 0) is staged as
  // zeros and its features are not read: it adds +0 as 0 * x would for finite x, and a frame holding NaN or Inf
  // (total NaN, weight 0) leaves the sums clean as it does in mode 1.
  auto fetch = [&](int s, double (&v)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int j = s * SB + 4 * k + srow;
      double a = 0.0;
      if (j < it.len) {
        const double wj = wgt[j];
        if (scol == 0) a = wj;
        else if (scol <= D && wj != 0.0) a = p.x[(size_t)ridx[j] * D + scol - 1];
      }
      v[k] = a;
    }
  };
  auto stage = [&](int s, const double (&v)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int r = 4 * k + srow;
      if (scol == 0) {
        ws[r] = v[k];
        xs[r * XS] = s * SB + r < it.len ? 1.0 : 0.0;
      } else {
        xs[r * XS + scol] = v[k];
      }
    }
  };
  full_f64x4 acc[PB];
#pragma unroll
  for (int i = 0; i < PB; i++) acc[i] = full_f64x4{0, 0, 0, 0};
  const int nsub = (it.len + SB - 1) / SB;
  double v[PER];
  fetch(0, v);
  for (int s = 0; s < nsub; s++) {
    stage(s, v);
    __syncthreads();
    if (s + 1 < nsub) fetch(s + 1, v);
#pragma unroll
    for (int q = 0; q < SB / 4; q++) {
      const double *row = xs + (4 * q + kq) * XS + r16;
      const double a = ws[4 * q + kq] * row[16 * R];
#pragma unroll
      for (int C = 0; C < PB; C++)
        if (C <= R) acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, row[16 * C], acc[C], 0, 0, 0);
    }
    __syncthreads();
  }
  double *out = p.slab + ((size_t)blockIdx.x * NT + (size_t)R * (R + 1) / 2) * 256;
#pragma unroll
  for (int C = 0; C < PB; C++) {
    if (C <= R) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[C * 256 + (kq + 4 * r) * 16 + r16] = acc[C][r];
    }
  }
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
  const int pb = scatter_pb(p.dim);
#define AASR_CASE(N)                                                                                  \
  case N:                                                                                             \
    hipLaunchKernelGGL(k_full_units<N>, dim3((unsigned)n_units), dim3(64 * N), 0, stream, p, unit0); \
    break;
  switch (pb) {
    AASR_CASE(1)
    AASR_CASE(2)
    AASR_CASE(3)
    AASR_CASE(4)
    AASR_CASE(5)
    AASR_CASE(6)
    AASR_CASE(7)
    AASR_CASE(8)
    default:
      raise(AASR_ERR_UNSUPPORTED, "stats: no full-statistics kernel for dimension %d (1 ... %d)", p.dim, SCATTER_MAX_DIM);
  }
#undef AASR_CASE
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

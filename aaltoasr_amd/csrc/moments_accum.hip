// moments_accum.hip -- blocked feature moments on the device: the block sums of aku/feanorm.cc:198-213 over many
// blocks at once (layout, items and slab arithmetic: moments.h).
//
// k_moments_diag: a workgroup of 256 threads per item.  An item is len rows of d contiguous doubles, so the threads
// read it as one flat run: thread t owns column t % d of the rows t / d, t / d + RP, ... with RP = 256 / d row lanes
// (the 256 % d threads past RP d rest), which keeps every thread on one column and every load coalesced.  Each thread
// sums x and x x in double in row order; the row lanes of a column are then added in lane order through LDS.  Past
// 256 dimensions a second block column takes the next 256 columns, and so on.
//
// k_moments_full<PB>: a workgroup of PB waves per item, wave R owning tile row R (the tiles (R, 0 ... R)) as in
// k_scatter_items.  The rows are contiguous, so nothing is staged: every lane reads its operands straight from global
// memory into registers -- per step of four rows, lanes 0-15 the 16 values of a column block of row t, lanes 16-31
// those of row t + 1, ... -- and xi's leading 1 and the zeros past d and past the item's end are made in registers.
// No LDS and no barrier; the waves of a workgroup read the same lines at about the same time, so the repeated reads
// of a column block (wave C ... PB - 1 all want block C) are served by the caches.
#include <hip/hip_runtime.h>

#include "common.h"
#include "moments.h"
#include "tri_scatter.h"

namespace aasr {

__global__ __launch_bounds__(MOMENTS_DIAG_THREADS) void k_moments_diag(const double *__restrict__ x,
                                                                      const MomentsItem *__restrict__ items, int item0, int D,
                                                                      double *__restrict__ slab) {
  constexpr int T = MOMENTS_DIAG_THREADS;
  __shared__ double s1[T];
  __shared__ double s2[T];
  const MomentsItem it = items[item0 + blockIdx.x];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * T;  // block column y: the columns c0 ... c0 + W - 1 (one block column up to 256 dimensions)
  const int W = min(T, D - c0);
  const int RP = T / W;
  const int lane_row = tid / W, c = c0 + tid - lane_row * W;
  double a1 = 0.0, a2 = 0.0;
  if (lane_row < RP) {
    const double *p = x + (size_t)it.first * D + c;
    for (int r = lane_row; r < it.len; r += RP) {
      const double v = p[(size_t)r * D];
      a1 += v;
      a2 += v * v;
    }
  }
  s1[tid] = a1;
  s2[tid] = a2;
  __syncthreads();
  double *out = slab + (size_t)blockIdx.x * (2 * (size_t)D + 1);
  if (tid < W) {
    double t1 = s1[tid], t2 = s2[tid];
    for (int k = 1; k < RP; k++) {
      t1 += s1[k * W + tid];
      t2 += s2[k * W + tid];
    }
    out[1 + c] = t1;
    out[1 + D + c] = t2;
  }
  if (tid == 0 && blockIdx.y == 0) out[0] = (double)it.len;
}

template <int PB>
__global__ __launch_bounds__(64 * PB) void k_moments_full(const double *__restrict__ x, const MomentsItem *__restrict__ items,
                                                          int item0, int D, double *__restrict__ slab) {
  const MomentsItem it = items[item0 + blockIdx.x];
  const int tid = threadIdx.x;
  const int lane = tid & 63, R = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const double *base = x + (size_t)it.first * D;
  tile_f64x4 acc[PB];
#pragma unroll
  for (int i = 0; i < PB; i++) acc[i] = tile_f64x4{0, 0, 0, 0};
  for (int t = 0; t < it.len; t += 4) {
    const int row = t + kq;
    const bool live = row < it.len;
    const double *xr = base + (size_t)row * D;  // xi's column q, 1 <= q <= d, is xr[q - 1]; read only when live
    double b[PB];
#pragma unroll
    for (int C = 0; C < PB; C++) {
      const int q = 16 * C + r16;
      double v = 0.0;
      if (C <= R && live) {
        if (q == 0) v = 1.0;
        else if (q <= D) v = xr[q - 1];
      }
      b[C] = v;
    }
    double a = 0.0;
#pragma unroll
    for (int C = 0; C < PB; C++)
      if (C == R) a = b[C];
#pragma unroll
    for (int C = 0; C < PB; C++)
      if (C <= R) acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[C], acc[C], 0, 0, 0);
  }
  tri_tiles_store(slab + ((size_t)blockIdx.x * (PB * (PB + 1) / 2) + (size_t)R * (R + 1) / 2) * 256, acc, R);
}

// a thread per value of a segment's sums; block row g: the items of one segment in this launch
__global__ __launch_bounds__(256) void k_moments_seg_add(const double *__restrict__ slab, const MomentsGroup *__restrict__ groups,
                                                         int64_t TS, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= TS) return;
  const MomentsGroup g = groups[blockIdx.y];
  double a = slab[(size_t)g.first * TS + e];
  for (int i = 1; i < g.count; i++) a += slab[(size_t)(g.first + i) * TS + e];
  out[(size_t)g.out * TS + e] = a;
}

void moments_launch(const double *x, int dim, bool full, const MomentsItem *items, int item0, int n_items,
                    const MomentsGroup *groups, int n_groups, double *slab, double *out, hipStream_t stream) {
  if (n_items <= 0 || n_groups <= 0) return;
  if (!full) {
    hipLaunchKernelGGL(k_moments_diag, dim3((unsigned)n_items, (unsigned)((dim + MOMENTS_DIAG_THREADS - 1) / MOMENTS_DIAG_THREADS)),
                       dim3(MOMENTS_DIAG_THREADS), 0, stream, x, items, item0, dim, slab);
  } else {
    const bool launched = dispatch_pb(scatter_pb(dim), [&](auto n) {
      hipLaunchKernelGGL(k_moments_full<n()>, dim3((unsigned)n_items), dim3(64 * n()), 0, stream, x, items, item0, dim, slab);
    });
    if (!launched) raise(AASR_ERR_UNSUPPORTED, "moments: no full-mode kernel for dimension %d", dim);
  }
  AASR_HIP(hipGetLastError());
  const int64_t TS = moments_doubles(dim, full);
  hipLaunchKernelGGL(k_moments_seg_add, dim3((unsigned)((TS + 255) / 256), (unsigned)n_groups), dim3(256), 0, stream, slab,
                     groups, TS, out);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

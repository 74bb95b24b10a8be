// scatter_accum.hip -- per-class scatter sums on the device: FullStatisticsAccumulator::accumulate
// (aku/Distributions.cc:133-141) over many frames at once, G_c = sum_t gamma_t xi_t xi_t^T with xi = [1, x]
// (layout and slab arithmetic: scatter.h).
//
// k_scatter_items<PB>: a workgroup of PB waves per work item (one class, at most SCATTER_ITEM rows of the row list).
// Wave R owns tile row R, the tiles (R, 0 ... R).  The item's rows are not contiguous, so they are gathered once per
// workgroup: all threads copy a sub-block of SCATTER_SB rows to LDS as xi (the leading 1, zeros past d and past the
// item's end) with the rows' weights beside them, and every wave reads its operands from there, four rows a step,
// for v_mfma_f64_16x16x4_f64.  The next sub-block's values are requested from global memory before the current
// one's matrix instructions and stored to LDS after them.  The weight goes to the A side in registers.  The
// accumulators never leave the registers before the item's end.
#include <hip/hip_runtime.h>

#include "common.h"
#include "scatter.h"

namespace aasr {

typedef double scatter_f64x4 __attribute__((ext_vector_type(4)));

// f64 16x16x4: lane l holds A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; result register r of lane l is
// D[row l / 16 + 4 r][col l % 16] (mllr_accum.hip).
template <int PB>
__global__ __launch_bounds__(64 * PB) void k_scatter_items(ScatterParams p, int item0, double *__restrict__ slab) {
  constexpr int NT = PB * (PB + 1) / 2;
  constexpr int W = 16 * PB;         // values of a padded row
  constexpr int XS = 16 * (PB | 1);  // LDS row stride: an odd number of 128-byte lines, so that the two rows a 32-lane
                                     // half reads (lanes 0-15 row t, 16-31 row t + 1) fall on different banks
  constexpr int SB = SCATTER_SB, PER = SB / 4;  // a pass of the 64 PB threads covers 4 rows
  __shared__ double xs[SB * XS];
  __shared__ double ws[SB];
  __shared__ int32_t ridx[SCATTER_ITEM];
  const ScatterItem it = p.items[item0 + blockIdx.x];
  const int D = p.dim;
  const int tid = threadIdx.x;
  const int lane = tid & 63, R = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  for (int j = tid; j < it.len; j += 64 * PB) ridx[j] = p.rows[it.start + j];
  __syncthreads();
  const int srow = tid / W, scol = tid - srow * W;  // the thread's place in a pass of the gather
  // the thread's PER values of sub-block s; column 0 carries the row's weight to ws and is 1 in xs
  auto fetch = [&](int s, double (&v)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int j = s * SB + 4 * k + srow;
      double a = 0.0;
      if (j < it.len) {
        const int row = ridx[j];
        if (scol == 0) a = p.weight ? p.weight[row] : 1.0;
        else if (scol <= D) a = p.x[(size_t)row * D + scol - 1];
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
  scatter_f64x4 acc[PB];
#pragma unroll
  for (int i = 0; i < PB; i++) acc[i] = scatter_f64x4{0, 0, 0, 0};
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
  double *out = slab + ((size_t)blockIdx.x * NT + (size_t)R * (R + 1) / 2) * 256;
#pragma unroll
  for (int C = 0; C < PB; C++) {
    if (C <= R) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[C * 256 + (kq + 4 * r) * 16 + r16] = acc[C][r];
    }
  }
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
  const int pb = scatter_pb(p.dim);
#define AASR_CASE(N)                                                                                              \
  case N:                                                                                                         \
    hipLaunchKernelGGL(k_scatter_items<N>, dim3((unsigned)n_items), dim3(64 * N), 0, stream, p, item0, slab); \
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
      raise(AASR_ERR_UNSUPPORTED, "scatter: no accumulation kernel for dimension %d", p.dim);
  }
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
  const int64_t TS = scatter_class_doubles(p.dim);
  hipLaunchKernelGGL(k_scatter_slab_add, dim3((unsigned)((TS + 255) / 256), (unsigned)n_groups), dim3(256), 0, stream, slab,
                     groups, TS, acc);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

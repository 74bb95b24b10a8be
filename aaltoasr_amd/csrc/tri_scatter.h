// tri_scatter.h -- sums of w xi xi^T with xi = [1, x] as lower-triangular 16 x 16 tiles on the f64 matrix pipe: what the
// kernels that keep such tiles share (scatter_accum.hip, stats_full_accum.hip, moments_accum.hip, mllr_accum.hip).
// Device code only; tile layout and slab arithmetic: scatter.h.
#pragma once
#include <hip/hip_runtime.h>

#include "scatter.h"

namespace aasr {

// v_mfma_f64_16x16x4_f64: lane l holds A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; result register r of lane l
// is D[row l / 16 + 4 r][col l % 16] (not the f32 shapes' 4 (l / 16) + r).
typedef double tile_f64x4 __attribute__((ext_vector_type(4)));

// the lane's values of the accumulator tiles 0 ... last (of N) to consecutive [row][col] tiles of 256 doubles at out
template <int N>
__device__ __forceinline__ void tri_tiles_store(double *out, const tile_f64x4 (&acc)[N], int last) {
  const int lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int C = 0; C < N; C++) {
    if (C <= last) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[C * 256 + (kq + 4 * r) * 16 + r16] = acc[C][r];
    }
  }
}

// Where entry j of an item (row `row` of the frames) gets its weight from w, and whether a weight of 0 keeps the row's
// features from being read.
struct WeightOfRow {  // per frame row; no array: 1
  static constexpr bool SKIPS_ZERO = false;
  static __device__ __forceinline__ double at(const double *w, int j, int row) { return w ? w[row] : 1.0; }
};
struct WeightOfEntry {  // per entry of the item.  A row of weight 0 is staged as zeros: it adds +0 as 0 * x would for
                        // finite x, and a frame holding NaN or Inf leaves the sums clean
  static constexpr bool SKIPS_ZERO = true;
  static __device__ __forceinline__ double at(const double *w, int j, int row) { return w[j]; }
};

// A workgroup of PB waves sums the len rows rows[start ... start + len) of x ([n x D]): wave R, the caller's
// wave-uniform tile row, leaves the tiles (R, 0 ... R) in acc[0 ... R], which it clears first.  The rows are not
// contiguous, so they are gathered once per workgroup: all threads copy a sub-block of SCATTER_SB rows to LDS as xi
// (the leading 1, zeros past d and past the item's end) with the rows' weights beside them, and every wave reads its
// operands from there, four rows a step.  The next sub-block's values are requested from global memory before the
// current one's matrix instructions and stored to LDS after them.  The weight goes to the A side in registers.  The
// accumulators never leave the registers before the item's end; they are the kernel's own array, which the kernel
// stores (tri_tiles_store): declared in here they are allocated otherwise, 24 and 32 accumulation registers at PB 3
// and 4 where the budgets of the kernel notes tests allow 8.
template <int PB, class Weight>
__device__ __forceinline__ void tri_scatter_item(const double *x, int D, const int32_t *rows, int start, int len,
                                                 const double *w, int R, tile_f64x4 (&acc)[PB]) {
  constexpr int W = 16 * PB;         // values of a padded row
  constexpr int XS = 16 * (PB | 1);  // LDS row stride: an odd number of 128-byte lines, so that the two rows a 32-lane
                                     // half reads (lanes 0-15 row t, 16-31 row t + 1) fall on different banks
  constexpr int SB = SCATTER_SB, PER = SB / 4;  // a pass of the 64 PB threads covers 4 rows
  __shared__ double xs[SB * XS];
  __shared__ double ws[SB];
  __shared__ int32_t ridx[SCATTER_ITEM];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  for (int j = tid; j < len; j += 64 * PB) ridx[j] = rows[start + j];
  __syncthreads();
  const int srow = tid / W, scol = tid - srow * W;  // the thread's place in a pass of the gather
  // the thread's PER values of sub-block s; column 0 carries the row's weight to ws and is 1 in xs
  auto fetch = [&](int s, double (&v)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int j = s * SB + 4 * k + srow;
      double a = 0.0;
      if (j < len) {
        const int row = ridx[j];
        double wj = 1.0;
        if (Weight::SKIPS_ZERO || scol == 0) wj = Weight::at(w, j, row);
        if (scol == 0) a = wj;
        else if (scol <= D && (!Weight::SKIPS_ZERO || wj != 0.0)) a = x[(size_t)row * D + scol - 1];
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
        xs[r * XS] = s * SB + r < len ? 1.0 : 0.0;
      } else {
        xs[r * XS + scol] = v[k];
      }
    }
  };
#pragma unroll
  for (int i = 0; i < PB; i++) acc[i] = tile_f64x4{0, 0, 0, 0};
  const int nsub = (len + SB - 1) / SB;
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
}

}  // namespace aasr

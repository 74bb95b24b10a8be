// mllt.hip -- the device passes of HmmSet::estimate_mllt (aku/HmmSet.cc:841-1056) over resident covariances
// (layout and slab arithmetic: mllt.h).
//
// k_mllt_cov: run once; a thread per (Gaussian, entry), FullStatisticsAccumulator::get_covariance_estimate
// (aku/Distributions.cc:123-130) into the entry-major array.
// k_mllt_var<PB>: a workgroup of PB waves per 64 Gaussians, a lane per Gaussian, wave R the rows 16 R ... 16 R + 15 of
// A.  One pass over the Gaussian's entries; the coefficients p[e][16 R ...] are the same for every lane.
// k_mllt_gsum<PB>: a workgroup of MLLT_WAVES waves per item and group of entry tiles.  f64 16x16x4: lane l holds
// A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; result register r of lane l is D[row l / 16 + 4 r][col l % 16]
// (mllr_accum.hip).  Here row = the dimension i (the weight w_gi), col = the entry, k = the Gaussian.  A lane loads
// four consecutive Gaussians of its entry at once, so the k index of matrix instruction j of a step is 4 (l / 16) + j:
// the weight operand takes the same Gaussian, and the order of the sum within an item is fixed.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mllt.h"

namespace aasr {

typedef double mllt_f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_mllt_cov(int dim, int64_t G, int64_t GP, const double *__restrict__ gamma,
                                                  const double *__restrict__ sum_x, const double *__restrict__ m2,
                                                  const int32_t *__restrict__ ok, double *__restrict__ cov) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y, c = blockIdx.z;
  if (g >= G || c > r) return;
  const int64_t e = (int64_t)r * (r + 1) / 2 + c;
  double v = 0.0;
  if (ok[g]) {
    const double inv = 1 / gamma[g];
    const double mr = sum_x[g * dim + r] * inv, mc = sum_x[g * dim + c] * inv;
    v = m2[g * ((int64_t)dim * (dim + 1) / 2) + e] * inv - mr * mc;
  }
  cov[e * GP + g] = v;
}

template <int PB>
__global__ __launch_bounds__(64 * PB) void k_mllt_var(int dim, int64_t G, int64_t GP, const double *__restrict__ cov,
                                                      const double *__restrict__ p, double *__restrict__ var) {
  constexpr int IP = 16 * PB;
  const int lane = threadIdx.x & 63, R = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * 64 + lane;  // < GP: the grid covers GP / 64 blocks
  const int E = dim * (dim + 1) / 2;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0;
  const double *pr = p + 16 * R;
#pragma unroll 4
  for (int e = 0; e < E; e++) {
    const double s = cov[(int64_t)e * GP + g];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = __builtin_fma(pr[(int64_t)e * IP + i], s, acc[i]);
  }
  if (g >= G) return;
#pragma unroll
  for (int i = 0; i < 16; i++)
    if (16 * R + i < dim) var[g * dim + 16 * R + i] = acc[i];
}

template <int PB>
__global__ __launch_bounds__(64 * MLLT_WAVES) void k_mllt_gsum(int ET, int64_t GP, const double *__restrict__ cov,
                                                               const double *__restrict__ w, int item0,
                                                               double *__restrict__ slab) {
  constexpr int IP = 16 * PB, NE = MLLT_NE;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int et0 = (blockIdx.y * MLLT_WAVES + wv) * NE;  // the wave's first entry tile
  if (et0 >= ET) return;                                // (no barrier in this kernel)
  const int64_t EP = (int64_t)16 * ET;
  mllt_f64x4 acc[PB][NE];
#pragma unroll
  for (int I = 0; I < PB; I++)
#pragma unroll
    for (int n = 0; n < NE; n++) acc[I][n] = mllt_f64x4{0, 0, 0, 0};
  const int64_t g0 = (int64_t)(item0 + blockIdx.x) * MLLT_ITEM + 4 * kq;
  // tiles past ET of the last wave read the array's zero rows (mllt_cov_rows) and are not written
  const double *crow = cov + (int64_t)(16 * et0 + r16) * GP + g0;
  const double *wrow = w + g0 * IP + r16;
  for (int s = 0; s < MLLT_ITEM / 16; s++) {
    mllt_f64x4 sv[NE];
#pragma unroll
    for (int n = 0; n < NE; n++) sv[n] = *(const mllt_f64x4 *)(crow + (int64_t)16 * n * GP + 16 * s);
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int I = 0; I < PB; I++) {
        const double a = wrow[(int64_t)(16 * s + j) * IP + 16 * I];
#pragma unroll
        for (int n = 0; n < NE; n++) acc[I][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sv[n][j], acc[I][n], 0, 0, 0);
      }
    }
  }
  double *out = slab + (int64_t)blockIdx.x * IP * EP;
#pragma unroll
  for (int n = 0; n < NE; n++) {
    if (et0 + n >= ET) break;
#pragma unroll
    for (int I = 0; I < PB; I++)
#pragma unroll
      for (int r = 0; r < 4; r++) out[(int64_t)(16 * I + kq + 4 * r) * EP + 16 * (et0 + n) + r16] = acc[I][n][r];
  }
}

// a thread per value of the sums: += the launch's slabs in item order
__global__ __launch_bounds__(256) void k_mllt_slab_add(const double *__restrict__ slab, int n_items, int64_t TS,
                                                       double *__restrict__ sums) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= TS) return;
  double a = sums[e];
  for (int i = 0; i < n_items; i++) a += slab[(int64_t)i * TS + e];
  sums[e] = a;
}

void mllt_cov_launch(int dim, int64_t n_gauss, const double *gamma, const double *sum_x, const double *m2, const int32_t *ok,
                     double *cov, hipStream_t stream) {
  if (n_gauss <= 0) return;
  hipLaunchKernelGGL(k_mllt_cov, dim3((unsigned)((n_gauss + 255) / 256), (unsigned)dim, (unsigned)dim), dim3(256), 0, stream,
                     dim, n_gauss, mllt_gp(n_gauss), gamma, sum_x, m2, ok, cov);
  AASR_HIP(hipGetLastError());
}

#define AASR_MLLT_INSTANCES(X) X(1) X(2) X(3) X(4)

void mllt_var_launch(int dim, int64_t n_gauss, const double *cov, const double *p, double *var, hipStream_t stream) {
  if (n_gauss <= 0) return;
  const int64_t GP = mllt_gp(n_gauss);
#define AASR_CASE(N)                                                                                                       \
  case N:                                                                                                                  \
    hipLaunchKernelGGL(k_mllt_var<N>, dim3((unsigned)(GP / 64)), dim3(64 * N), 0, stream, dim, n_gauss, GP, cov, p, var); \
    break;
  switch (mllt_pb(dim)) {
    AASR_MLLT_INSTANCES(AASR_CASE)
    default:
      raise(AASR_ERR_UNSUPPORTED, "mllt: no variance kernel for dimension %d", dim);
  }
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
}

void mllt_gsum_launch(int dim, int64_t gp, const double *cov, const double *w, int item0, int n_items, double *slab,
                      double *sums, hipStream_t stream) {
  if (n_items <= 0) return;
  const int ET = mllt_et(dim);
  const unsigned gy = (unsigned)((ET + MLLT_NE * MLLT_WAVES - 1) / (MLLT_NE * MLLT_WAVES));
#define AASR_CASE(N)                                                                                                  \
  case N:                                                                                                             \
    hipLaunchKernelGGL(k_mllt_gsum<N>, dim3((unsigned)n_items, gy), dim3(64 * MLLT_WAVES), 0, stream, ET, gp, cov, w, \
                       item0, slab);                                                                                  \
    break;
  switch (mllt_pb(dim)) {
    AASR_MLLT_INSTANCES(AASR_CASE)
    default:
      raise(AASR_ERR_UNSUPPORTED, "mllt: no G kernel for dimension %d", dim);
  }
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
  const int64_t TS = mllt_slab_doubles(dim);
  hipLaunchKernelGGL(k_mllt_slab_add, dim3((unsigned)((TS + 255) / 256)), dim3(256), 0, stream, slab, n_items, TS, sums);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

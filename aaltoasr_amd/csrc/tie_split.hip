// tie_split.hip -- the device side of the state-tying search: masked sums of context-phone statistics on the FP64
// matrix pipe, and the likelihood gain of a split or a merge from the reference's column Cholesky (layout and the
// arithmetic's order: tie.h).
#include <hip/hip_runtime.h>

#include "common.h"
#include "tie.h"

namespace aasr {

typedef double tie_f64x4 __attribute__((ext_vector_type(4)));

// a thread per value of a row; block column: the class
__global__ __launch_bounds__(256) void k_tie_pack(const double *__restrict__ acc, int64_t TS, const int32_t *__restrict__ map,
                                                  int E, int EP, double *__restrict__ rows) {
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= EP) return;
  const int64_t c = blockIdx.x;
  rows[c * EP + e] = e < E ? acc[c * TS + map[e]] : 0.0;
}

// f64 16x16x4: lane l holds A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; result register r of lane l is
// D[row l / 16 + 4 r][col l % 16] (mllr_accum.hip).  Here row = the mask row, col = the value, k = the list position.
__global__ __launch_bounds__(64) void k_tie_masked_sum(int EP, const double *__restrict__ in, const int32_t *__restrict__ idx,
                                                       const uint32_t *__restrict__ mask, const TieJob *__restrict__ jobs,
                                                       const TieItem *__restrict__ items, double *__restrict__ out) {
  constexpr int NE = TIE_NE;
  const TieItem it = items[blockIdx.x];
  const TieJob jb = jobs[it.job];
  const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
  const int ET = EP / 16;
  const int row = 16 * it.rtile + r16;  // the mask row this lane brings to the A side
  const bool row_ok = row < jb.n_rows;
  const uint32_t *mrow = mask + jb.mask0 + (int64_t)(row_ok ? row : 0) * jb.wpr;
  const int32_t *list = idx + jb.idx0;
  const int col = 16 * it.ctile0 + r16;
  tie_f64x4 acc[NE];
#pragma unroll
  for (int n = 0; n < NE; n++) acc[n] = tie_f64x4{0, 0, 0, 0};
  for (int k0 = 0; k0 < jb.n_k; k0 += 4) {
    const int k = k0 + kq;
    const bool kin = k < jb.n_k;
    double a = 0.0;
    if (kin && row_ok) a = (mrow[k >> 5] >> (k & 31)) & 1u ? 1.0 : 0.0;
    const double *src = in + (int64_t)(kin ? list[k] : 0) * EP + col;
    double b[NE];
#pragma unroll
    for (int n = 0; n < NE; n++) b[n] = (kin && it.ctile0 + n < ET) ? src[16 * n] : 0.0;
#pragma unroll
    for (int n = 0; n < NE; n++) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[n], acc[n], 0, 0, 0);
  }
#pragma unroll
  for (int n = 0; n < NE; n++) {
    if (it.ctile0 + n >= ET) break;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int orow = 16 * it.rtile + kq + 4 * r;
      if (orow < jb.n_rows) out[(int64_t)(jb.out0 + orow) * EP + col + 16 * n] = acc[n][r];
    }
  }
}

// a wave per side; MD: the largest dimension of the instance, LDS row stride MD | 1 (odd: the 32 rows of a half
// wave fall on different banks)
template <int MD>
__global__ __launch_bounds__(64) void k_tie_logdet(int d, int EP, const double *__restrict__ sums,
                                                   const TieSide *__restrict__ sides, double *__restrict__ ld_gamma) {
  constexpr int ST = MD | 1;
  __shared__ double L[MD * ST];
  __shared__ double mu[64];
  const TieSide sd = sides[blockIdx.x];
  const int lane = threadIdx.x;
  const double *A = sums + (int64_t)sd.a * EP;
  const double *B = sums + (int64_t)(sd.op == TIE_SIDE_ROW ? sd.a : sd.b) * EP;
  const int op = sd.op;
  auto value = [&](int e) {
    const double a = A[e];
    if (op == TIE_SIDE_ROW) return a;
    const double b = B[e];
    return op == TIE_SIDE_SUB ? a - b : a + b;
  };
  const double gamma = value(0);
  if (lane < d) mu[lane] = value(1 + lane) / gamma;
  __syncthreads();
  const double my_mu = lane < d ? mu[lane] : 0.0;
  for (int i = 0; i < d; i++) {  // row i of the lower triangle: lane j <= i
    if (lane <= i) L[i * ST + lane] = value(1 + d + i * (i + 1) / 2 + lane) / gamma - mu[i] * my_mu;
  }
  __syncthreads();
  // LinearAlgebra::cholesky_factor: lane = row
  double logsum = 0.0;
  for (int j = 0; j < d; j++) {
    double acc = 0.0;
    if (lane >= j && lane < d) {
      acc = L[lane * ST + j];
      for (int k = 0; k < j; k++) acc = acc - L[lane * ST + k] * L[j * ST + k];
    }
    const double ljj = sqrt(__shfl(acc, j));
    if (lane == j) L[j * ST + j] = ljj;
    else if (lane > j && lane < d) L[lane * ST + j] = acc / ljj;
    logsum += log(ljj);
    __syncthreads();
  }
  if (lane == 0) {
    ld_gamma[2 * (int64_t)blockIdx.x] = logsum * 2;
    ld_gamma[2 * (int64_t)blockIdx.x + 1] = gamma;
  }
}

__global__ __launch_bounds__(256) void k_tie_gain(const double *__restrict__ ld_gamma, const TieCand *__restrict__ cands,
                                                  int n, double *__restrict__ gain) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const TieCand cd = cands[c];
  const double *p = ld_gamma + 2 * (int64_t)cd.parent, *a = ld_gamma + 2 * (int64_t)cd.child1,
               *b = ld_gamma + 2 * (int64_t)cd.child2;
  gain[c] = (p[0] * p[1] - a[0] * a[1] - b[0] * b[1]) / 2;
}

void tie_pack_launch(const double *acc, int64_t TS, const int32_t *map, int dim, int n_classes, double *rows,
                     hipStream_t stream) {
  if (n_classes <= 0) return;
  const int E = (int)tie_row_values(dim), EP = (int)tie_row_stride(dim);
  hipLaunchKernelGGL(k_tie_pack, dim3((unsigned)n_classes, (unsigned)((EP + 255) / 256)), dim3(256), 0, stream, acc, TS, map,
                     E, EP, rows);
  AASR_HIP(hipGetLastError());
}

void tie_masked_sum_launch(int dim, const double *in, const int32_t *idx, const uint32_t *mask, const TieJob *jobs,
                           const TieItem *items, int n_items, double *out, hipStream_t stream) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(k_tie_masked_sum, dim3((unsigned)n_items), dim3(64), 0, stream, (int)tie_row_stride(dim), in, idx, mask,
                     jobs, items, out);
  AASR_HIP(hipGetLastError());
}

void tie_logdet_launch(int dim, const double *sums, const TieSide *sides, int n_sides, double *ld_gamma, hipStream_t stream) {
  if (n_sides <= 0) return;
  const int EP = (int)tie_row_stride(dim);
#define AASR_CASE(N)                                                                                                   \
  hipLaunchKernelGGL(k_tie_logdet<N>, dim3((unsigned)n_sides), dim3(64), 0, stream, dim, EP, sums, sides, ld_gamma)
  if (dim < 1 || dim > TIE_MAX_DIM) raise(AASR_ERR_UNSUPPORTED, "tie: no gain kernel for dimension %d (1 ... %d)", dim, TIE_MAX_DIM);
  if (dim <= 16) AASR_CASE(16);
  else if (dim <= 32) AASR_CASE(32);
  else if (dim <= 48) AASR_CASE(48);
  else AASR_CASE(63);
#undef AASR_CASE
  AASR_HIP(hipGetLastError());
}

void tie_gain_launch(const double *ld_gamma, const TieCand *cands, int n_cands, double *gain, hipStream_t stream) {
  if (n_cands <= 0) return;
  hipLaunchKernelGGL(k_tie_gain, dim3((unsigned)((n_cands + 255) / 256)), dim3(256), 0, stream, ld_gamma, cands, n_cands, gain);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

// mllr_accum.hip -- CMLLR statistics on the device: MllrTrainer::collect_data and
// MllTrainerComponent::collect_data (aku/MllrTrainer.cc:22-60, 147-163) over many frames at once, with the
// likelihoods of DiagonalGaussian::compute_log_likelihood (Distributions.cc:1040-1062) in double, operation by
// operation as k_stats_items computes them.
//
// Three passes (mllr.h).  Pass 1: a workgroup per 64 frames, one lane per frame for the posteriors, then one
// thread per (frame, dimension) for the weights w_ti, u_ti, the components summed in mixture order.  Pass 2: a
// wave per (chunk of frames, job) -- job i < d owns G_i, job d + R owns row block R of k -- steps through the
// chunk four frames at a time with v_mfma_f64_16x16x4_f64; both operands are the frame vector xi (lane l holds
// element 16 b + l % 16 of frame t + l / 16 for every block b), the A side scaled by the frame's weight in
// registers.  The accumulators of a job never leave the registers before the chunk's end.  Pass 3: one thread per
// accumulator value adds the chunks' slabs in chunk order.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mllr.h"
#include "mllr_pass1.h"
#include "tri_scatter.h"

namespace aasr {

size_t mllr_weights_lds_bytes(int dim, int max_comps) {
  return (size_t)MLLR_P1_FRAMES * ((dim | 1) + max_comps + 1) * sizeof(double) + (size_t)2 * MLLR_P1_FRAMES * sizeof(int32_t);
}

// LDS: [frames: 64 x (dim | 1)][posteriors: 64 x max_comps][beta share: 64][first record: 64][components: 64]
__global__ __launch_bounds__(MLLR_THREADS) void k_mllr_weights(MllrParams p) {
  extern __shared__ double lds[];
  const int D = p.dim, XS = D | 1, MC = p.max_comps, B = MLLR_P1_FRAMES;
  double *xs = lds;
  double *lg = xs + B * XS;
  double *lbeta = lg + B * MC;
  int32_t *lr0 = (int32_t *)(lbeta + B);
  int32_t *lm = lr0 + B;
  const int f0 = blockIdx.x * B, nb = min(B, p.n - f0);
  const int tid = threadIdx.x;
  for (int j = tid; j < nb * D; j += MLLR_THREADS) {
    const int t = j / D, d = j - t * D;
    xs[t * XS + d] = p.x[(size_t)(f0 + t) * D + d];
  }
  __syncthreads();
  if (tid < nb) {
    const int t = tid;
    const int pdf = p.pdf[f0 + t];
    int r0 = 0, M = 0;
    if (pdf >= 0) {
      r0 = p.state_off[pdf];
      M = p.state_off[pdf + 1] - r0;
    }
    // the .phn segmentation's prior of 1
    const double beta = mllr_posteriors(p, xs + t * XS, r0, M, 1.0, lg + t * MC, 0.0);
    lbeta[t] = beta;
    lr0[t] = r0;
    lm[t] = M;
    p.ok[f0 + t] = beta > 0 ? 1 : 0;
  }
  __syncthreads();
  const int DU = D + 1;
  for (int j = tid; j < nb * DU; j += MLLR_THREADS) {
    const int t = j / DU, i = j - t * DU;
    if (i == D) {
      p.u[(size_t)(f0 + t) * DU + D] = lbeta[t];
      continue;
    }
    const int r0 = lr0[t], M = lm[t];
    double w = 0, u = 0;
    for (int g = 0; g < M; g++) {
      const double pr = lg[t * MC + g];
      if (!(pr > 0)) continue;
      w += p.inv_var[(size_t)(r0 + g) * D + i] * pr;   // 1 / covar(i) * prob
      u += p.mean_var[(size_t)(r0 + g) * D + i] * pr;  // mean(i) / covar(i) * prob
    }
    p.w[(size_t)(f0 + t) * D + i] = w;
    p.u[(size_t)(f0 + t) * DU + i] = u;
  }
}

template <int PB>
__global__ __launch_bounds__(MLLR_THREADS) void k_mllr_rank(MllrParams p, double *__restrict__ slab) {
  constexpr int NT = PB * (PB + 1) / 2;
  const int D = p.dim, DU = D + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int job = blockIdx.y * (MLLR_THREADS / 64) + wave;
  if (job >= D + PB) return;
  const int r16 = lane & 15, kq = lane >> 4;
  const int t0 = blockIdx.x * MLLR_CHUNK, t1 = min(p.n, t0 + MLLR_CHUNK);
  const bool is_g = job < D;
  const int krow = (job - D) * 16 + r16;  // k jobs: the lane's row of U^T
  tile_f64x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc[i] = tile_f64x4{0, 0, 0, 0};
  // the lane's operands of the step at frame t: xi per block and the weight of its A side
  auto load = [&](int t, double (&xi)[PB], double &wt) {
    const bool v = t < t1 && p.ok[t] != 0;
#pragma unroll
    for (int b = 0; b < PB; b++) {
      const int e = 16 * b + r16;
      xi[b] = !v ? 0.0 : e == 0 ? 1.0 : e <= D ? p.x[(size_t)t * D + e - 1] : 0.0;
    }
    if (is_g) wt = v ? p.w[(size_t)t * D + job] : 0.0;
    else wt = v && krow <= D ? p.u[(size_t)t * DU + krow] : 0.0;
  };
  double xi[PB], wt;
  load(t0 + kq, xi, wt);
  for (int t = t0; t < t1; t += 4) {
    double nxi[PB], nwt;  // the next step's operands, requested before this step's matrix instructions
    load(t + 4 + kq, nxi, nwt);
    if (is_g) {
      double a[PB];
#pragma unroll
      for (int b = 0; b < PB; b++) a[b] = wt * xi[b];
#pragma unroll
      for (int R = 0; R < PB; R++)
#pragma unroll
        for (int C = 0; C <= R; C++)
          acc[R * (R + 1) / 2 + C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[R], xi[C], acc[R * (R + 1) / 2 + C], 0, 0, 0);
    } else {
#pragma unroll
      for (int C = 0; C < PB; C++) acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(wt, xi[C], acc[C], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < PB; b++) xi[b] = nxi[b];
    wt = nwt;
  }
  const size_t SL = ((size_t)D * NT + PB * PB) * 256;
  double *out = slab + (size_t)blockIdx.x * SL + (is_g ? (size_t)job * NT : (size_t)D * NT + (size_t)(job - D) * PB) * 256;
  tri_tiles_store(out, acc, (is_g ? NT : PB) - 1);
}

__global__ __launch_bounds__(MLLR_THREADS) void k_mllr_slab_add(const double *__restrict__ slab, int n_chunks, int64_t SL,
                                                                double *__restrict__ acc) {
  const int64_t e = (int64_t)blockIdx.x * MLLR_THREADS + threadIdx.x;
  if (e >= SL) return;
  double a = acc[e];
  for (int c = 0; c < n_chunks; c++) a += slab[(size_t)c * SL + e];
  acc[e] = a;
}

void mllr_weights_launch(const MllrParams &p, hipStream_t stream) {
  if (p.n <= 0) return;
  const unsigned blocks = (unsigned)((p.n + MLLR_P1_FRAMES - 1) / MLLR_P1_FRAMES);
  hipLaunchKernelGGL(k_mllr_weights, dim3(blocks), dim3(MLLR_THREADS), mllr_weights_lds_bytes(p.dim, p.max_comps), stream, p);
  AASR_HIP(hipGetLastError());
}

void mllr_rank_launch(const MllrParams &p, double *slab, double *acc, hipStream_t stream) {
  if (p.n <= 0) return;
  const int pb = mllr_pb(p.dim);
  const int chunks = (p.n + MLLR_CHUNK - 1) / MLLR_CHUNK;
  if (chunks > MLLR_MAX_CHUNKS) raise(AASR_ERR_INVALID, "mllr: %d frames in one launch", p.n);
  const dim3 grid((unsigned)chunks, (unsigned)((p.dim + pb + MLLR_THREADS / 64 - 1) / (MLLR_THREADS / 64)));
  const bool launched = dispatch_among<1, 2, 3, 4>(pb, [&](auto n) {
    hipLaunchKernelGGL(k_mllr_rank<n()>, grid, dim3(MLLR_THREADS), 0, stream, p, slab);
  });
  if (!launched) raise(AASR_ERR_UNSUPPORTED, "mllr: no accumulation kernel for dimension %d", p.dim);
  AASR_HIP(hipGetLastError());
  const int64_t SL = mllr_slab_doubles(p.dim);
  hipLaunchKernelGGL(k_mllr_slab_add, dim3((unsigned)((SL + MLLR_THREADS - 1) / MLLR_THREADS)), dim3(MLLR_THREADS), 0,
                     stream, slab, chunks, SL, acc);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

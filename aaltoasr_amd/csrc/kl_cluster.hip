// kl_cluster.hip -- the assignment and centre kernels of Gaussian-pool clustering (aku/gcluster.cc, diagonal mode).
// Layout, summation orders and the tie rule: kl_cluster.h.
//
// The arithmetic is the reference's, operation by operation: t = mean_i[k] - mean_j[k]; the Euclidean pass adds t * t
// and takes the square root of the sum, the divergence pass adds (cov_i[k] + t * t) / cov_j[k] -- a division, never a
// product with a reciprocal -- and forms (ldet_j - ldet_i + dist - dim) / 2.0 from left to right.  The library is
// built with -ffp-contract=off: no product here may fuse with the sum that follows it.
#include "kl_cluster.h"

#include "common.h"

namespace aasr {

// Not modelled: the reference's norm is BLAS dnrm2 (scaled summation), which can differ from sqrt(sum t * t) in the
// last place.
template <bool EUCLID>
__global__ __launch_bounds__(64 * KLC_WAVES) void k_klc_assign(const double2 *__restrict__ gauss,
                                                               const double *__restrict__ g_ldet,
                                                               const double *__restrict__ centres,
                                                               const double *__restrict__ c_ldet,
                                                               const int32_t *__restrict__ c_valid, int D, int G, int C,
                                                               int32_t *__restrict__ out_index,
                                                               double *__restrict__ out_dist) {
  __shared__ double s_min[KLC_WAVES][64];
  __shared__ int32_t s_idx[KLC_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t gi = (int64_t)blockIdx.x * 64 + lane;
  const int64_t i = gi < G ? gi : (int64_t)G - 1;  // lanes past the pool read the last Gaussian and store nothing
  const double ldet_i = EUCLID ? 0.0 : g_ldet[i];
  const double2 *gp = gauss + i;
  double best = KLC_NONE;
  int32_t best_j = 0;
  const int chunks = (C + KLC_CHUNK - 1) / KLC_CHUNK;
  for (int ch = 0; ch < chunks; ch++) {  // ascending: the strict < below keeps the lowest index of equal values
    const int j0 = ch * KLC_CHUNK + wave * KLC_PER_WAVE;
    if (j0 >= C) continue;  // (the whole wave)
    const double *cw = centres + ((int64_t)ch * D * KLC_CHUNK + wave * KLC_PER_WAVE) * 2;
    double acc[KLC_PER_WAVE];
#pragma unroll
    for (int q = 0; q < KLC_PER_WAVE; q++) acc[q] = 0.0;
    for (int k = 0; k < D; k++) {
      const double2 mc = gp[(int64_t)k * G];
      const double *ck = cw + (int64_t)k * KLC_CHUNK * 2;  // the same address in every lane
#pragma unroll
      for (int q = 0; q < KLC_PER_WAVE; q++) {
        const double t = mc.x - ck[2 * q];
        if (EUCLID) acc[q] += t * t;
        else acc[q] += (mc.y + t * t) / ck[2 * q + 1];
      }
    }
#pragma unroll
    for (int q = 0; q < KLC_PER_WAVE; q++) {
      const int j = j0 + q;
      if (j < C) {
        double d;
        bool use = true;
        if (EUCLID) {
          d = sqrt(acc[q]);
        } else {
          d = (c_ldet[j] - ldet_i + acc[q] - (double)D) / 2.0;
          use = c_valid[j] != 0;
        }
        if (use && d < best) {
          best = d;
          best_j = j;
        }
      }
    }
  }
  s_min[wave][lane] = best;
  s_idx[wave][lane] = best_j;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < KLC_WAVES; w++) {
      const double m = s_min[w][lane];
      const int32_t j = s_idx[w][lane];
      // a wave that found nothing holds (1e100, 0); a found value is below 1e100, so it never ties with that
      if (m < best || (m == best && j < best_j)) {
        best = m;
        best_j = j;
      }
    }
    if (gi < G) {
      out_index[gi] = best_j;
      out_dist[gi] = best;
    }
  }
}

void klc_assign_launch(const KlcAssignParams &p, bool euclid, hipStream_t stream) {
  const unsigned blocks = (unsigned)(((int64_t)p.G + 63) / 64);
  if (euclid)
    hipLaunchKernelGGL(k_klc_assign<true>, dim3(blocks), dim3(64 * KLC_WAVES), 0, stream, (const double2 *)p.gauss, p.g_ldet,
                       p.centres, p.c_ldet, p.c_valid, p.dim, p.G, p.C, p.out_index, p.out_dist);
  else
    hipLaunchKernelGGL(k_klc_assign<false>, dim3(blocks), dim3(64 * KLC_WAVES), 0, stream, (const double2 *)p.gauss, p.g_ldet,
                       p.centres, p.c_ldet, p.c_valid, p.dim, p.G, p.C, p.out_index, p.out_dist);
  AASR_HIP(hipGetLastError());
}

// blockIdx.x: the cluster; blockIdx.y * blockDim.x + threadIdx.x: the dimension
__global__ __launch_bounds__(256) void k_klc_centres(const double *__restrict__ mean, const double *__restrict__ cov,
                                                     const int32_t *__restrict__ map, int D, int G, int C,
                                                     double *__restrict__ c_mean, double *__restrict__ c_cov,
                                                     double2 *__restrict__ centres, int32_t *__restrict__ c_count) {
  const int c = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.y * blockDim.x + threadIdx.x;
  const bool live = k < D;
  double sm = 0.0, sc = 0.0;
  int32_t count = 0;
  for (int64_t i0 = 0; i0 < G; i0 += 64) {
    const int64_t i = i0 + lane;
    unsigned long long members = __ballot(i < G && map[i] == c);
    count += __popcll(members);
    while (members) {  // from the lowest bit up: Gaussian order
      const int b = __ffsll((long long)members) - 1;
      members &= members - 1;
      if (live) {
        const int64_t at = (i0 + b) * D + k;
        sm += mean[at];
        sc += cov[at];
      }
    }
  }
  if (live) {
    if (count > 0) {
      const double scale = 1 / (double)count;
      sm *= scale;
      sc *= scale;
    }
    c_mean[(int64_t)c * D + k] = sm;
    c_cov[(int64_t)c * D + k] = sc;
    centres[((int64_t)(c / KLC_CHUNK) * D + k) * KLC_CHUNK + c % KLC_CHUNK] = make_double2(sm, sc);
  }
  if (k == 0) c_count[c] = count;
}

void klc_centres_launch(const KlcCentreParams &p, hipStream_t stream) {
  const int threads = p.dim >= 256 ? 256 : (p.dim + 63) / 64 * 64;
  hipLaunchKernelGGL(k_klc_centres, dim3((unsigned)p.C, (unsigned)((p.dim + threads - 1) / threads)), dim3(threads), 0, stream,
                     p.mean, p.cov, p.map, p.dim, p.G, p.C, p.c_mean, p.c_cov, (double2 *)p.centres, p.c_count);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

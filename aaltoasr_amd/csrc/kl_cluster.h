// kl_cluster.h -- device layout of the Gaussian-pool clustering kernels (kl_cluster.hip), shared with their host
// driver (gcluster.cc).
//
// aku/gcluster.cc in its diagonal mode assigns every pool Gaussian to the nearest of C centres -- Euclidean distance of
// the means for the initial clusters (gcluster.cc:272-288), Kullback-Leibler divergence of diagonal Gaussians for the
// four refinement passes (gcluster.cc:134-165, 300-310) -- and forms a centre from its members' means and covariance
// diagonals in Gaussian order (gcluster.cc:182-223).  Every sum here is the reference's sum, term by term and in its
// order, in double without contraction, so that the maps are equal, not close.
//
// Operands.  The Gaussians as [dim][G][2] (mean, covariance) -- a lane reads its Gaussian's pair of dimension k as one
// 16-byte load, a wave 1 KiB in a row.  The centres in chunks of KLC_CHUNK: [chunk][dim][KLC_CHUNK][2]; the tail of
// the last chunk is (0, 1) and never compared.  ldet [C] and valid [C] are plain.
//
// k_klc_assign: a workgroup is 64 Gaussians (the lane) x KLC_WAVES waves.  The centres are walked in chunks of
// KLC_CHUNK in ascending order; within a chunk wave w takes the KLC_PER_WAVE consecutive centres from
// w * KLC_PER_WAVE on, reads them wave-uniformly (scalar loads: 16 consecutive doubles per dimension) and keeps their
// distances in registers while the dimensions go by in order.  A wave carries (min, index) over the chunks with the
// reference's strict <, from (1e100, 0); its centres come in ascending order, so it ends with the lowest index of its
// smallest value.  The waves' results meet in LDS: the smaller value wins, between equal values the lower index.  That
// is the sequential scan's answer: the first index of the smallest value below 1e100, or 0 when there is none.
//
// k_klc_centres: a workgroup per cluster, a thread per dimension.  Every wave reads the map 64 entries at a time; the
// members' bits of the ballot are taken from the lowest up, so a thread adds its members' values in Gaussian order.
// No atomics, no tree: the same input gives the same bytes.  The sums are scaled by 1 / count (a product, as
// Blas_Scale does it) and written plain ([C][dim], for the host's ldet) and into the chunked operand.
//
// Not modelled: the reference's Euclidean norm is BLAS dnrm2, whose scaled summation can differ from
// sqrt(sum of squares in dimension order) in the last place; two centres that tie under one need not tie under the
// other.  The kernel compares the correctly rounded square root of the in-order sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int KLC_WAVES = 4;                           // waves of an assignment workgroup
constexpr int KLC_PER_WAVE = 8;                        // centres a wave holds distances for
constexpr int KLC_CHUNK = KLC_WAVES * KLC_PER_WAVE;    // centres per chunk
constexpr double KLC_NONE = 1e100;                     // the reference's starting minimum

inline int64_t klc_chunks(int n_clusters) { return ((int64_t)n_clusters + KLC_CHUNK - 1) / KLC_CHUNK; }
// doubles of the chunked centre operand
inline int64_t klc_centre_doubles(int dim, int n_clusters) { return klc_chunks(n_clusters) * dim * KLC_CHUNK * 2; }
// where centre c's (mean, covariance) of dimension k sits in it
inline int64_t klc_centre_at(int dim, int c, int k) {
  return (((int64_t)(c / KLC_CHUNK) * dim + k) * KLC_CHUNK + c % KLC_CHUNK) * 2;
}

struct KlcAssignParams {
  const double *gauss;     // [dim][G][2]
  const double *g_ldet;    // [G] (not read by the Euclidean pass)
  const double *centres;   // chunked
  const double *c_ldet;    // [C]
  const int32_t *c_valid;  // [C]
  int32_t dim, G, C;
  int32_t *out_index;      // [G]
  double *out_dist;        // [G]
};
// euclid: the norm of the mean difference over ALL centres; otherwise the divergence over the valid ones
void klc_assign_launch(const KlcAssignParams &p, bool euclid, hipStream_t stream);

struct KlcCentreParams {
  const double *mean, *cov;  // plain [G][dim]
  const int32_t *map;        // [G], every entry in 0 ... C - 1
  int32_t dim, G, C;
  double *c_mean, *c_cov;    // plain [C][dim]
  double *centres;           // chunked (the tail of the last chunk is left as it is)
  int32_t *c_count;          // [C] members
};
void klc_centres_launch(const KlcCentreParams &p, hipStream_t stream);

}  // namespace aasr

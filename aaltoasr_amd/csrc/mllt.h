// mllt.h -- device layout of the MLLT estimation kernels (mllt.hip), shared with their host driver (estimate.cc).
//
// HmmSet::estimate_mllt (aku/HmmSet.cc:841-1056) walks the pool dim + 1 times per outer iteration and rebuilds every
// Gaussian's sample covariance each time.  Here the covariances S_g = M2_g / gamma_g - mean_g mean_g^T are built once
// (k_mllt_cov) and stay on the device, and an iteration is two passes over them:
//   k_mllt_var:   sigma2_gi = a_i S_g a_i^T for every Gaussian g and row i of the current A,
//   k_mllt_gsum:  G_i = sum_g w_gi S_g for every i, a [dim x G] [G x E] product on the FP64 matrix pipe.
//
// Layout.  A covariance is its packed lower triangle, entry e = r (r + 1) / 2 + c (c <= r), E = dim (dim + 1) / 2
// entries padded to EP = 16 ET.  The resident array is ENTRY-MAJOR: cov[e][g], rows of GP doubles, GP = the pool
// padded to whole items of MLLT_ITEM Gaussians.  Both passes then read whole lines: k_mllt_var has a lane per
// Gaussian, so a wave's load of one entry is 64 consecutive doubles; k_mllt_gsum's lane loads four consecutive
// Gaussians of its entry, a wave 16 entries x 16 Gaussians.  Padding entries, padding Gaussians and Gaussians
// without statistics are zero in cov and in the weights, so neither pass needs a bound inside an item.
//
// k_mllt_var multiplies an entry by a host-made coefficient table p[e][i] = a_ir a_ic (twice that off the diagonal),
// which every lane of a wave reads at the same address: sigma2_gi = sum_e p_ie S_g(e), one FMA per entry and row.
//
// k_mllt_gsum cuts the pool into items of MLLT_ITEM consecutive Gaussians.  A wave owns MLLT_NE entry tiles of 16
// and all PB = ceil(dim / 16) row blocks of one item and writes them to the item's slab [16 PB][EP];
// k_mllt_slab_add adds a launch's slabs in item order to the sums.  No atomics: the same input gives the same bytes,
// whatever the slab bound cuts a call into (the rule of scatter.h).
//
// Slab memory: an item's slab is 16 PB x EP doubles -- 48 x 784 x 8 = 294 KiB at 39 dimensions, 64 x 2 016 x 8 =
// 1 008 KiB at 63.  A launch holds at most MLLT_SLAB_BYTES = 64 MiB of slabs: 222 items (56 832 Gaussians) at 39
// dimensions, 65 items at 63.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace aasr {

constexpr int MLLT_ITEM = 256;  // Gaussians per work item
constexpr int MLLT_NE = 2;      // entry tiles per wave
constexpr int MLLT_WAVES = 4;   // waves per workgroup of k_mllt_gsum
constexpr int MLLT_MAX_DIM = 63;
constexpr int64_t MLLT_SLAB_BYTES = (int64_t)64 << 20;

inline int mllt_pb(int dim) { return (dim + 15) / 16; }
inline int mllt_entries(int dim) { return dim * (dim + 1) / 2; }
inline int mllt_et(int dim) { return (mllt_entries(dim) + 15) / 16; }
// rows of the resident array: the entry tiles padded to whole workgroups of k_mllt_gsum, so that its loads need no bound
inline int64_t mllt_cov_rows(int dim) {
  const int per = MLLT_NE * MLLT_WAVES;
  return (int64_t)16 * ((mllt_et(dim) + per - 1) / per * per);
}
inline int64_t mllt_gp(int64_t n_gauss) { return (n_gauss + MLLT_ITEM - 1) / MLLT_ITEM * MLLT_ITEM; }
// doubles of one item's slab and of the sums
inline int64_t mllt_slab_doubles(int dim) { return (int64_t)16 * mllt_pb(dim) * 16 * mllt_et(dim); }

// cov[e][g] = m2[g][e] (1 / gamma_g) - mean_gr mean_gc with mean = sum_x (1 / gamma), zero where ok[g] == 0.
// gamma [G], sum_x [G x dim], m2 [G x E] (device); cov [mllt_cov_rows x GP] must be zero beforehand.
void mllt_cov_launch(int dim, int64_t n_gauss, const double *gamma, const double *sum_x, const double *m2, const int32_t *ok,
                     double *cov, hipStream_t stream);
// var[g][i] = sum_e p[e][i] cov[e][g]; p [E x 16 PB] (device, zero past dim), var [G x dim]
void mllt_var_launch(int dim, int64_t n_gauss, const double *cov, const double *p, double *var, hipStream_t stream);
// slabs of items [item0, item0 + n_items) from the weights w [GP x 16 PB], then sums += the slabs in item order
void mllt_gsum_launch(int dim, int64_t gp, const double *cov, const double *w, int item0, int n_items, double *slab,
                      double *sums, hipStream_t stream);

// LU inverse with partial pivoting (mllr.cc): a becomes its inverse, *det the product of U's diagonal without the
// permutation's sign.  false: a zero pivot.
bool lu_inverse(std::vector<double> &a, int n, double *det);

}  // namespace aasr

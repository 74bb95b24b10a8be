// gmm_build.h -- what the model-builder units share (gmm_files.cc, gmm_model.cc, gmm_tracks.cc, gmm_parts.cc,
// gmm_centred.cc, gmm_fullcov.cc).  Internal: nothing else includes it; the builder's entry points are in gmm.h.
#pragma once
#include <cstring>

#include "gmm.h"

namespace aasr {

static const double kLog2e = 1.4426950408889634073599246810019;
// log2-domain value standing in for log(0): exp2(x - max) underflows to 0 for
// any live component, and an all-null segment still reduces to a finite value
// that the 1e-50 floor then clamps.
static const float kNullConst = -1.0e30f;
// reference exponent of the track layouts and the factor rows (gmm_tracks.cc, "Track layouts")
static const double kRefMin = 56.0, kRefMax = 72.0;
static const double kPeakMax = 120.0;  // max (peak*log2e + ref) accepted

struct RowSpec {
  int64_t g;        // pool Gaussian, < 0 for a null (padding) row
  double logw;      // log mixture weight (natural), -inf for zero weight
  double bias = 0;  // added to the constant in log2 units (paired layout reference)
  int pg = 0;       // pivot group of the row's state (multi-pivot layouts; the model's one pivot otherwise)
};

// gmm_model.cc: the f32 tile packers
void pack_coef_rows(int nkk, const std::vector<double> &coef, int64_t n_rows, PackedRows &out);
void pack_rows(const aasr_gmm *g, const std::vector<RowSpec> &rows, PackedRows &out, std::vector<double> *a64_host,
               bool upload_f32 = true);
// gmm_parts.cc
void build_pg_model(aasr_gmm *g);
// gmm_tracks.cc
void f16x2_state_eligibility(const aasr_gmm *g, std::vector<uint8_t> &ok);
// gmm_centred.cc
int centred_dimp_for(int D);
void find_outliers(aasr_gmm *g);

// Index of element (row r, K index k = 2*kk + h) in the [tiles][nkk/2][64][4] layout of PackedRows::a: lane
// l = h*32 + r32 of kk-pair q holds
//   { A[r32][2(2q)+h], A[r32][2(2q+1)+h], A[32+r32][2(2q)+h], A[32+r32][2(2q+1)+h] }
inline size_t coef_tile_index(int nkk, int64_t r, int kk, int h) {
  const size_t tile_floats = (size_t)(nkk / 2) * 64 * 4;
  const int64_t t = r / TILE_ROWS;
  const int j = (int)(r % TILE_ROWS);
  const int mb = j / 32, r32 = j % 32;
  const int q = kk / 2, e = kk % 2;
  return (size_t)t * tile_floats + ((size_t)q * 64 + (size_t)(h * 32 + r32)) * 4 + (size_t)(mb * 2 + e);
}

// Index of term sp (of n_sp) of element (row r, K index k) in the [tiles][nk16][n_sp][2][64][8] layout of the
// split-term rows (TrackLayout / FullLayout: a16 with three bf16 terms, a16h with two fp16 terms)
inline size_t split_tile_index(int nk16, int n_sp, int64_t r, int k, int sp) {
  const size_t tile_elems = (size_t)nk16 * n_sp * 2 * 64 * 8;
  const int64_t t = r / TILE_ROWS;
  const int jrow = (int)(r % TILE_ROWS);
  const int mb = jrow / 32, m32 = jrow % 32;
  const int slab = k / 16, hk = (k % 16) / 8, i = k % 8;
  const int lane = hk * 32 + m32;
  return (size_t)t * tile_elems + ((((size_t)slab * n_sp + sp) * 2 + mb) * 64 + lane) * 8 + i;
}

inline int64_t track_row(int64_t pos, int h, int e) {
  // quad position `pos` of track h, element e -> row in the tile-major layout
  int64_t t = pos / 8;
  int mb = (int)((pos / 4) % 2), q = (int)(pos % 4);
  return t * TILE_ROWS + mb * 32 + 8 * q + 4 * h + e;
}

inline uint16_t bf16_rne(float x, float *back) {
  uint32_t u;
  memcpy(&u, &x, 4);
  uint32_t r = u + 0x7fffu + ((u >> 16) & 1u);
  uint16_t h = (uint16_t)(r >> 16);
  uint32_t b = (uint32_t)h << 16;
  memcpy(back, &b, 4);
  return h;
}

// log sqrt(prod_d 1 / var_d) of a diagonal Gaussian: DiagonalGaussian::read + set_constant (aku/Distributions.cc:1144-1147,
// 1273-1288).  A non-positive variance is a precision of 0; a product that is not positive comes back as it is (0: the
// reference's "invalid" Gaussian; NaN: for the caller to refuse).
inline double diag_log_sqrt_det(const double *var, int D) {
  double prod = 1;
  for (int d = 0; d < D; d++) prod *= var[d] > 0 ? 1 / var[d] : 0;
  return prod > 0 ? std::log(std::sqrt(prod)) : prod;
}

// Conditioning of one Gaussian's expanded form around `pivot` (gmm.h, KAPPA_LIMIT): returns kappa = sum_d t_d with
// t_d = p_d (mu_d - pivot_d)^2, and sum_d t_d^2 in *k2 (the limits on kappa2 compare its square root).
inline double kappa_terms(const double *mu, const double *var, const float *pivot, int D, double *k2) {
  double k = 0;
  *k2 = 0;
  for (int d = 0; d < D; d++) {
    const double p = var[d] > 0 ? 1 / var[d] : 0;
    const double mc = mu[d] - (double)pivot[d];
    k += p * mc * mc;
    *k2 += (p * mc * mc) * (p * mc * mc);
  }
  return k;
}

// The product of the diagonal of A in a CMLLR matrix W = [b | A] (D rows of D + 1): the reference's "determinant"
// (full_matrix_determinant, aku/LinearAlgebra.cc:73-86, LU-factorises a copy and then multiplies the diagonal of the
// matrix it was given), which AdaptedGaussian::compute_likelihood multiplies the likelihood by
// (aku/ModelModules.hh:172-173).  Multiplied in row order.
inline double transform_diag_product(const double *W, int D) {
  double det = 1;
  for (int i = 0; i < D; i++) det *= W[(size_t)i * (D + 1) + 1 + i];
  return det;
}

// Splits W = [b | A] (ConstrainedMllr::load_transform) into A [D x D] and b [D]; returns transform_diag_product(W).
inline double split_transform(const double *W, int D, double *A, double *b) {
  for (int i = 0; i < D; i++) {
    b[i] = W[(size_t)i * (D + 1)];
    for (int j = 0; j < D; j++) A[(size_t)i * D + j] = W[(size_t)i * (D + 1) + 1 + j];
  }
  return transform_diag_product(W, D);
}

// Lower Cholesky factor of the symmetrised a (row-major d x d): a = r r^T.  False when a is not positive definite.
inline bool cholesky_lower(int d, const double *a, std::vector<double> &r) {
  r.assign((size_t)d * d, 0.0);
  for (int j = 0; j < d; j++) {
    double s = a[(size_t)j * d + j];
    for (int k = 0; k < j; k++) s -= r[(size_t)j * d + k] * r[(size_t)j * d + k];
    if (!(s > 0)) return false;
    double rjj = std::sqrt(s);
    r[(size_t)j * d + j] = rjj;
    for (int i = j + 1; i < d; i++) {
      double t = 0.5 * (a[(size_t)i * d + j] + a[(size_t)j * d + i]);
      for (int k = 0; k < j; k++) t -= r[(size_t)i * d + k] * r[(size_t)j * d + k];
      r[(size_t)i * d + j] = t / rjj;
    }
  }
  return true;
}

// w = r^-1 of a lower-triangular r
inline void invert_lower(int d, const std::vector<double> &r, std::vector<double> &w) {
  w.assign((size_t)d * d, 0.0);
  for (int c = 0; c < d; c++) {
    w[(size_t)c * d + c] = 1.0 / r[(size_t)c * d + c];
    for (int i = c + 1; i < d; i++) {
      double s = 0;
      for (int k = c; k < i; k++) s += r[(size_t)i * d + k] * w[(size_t)k * d + c];
      w[(size_t)i * d + c] = -s / r[(size_t)i * d + i];
    }
  }
}

}  // namespace aasr

// tie.h -- device layout of the state-tying search (tie_split.hip), shared with its host driver (tie.cc).
//
// PhonePool (aku/PhonePool.cc) keeps a full-covariance Gaussian per context-phone state and rebuilds a cluster's
// Gaussian from its members' occ (Sigma + mu mu^T) whenever it tries a rule (Gaussian::merge,
// aku/Distributions.cc:854-897).  Here every context-phone state keeps its RAW sums as one row
//   M_p = [gamma, sum x (d), packed lower triangle of sum x x^T (row-major, j <= i)],   E = 1 + d + d (d + 1) / 2
// doubles, padded with zeros to EP = a multiple of 16.  A cluster's or a candidate's statistic is the sum of its
// members' rows, and mean and covariance come from the summed row once: mu = sum x / gamma,
// Sigma = sum x x^T / gamma - mu mu^T.
//
// k_tie_pack: the rows from the scatter accumulator's tiles (scatter.h), a thread per value, through a table of the
// E tile offsets.
//
// k_tie_masked_sum: out[r][e] = sum_k bit(r, k) In[idx[k]][e] for many jobs in one launch.  A job is a list of
// n_k input rows (idx, any order, repeats allowed) and n_rows 0/1 masks over that list, kept as 32-bit words
// (bit k % 32 of word k / 32, wpr words a row).  Work item = one wave: (job, tile of 16 mask rows, group of
// TIE_NE tiles of 16 columns).  f64 16x16x4 with A[row][k] = the mask bit as 0.0 / 1.0 and B[k][col] = the input
// value; k runs over the list four at a time from its start, a list position past n_k contributes 0 x 0.  One
// accumulator per output value, no atomics, no second pass: the order of the sum is the order of the list, and the
// same call gives the same bytes.  The inputs must be finite (0 x inf would spoil a row that masks it out).
//
// k_tie_logdet: a wave per SIDE.  A side is a row of the sums, or the difference or the sum of two rows
// (TIE_SIDE_ROW / _SUB / _ADD): parent - yes for the other half of a split, a + b for the parent of a merge.  The
// wave builds Sigma in LDS (d x d doubles, row stride d | 1: 63 x 63 x 8 = 31 752 bytes at the largest d), runs
// the reference's column Cholesky (LinearAlgebra::cholesky_factor: column j takes its earlier columns off in k
// order, then the square root, then the division -- a lane per row, no pivot test, so a matrix that is not positive
// definite yields NaN or an infinity exactly as IEEE arithmetic does on the host), and leaves gamma and
// 2 sum log L_ii.
// k_tie_gain: a thread per candidate (parent side, child 1 side, child 2 side):
// (gamma_p ld_p - gamma_1 ld_1 - gamma_2 ld_2) / 2, PhonePool::compute_log_likelihood_gain's expression.
// A parent that many candidates share is factored once.
//
// d = 1 ... TIE_MAX_DIM = 63 (MLLT's range): one matrix stays within 32 KiB of LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int TIE_MAX_DIM = 63;
constexpr int TIE_NE = 4;  // column tiles of a masked-sum work item

inline int64_t tie_row_values(int dim) { return 1 + (int64_t)dim + (int64_t)dim * (dim + 1) / 2; }
inline int64_t tie_row_stride(int dim) { return (tie_row_values(dim) + 15) / 16 * 16; }
inline int tie_lds_stride(int dim) { return dim | 1; }
inline size_t tie_lds_bytes(int dim) { return (size_t)dim * tie_lds_stride(dim) * sizeof(double); }

struct TieJob {
  int32_t idx0;   // first entry of the job's list in idx
  int32_t n_k;    // entries of the list
  int32_t mask0;  // first word of the job's masks
  int32_t wpr;    // words per mask row: (n_k + 31) / 32
  int32_t n_rows;
  int32_t out0;  // first output row
};

struct TieItem {
  int32_t job;
  int32_t rtile;   // mask rows 16 rtile ... 16 rtile + 15
  int32_t ctile0;  // column tiles ctile0 ... ctile0 + TIE_NE - 1
  int32_t pad;
};

enum { TIE_SIDE_ROW = 0, TIE_SIDE_SUB = 1, TIE_SIDE_ADD = 2 };
struct TieSide {
  int32_t a, b;  // rows of the sums; b unused for TIE_SIDE_ROW
  int32_t op;
  int32_t pad;
};

struct TieCand {
  int32_t parent, child1, child2;  // sides
  int32_t pad;
};

// rows [n_classes x EP] from the accumulator (class stride TS); map: the E tile offsets
void tie_pack_launch(const double *acc, int64_t TS, const int32_t *map, int dim, int n_classes, double *rows,
                     hipStream_t stream);
void tie_masked_sum_launch(int dim, const double *in, const int32_t *idx, const uint32_t *mask, const TieJob *jobs,
                           const TieItem *items, int n_items, double *out, hipStream_t stream);
// ld_gamma: [n_sides x 2] = (2 sum log L_ii, gamma)
void tie_logdet_launch(int dim, const double *sums, const TieSide *sides, int n_sides, double *ld_gamma, hipStream_t stream);
void tie_gain_launch(const double *ld_gamma, const TieCand *cands, int n_cands, double *gain, hipStream_t stream);

}  // namespace aasr

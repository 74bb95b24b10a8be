// mllr.h -- device layout of the CMLLR statistics accumulation (mllr_accum.hip), shared with its host
// driver (mllr.cc).
//
// MllrTrainer::collect_data (aku/MllrTrainer.cc:22-60, 147-163) adds, per frame and Gaussian g of the frame's
// mixture, (gamma_g / var_gi) xi xi^T to G_i and (gamma_g mu_gi / var_gi) xi to k_i for every dimension i, with
// xi = [1, x].  Summed over g first that is G_i += w_ti xi xi^T and k_i += u_ti xi with per-frame weights
//   w_ti = sum_g gamma_tg / var_gi,   u_ti = sum_g gamma_tg mu_gi / var_gi,   beta += sum_g gamma_tg.
// Pass 1 forms w, u and the frame's share of beta; pass 2 computes the rank-k updates of a chunk of frames on the
// f64 matrix pipe into a slab of 16 x 16 tiles; pass 3 adds the slabs of a launch in chunk order to the
// accumulators.  No atomics: the same input gives the same bytes.
//
// Tiles: d + 1 is padded to PB blocks of 16.  G_i keeps the tiles (R, C) with R >= C, tile R (R + 1) / 2 + C, each
// [row][col] of 256 doubles; k is the (d + 1) x (d + 1 padded) product U^T Xi with U = [u | beta share], so
// that row d, column 0 of it is beta: PB x PB tiles after the d G blocks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

constexpr int MLLR_CHUNK = 1024;     // frames per slab
constexpr int MLLR_MAX_CHUNKS = 64;  // slabs per launch: a call is cut into launches of 65 536 frames
constexpr int MLLR_THREADS = 256;
constexpr int MLLR_P1_FRAMES = 64;   // frames per workgroup of pass 1
constexpr int MLLR_MAX_DIM = 63;

inline int mllr_pb(int dim) { return (dim + 1 + 15) / 16; }
inline int mllr_g_tiles(int pb) { return pb * (pb + 1) / 2; }
// doubles of one slab (and of the accumulator)
inline int64_t mllr_slab_doubles(int dim) {
  const int pb = mllr_pb(dim);
  return ((int64_t)dim * mllr_g_tiles(pb) + pb * pb) * 256;
}

struct MllrParams {
  const double *x;           // frame rows [n x dim]
  const int32_t *pdf;        // per frame, -1: skip
  int32_t n, dim;
  const double *recs;        // AASR_PREC_F64 records: [mean x dimp][precision x dimp][constant, weight]
  int32_t rec, dimp;
  const int32_t *state_off;  // first record of every pdf
  const double *inv_var;     // per record [dim]: 1 / var
  const double *mean_var;    // per record [dim]: mean / var
  int32_t max_comps;
  double *w;                 // [n x dim]
  double *u;                 // [n x (dim + 1)], column dim: the frame's share of beta
  int32_t *ok;               // [n] 1: the frame contributes
};

void mllr_weights_launch(const MllrParams &p, hipStream_t stream);
// slabs of the chunks of n frames (n <= MLLR_CHUNK MLLR_MAX_CHUNKS), then acc += the slabs in chunk order
void mllr_rank_launch(const MllrParams &p, double *slab, double *acc, hipStream_t stream);
size_t mllr_weights_lds_bytes(int dim, int max_comps);

// Pass 1 from weighted entries (mllr_entries.hip): frame t has the entries off[t] .. off[t + 1] of (pdf, weight), walked
// in list order; entry (pdf, p) adds p lik_g / sum_g lik_g per Gaussian to the frame's running w, u and beta share.  It
// writes the w, u and ok that passes 2 and 3 read, for every frame of the launch (zeros for a frame without entries).
struct MllrEntryParams {
  MllrParams p;           // pdf unused; x, w, u, ok of the launch's frames
  const int64_t *off;     // [n + 1] of the launch's frames, absolute into pdf / weight
  const int32_t *pdf;     // per entry; outside 0 .. n_states: the entry is skipped
  const double *weight;   // per entry
  int64_t n_entries;      // an offset outside 0 .. n_entries ends the frame's list
  int32_t n_states;
};
void mllr_entry_weights_launch(const MllrEntryParams &p, hipStream_t stream);
size_t mllr_entry_weights_lds_bytes(int dim, int max_comps);

}  // namespace aasr

// stats.h -- device layout of ML statistics accumulation (stats_accum.hip), shared with its host
// driver (stats.cc), and the statistics handle as its writers (stats_files.cc) and the recipe driver
// (stats_recipe.cc) see it.
//
// Frames are grouped by pdf on the host: a compressed row list of the frames of every pdf, cut into
// work items of at most STATS_CHUNK frames.  An item's workgroup writes one slab of partial sums:
// per mixture component [gamma, aux gamma, sum gamma x (dim), sum gamma x^2 (dim)] and then
// [frames with a positive total, mixture_ll].  The pdf pass adds the slabs of a pdf in item order
// to the per-record accumulators; the Gaussian pass adds the records that share a pool Gaussian in
// record order.  No atomics: the same input gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "stats_full.h"

struct aasr_gmm;

namespace aasr {

constexpr int STATS_CHUNK = 1024;  // frames per work item at most
constexpr int STATS_THREADS = 256;

struct StatsItem {
  int64_t row_begin;  // first entry of the item's frames in the row list
  int64_t slab;       // first double of its slab
  int32_t pdf, n;
};

struct StatsParams {
  const double *x;           // frame rows [n_frames x dim]
  int32_t dim;
  const int32_t *rows;       // row list grouped by pdf, frame order within a pdf
  const StatsItem *items;
  const double *recs;        // AASR_PREC_F64 records: [mean x dimp][precision x dimp][constant, weight]
  int32_t rec;               // doubles per record (2 dimp + 2)
  const int32_t *state_off;  // first record of every pdf
  double *slab;
  double *frame_ll;          // per frame safe_log(total), or null
  int32_t block;             // frames per sub-block (posteriors held in LDS)
  int32_t lds_recs;          // 1: the mixture's records are staged in LDS
  int32_t max_comps;         // largest mixture of the launch
};

// Host: the row list of a call, shared by the handles that take frames with a pdf each (stats.cc, seg_loglik.cc).
// rows: the frames with a pdf >= 0 grouped by pdf, frame order within a pdf; cnt[s] the first entry of pdf s
// (S + 1 entries).  A pdf >= S raises "<what>: pdf %d of frame %ld out of range" (AASR_ERR_INVALID) before anything
// is written; frames with a negative pdf are left out.
void rows_by_pdf(const char *what, int S, const int32_t *pdf, int64_t n_frames, std::vector<int64_t> *cnt,
                 std::vector<int32_t> *rows);
// Host: the models these handles refuse (AASR_ERR_UNSUPPORTED, "<tool>: ..."): full-covariance and subspace
// Gaussians, model-side transforms.  Asks the device for nothing.
void check_stats_model(const aasr_gmm *g, const char *tool = "stats");

// per-item partial sums (one workgroup per item)
void stats_items_launch(const StatsParams &p, int dimp, int n_items, hipStream_t stream);
// The same with a weight per entry of the row list (stats_weighted.hip): Mixture::accumulate with gamma = weights[e]
// for entry e, rows a device array like the weights.  p.frame_ll is not written (a frame may have several pdfs).  An
// entry whose row is outside 0 .. n_frames is the caller's mistake: no frame is read for it and it adds nothing.
void stats_items_w_launch(const StatsParams &p, const double *weights, int64_t n_frames, int dimp, int n_items,
                          hipStream_t stream);
// per-pdf sums of the items' slabs into the record accumulators racc [records x (2 + 2 dim)] and
// the pdf accumulators pacc [pdfs x 2] (frames with a positive total, mixture_ll)
void stats_pdf_reduce_launch(const int32_t *pdfs, const int32_t *item_begin, int n_pdfs, const StatsItem *items,
                             const double *slab, const int32_t *state_off, int dim, double *racc, double *pacc,
                             hipStream_t stream);
// per pool Gaussian: [feacount, gamma, aux gamma, sum x (dim), sum x^2 (dim)] from the records
// g_rec[g_off[g] .. g_off[g+1]) (rec_pdf: the pdf of every record)
void stats_gauss_reduce_launch(const double *racc, const double *pacc, const int32_t *g_off, const int32_t *g_rec,
                               const int32_t *rec_pdf, int n_gauss, int dim, double *gacc, hipStream_t stream);

}  // namespace aasr

// ---- the statistics handle ---------------------------------------------------------------------

struct aasr_stats {
  aasr_gmm *gmm = nullptr;
  int D = 0, S = 0, G = 0, K = 0, W = 0, dimp = 0, rec = 0, max_comps = 0;
  std::vector<int32_t> mix_off, mix_idx;
  std::vector<int32_t> tr_source, tr_offset;
  std::vector<double> tr_count;
  aasr::DevBuf<double> racc, pacc, gacc, slab;
  aasr::DevBuf<int32_t> d_rows, d_pdfs, d_item_begin, g_off, g_rec, rec_pdf;
  aasr::DevBuf<aasr::StatsItem> d_items;
  // host staging of the last accumulate call, kept until its uploads are done
  std::vector<int32_t> h_rows, h_pdfs, h_item_begin;
  std::vector<aasr::StatsItem> h_items;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  // shape of the last launch of the item kernel (aasr_debug_stats_shape): dimp, block, lds_recs, max_comps, items
  int32_t last_shape[5] = {0, 0, 0, 0, 0};
  // host copies after aasr_stats_fetch
  bool fetched = false;
  std::vector<double> h_racc, h_pacc, h_gacc;
  // full second moments (aasr_stats_create_full): per pool Gaussian the tiles of sum gamma xi xi^T (stats_full.h)
  bool full = false;
  int64_t TS = 0;  // doubles of a Gaussian's accumulator and of a unit's slab
  int64_t full_slab_bytes = aasr::STATS_FULL_SLAB_BYTES;
  aasr::DevBuf<double> facc, fslab, fgam, fpacked;
  aasr::DevBuf<aasr::FullItem> d_fitems;
  aasr::DevBuf<aasr::FullUnit> d_funits;
  aasr::DevBuf<aasr::FullGroup> d_fgroups;
  aasr::DevBuf<int32_t> d_fentries;
  std::vector<aasr::FullItem> h_fitems;
  std::vector<aasr::FullUnit> h_funits;
  std::vector<aasr::FullGroup> h_fgroups;
  std::vector<int32_t> h_fentries;
  int32_t full_shape[4] = {0, 0, 0, 0};  // PB, work items, launches, units of the last call (aasr_debug_stats_full_shape)
  std::vector<double> h_full;            // after a fetch: [G x dim (dim + 1) / 2]
  ~aasr_stats() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace aasr {

// "<what>: null argument" / "<what>: call aasr_stats_fetch after the last accumulation"
void require_fetched(const aasr_stats *h, const char *what);

}  // namespace aasr

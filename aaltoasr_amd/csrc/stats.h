// stats.h -- device layout of ML statistics accumulation (stats_accum.hip), shared with its host
// driver (stats.cc).
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

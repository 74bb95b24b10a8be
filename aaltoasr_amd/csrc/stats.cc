// stats.cc -- ML statistics collection (aku/stats.cc with --ml over .phn segmentations): the statistics
// handle that drives the device accumulation (stats_accum.hip), the dump writers of
// HmmSet::dump_statistics and the stats main loop over a recipe (aasr_run_stats_recipe,
// stats.cc:73-170, 540-620, 740-795) over .phn segmentations, or with aasr_run_stats_networks_recipe Baum-Welch over
// the recipe's HMM networks (hmmnet_fb.hip, fb_entries.hip, stats_weighted.hip).  The segmentation reader is
// recipe_pass.cc's.  A handle made by aasr_stats_create_full also collects the full second moments
// (stats_full_accum.hip) and dumps mode 3.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "hmmnet.h"
#include "hmmnet_fb.h"
#include "recipe_pass.h"
#include "stats.h"
#include "stats_full.h"

using namespace aasr;

namespace aasr {

static double safe_log(double x) { return x < 1e-50 ? std::log(1e-50) : std::log(x); }

}  // namespace aasr

// ---- the statistics handle ---------------------------------------------------------------------

struct aasr_stats {
  aasr_gmm *gmm = nullptr;
  int D = 0, S = 0, G = 0, K = 0, W = 0, dimp = 0, rec = 0, max_comps = 0;
  std::vector<int32_t> mix_off, mix_idx;
  std::vector<int32_t> tr_source, tr_offset;
  std::vector<double> tr_count;
  DevBuf<double> racc, pacc, gacc, slab;
  DevBuf<int32_t> d_rows, d_pdfs, d_item_begin, g_off, g_rec, rec_pdf;
  DevBuf<StatsItem> d_items;
  // host staging of the last accumulate call, kept until its uploads are done
  std::vector<int32_t> h_rows, h_pdfs, h_item_begin;
  std::vector<StatsItem> h_items;
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
  int64_t full_slab_bytes = STATS_FULL_SLAB_BYTES;
  DevBuf<double> facc, fslab, fgam, fpacked;
  DevBuf<FullItem> d_fitems;
  DevBuf<FullUnit> d_funits;
  DevBuf<FullGroup> d_fgroups;
  DevBuf<int32_t> d_fentries;
  std::vector<FullItem> h_fitems;
  std::vector<FullUnit> h_funits;
  std::vector<FullGroup> h_fgroups;
  std::vector<int32_t> h_fentries;
  int32_t full_shape[4] = {0, 0, 0, 0};  // PB, work items, launches, units of the last call (aasr_debug_stats_full_shape)
  std::vector<double> h_full;            // after a fetch: [G x dim (dim + 1) / 2]
  ~aasr_stats() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace aasr {

void rows_by_pdf(const char *what, int S, const int32_t *pdf, int64_t n_frames, std::vector<int64_t> *cnt_out,
                 std::vector<int32_t> *rows) {
  std::vector<int64_t> &cnt = *cnt_out;
  cnt.assign((size_t)S + 1, 0);
  for (int64_t f = 0; f < n_frames; f++) {
    if (pdf[f] >= S) raise(AASR_ERR_INVALID, "%s: pdf %d of frame %ld out of range", what, pdf[f], (long)f);
    if (pdf[f] >= 0) cnt[(size_t)pdf[f] + 1]++;
  }
  for (int s = 0; s < S; s++) cnt[(size_t)s + 1] += cnt[(size_t)s];
  rows->resize((size_t)std::max<int64_t>(1, cnt[(size_t)S]));
  std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
  for (int64_t f = 0; f < n_frames; f++)
    if (pdf[f] >= 0) (*rows)[(size_t)fill[(size_t)pdf[f]]++] = (int32_t)f;
}

void check_stats_model(const aasr_gmm *g, const char *tool) {
  if (g->host.any_full())
    raise(AASR_ERR_UNSUPPORTED, "%s: full-covariance and subspace Gaussians are not supported (diagonal pools only)", tool);
  if (!g->host.gauss_bias.empty())
    raise(AASR_ERR_UNSUPPORTED, "%s: subspace Gaussians are not supported (diagonal pools only)", tool);
  if (g->host.n_transforms > 0)
    raise(AASR_ERR_UNSUPPORTED, "%s: model-side transforms (cmllr) are not supported", tool);
}

// The item kernel's shape for a model whose largest mixture has max_comps components of rec doubles a record.
// Sub-block: as many frames as the posteriors of the largest mixture allow in 48 KB of LDS, 64 at least (60 KB then,
// beyond that the model is refused); the mixture's records are staged in LDS where 64 KB hold them as well.
static void stats_launch_shape(int max_comps, int rec, int32_t *block, int32_t *lds_recs) {
  int b = STATS_THREADS;
  while (b > 64 && (size_t)b * (max_comps + 2) * 8 > 48 * 1024) b -= 64;
  if ((size_t)b * (max_comps + 2) * 8 > 60 * 1024)
    raise(AASR_ERR_UNSUPPORTED, "stats: mixtures of %d components exceed the accumulation kernel's LDS", max_comps);
  *block = b;
  *lds_recs = (size_t)(b * (max_comps + 2) + max_comps * rec) * 8 + (size_t)b * 8 <= 64 * 1024 ? 1 : 0;
}

// The work items of a call from the first entry of every pdf in its row list (cnt, S + 1 entries): per pdf with entries
// items of at most STATS_CHUNK of them, the pdfs that have items and their first item -> the doubles of the slabs.
static int64_t stats_build_items(aasr_stats *h, const std::vector<int64_t> &cnt) {
  h->h_items.clear();
  h->h_pdfs.clear();
  h->h_item_begin.assign(1, 0);
  int64_t slab_total = 0;
  for (int s = 0; s < h->S; s++) {
    const int64_t c = cnt[(size_t)s + 1] - cnt[(size_t)s];
    const int M = h->mix_off[(size_t)s + 1] - h->mix_off[(size_t)s];
    if (c == 0) continue;  // (a mixture without components still gets its items: total 0, safe_log(0) per frame)
    const int64_t pieces = (c + STATS_CHUNK - 1) / STATS_CHUNK, per = (c + pieces - 1) / pieces;
    for (int64_t b = 0; b < c; b += per) {
      StatsItem it;
      it.row_begin = cnt[(size_t)s] + b;
      it.n = (int32_t)std::min(per, c - b);
      it.pdf = s;
      it.slab = slab_total;
      slab_total += (int64_t)M * h->W + 2;
      h->h_items.push_back(it);
    }
    h->h_pdfs.push_back(s);
    h->h_item_begin.push_back((int32_t)h->h_items.size());
  }
  return slab_total;
}

// The full second moments of a call whose row list (grouped by pdf, cnt[s] the first entry of pdf s) is on its way to
// h->d_rows: items of at most SCATTER_ITEM rows, a unit per (item, component), launches of whole items within the
// slab bound, and per launch the units of every pool Gaussian in unit order (stats_full.h).
struct FullLaunch {
  int item0, n_items, unit0, n_units, group0, n_groups;
};

// Host side and device buffers of the pass: everything that can fail for want of memory, done before the call's
// mode-1 kernels are queued, so that an error leaves both accumulators where they were.
static std::vector<FullLaunch> stats_full_prepare(aasr_stats *h, const std::vector<int64_t> &cnt) {
  h->h_fitems.clear();
  h->h_funits.clear();
  h->h_fgroups.clear();
  h->h_fentries.clear();
  const int64_t max_units = std::max<int64_t>(
      1, std::min<int64_t>(SCATTER_MAX_ITEMS, h->full_slab_bytes / (h->TS * (int64_t)sizeof(double))));
  typedef FullLaunch Launch;
  std::vector<Launch> launches;
  int64_t gam = 0, max_gam = 0, most_units = 0;
  for (int s = 0; s < h->S; s++) {
    const int M = h->mix_off[(size_t)s + 1] - h->mix_off[(size_t)s];
    if (M == 0) continue;  // (nothing to weigh the frames with)
    for (int64_t b = cnt[(size_t)s]; b < cnt[(size_t)s + 1]; b += SCATTER_ITEM) {
      const int32_t len = (int32_t)std::min<int64_t>(SCATTER_ITEM, cnt[(size_t)s + 1] - b);
      if (launches.empty() || launches.back().n_units + M > max_units) {
        launches.push_back(Launch{(int)h->h_fitems.size(), 0, (int)h->h_funits.size(), 0, 0, 0});
        gam = 0;
      }
      Launch &L = launches.back();
      for (int k = 0; k < M; k++) h->h_funits.push_back(FullUnit{(int32_t)h->h_fitems.size(), k});
      h->h_fitems.push_back(FullItem{(int32_t)b, len, s, 0, gam});
      gam += (int64_t)M * len;
      max_gam = std::max(max_gam, gam);
      L.n_items++;
      L.n_units += M;
      most_units = std::max<int64_t>(most_units, L.n_units);
    }
  }
  h->full_shape[0] = scatter_pb(h->D);
  h->full_shape[1] = (int32_t)h->h_fitems.size();
  h->full_shape[2] = (int32_t)launches.size();
  h->full_shape[3] = (int32_t)h->h_funits.size();
  if (launches.empty()) return launches;
  // per launch: its units sorted by pool Gaussian, unit order kept within a Gaussian
  std::vector<std::pair<int32_t, int32_t>> order;
  for (Launch &L : launches) {
    order.clear();
    for (int u = 0; u < L.n_units; u++) {
      const FullUnit &fu = h->h_funits[(size_t)(L.unit0 + u)];
      order.emplace_back(h->mix_idx[(size_t)(h->mix_off[(size_t)h->h_fitems[(size_t)fu.item].pdf] + fu.comp)], u);
    }
    std::sort(order.begin(), order.end());  // (pairs: by Gaussian, then by unit)
    L.group0 = (int)h->h_fgroups.size();
    for (const auto &o : order) {
      if (L.n_groups > 0 && h->h_fgroups.back().g == o.first) h->h_fgroups.back().count++;
      else {
        h->h_fgroups.push_back(FullGroup{o.first, (int32_t)h->h_fentries.size(), 1, 0});
        L.n_groups++;
      }
      h->h_fentries.push_back(o.second);
    }
  }
  h->d_fitems.ensure(h->h_fitems.size());
  h->d_funits.ensure(h->h_funits.size());
  h->d_fgroups.ensure(h->h_fgroups.size());
  h->d_fentries.ensure(h->h_fentries.size());
  h->fslab.ensure((size_t)most_units * h->TS);
  h->fgam.ensure((size_t)max_gam);
  return launches;
}

// the uploads and the launches of a prepared pass, after the mode-1 kernels on the same stream
static void stats_full_pass(aasr_stats *h, const double *d_frames, const std::vector<FullLaunch> &launches, hipStream_t st) {
  if (launches.empty()) return;
  AASR_HIP(hipMemcpyAsync(h->d_fitems.p, h->h_fitems.data(), h->h_fitems.size() * sizeof(FullItem), hipMemcpyHostToDevice, st));
  AASR_HIP(hipMemcpyAsync(h->d_funits.p, h->h_funits.data(), h->h_funits.size() * sizeof(FullUnit), hipMemcpyHostToDevice, st));
  AASR_HIP(hipMemcpyAsync(h->d_fgroups.p, h->h_fgroups.data(), h->h_fgroups.size() * sizeof(FullGroup), hipMemcpyHostToDevice, st));
  AASR_HIP(hipMemcpyAsync(h->d_fentries.p, h->h_fentries.data(), h->h_fentries.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  AASR_HIP(hipEventRecord(h->staged, st));  // (now after these uploads as well)
  FullParams p{};
  p.x = d_frames;
  p.dim = h->D;
  p.rows = h->d_rows.p;
  p.items = h->d_fitems.p;
  p.units = h->d_funits.p;
  p.recs = h->gmm->f64_recs.p;
  p.rec = h->rec;
  p.state_off = h->gmm->f64_state_off.p;
  p.gam = h->fgam.p;
  p.slab = h->fslab.p;
  for (const FullLaunch &L : launches)  // (the launches of a call follow each other on the stream and share the buffers)
    stats_full_launch(p, L.item0, L.n_items, L.unit0, L.n_units, h->d_fgroups.p + L.group0, L.n_groups, h->d_fentries.p,
                      h->facc.p, st);
}

}  // namespace aasr

extern "C" {

static aasr_status stats_create(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out, bool full) {
  return guarded([&] {
    if (!gmm || !topo || !out) raise(AASR_ERR_INVALID, "%s: null argument", full ? "aasr_stats_create_full" : "aasr_stats_create");
    *out = nullptr;
    check_stats_model(gmm);
    if (full && gmm->host.dim > SCATTER_MAX_DIM)  // (before the device is asked for anything)
      raise(AASR_ERR_UNSUPPORTED, "stats: full statistics are collected for at most %d dimensions, the model has %d",
            SCATTER_MAX_DIM, gmm->host.dim);
    {
      const aasr_status st = aasr_topo_validate(topo, gmm);
      if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    }
    require_device();
    std::unique_ptr<aasr_stats> h(new aasr_stats());
    const HostModel &m = gmm->host;
    h->gmm = gmm;
    h->D = m.dim;
    h->S = (int)m.S;
    h->G = (int)m.G;
    h->K = (int)m.mix_idx.size();
    h->W = 2 + 2 * h->D;
    h->mix_off = m.mix_off;
    h->mix_idx = m.mix_idx;
    for (int s = 0; s < h->S; s++) h->max_comps = std::max(h->max_comps, m.mix_off[(size_t)s + 1] - m.mix_off[(size_t)s]);
    gmm_build_f64(gmm);
    h->dimp = gmm->f64_dimp ? gmm->f64_dimp : 0;
    h->rec = 2 * h->dimp + 2;
    {  // a model no launch shape holds is refused here, where it is known, not at its first frames
      int32_t block, lds_recs;
      stats_launch_shape(h->max_comps, h->rec, &block, &lds_recs);
    }
    // transitions in HmmSet::read_ph order
    TopoTables tt(topo);
    for (size_t s = 0; s < tt.offsets.size(); s++)
      for (int32_t o : tt.offsets[s]) {
        h->tr_source.push_back((int32_t)s);
        h->tr_offset.push_back(o);
      }
    h->tr_count.assign(h->tr_source.size(), 0.0);
    h->racc.alloc((size_t)std::max(1, h->K) * h->W);
    h->pacc.alloc((size_t)std::max(1, h->S) * 2);
    h->gacc.alloc((size_t)std::max(1, h->G) * (h->W + 1));
    AASR_HIP(hipMemset(h->racc.p, 0, h->racc.n * sizeof(double)));
    AASR_HIP(hipMemset(h->pacc.p, 0, h->pacc.n * sizeof(double)));
    // pool Gaussian -> its records, in record order
    std::vector<int32_t> goff((size_t)h->G + 1, 0), grec((size_t)std::max(1, h->K)), rpdf((size_t)std::max(1, h->K));
    for (int k = 0; k < h->K; k++) goff[(size_t)m.mix_idx[(size_t)k] + 1]++;
    for (int g = 0; g < h->G; g++) goff[(size_t)g + 1] += goff[(size_t)g];
    std::vector<int32_t> fill(goff.begin(), goff.end() - 1);
    for (int s = 0; s < h->S; s++)
      for (int k = m.mix_off[(size_t)s]; k < m.mix_off[(size_t)s + 1]; k++) {
        grec[(size_t)fill[(size_t)m.mix_idx[(size_t)k]]++] = k;
        rpdf[(size_t)k] = s;
      }
    h->g_off.upload(goff.data(), goff.size());
    h->g_rec.upload(grec.data(), grec.size());
    h->rec_pdf.upload(rpdf.data(), rpdf.size());
    if (full) {
      h->full = true;
      h->TS = scatter_class_doubles(h->D);
      h->facc.alloc((size_t)std::max(1, h->G) * h->TS);
      AASR_HIP(hipMemset(h->facc.p, 0, h->facc.n * sizeof(double)));
    }
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

aasr_status aasr_stats_create(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out) {
  return stats_create(gmm, topo, out, false);
}

aasr_status aasr_stats_create_full(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out) {
  return stats_create(gmm, topo, out, true);
}

int32_t aasr_stats_mode(const aasr_stats *h) { return h ? (h->full ? 3 : 1) : -1; }

void aasr_stats_destroy(aasr_stats *h) { delete h; }

int32_t aasr_stats_num_transitions(const aasr_stats *h) { return h ? (int32_t)h->tr_source.size() : -1; }

// Diagnostic: the shape of the item kernel's launch in the last aasr_stats_accumulate_dev call that launched one --
// out[0] the dimension instance (dimp), out[1] frames per sub-block, out[2] 1 when the records were staged in LDS,
// out[3] the largest mixture, out[4] the number of work items; zeros before the first launch
void aasr_debug_stats_shape(const aasr_stats *h, int32_t *out) {
  if (!h || !out) return;
  std::copy(h->last_shape, h->last_shape + 5, out);
}

aasr_status aasr_stats_accumulate_dev(aasr_stats *h, const double *d_frames, int64_t n_frames, const int32_t *pdf,
                                      double *d_frame_ll, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || (n_frames > 0 && (!d_frames || !pdf)))
      raise(AASR_ERR_INVALID, "aasr_stats_accumulate_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_dev: more than 2^31 frames in one call");
    if (n_frames == 0) return;
    const hipStream_t st = (hipStream_t)stream;
    // the host tables of the previous call may still be on their way to the device
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    // frames grouped by pdf (frame order within a pdf), cut into items of at most STATS_CHUNK frames
    std::vector<int64_t> cnt;
    rows_by_pdf("aasr_stats_accumulate_dev", h->S, pdf, n_frames, &cnt, &h->h_rows);
    const int64_t slab_total = stats_build_items(h, cnt);
    if (h->h_items.empty()) return;
    std::vector<FullLaunch> full_launches;
    if (h->full) full_launches = stats_full_prepare(h, cnt);
    StatsParams p{};
    p.max_comps = h->max_comps;
    p.rec = h->rec;
    stats_launch_shape(p.max_comps, p.rec, &p.block, &p.lds_recs);
    h->d_rows.ensure(h->h_rows.size());
    h->d_items.ensure(h->h_items.size());
    h->d_pdfs.ensure(h->h_pdfs.size());
    h->d_item_begin.ensure(h->h_item_begin.size());
    h->slab.ensure((size_t)slab_total);
    AASR_HIP(hipMemcpyAsync(h->d_rows.p, h->h_rows.data(), h->h_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(StatsItem),
                            hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_pdfs.p, h->h_pdfs.data(), h->h_pdfs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_item_begin.p, h->h_item_begin.data(), h->h_item_begin.size() * sizeof(int32_t),
                            hipMemcpyHostToDevice, st));
    AASR_HIP(hipEventRecord(h->staged, st));
    h->staged_pending = true;
    p.x = d_frames;
    p.dim = h->D;
    p.rows = h->d_rows.p;
    p.items = h->d_items.p;
    p.recs = h->gmm->f64_recs.p;
    p.state_off = h->gmm->f64_state_off.p;
    p.slab = h->slab.p;
    p.frame_ll = d_frame_ll;
    const int32_t shape[5] = {h->dimp, p.block, p.lds_recs, p.max_comps, (int32_t)h->h_items.size()};
    std::copy(shape, shape + 5, h->last_shape);
    stats_items_launch(p, h->dimp, (int)h->h_items.size(), st);
    stats_pdf_reduce_launch(h->d_pdfs.p, h->d_item_begin.p, (int)h->h_pdfs.size(), h->d_items.p, h->slab.p,
                            h->gmm->f64_state_off.p, h->D, h->racc.p, h->pacc.p, st);
    if (h->full) stats_full_pass(h, d_frames, full_launches, st);
    h->fetched = false;
  });
}

aasr_status aasr_stats_accumulate_weighted_dev(aasr_stats *h, const double *d_frames, int64_t n_frames, const int64_t *cnt,
                                               const int32_t *d_rows, const double *d_weights, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || !cnt) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: bad argument");
    if (h->full)  // (before anything is queued)
      raise(AASR_ERR_UNSUPPORTED, "aasr_stats_accumulate_weighted_dev: full second moments are not collected from weighted "
                                  "entries (a handle of aasr_stats_create_full)");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: more than 2^31 frames in one call");
    if (cnt[0] != 0) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: cnt[0] is %lld, not 0", (long long)cnt[0]);
    for (int s = 0; s < h->S; s++)
      if (cnt[s + 1] < cnt[s]) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: cnt decreases at pdf %d", s);
    const int64_t entries = cnt[h->S];
    if (entries > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: more than 2^31 entries in one call");
    if (entries == 0) return;
    if (!d_frames || !d_rows || !d_weights || n_frames == 0)
      raise(AASR_ERR_INVALID, "aasr_stats_accumulate_weighted_dev: %lld entries without frames, rows or weights", (long long)entries);
    const hipStream_t st = (hipStream_t)stream;
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    const int64_t slab_total = stats_build_items(h, std::vector<int64_t>(cnt, cnt + h->S + 1));
    if (h->h_items.empty()) return;
    StatsParams p{};
    p.max_comps = h->max_comps;
    p.rec = h->rec;
    stats_launch_shape(p.max_comps, p.rec, &p.block, &p.lds_recs);
    h->d_items.ensure(h->h_items.size());
    h->d_pdfs.ensure(h->h_pdfs.size());
    h->d_item_begin.ensure(h->h_item_begin.size());
    h->slab.ensure((size_t)slab_total);
    AASR_HIP(hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(StatsItem), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_pdfs.p, h->h_pdfs.data(), h->h_pdfs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_item_begin.p, h->h_item_begin.data(), h->h_item_begin.size() * sizeof(int32_t),
                            hipMemcpyHostToDevice, st));
    AASR_HIP(hipEventRecord(h->staged, st));
    h->staged_pending = true;
    p.x = d_frames;
    p.dim = h->D;
    p.rows = d_rows;
    p.items = h->d_items.p;
    p.recs = h->gmm->f64_recs.p;
    p.state_off = h->gmm->f64_state_off.p;
    p.slab = h->slab.p;
    p.frame_ll = nullptr;
    const int32_t shape[5] = {h->dimp, p.block, p.lds_recs, p.max_comps, (int32_t)h->h_items.size()};
    std::copy(shape, shape + 5, h->last_shape);
    stats_items_w_launch(p, d_weights, n_frames, h->dimp, (int)h->h_items.size(), st);
    stats_pdf_reduce_launch(h->d_pdfs.p, h->d_item_begin.p, (int)h->h_pdfs.size(), h->d_items.p, h->slab.p,
                            h->gmm->f64_state_off.p, h->D, h->racc.p, h->pacc.p, st);
    h->fetched = false;
  });
}

aasr_status aasr_stats_add_transitions(aasr_stats *h, const int32_t *transition, int64_t n) {
  return guarded([&] {
    if (!h || n < 0 || (n > 0 && !transition)) raise(AASR_ERR_INVALID, "aasr_stats_add_transitions: bad argument");
    for (int64_t i = 0; i < n; i++) {
      const int32_t t = transition[i];
      if (t < 0) continue;
      if (t >= (int32_t)h->tr_count.size()) raise(AASR_ERR_INVALID, "aasr_stats_add_transitions: index %d out of range", t);
      h->tr_count[(size_t)t] += 1.0;
    }
  });
}

aasr_status aasr_stats_fetch(aasr_stats *h, void *stream) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_stats_fetch: null argument");
    const hipStream_t st = (hipStream_t)stream;
    stats_gauss_reduce_launch(h->racc.p, h->pacc.p, h->g_off.p, h->g_rec.p, h->rec_pdf.p, h->G, h->D, h->gacc.p, st);
    h->h_racc.resize(h->racc.n);
    h->h_pacc.resize(h->pacc.n);
    h->h_gacc.resize(h->gacc.n);
    AASR_HIP(hipMemcpyAsync(h->h_racc.data(), h->racc.p, h->racc.n * sizeof(double), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(h->h_pacc.data(), h->pacc.p, h->pacc.n * sizeof(double), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(h->h_gacc.data(), h->gacc.p, h->gacc.n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (h->full) {
      h->h_full.resize((size_t)std::max(1, h->G) * h->D * (h->D + 1) / 2);
      h->fpacked.ensure(h->h_full.size());
      stats_full_pack_launch(h->facc.p, h->G, h->D, h->fpacked.p, st);
      if (h->G > 0)
        AASR_HIP(hipMemcpyAsync(h->h_full.data(), h->fpacked.p, h->h_full.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    AASR_HIP(hipStreamSynchronize(st));
    h->staged_pending = false;
    h->fetched = true;
  });
}

static void require_fetched(const aasr_stats *h, const char *what) {
  if (!h) raise(AASR_ERR_INVALID, "%s: null argument", what);
  if (!h->fetched) raise(AASR_ERR_INVALID, "%s: call aasr_stats_fetch after the last accumulation", what);
}

aasr_status aasr_stats_gaussians(const aasr_stats *h, int64_t *feacount, double *gamma, double *aux_gamma,
                                 double *sum_x, double *sum_xx) {
  return guarded([&] {
    require_fetched(h, "aasr_stats_gaussians");
    const int D = h->D, W1 = h->W + 1;
    for (int g = 0; g < h->G; g++) {
      const double *a = &h->h_gacc[(size_t)g * W1];
      if (feacount) feacount[g] = (int64_t)a[0];
      if (gamma) gamma[g] = a[1];
      if (aux_gamma) aux_gamma[g] = a[2];
      for (int d = 0; d < D; d++) {
        if (sum_x) sum_x[(size_t)g * D + d] = a[3 + d];
        if (sum_xx) sum_xx[(size_t)g * D + d] = a[3 + D + d];
      }
    }
  });
}

aasr_status aasr_stats_full_moments(const aasr_stats *h, double *sum_xx) {
  return guarded([&] {
    require_fetched(h, "aasr_stats_full_moments");
    if (!h->full) raise(AASR_ERR_INVALID, "aasr_stats_full_moments: the handle collects no full statistics (aasr_stats_create_full)");
    if (!sum_xx) raise(AASR_ERR_INVALID, "aasr_stats_full_moments: null argument");
    std::copy(h->h_full.begin(), h->h_full.begin() + (size_t)h->G * h->D * (h->D + 1) / 2, sum_xx);
  });
}

void aasr_debug_stats_full_shape(const aasr_stats *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 4; i++) out[i] = h ? h->full_shape[i] : 0;
}

aasr_status aasr_debug_stats_set_slab_bytes(aasr_stats *h, int64_t bytes) {
  return guarded([&] {
    if (!h || bytes < 1) raise(AASR_ERR_INVALID, "aasr_debug_stats_set_slab_bytes: bad argument");
    if (!h->full) raise(AASR_ERR_INVALID, "aasr_debug_stats_set_slab_bytes: the handle collects no full statistics");
    h->full_slab_bytes = bytes;
  });
}

aasr_status aasr_stats_mixtures(const aasr_stats *h, int64_t *count, double *gamma, double *mixture_ll) {
  return guarded([&] {
    require_fetched(h, "aasr_stats_mixtures");
    for (int s = 0; s < h->S; s++) {
      if (count) count[s] = (int64_t)h->h_pacc[2 * (size_t)s];
      if (mixture_ll) mixture_ll[s] = h->h_pacc[2 * (size_t)s + 1];
    }
    if (gamma)
      for (int k = 0; k < h->K; k++) gamma[k] = h->h_racc[(size_t)k * h->W];
  });
}

aasr_status aasr_stats_transitions(const aasr_stats *h, int32_t *source, int32_t *target_offset, double *count) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_stats_transitions: null argument");
    for (size_t t = 0; t < h->tr_source.size(); t++) {
      if (source) source[t] = h->tr_source[t];
      if (target_offset) target_offset[t] = h->tr_offset[t];
      if (count) count[t] = h->tr_count[t];
    }
  });
}

// ---- dump writers (HmmSet::dump_statistics, HmmSet.cc:546-625) --------------------------------

aasr_status aasr_stats_write_gks(const char *path, int32_t pool_size, int32_t dim, int32_t mode, const int64_t *feacount,
                                 const double *gamma, const double *aux_gamma, const double *sum_x, const double *sum_xx) {
  return guarded([&] {
    if (!path || pool_size < 0 || dim < 0 || (pool_size > 0 && (!feacount || !gamma || !aux_gamma || !sum_x || !sum_xx)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_gks: bad argument");
    std::ofstream gks(path, std::ofstream::binary);
    if (!gks) raise(AASR_ERR_IO, "HmmSet::dump_gk_statistics(): could not open %s", path);
    gks.write((const char *)&pool_size, sizeof(int));
    gks.write((const char *)&dim, sizeof(int));
    gks.write((const char *)&mode, sizeof(int));
    const int zero = 0, end = -1;
    for (int g = 0; gks && g < pool_size; g++) {
      gks.write((const char *)&g, sizeof(int));
      if (feacount[g] > 0) {  // Gaussian::dump_statistics: the ML buffer, when it was accumulated
        gks.write((const char *)&zero, sizeof(int));
        const int fc = (int)feacount[g];
        gks.write((const char *)&fc, sizeof(int));
        gks.write((const char *)&gamma[g], sizeof(double));
        gks.write((const char *)&aux_gamma[g], sizeof(double));
        for (int d = 0; d < dim; d++) {
          const float t = (float)sum_x[(size_t)g * dim + d];
          gks.write((const char *)&t, sizeof(float));
        }
        for (int d = 0; d < dim; d++) {
          const float t = (float)sum_xx[(size_t)g * dim + d];
          gks.write((const char *)&t, sizeof(float));
        }
      }
      gks.write((const char *)&end, sizeof(int));
    }
    if (!gks) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

// FullStatisticsAccumulator::dump_statistics (Distributions.cc:42-60) under HmmSet::dump_gk_statistics
aasr_status aasr_stats_write_gks_full(const char *path, int32_t pool_size, int32_t dim, const int64_t *feacount,
                                      const double *gamma, const double *aux_gamma, const double *sum_x,
                                      const double *sum_xx_packed) {
  return guarded([&] {
    if (!path || pool_size < 0 || dim < 0 || (pool_size > 0 && (!feacount || !gamma || !aux_gamma || !sum_x || !sum_xx_packed)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_gks_full: bad argument");
    std::ofstream gks(path, std::ofstream::binary);
    if (!gks) raise(AASR_ERR_IO, "HmmSet::dump_gk_statistics(): could not open %s", path);
    const int mode = 3;  // PDF_ML_STATS | PDF_ML_FULL_STATS
    gks.write((const char *)&pool_size, sizeof(int));
    gks.write((const char *)&dim, sizeof(int));
    gks.write((const char *)&mode, sizeof(int));
    const int zero = 0, end = -1;
    const size_t tri = (size_t)dim * (dim + 1) / 2;
    std::vector<float> t((size_t)dim + tri);
    for (int g = 0; gks && g < pool_size; g++) {
      gks.write((const char *)&g, sizeof(int));
      if (feacount[g] > 0) {
        gks.write((const char *)&zero, sizeof(int));
        const int fc = (int)feacount[g];
        gks.write((const char *)&fc, sizeof(int));
        gks.write((const char *)&gamma[g], sizeof(double));
        gks.write((const char *)&aux_gamma[g], sizeof(double));
        for (int d = 0; d < dim; d++) t[(size_t)d] = (float)sum_x[(size_t)g * dim + d];
        for (size_t e = 0; e < tri; e++) t[(size_t)dim + e] = (float)sum_xx_packed[(size_t)g * tri + e];  // row by row, j <= i
        gks.write((const char *)t.data(), (std::streamsize)(t.size() * sizeof(float)));
      }
      gks.write((const char *)&end, sizeof(int));
    }
    if (!gks) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_mcs(const char *path, int32_t num_pdfs, int32_t mode, const int32_t *mix_off,
                                 const int32_t *mix_idx, const int64_t *count, const double *gamma,
                                 const double *aux_gamma, const double *mixture_ll) {
  return guarded([&] {
    if (!path || num_pdfs < 0 || (num_pdfs > 0 && (!mix_off || !mix_idx || !count || !gamma || !mixture_ll)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_mcs: bad argument");
    std::ofstream mcs(path);
    if (!mcs) raise(AASR_ERR_IO, "HmmSet::dump_mc_statistics(): could not open %s", path);
    mcs << num_pdfs << std::endl;
    mcs << mode << std::endl;
    for (int i = 0; i < num_pdfs; i++) {
      mcs << i << std::endl;
      // Mixture::dump_statistics (Distributions.cc:2192-2208)
      mcs.precision(10);
      if (count[i] > 0) {
        const int n = mix_off[i + 1] - mix_off[i];
        mcs << 0 << " " << n;
        for (int k = 0; k < n; k++) mcs << " " << mix_idx[mix_off[i] + k] << " " << gamma[mix_off[i] + k];
        mcs << " " << (aux_gamma ? aux_gamma[i] : 0.0) << " " << mixture_ll[i];
        mcs << std::endl;
      }
      mcs << "-1" << std::endl;
    }
    if (!mcs) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_phs(const char *path, int32_t num_transitions, const int32_t *source,
                                 const int32_t *target_offset, const double *count) {
  return guarded([&] {
    if (!path || num_transitions < 0 || (num_transitions > 0 && (!source || !target_offset || !count)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_phs: bad argument");
    if (num_transitions == 0) return;  // dump_ph_statistics writes nothing without transitions
    std::ofstream phs(path);
    if (!phs) raise(AASR_ERR_IO, "HmmSet::dump_ph_statistics(): could not open %s", path);
    phs << num_transitions << std::endl;
    for (int t = 0; t < num_transitions; t++)
      if (count[t] > 0) {
        phs << source[t] << " ";
        phs << target_offset[t] << " ";
        phs << count[t] << std::endl;
      }
    if (!phs) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_lls(const char *path, double loglik, int64_t frames) {
  return guarded([&] {
    if (!path) raise(AASR_ERR_INVALID, "aasr_stats_write_lls: null argument");
    std::ofstream lls(path);
    if (!lls) return;  // stats.cc:779: no file, no message
    lls.precision(12);
    lls << "Numerator loglikelihood: " << loglik << std::endl;
    lls << "Number of frames: " << frames << std::endl;
  });
}

aasr_status aasr_stats_write(const aasr_stats *h, const char *base) {
  return guarded([&] {
    require_fetched(h, "aasr_stats_write");
    if (!base) raise(AASR_ERR_INVALID, "aasr_stats_write: null argument");
    const std::string b(base);
    auto ok = [](aasr_status s) {
      if (s != AASR_OK) raise(s, "%s", last_error().c_str());
    };
    ok(aasr_stats_write_phs((b + ".phs").c_str(), (int32_t)h->tr_source.size(), h->tr_source.data(), h->tr_offset.data(),
                            h->tr_count.data()));
    std::vector<int64_t> count((size_t)std::max(1, h->S));
    std::vector<double> gamma((size_t)std::max(1, h->K)), mll((size_t)std::max(1, h->S)), aux((size_t)std::max(1, h->S), 0.0);
    ok(aasr_stats_mixtures(h, count.data(), gamma.data(), mll.data()));
    ok(aasr_stats_write_mcs((b + ".mcs").c_str(), h->S, h->full ? 3 : 1, h->mix_off.data(), h->mix_idx.data(), count.data(),
                            gamma.data(), aux.data(), mll.data()));
    const size_t G1 = (size_t)std::max(1, h->G);
    std::vector<int64_t> fc(G1);
    std::vector<double> gg(G1), ga(G1), sx(G1 * h->D + 1), sxx(G1 * h->D + 1);
    ok(aasr_stats_gaussians(h, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
    if (h->full)
      ok(aasr_stats_write_gks_full((b + ".gks").c_str(), h->G, h->D, fc.data(), gg.data(), ga.data(), sx.data(), h->h_full.data()));
    else
      ok(aasr_stats_write_gks((b + ".gks").c_str(), h->G, h->D, 1, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
  });
}

// ---- host-only segmentation reader ---------------------------------------------------------------

static aasr_status read_segmentation_call(const char *what, const aasr_topo *topo, const char *path, float frame_rate,
                                          int32_t first_frame, int32_t last_frame, int32_t eof_frame, int32_t flags,
                                          int32_t transitions, int32_t *start_frame, int32_t **pdf, int32_t **transition,
                                          int32_t *n_frames) {
  return guarded([&] {
    if (!topo || !path || !start_frame || !pdf || !transition || !n_frames) raise(AASR_ERR_INVALID, "%s: null argument", what);
    *pdf = nullptr;
    *transition = nullptr;
    if (flags & ~(AASR_PHN_STATE_NUM_LABELS | AASR_PHN_RELATIVE_SAMPLES)) raise(AASR_ERR_INVALID, "%s: unknown flags %d", what, flags);
    TopoTables tt(topo);
    Segmentation seg = read_segmentation(topo, tt, path, frame_rate, first_frame, last_frame, eof_frame, transitions != 0, flags);
    const size_t n = seg.pdf.size();
    *pdf = (int32_t *)malloc(std::max<size_t>(1, n) * sizeof(int32_t));
    *transition = (int32_t *)malloc(std::max<size_t>(1, n) * sizeof(int32_t));
    if (!*pdf || !*transition) {
      free(*pdf);
      free(*transition);
      *pdf = *transition = nullptr;
      raise(AASR_ERR_INVALID, "out of memory");
    }
    std::copy(seg.pdf.begin(), seg.pdf.end(), *pdf);
    std::fill(*transition, *transition + n, -1);  // (what the reader leaves out when no transitions are asked for)
    std::copy(seg.tr.begin(), seg.tr.end(), *transition);
    *start_frame = seg.start_frame;
    *n_frames = seg.initialized ? (int32_t)n : -1;
  });
}

aasr_status aasr_stats_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate, int32_t first_frame,
                                         int32_t last_frame, int32_t eof_frame, int32_t transitions,
                                         int32_t *start_frame, int32_t **pdf, int32_t **transition, int32_t *n_frames) {
  return read_segmentation_call("aasr_stats_read_segmentation", topo, path, frame_rate, first_frame, last_frame, eof_frame, 0,
                                transitions, start_frame, pdf, transition, n_frames);
}

aasr_status aasr_phn_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate, int32_t first_frame,
                                       int32_t last_frame, int32_t eof_frame, int32_t flags, int32_t transitions,
                                       int32_t *start_frame, int32_t **pdf, int32_t **transition, int32_t *n_frames) {
  return read_segmentation_call("aasr_phn_read_segmentation", topo, path, frame_rate, first_frame, last_frame, eof_frame,
                                flags, transitions, start_frame, pdf, transition, n_frames);
}

void aasr_stats_default_options(aasr_stats_options *o) {
  if (o) memset(o, 0, sizeof *o);
}

}  // extern "C"

// ---- the stats main loop over a recipe ---------------------------------------------------------

// ---- Baum-Welch over the recipe's HMM networks (aku/stats.cc with -H) ----------------------------

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// HmmNetBaumWelch::next_frame's label of an emitting arc (:763-768): the arc's label without its '#' end marks
// (LatticeLabel::remove_end_marks) -- the transition index, then the ";..." part the reader kept -- and, where that
// splits at ';' into three or more fields (mixture;state;phone;...), "phone.state"
std::string alignment_label(const aasr_hmmnet &net, int32_t arc) {
  std::string label = std::to_string(net.em_tr[(size_t)arc]);
  for (char c : net.em_label[(size_t)arc])
    if (c != '#') label += c;
  std::vector<std::string> fields;
  size_t at = 0;
  for (;;) {
    const size_t stop = label.find(';', at);
    fields.push_back(label.substr(at, stop == std::string::npos ? std::string::npos : stop - at));
    if (stop == std::string::npos) break;
    at = stop + 1;
  }
  return fields.size() >= 3 ? fields[2] + "." + fields[1] : label;
}

// The alignment file of one utterance as simple_train writes it (aku/stats.cc:116-131, 179-188): runs of one label text,
// "start end label" in samples; the last line ends one frame past the range (the reference's own "+1": next_frame has
// stepped once more before it returned false).  cache: the network's labels, filled as they are asked for.
std::string alignment_text(const aasr_hmmnet &net, std::vector<std::string> &cache, const std::vector<int32_t> &path, int first_frame,
                           int frame_mult) {
  cache.resize(net.em_src.size());
  std::string text;
  char head[64];
  int cur_start = -1;
  const std::string *cur = nullptr;
  auto put = [&](int end) {
    snprintf(head, sizeof head, "%d %d ", cur_start * frame_mult, end * frame_mult);
    text += head;
    text += *cur;
    text += '\n';
  };
  for (size_t t = 0; t < path.size(); t++) {
    std::string &label = cache[(size_t)path[t]];
    if (label.empty()) label = alignment_label(net, path[t]);
    const int frame = first_frame + (int)t;
    if (cur_start < 0) {
      cur_start = frame;
      cur = &label;
    } else if (*cur != label) {
      put(frame);
      cur_start = frame;
      cur = &label;
    }
  }
  if (cur_start >= 0) put(first_frame + (int)path.size() + 1);
  return text;
}

// The network mode of aasr_run_stats_recipe: per group the steps of logl.cc's network branch, then the occupancies as
// weighted entries into the accumulation.  -> total_ll, num_frames of the utterances that ran
void run_stats_networks(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const std::vector<RecipeInfo> &infos,
                        const aasr_stats_options *opt, const aasr_stats_network_options *nopt, aasr_stats *h,
                        GroupStager &stager, double *total_ll, int64_t *num_frames) {
  const hipStream_t stream = stager.stream;
  const bool accumulate = !opt->no_train, transitions = opt->transitions != 0;
  const bool timing = getenv("AASR_RECIPE_TIMING") != nullptr;
  double t_host = 0, t_feat = 0, t_score = 0, t_fb = 0, t_acc = 0;
  aasr_fb_options fo;
  aasr_fb_default_options(&fo);
  if (nopt->fw_beam > 0) fo.fw_beam = nopt->fw_beam;  // set_pruning_thresholds: 0 keeps the default
  if (nopt->bw_beam > 0) fo.bw_beam = nopt->bw_beam;
  if (nopt->ac_scale_given) fo.ac_scale = nopt->ac_scale;
  fo.mode = nopt->viterbi ? AASR_FB_VITERBI : AASR_FB_BAUM_WELCH;
  fo.want_pdf_occ = 1;
  fo.device_occ = 1;
  fo.want_tr_occ = transitions ? 1 : 0;
  fo.want_path = nopt->alignment ? 1 : 0;
  std::map<const aasr_hmmnet *, std::vector<std::string>> labels;  // per network, per emitting arc ("" until asked for)
  std::vector<int32_t> path;
  const int frame_mult = (int)(16000 / aasr_feat_frame_rate(feat));  // print_alignment_line (aku/stats.cc:59-70)
  const int S = aasr_gmm_num_states(gmm);
  const bool f64 = aasr_gmm_get_precision(gmm) == AASR_PREC_F64;
  const float fr = aasr_feat_frame_rate(feat);
  constexpr int64_t group_frames = (int64_t)1 << 18, group_scores = (int64_t)1 << 27;  // as logl.cc cuts its groups
  NetworkCache net_cache(topo, S);
  GroupScores scores;
  std::vector<int64_t> cnt((size_t)S + 1);
  std::vector<double> sums, tr_occ;
  double max_dev = 0;  // max |1 - s_t| over the run
  int64_t entries = 0;
  size_t next = 0;
  while (next < infos.size()) {
    double t = now_s();
    const size_t group_first = next;
    std::vector<std::vector<int16_t>> audio;
    std::vector<int32_t> start, rows;
    std::vector<const aasr_hmmnet *> group_nets;
    std::vector<char> align_open;  // with -a: the utterance's alignment file could be opened
    int64_t rows_total = 0;
    while (next < infos.size() && audio.size() < 1024 &&
           (audio.empty() || (rows_total < group_frames && rows_total * S < group_scores))) {
      const RecipeInfo &u = infos[next++];
      announce(u, opt->info);
      if (nopt->alignment) {  // aku/stats.cc:565-572: the file exists, empty, before the utterance is looked at
        FILE *af = fopen(u.alignment_path.c_str(), "w");
        if (!af) fprintf(stderr, "Could not open alignment file %s\n", u.alignment_path.c_str());
        else fclose(af);
        align_open.push_back(af != nullptr);
      }
      audio.push_back(load_utterance_input(feat, u));
      // Recipe::Info::init_hmmnet_files (Recipe.cc:198-231)
      if (u.hmmnet_path.empty()) raise(AASR_ERR_INVALID, "Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe.");
      group_nets.push_back(net_cache.get(u.hmmnet_path));
      int first, n;
      network_frame_range(u, fr, aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), &first, &n);
      start.push_back(first);
      rows.push_back(n);
      rows_total += n;
    }
    t_host += now_s() - t;
    t = now_s();
    stager.stage(audio, start, rows, [&](size_t i) {
      if (!opt->speakers) return;
      const RecipeInfo &u = infos[group_first + i];
      if (aasr_spkc_set_speaker(opt->speakers, u.speaker_id.c_str()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (opt->uttadap && !u.utterance_id.empty() && aasr_spkc_set_utterance(opt->speakers, u.utterance_id.c_str()) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      check_stats_model(gmm);
    });
    if (timing) AASR_HIP(hipStreamSynchronize(stream));
    t_feat += now_s() - t;
    t = now_s();
    const void *d_scores = scores.score(gmm, stager.d_x.p, rows_total, f64, stream);
    if (timing) AASR_HIP(hipStreamSynchronize(stream));
    t_score += now_s() - t;
    t = now_s();
    aasr_fb_batch *b = nullptr;
    if (aasr_fb_batch_create(&fo, (int32_t)group_nets.size(), group_nets.data(), rows.data(), &b) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    std::unique_ptr<aasr_fb_batch, void (*)(aasr_fb_batch *)> bguard(b, aasr_fb_batch_destroy);
    std::vector<int64_t> row0;
    int64_t at = 0;
    for (int32_t r : rows) {
      row0.push_back(at);
      at += r;
    }
    // simple_train (aku/stats.cc:79-102): a failed initialisation is run again with 2x ... 5x the backward beam -- new
    // launches over the failed utterances only
    int32_t failed = 0;
    for (int attempt = 1; attempt <= fo.max_attempts; attempt++) {
      if (aasr_fb_batch_dev(b, d_scores, S, rows_total, f64 ? 1 : 0, row0.data(), attempt, stream) != AASR_OK ||
          aasr_fb_batch_sync(b, stream, &failed) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (failed == 0) break;
    }
    const int32_t *d_rows = nullptr;
    const double *d_weights = nullptr;
    if (aasr_fb_batch_entries_dev(b, S, row0.data(), stream, cnt.data(), &d_rows, &d_weights) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    entries += cnt[(size_t)S];
    t_fb += now_s() - t;
    t = now_s();
    // the messages in recipe order, and the frame sums: HmmNetBaumWelch::next_frame's sanity check (:772-779)
    std::vector<char> ran(group_nets.size(), 0);
    for (size_t i = 0; i < group_nets.size(); i++) {
      int32_t status = 0, attempts = 0;
      if (aasr_fb_batch_result(b, (int32_t)i, &status, nullptr, nullptr, &attempts, nullptr, nullptr) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (attempts > 1 || status == FB_FAILED_BACKWARD) fprintf(stderr, "Could not initialize the utterance segmentation.\n");
      for (int k = 2; k <= attempts; k++) fprintf(stderr, "Increasing beam to %.1f\n", k * fo.bw_beam);
      if (status == FB_FAILED_BACKWARD) {
        fprintf(stderr, "Giving up for this file\n");
        continue;
      }
      if (status != FB_OK) raise(AASR_ERR_INVALID, "No paths survived to the end of the network!");
      ran[i] = 1;
      sums.resize((size_t)rows[i]);
      if (aasr_fb_batch_frame_sums(b, (int32_t)i, sums.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      for (int32_t f = 0; f < rows[i]; f++) {
        const double dev = std::fabs(1 - sums[(size_t)f]);
        if (dev > 0.02) {
          fprintf(stderr, "Warning: Sum of PDF probabilities is %g at frame %i\n", sums[(size_t)f], start[i] + f);
          if (sums[(size_t)f] < 0.01)  // (the reference exits here)
            raise(AASR_ERR_INVALID, "HmmNetBaumWelch: the sum of PDF probabilities is %g at frame %d of %s", sums[(size_t)f],
                  start[i] + f, infos[group_first + i].audio_path.c_str());
        }
        max_dev = std::max(max_dev, dev);
      }
      if (nopt->alignment && align_open[i]) {
        path.resize((size_t)rows[i]);
        if (aasr_fb_batch_path(b, (int32_t)i, path.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        const std::string text = alignment_text(*group_nets[i], labels[group_nets[i]], path, start[i], frame_mult);
        write_text_file(infos[group_first + i].alignment_path.c_str(), text.data(), text.size());
      }
    }
    if (accumulate && cnt[(size_t)S] > 0 &&
        aasr_stats_accumulate_weighted_dev(h, stager.d_x.p, rows_total, cnt.data(), d_rows, d_weights, stream) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    for (size_t i = 0; i < group_nets.size(); i++) {
      if (!ran[i]) continue;
      const aasr_hmmnet &net = *group_nets[i];
      double fw = 0;
      tr_occ.assign(std::max<size_t>(1, net.trs.size()), 0.0);
      if (aasr_fb_batch_result(b, (int32_t)i, nullptr, nullptr, &fw, nullptr, nullptr, transitions ? tr_occ.data() : nullptr) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (accumulate && transitions)
        for (size_t k = 0; k < net.trs.size(); k++) {
          if (net.trs[k] < 0 || (size_t)net.trs[k] >= h->tr_count.size())
            raise(AASR_ERR_INVALID, "%s: transition %d is not one of the model's %zu", infos[group_first + i].hmmnet_path.c_str(),
                  net.trs[k], h->tr_count.size());
          h->tr_count[(size_t)net.trs[k]] += tr_occ[k];
        }
      fprintf(stderr, "  %g\n", fw);  // simple_train: the segmentator's total log-likelihood
      *total_ll += fw;
      *num_frames += rows[i];
    }
    // the batch owns the entries that the accumulation reads: it goes when the stream is done with them
    AASR_HIP(hipStreamSynchronize(stream));
    t_acc += now_s() - t;
  }
  if (opt->info > 0) {
    fprintf(stderr, "Largest |1 - sum of PDF probabilities| of a frame: %g\n", max_dev);
    fprintf(stderr, "Weighted entries: %lld over %lld frames\n", (long long)entries, (long long)*num_frames);
  }
  if (timing)
    fprintf(stderr,
            "stats timing: input and networks %.3f s, features %.3f s, scoring %.3f s, forward-backward and entries %.3f s, "
            "accumulation %.3f s\n",
            t_host, t_feat, t_score, t_fb, t_acc);
}

}  // namespace

static aasr_status run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                    const aasr_stats_options *opt, const aasr_stats_network_options *nopt,
                                    aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || (!opt->no_train && !opt->out))
      raise(AASR_ERR_INVALID, "%s: null argument", nopt ? "aasr_run_stats_networks_recipe" : "aasr_run_stats_recipe");
    const auto t0 = std::chrono::steady_clock::now();
    check_feature_dim(gmm, feat);
    if (nopt && opt->full_stats)
      raise(AASR_ERR_UNSUPPORTED, "stats: --full-stats is not supported with --networks (full second moments are collected over .phn files only)");
    if (nopt && nopt->alignment && opt->ophn) raise(AASR_ERR_INVALID, "Can not read and write to output PHNs");  // aku/stats.cc:516-517
    if (nopt && nopt->alignment && !nopt->viterbi)
      raise(AASR_ERR_UNSUPPORTED, "stats: alignment output needs the Viterbi mode (-M vit): under Baum-Welch no single arc belongs to a frame");
    if (nopt && opt->ophn)
      raise(AASR_ERR_UNSUPPORTED, "stats: -O is not supported with --networks (a network line has no segmentation to choose)");
    // stats reads its recipe with cluster_speakers = false (aku/stats.cc:422-424)
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, false);
    refuse_line_limits(infos, "stats");
    aasr_stats *h = nullptr;
    {  // (a model the accumulation kernel has no shape for keeps its AASR_ERR_UNSUPPORTED)
      const aasr_status cs = opt->full_stats && !opt->no_train ? aasr_stats_create_full(gmm, topo, &h) : aasr_stats_create(gmm, topo, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_stats, void (*)(aasr_stats *)> hguard(h, aasr_stats_destroy);
    const TopoTables tt(topo);
    const float fr = aasr_feat_frame_rate(feat);
    const bool accumulate = !opt->no_train, transitions = opt->transitions != 0;
    GroupStager stager(feat, opt->speakers);
    const hipStream_t stream = stager.stream;
    DevBuf<double> d_ll;
    double total_ll = 0;
    int64_t num_frames = 0;
    // groups of utterances accumulated in one launch; their frames stay on the device
    const int64_t max_group_frames = (int64_t)1 << 20;
    size_t next = 0;
    if (nopt) {
      run_stats_networks(feat, gmm, topo, infos, opt, nopt, h, stager, &total_ll, &num_frames);
      next = infos.size();
    }
    while (next < infos.size()) {
      // host side first: audio and segmentation, the -i messages in recipe order
      const size_t group_first = next;
      std::vector<std::vector<int16_t>> audio;
      std::vector<Segmentation> segs;
      std::vector<int32_t> start, rows, pdfs;
      int64_t rows_total = 0;
      while (next < infos.size() && audio.size() < 1024 && rows_total < max_group_frames) {
        const RecipeInfo &u = infos[next++];
        announce(u, opt->info);
        audio.push_back(load_utterance_input(feat, u));
        int first, last;
        frame_range(u, fr, &first, &last);
        segs.push_back(read_segmentation(topo, tt, (opt->ophn ? u.alignment_path : u.transcript_path).c_str(), fr, first,
                                         last, aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), transitions));
        const Segmentation &seg = segs.back();
        if (!seg.initialized) {
          fprintf(stderr, "Could not initialize the utterance segmentation.\n");
          fprintf(stderr, "Giving up for this file\n");
          audio.back().clear();  // no frames; kept in the group for its speaker settings (stats.cc:560-565 run first)
        }
        start.push_back(seg.start_frame);
        rows.push_back((int32_t)seg.pdf.size());
        pdfs.insert(pdfs.end(), seg.pdf.begin(), seg.pdf.end());
        rows_total += (int64_t)seg.pdf.size();
      }
      d_ll.ensure((size_t)std::max<int64_t>(1, rows_total));
      // features of the group into one device buffer, speaker configuration per utterance
      stager.stage(audio, start, rows, [&](size_t i) {
        if (!opt->speakers) return;
        const RecipeInfo &u = infos[group_first + i];
        if (aasr_spkc_set_speaker(opt->speakers, u.speaker_id.c_str()) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        if (opt->uttadap && !u.utterance_id.empty() &&
            aasr_spkc_set_utterance(opt->speakers, u.utterance_id.c_str()) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        check_stats_model(gmm);
      });
      if (accumulate && transitions)
        for (const Segmentation &seg : segs)
          if (aasr_stats_add_transitions(h, seg.tr.data(), (int64_t)seg.tr.size()) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (rows_total == 0) continue;
      if (aasr_stats_accumulate_dev(h, stager.d_x.p, rows_total, pdfs.data(), d_ll.p, stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      // the .lls figure in frame order: state likelihoods, then the transition taken (stats.cc:130-160)
      std::vector<double> ll((size_t)rows_total);
      AASR_HIP(hipMemcpyAsync(ll.data(), d_ll.p, ll.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
      AASR_HIP(hipStreamSynchronize(stream));
      size_t row = 0;
      for (const Segmentation &seg : segs)
        for (size_t f = 0; f < seg.pdf.size(); f++) {
          total_ll += ll[row++];  // safe_log(1.0 * state_likelihood): the kernel's safe_log(total)
          if (!(transitions && accumulate) || seg.tr[f] < 0) continue;
          const int t = seg.tr[f], s = h->tr_source[(size_t)t];
          total_ll += safe_log(1.0 * tt.probs[(size_t)s][(size_t)(t - tt.tr_base[(size_t)s])]);
        }
      num_frames += rows_total;
    }
    if (opt->info > 0) {
      fprintf(stderr, "Finished collecting statistics (%i/%i)\n", opt->batch_index, opt->num_batches);
      fprintf(stderr, "Total num log likelihood: %g\n", total_ll);
    }
    const std::string out = opt->out ? opt->out : "";
    if (accumulate) {
      if (aasr_stats_fetch(h, stream) != AASR_OK || aasr_stats_write(h, out.c_str()) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    if (opt->out) {
      const aasr_status st = aasr_stats_write_lls((out + ".lls").c_str(), total_ll, num_frames);
      if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    }
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, 0);
  });
}

extern "C" {

aasr_status aasr_run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                  const aasr_stats_options *opt, aasr_run_stats *stats) {
  return run_stats_recipe(feat, gmm, topo, recipe_path, opt, nullptr, stats);
}

void aasr_stats_network_default_options(aasr_stats_network_options *o) {
  if (o) memset(o, 0, sizeof *o);
  if (o) o->ac_scale = 1;
}

aasr_status aasr_run_stats_networks_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                           const aasr_stats_options *opt, const aasr_stats_network_options *net,
                                           aasr_run_stats *stats) {
  aasr_stats_network_options defaults;
  aasr_stats_network_default_options(&defaults);
  return run_stats_recipe(feat, gmm, topo, recipe_path, opt, net ? net : &defaults, stats);
}

}  // extern "C"

// stats.cc -- ML statistics collection (aku/stats.cc with --ml): the statistics handle that drives the device
// accumulation (stats_accum.hip, stats_weighted.hip) -- create, accumulate, fetch and the getters.  The dump writers
// are in stats_files.cc, the stats main loop over a recipe in stats_recipe.cc.  A handle made by
// aasr_stats_create_full also collects the full second moments (stats_full_accum.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "recipe_pass.h"
#include "stats.h"
#include "stats_full.h"

using namespace aasr;

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

// The item and pdf passes of a call once stats_build_items has filled h_items, h_pdfs and h_item_begin (the caller has
// waited for the previous call's staging before): their uploads, the launch shape and its record, the item kernel over
// the device row list d_rows -- every entry with gamma 1, or with d_weights, where an entry may name a row outside
// 0 .. n_frames (stats.h) -- and the pdf reduce.
static void stats_items_step(aasr_stats *h, const double *d_frames, int64_t n_frames, int64_t slab_total, const int32_t *d_rows,
                             const double *d_weights, double *d_frame_ll, hipStream_t st) {
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
  p.frame_ll = d_frame_ll;
  const int32_t shape[5] = {h->dimp, p.block, p.lds_recs, p.max_comps, (int32_t)h->h_items.size()};
  std::copy(shape, shape + 5, h->last_shape);
  if (d_weights) stats_items_w_launch(p, d_weights, n_frames, h->dimp, (int)h->h_items.size(), st);
  else stats_items_launch(p, h->dimp, (int)h->h_items.size(), st);
  stats_pdf_reduce_launch(h->d_pdfs.p, h->d_item_begin.p, (int)h->h_pdfs.size(), h->d_items.p, h->slab.p,
                          h->gmm->f64_state_off.p, h->D, h->racc.p, h->pacc.p, st);
}

void require_fetched(const aasr_stats *h, const char *what) {
  if (!h) raise(AASR_ERR_INVALID, "%s: null argument", what);
  if (!h->fetched) raise(AASR_ERR_INVALID, "%s: call aasr_stats_fetch after the last accumulation", what);
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
    h->d_rows.ensure(h->h_rows.size());
    AASR_HIP(hipMemcpyAsync(h->d_rows.p, h->h_rows.data(), h->h_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    stats_items_step(h, d_frames, n_frames, slab_total, h->d_rows.p, nullptr, d_frame_ll, st);
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
    stats_items_step(h, d_frames, n_frames, slab_total, d_rows, d_weights, nullptr, st);
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
}  // extern "C"

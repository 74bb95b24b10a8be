// stats.cc -- ML statistics collection (aku/stats.cc with --ml over .phn segmentations): the
// segmentation reader (PhnReader::next_frame as stats configures it), the statistics handle that
// drives the device accumulation (stats_accum.hip), the dump writers of HmmSet::dump_statistics and
// the stats main loop over a recipe (aasr_run_stats_recipe, stats.cc:73-170, 540-620, 740-795).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "phn_line.h"
#include "pipeline.h"
#include "stats.h"

using namespace aasr;

namespace aasr {

static double safe_log(double x) { return x < 1e-50 ? std::log(1e-50) : std::log(x); }

// What the segmentation reader needs of the topology: per HMM its states, per state its
// transitions' target offsets and the global index of its first transition (HmmSet::read_ph numbers
// transitions state by state, HmmSet.cc:319-328).
struct TopoTables {
  std::vector<std::vector<int32_t>> hmm_states;
  std::vector<std::vector<int32_t>> offsets;
  std::vector<std::vector<double>> probs;
  std::vector<int32_t> tr_base;
  int32_t n_transitions = 0;
  explicit TopoTables(const aasr_topo *topo) {
    const int H = aasr_topo_num_hmms(topo), S = aasr_topo_num_states(topo);
    hmm_states.resize((size_t)std::max(0, H));
    for (int h = 0; h < H; h++) {
      hmm_states[(size_t)h].resize((size_t)std::max(0, aasr_topo_hmm_num_states(topo, h)));
      if (aasr_topo_hmm_states(topo, h, hmm_states[(size_t)h].data()) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    offsets.resize((size_t)std::max(0, S));
    probs.resize((size_t)std::max(0, S));
    for (int s = 0; s < S; s++) {
      const int n = aasr_topo_state_num_transitions(topo, s);
      offsets[(size_t)s].resize((size_t)n);
      probs[(size_t)s].resize((size_t)n);
      if (aasr_topo_state_transitions(topo, s, offsets[(size_t)s].data(), probs[(size_t)s].data()) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      tr_base.push_back(n_transitions);
      n_transitions += n;
    }
  }
};

struct Segmentation {
  bool initialized = false;  // init_utterance_segmentation succeeded
  int32_t start_frame = 0;   // frame of pdf[0]
  std::vector<int32_t> pdf;  // per frame
  std::vector<int32_t> tr;   // per frame: global transition index, -1: none
};

// PhnReader::next_frame (aku/PhnReader.cc:138-292) with state_num_labels = false and
// relative_sample_numbers = false, driven as stats.cc:simple_train drives it: frames until the
// reader's end, the frame loop leaving at eof_frame (< 0: no limit) after next_frame has run for it.
static Segmentation read_segmentation(const aasr_topo *topo, const TopoTables &tt, const char *path, float frame_rate,
                                      int first_frame, int last_frame, int eof_frame, bool transitions) {
  FILE *f = fopen(path, "r");
  if (!f) raise(AASR_ERR_IO, "PhnReader::open(): could not open %s", path);
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
  const float spf = 16000 / frame_rate;
  int line_no = 0;
  if (first_frame > 0 || last_frame > 0) phn_skip_to_first_frame(f, spf, first_frame, last_frame, &line_no);
  Segmentation seg;
  PhnLine cur;
  if (!next_phn_line(f, spf, first_frame, last_frame, &line_no, &cur)) return seg;
  seg.initialized = true;
  int frame = -1;
  bool eof_flag = false;
  while (!eof_flag) {
    frame = frame == -1 ? cur.start : frame + 1;
    if (cur.state < 0) raise(AASR_ERR_INVALID, "PhnReader::next_frame(): A state segmented phn file is required");
    const int h = aasr_topo_hmm_index(topo, cur.label.c_str());
    if (h < 0) raise(AASR_ERR_INVALID, "Unknown HMM in transcription: '%s' in %s", cur.label.c_str(), path);
    const std::vector<int32_t> &states = tt.hmm_states[(size_t)h];
    if (cur.state >= (int)states.size())
      raise(AASR_ERR_INVALID, "%s: state %d of HMM %s does not exist", path, cur.state, cur.label.c_str());
    const int state = states[(size_t)cur.state];
    bool new_phn_loaded = false;
    const PhnLine prev = cur;
    while (frame + 1 >= cur.end) {
      if (!next_phn_line(f, spf, first_frame, last_frame, &line_no, &cur)) {
        eof_flag = true;
        break;
      }
      new_phn_loaded = true;
    }
    int transition = -1;
    if (transitions && !eof_flag) {
      const std::vector<int32_t> &off = tt.offsets[(size_t)state];
      int found = -1;
      if (new_phn_loaded) {
        const int cur_state = prev.state;
        const int n_states = (int)tt.hmm_states[(size_t)aasr_topo_hmm_index(topo, prev.label.c_str())].size();
        for (size_t i = 0; i < off.size(); i++) {
          const int next_state = off[i] + cur_state;
          if ((next_state >= n_states && cur.state == 0) || (off[i] != 0 && next_state == cur.state)) {
            found = (int)i;
            break;
          }
        }
      } else {
        for (size_t i = 0; i < off.size(); i++)
          if (off[i] == 0) {
            found = (int)i;
            break;
          }
      }
      if (found < 0) raise(AASR_ERR_INVALID, "PhnReader::next_frame(): Correct transition was not found");
      transition = tt.tr_base[(size_t)state] + found;
    }
    if (eof_frame >= 0 && frame >= eof_frame) break;  // EOF in FeatureGenerator (stats.cc:105-112)
    if (seg.pdf.empty()) seg.start_frame = frame;
    seg.pdf.push_back(state);  // legacy .ph: a state's emission pdf is the state itself
    seg.tr.push_back(transition);
  }
  return seg;
}

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
  ~aasr_stats() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace aasr {

static void check_stats_model(const aasr_gmm *g) {
  if (g->host.any_full())
    raise(AASR_ERR_UNSUPPORTED, "stats: full-covariance and subspace Gaussians are not supported (diagonal pools only)");
  if (!g->host.gauss_bias.empty())
    raise(AASR_ERR_UNSUPPORTED, "stats: subspace Gaussians are not supported (diagonal pools only)");
  if (g->host.n_transforms > 0)
    raise(AASR_ERR_UNSUPPORTED, "stats: model-side transforms (cmllr) are not supported");
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

}  // namespace aasr

extern "C" {

aasr_status aasr_stats_create(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out) {
  return guarded([&] {
    if (!gmm || !topo || !out) raise(AASR_ERR_INVALID, "aasr_stats_create: null argument");
    *out = nullptr;
    check_stats_model(gmm);
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
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

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
    std::vector<int64_t> cnt((size_t)h->S + 1, 0);
    for (int64_t f = 0; f < n_frames; f++) {
      if (pdf[f] >= h->S) raise(AASR_ERR_INVALID, "aasr_stats_accumulate_dev: pdf %d of frame %ld out of range", pdf[f], (long)f);
      if (pdf[f] >= 0) cnt[(size_t)pdf[f] + 1]++;
    }
    for (int s = 0; s < h->S; s++) cnt[(size_t)s + 1] += cnt[(size_t)s];
    h->h_rows.resize((size_t)std::max<int64_t>(1, cnt[(size_t)h->S]));
    {
      std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
      for (int64_t f = 0; f < n_frames; f++)
        if (pdf[f] >= 0) h->h_rows[(size_t)fill[(size_t)pdf[f]]++] = (int32_t)f;
    }
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
    if (h->h_items.empty()) return;
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
    ok(aasr_stats_write_mcs((b + ".mcs").c_str(), h->S, 1, h->mix_off.data(), h->mix_idx.data(), count.data(),
                            gamma.data(), aux.data(), mll.data()));
    const size_t G1 = (size_t)std::max(1, h->G);
    std::vector<int64_t> fc(G1);
    std::vector<double> gg(G1), ga(G1), sx(G1 * h->D + 1), sxx(G1 * h->D + 1);
    ok(aasr_stats_gaussians(h, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
    ok(aasr_stats_write_gks((b + ".gks").c_str(), h->G, h->D, 1, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
  });
}

// ---- host-only segmentation reader ---------------------------------------------------------------

aasr_status aasr_stats_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate, int32_t first_frame,
                                         int32_t last_frame, int32_t eof_frame, int32_t transitions,
                                         int32_t *start_frame, int32_t **pdf, int32_t **transition, int32_t *n_frames) {
  return guarded([&] {
    if (!topo || !path || !start_frame || !pdf || !transition || !n_frames)
      raise(AASR_ERR_INVALID, "aasr_stats_read_segmentation: null argument");
    *pdf = nullptr;
    *transition = nullptr;
    TopoTables tt(topo);
    Segmentation seg = read_segmentation(topo, tt, path, frame_rate, first_frame, last_frame, eof_frame, transitions != 0);
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
    std::copy(seg.tr.begin(), seg.tr.end(), *transition);
    *start_frame = seg.start_frame;
    *n_frames = seg.initialized ? (int32_t)n : -1;
  });
}

void aasr_stats_default_options(aasr_stats_options *o) {
  if (o) memset(o, 0, sizeof *o);
}

}  // extern "C"

// ---- the stats main loop over a recipe ---------------------------------------------------------

namespace aasr {

struct StatsUtt {
  std::string audio, transcript, alignment, speaker, utterance;
  float start_time = 0, end_time = 0;
  int start_line = 0, end_line = 0;
};

static std::vector<StatsUtt> read_stats_recipe(const char *recipe_path, int num_batches, int batch_index) {
  FILE *f = fopen(recipe_path, "rb");
  if (!f) raise(AASR_ERR_IO, "could not open recipe %s", recipe_path);
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  fclose(f);
  char *table = nullptr;
  int64_t len = 0;
  // stats reads its recipe with cluster_speakers = false (aku/stats.cc:422-424)
  if (aasr_recipe_read_all(text.c_str(), num_batches, batch_index, 0, &table, &len) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  const std::string t(table, (size_t)len);
  aasr_free(table);
  std::vector<StatsUtt> out;
  size_t pos = 0;
  while (pos < t.size()) {
    size_t eol = t.find('\n', pos);
    if (eol == std::string::npos) eol = t.size();
    std::vector<std::string> fl;
    size_t a = pos;
    while (a <= eol) {
      size_t b = t.find('\x1f', a);
      if (b == std::string::npos || b > eol) b = eol;
      fl.push_back(t.substr(a, b - a));
      a = b + 1;
    }
    if (fl.size() == 13) {
      StatsUtt u;
      u.audio = fl[0];
      u.transcript = fl[2];
      u.alignment = fl[3];
      u.start_time = (float)atof(fl[7].c_str());
      u.end_time = (float)atof(fl[8].c_str());
      u.start_line = atoi(fl[9].c_str());
      u.end_line = atoi(fl[10].c_str());
      u.speaker = fl[11];
      u.utterance = fl[12];
      out.push_back(u);
    }
    pos = eol + 1;
  }
  return out;
}

}  // namespace aasr

extern "C" aasr_status aasr_run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                             const char *recipe_path, const aasr_stats_options *opt,
                                             aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || (!opt->no_train && !opt->out))
      raise(AASR_ERR_INVALID, "aasr_run_stats_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    if (aasr_gmm_dim(gmm) != aasr_feat_dim(feat))
      raise(AASR_ERR_INVALID, "gaussian dimension is %d but feature dimension is %d", aasr_gmm_dim(gmm),
            aasr_feat_dim(feat));
    std::vector<StatsUtt> utts = read_stats_recipe(recipe_path, opt->num_batches, opt->batch_index);
    for (const StatsUtt &u : utts)
      if (u.start_line > 0 || u.end_line > 0)
        raise(AASR_ERR_UNSUPPORTED, "stats: recipe line limits (start-line / end-line) are not supported");
    aasr_stats *h = nullptr;
    {  // (a model the accumulation kernel has no shape for keeps its AASR_ERR_UNSUPPORTED)
      const aasr_status cs = aasr_stats_create(gmm, topo, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_stats, void (*)(aasr_stats *)> hguard(h, aasr_stats_destroy);
    const TopoTables tt(topo);
    const float fr = aasr_feat_frame_rate(feat);
    const int D = aasr_gmm_dim(gmm);
    const bool accumulate = !opt->no_train;
    hipStream_t stream;
    AASR_HIP(hipStreamCreate(&stream));
    std::unique_ptr<void, void (*)(void *)> sguard((void *)stream, [](void *s) { (void)hipStreamDestroy((hipStream_t)s); });
    // -S: a speaker change that rewrites feature parameters waits for the features queued with the old ones;
    // utterances whose settings stay the same stay in flight together
    struct Unhook {
      aasr_spkc *s;
      ~Unhook() {
        if (s) spkc_set_before_change(s, nullptr);
      }
    } unhook{opt->speakers};
    if (opt->speakers) spkc_set_before_change(opt->speakers, [stream]() { AASR_HIP(hipStreamSynchronize(stream)); });
    DevBuf<int16_t> d_pcm;
    DevBuf<double> d_x, d_ll;
    double total_ll = 0;
    int64_t num_frames = 0;
    // groups of utterances accumulated in one launch; their frames stay on the device
    const int64_t max_group_frames = (int64_t)1 << 20;
    struct Pending {
      size_t utt;
      std::vector<int16_t> pcm;
      Segmentation seg;
    };
    size_t next = 0;
    while (next < utts.size()) {
      // host side first: audio and segmentation, the -i messages in recipe order
      std::vector<Pending> group;
      int64_t rows_total = 0;
      while (next < utts.size() && group.size() < 1024 && rows_total < max_group_frames) {
        const StatsUtt &u = utts[next];
        if (opt->info > 0) {
          fprintf(stderr, "Processing file: %s", u.audio.c_str());
          if (u.start_time || u.end_time) fprintf(stderr, " (%.2f-%.2f)", u.start_time, u.end_time);
          fprintf(stderr, "\n");
        }
        int16_t *pcm = nullptr;
        int64_t n_samples = 0;
        int32_t rate = 0;
        if (aasr_feat_input_is_features(feat)) {  // a pre module: feacat's feature file, in the engine's input units
          std::ifstream in(u.audio, std::ios::binary);
          if (!in) raise(AASR_ERR_IO, "could not open %s", u.audio.c_str());
          const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
          if (aasr_audio_decode(feat, bytes.data(), (int64_t)bytes.size(), &pcm, &n_samples, &rate) != AASR_OK)
            raise(AASR_ERR_IO, "%s: %s", u.audio.c_str(), aasr_last_error());
        } else if (aasr_audio_read(feat, u.audio.c_str(), &pcm, &n_samples, &rate) != AASR_OK) {
          raise(AASR_ERR_IO, "%s", aasr_last_error());
        }
        Pending pd;
        pd.utt = next;
        pd.pcm.assign(pcm, pcm + n_samples);
        aasr_free(pcm);
        const int eof = aasr_feat_eof_frame(feat, n_samples);
        int first = 0, last = 0;
        if (u.start_time > 0 || u.end_time > 0) {
          first = (int)(u.start_time * fr);
          last = (int)(u.end_time * fr);
        }
        pd.seg = read_segmentation(topo, tt, (opt->ophn ? u.alignment : u.transcript).c_str(), fr, first, last, eof,
                                   opt->transitions != 0);
        next++;
        if (!pd.seg.initialized) {
          fprintf(stderr, "Could not initialize the utterance segmentation.\n");
          fprintf(stderr, "Giving up for this file\n");
          pd.pcm.clear();  // no frames; kept in the group for its speaker settings (stats.cc:560-565 run first)
        }
        rows_total += (int64_t)pd.seg.pdf.size();
        group.push_back(std::move(pd));
      }
      // features of the group into one device buffer, speaker configuration per utterance
      d_x.ensure((size_t)std::max<int64_t>(1, rows_total) * D);
      d_ll.ensure((size_t)std::max<int64_t>(1, rows_total));
      std::vector<int32_t> pdfs;
      pdfs.reserve((size_t)rows_total);
      size_t samples = 1;
      for (const Pending &pd : group) samples += pd.pcm.size();
      if (samples > d_pcm.n) {
        AASR_HIP(hipStreamSynchronize(stream));
        d_pcm.alloc(samples);
      }
      size_t pcm_at = 0;
      int64_t row = 0;
      for (Pending &pd : group) {
        const StatsUtt &u = utts[pd.utt];
        if (opt->speakers) {  // (a parameter change waits for the queued features: the hook above)
          if (aasr_spkc_set_speaker(opt->speakers, u.speaker.c_str()) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
          if (opt->uttadap && !u.utterance.empty() && aasr_spkc_set_utterance(opt->speakers, u.utterance.c_str()) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
          check_stats_model(gmm);
        }
        const int64_t n = (int64_t)pd.seg.pdf.size();
        if (n > 0) {  // (the group's audio stays on the host until the group's wait below)
          if (!pd.pcm.empty())
            AASR_HIP(hipMemcpyAsync(d_pcm.p + pcm_at, pd.pcm.data(), pd.pcm.size() * sizeof(int16_t),
                                    hipMemcpyHostToDevice, stream));
          if (aasr_feat_run_f64_dev(feat, d_pcm.p + pcm_at, (int64_t)pd.pcm.size(), pd.seg.start_frame, (int32_t)n,
                                    d_x.p + (size_t)row * D, stream) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
          pcm_at += pd.pcm.size();
        }
        pdfs.insert(pdfs.end(), pd.seg.pdf.begin(), pd.seg.pdf.end());
        if (accumulate && opt->transitions && aasr_stats_add_transitions(h, pd.seg.tr.data(), n) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        row += n;
      }
      if (rows_total == 0) continue;
      if (aasr_stats_accumulate_dev(h, d_x.p, rows_total, pdfs.data(), d_ll.p, stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      // the .lls figure in frame order: state likelihoods, then the transition taken (stats.cc:130-160)
      std::vector<double> ll((size_t)rows_total);
      AASR_HIP(hipMemcpyAsync(ll.data(), d_ll.p, ll.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
      AASR_HIP(hipStreamSynchronize(stream));
      row = 0;
      for (const Pending &pd : group) {
        for (size_t f = 0; f < pd.seg.pdf.size(); f++) {
          total_ll += ll[(size_t)row + f];  // safe_log(1.0 * state_likelihood): the kernel's safe_log(total)
          const int t = pd.seg.tr[f];
          if (opt->transitions && accumulate && t >= 0) {
            const int s = h->tr_source[(size_t)t];
            total_ll += safe_log(1.0 * tt.probs[(size_t)s][(size_t)(t - tt.tr_base[(size_t)s])]);
          }
        }
        row += (int64_t)pd.seg.pdf.size();
        num_frames += (int64_t)pd.seg.pdf.size();
      }
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
    if (stats) {
      stats->utterances = (int64_t)utts.size();
      stats->frames = num_frames;
      stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      stats->seconds_device = 0;
      stats->seconds_copy_out = 0;
    }
  });
}

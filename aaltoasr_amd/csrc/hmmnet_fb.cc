// hmmnet_fb.cc -- the handle of the forward-backward pass over HMM networks (aasr_fb_batch_*): packs the
// utterances' networks (hmmnet.h) into the blobs of hmmnet_fb.h, launches k_hmmnet_fb over the batch, and
// relaunches the utterances whose backward pass missed the initial node with a wider backward beam
// (aku/logl.cc:183-199: 2x, 3x, ... the original, the forward beam unchanged).  With device_occ the occupancies stay on
// the device and aasr_fb_batch_entries_dev turns them into the weighted entries of the statistics accumulation
// (fb_entries.hip), aasr_fb_batch_frame_entries_dev into the frame-major (pdf, weight) lists of the CMLLR accumulation
// (fb_frame_entries.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

#include "common.h"
#include "fb_entries.h"
#include "fb_frame_entries.h"
#include "hmmnet.h"
#include "hmmnet_fb.h"

using namespace aasr;

struct aasr_fb_batch {
  aasr_fb_options opt{};
  int32_t n = 0;
  bool lds_form = true;
  std::vector<const aasr_hmmnet *> nets;
  std::vector<FbUttDev> utt;
  std::vector<FbResult> result;
  std::vector<int32_t> list;
  std::vector<double> occ, trocc;  // host copies after a sync
  std::vector<int32_t> path;       // host copy of the paths (want_path), fetched by the first aasr_fb_batch_path
  bool synced = false, path_fetched = false;
  hipStream_t sync_stream = nullptr;
  DevBuf<int32_t> d_ints, d_list, d_path;
  DevBuf<double> d_doubles, d_work, d_occ, d_trocc;
  DevBuf<FbUttDev> d_utt;
  DevBuf<FbResult> d_result;
  int64_t bytes = 0;
  // the last launch (aasr_debug_fb_shape): utterances, 1 = LDS node vectors / 0 = global, LDS bytes, attempt
  int32_t last_shape[4] = {0, 0, 0, 0};
  // the entries of the last aasr_fb_batch_entries_dev call (fb_entries.h)
  std::vector<FbEntryUtt> e_utt;
  std::vector<FbEntryPair> e_pairs;
  std::vector<int32_t> e_counts, e_index;  // entries per pair; per utterance its place in e_utt, -1: not covered
  std::vector<int64_t> e_out;
  std::vector<double> e_sums;  // host copy of the frame sums, fetched by the first aasr_fb_batch_frame_sums
  bool e_built = false, e_sums_fetched = false;
  bool s_built = false;  // e_utt, e_index and the frame sums on the device are those of the last entries call of either kind
  hipStream_t e_stream = nullptr;
  DevBuf<FbEntryUtt> d_e_utt;
  DevBuf<FbEntryPair> d_e_pairs;
  DevBuf<int32_t> d_e_counts, d_e_rows;
  DevBuf<int64_t> d_e_out;
  DevBuf<double> d_e_sums, d_e_weights;
  // aasr_debug_fb_entries_shape: entries, utterances covered, workgroups of the sum, count and fill kernels
  int32_t entries_shape[5] = {0, 0, 0, 0, 0};
  // the frame-major entries of the last aasr_fb_batch_frame_entries_dev call (fb_frame_entries.h)
  std::vector<int64_t> f_pdf_at;  // per covered utterance the start of its network's pdf list in f_pdfs
  std::vector<int32_t> f_pdfs;
  bool f_built = false;
  int64_t f_total = 0, f_rows = 0;
  DevBuf<int64_t> d_f_pdf_at, d_f_off, d_f_block_sums;
  DevBuf<int32_t> d_f_pdfs, d_f_counts, d_f_pdf;
  DevBuf<double> d_f_weight;
  // aasr_debug_fb_frame_entries_shape: entries, utterances covered, workgroups of the count, offset and fill kernels
  int32_t frame_entries_shape[5] = {0, 0, 0, 0, 0};
};

extern "C" {

void aasr_fb_default_options(aasr_fb_options *o) {
  if (!o) return;
  *o = aasr_fb_options();
  o->fw_beam = 15;   // HmmNetBaumWelch's constructor
  o->bw_beam = 200;
  o->ac_scale = 1;
  o->mode = AASR_FB_BAUM_WELCH;
  o->max_attempts = 5;
}

aasr_status aasr_fb_batch_create(const aasr_fb_options *opt, int32_t n_utt, const aasr_hmmnet *const *nets,
                                 const int32_t *n_frames, aasr_fb_batch **out) {
  return guarded([&] {
    if (!opt || n_utt < 0 || !out || (n_utt > 0 && (!nets || !n_frames)))
      raise(AASR_ERR_INVALID, "aasr_fb_batch_create: null argument");
    *out = nullptr;
    if (!(opt->fw_beam > 0) || !(opt->bw_beam > 0) || !std::isfinite(opt->fw_beam) || !std::isfinite(opt->bw_beam))
      raise(AASR_ERR_INVALID, "aasr_fb_batch_create: beams must be positive and finite");
    if (!std::isfinite(opt->ac_scale)) raise(AASR_ERR_INVALID, "aasr_fb_batch_create: acoustic scale must be finite");
    if (opt->mode != AASR_FB_BAUM_WELCH && opt->mode != AASR_FB_VITERBI)
      raise(AASR_ERR_UNSUPPORTED, "aasr_fb_batch_create: mode %d (multipath Viterbi is not built)", opt->mode);
    if (opt->max_attempts < 1) raise(AASR_ERR_INVALID, "aasr_fb_batch_create: max_attempts must be at least 1");
    if (opt->want_path && opt->mode != AASR_FB_VITERBI)
      raise(AASR_ERR_UNSUPPORTED, "aasr_fb_batch_create: want_path needs the Viterbi mode (Baum-Welch has no single arc per frame)");
    for (int u = 0; u < n_utt; u++) {
      if (!nets[u]) raise(AASR_ERR_INVALID, "aasr_fb_batch_create: utterance %d has no network", u);
      if (n_frames[u] < 1) raise(AASR_ERR_INVALID, "aasr_fb_batch_create: utterance %d has %d frames", u, n_frames[u]);
    }
    require_device();
    std::unique_ptr<aasr_fb_batch> b(new aasr_fb_batch());
    b->opt = *opt;
    b->n = n_utt;
    b->nets.assign(nets, nets + n_utt);
    // each distinct network once in the blobs
    std::vector<int32_t> ints;
    std::vector<double> doubles;
    std::map<const aasr_hmmnet *, FbNetDev> packed;
    auto put_i = [&](const std::vector<int32_t> &v) {
      const int32_t at = (int32_t)ints.size();
      ints.insert(ints.end(), v.begin(), v.end());
      return at;
    };
    auto put_d = [&](const std::vector<double> &v) {
      const int32_t at = (int32_t)doubles.size();
      doubles.insert(doubles.end(), v.begin(), v.end());
      return at;
    };
    int32_t max_nodes = 0;
    int64_t work = 0, occ = 0, trocc = 0, path = 0;
    b->utt.resize((size_t)n_utt);
    for (int u = 0; u < n_utt; u++) {
      const aasr_hmmnet &h = *nets[u];
      if (ints.size() + 8 * (h.em_src.size() + h.ep_src.size() + (size_t)h.n_nodes) > (size_t)INT32_MAX)
        raise(AASR_ERR_UNSUPPORTED, "aasr_fb_batch_create: the batch's networks exceed 2^31 table entries");
      if (!packed.count(&h)) {
        FbNetDev d{};
        d.n_nodes = h.n_nodes;
        d.n_em = (int32_t)h.em_src.size();
        d.n_ep = (int32_t)h.ep_src.size();
        d.n_bl = (int32_t)h.bl_begin.size() - 1;
        d.n_fl = (int32_t)h.fl_begin.size() - 1;
        d.n_pdf = (int32_t)h.pdfs.size();
        d.n_tr = (int32_t)h.trs.size();
        d.initial = h.initial;
        d.final_node = h.final_node;
        d.em_begin = put_i(h.em_begin);
        d.em_src = put_i(h.em_src);
        d.em_tgt = put_i(h.em_tgt);
        d.em_pdf = put_i(h.em_pdf);
        d.em_slot = put_i(h.em_slot);
        d.em_trslot = put_i(h.em_trslot);
        d.in_begin = put_i(h.in_begin);
        d.in_arcs = put_i(h.in_arcs);
        d.pdf_begin = put_i(h.pdf_begin);
        d.pdf_arcs = put_i(h.pdf_arcs);
        d.tr_begin = put_i(h.tr_begin);
        d.tr_arcs = put_i(h.tr_arcs);
        d.eo_begin = put_i(h.eo_begin);
        d.ep_src = put_i(h.ep_src);
        d.ep_tgt = put_i(h.ep_tgt);
        d.ei_begin = put_i(h.ei_begin);
        d.ei_arcs = put_i(h.ei_arcs);
        d.bl_begin = put_i(h.bl_begin);
        d.bl_nodes = put_i(h.bl_nodes);
        d.fl_begin = put_i(h.fl_begin);
        d.fl_nodes = put_i(h.fl_nodes);
        d.em_logp = put_d(h.em_logp);
        d.em_static = put_d(h.em_static);
        d.ep_score = put_d(h.ep_score);
        packed[&h] = d;
      }
      FbUttDev &d = b->utt[(size_t)u];
      d.net = packed[&h];
      d.row0 = 0;
      d.T = n_frames[u];
      d.beta = work;
      work += ((int64_t)d.T + 1) * h.n_nodes;
      d.best = work;
      work += d.T;
      d.arcs = work;
      work += 2 * (int64_t)d.net.n_em;
      d.nodes = work;
      work += 2 * (int64_t)h.n_nodes;
      d.occ = occ;
      occ += (int64_t)d.T * d.net.n_pdf;
      d.trocc = trocc;
      trocc += d.net.n_tr;
      d.path = path;
      path += d.T;
      max_nodes = std::max(max_nodes, h.n_nodes);
    }
    b->lds_form = max_nodes <= FB_LDS_NODES && !opt->force_global;
    if (ints.empty()) ints.push_back(0);
    if (doubles.empty()) doubles.push_back(0);
    b->d_ints.upload(ints.data(), ints.size());
    b->d_doubles.upload(doubles.data(), doubles.size());
    const size_t nu = (size_t)std::max(1, n_utt);
    b->d_utt.alloc(nu);
    b->d_result.alloc(nu);
    b->d_list.alloc(nu);
    b->d_work.alloc((size_t)std::max<int64_t>(1, work));
    if (opt->want_pdf_occ) b->d_occ.alloc((size_t)std::max<int64_t>(1, occ));
    if (opt->want_tr_occ) b->d_trocc.alloc((size_t)std::max<int64_t>(1, trocc));
    if (opt->want_path) b->d_path.alloc((size_t)std::max<int64_t>(1, path));
    if (opt->device_occ && !opt->want_pdf_occ)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_create: device_occ without want_pdf_occ");
    b->occ.assign(opt->want_pdf_occ && !opt->device_occ ? (size_t)occ : 0, 0.0);
    b->trocc.assign(opt->want_tr_occ ? (size_t)trocc : 0, 0.0);
    b->path.assign(opt->want_path ? (size_t)path : 0, -1);
    b->result.assign((size_t)n_utt, FbResult{FB_ZERO, FB_ZERO, 0, 0});
    b->bytes = (int64_t)(ints.size() * 4 + doubles.size() * 8 + (size_t)work * 8 + (opt->want_pdf_occ ? (size_t)occ : 0) * 8 + b->trocc.size() * 8 +
                         b->path.size() * 4 + nu * (sizeof(FbUttDev) + sizeof(FbResult) + 4));
    *out = b.release();
  });
}

void aasr_fb_batch_destroy(aasr_fb_batch *b) { delete b; }

int64_t aasr_fb_batch_device_bytes(const aasr_fb_batch *b) { return b ? b->bytes : -1; }

void aasr_debug_fb_shape(const aasr_fb_batch *b, int32_t *out) {
  if (!b || !out) return;
  std::copy(b->last_shape, b->last_shape + 4, out);
}

aasr_status aasr_fb_batch_dev(aasr_fb_batch *b, const void *d_state_loglik, int64_t pitch, int64_t n_rows, int32_t f64,
                              const int64_t *row0, int32_t attempt, void *stream) {
  return guarded([&] {
    if (!b || (b->n > 0 && (!d_state_loglik || !row0)) || pitch < 1)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_dev: bad argument");
    if (attempt < 1 || attempt > b->opt.max_attempts)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_dev: attempt %d outside 1 .. %d", attempt, b->opt.max_attempts);
    const hipStream_t st = (hipStream_t)stream;
    b->e_built = b->e_sums_fetched = false;  // (entries of an earlier pass describe occupancies this one rewrites)
    b->s_built = b->f_built = false;
    b->synced = b->path_fetched = false;     // (and so do its results and paths)
    b->list.clear();
    for (int u = 0; u < b->n; u++) {
      const aasr_hmmnet &h = *b->nets[(size_t)u];
      for (int32_t pdf : h.pdfs)
        if (pdf >= pitch) raise(AASR_ERR_INVALID, "aasr_fb_batch_dev: utterance %d uses pdf %d, rows have %lld columns", u, pdf, (long long)pitch);
      if (row0[u] < 0 || row0[u] + b->utt[(size_t)u].T > n_rows)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_dev: utterance %d reads rows %lld .. %lld of %lld", u, (long long)row0[u],
              (long long)(row0[u] + b->utt[(size_t)u].T), (long long)n_rows);
      b->utt[(size_t)u].row0 = row0[u];
      // the first attempt runs every utterance, a later one those whose backward pass failed (results of a sync)
      if (attempt == 1 || b->result[(size_t)u].status == FB_FAILED_BACKWARD) b->list.push_back(u);
    }
    if (attempt == 1) {
      for (FbResult &r : b->result) r = FbResult{FB_ZERO, FB_ZERO, 0, 0};
      if (b->n) AASR_HIP(hipMemcpyAsync(b->d_result.p, b->result.data(), b->result.size() * sizeof(FbResult), hipMemcpyHostToDevice, st));
    }
    b->last_shape[0] = (int32_t)b->list.size();
    b->last_shape[1] = b->lds_form ? 1 : 0;
    b->last_shape[2] = (int32_t)((b->lds_form ? 2 * FB_LDS_NODES : 1) * sizeof(double) + FB_THREADS * sizeof(double));
    b->last_shape[3] = attempt;
    if (b->list.empty()) return;
    AASR_HIP(hipMemcpyAsync(b->d_utt.p, b->utt.data(), b->utt.size() * sizeof(FbUttDev), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(b->d_list.p, b->list.data(), b->list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FbParams p{};
    p.ints = b->d_ints.p;
    p.doubles = b->d_doubles.p;
    p.utt = b->d_utt.p;
    p.list = b->d_list.p;
    p.scores = d_state_loglik;
    p.pitch = pitch;
    p.f64 = f64 ? 1 : 0;
    p.mode = b->opt.mode == AASR_FB_VITERBI ? FB_MODE_VITERBI : FB_MODE_BAUM_WELCH;
    p.want_pdf_occ = b->opt.want_pdf_occ ? 1 : 0;
    p.want_tr_occ = b->opt.want_tr_occ ? 1 : 0;
    p.fw_beam = b->opt.fw_beam;
    p.bw_beam = attempt * b->opt.bw_beam;
    p.ac_scale = b->opt.ac_scale;
    p.work = b->d_work.p;
    p.occ = b->d_occ.p;
    p.trocc = b->d_trocc.p;
    p.result = b->d_result.p;
    p.path = b->opt.want_path ? b->d_path.p : nullptr;
    hmmnet_fb_launch(p, (int32_t)b->list.size(), b->lds_form, st);
    AASR_HIP(hipGetLastError());
    // the host tables of this call are read by the copies above: wait for them before the next call rewrites them
    AASR_HIP(hipStreamSynchronize(st));
  });
}

aasr_status aasr_fb_batch_sync(aasr_fb_batch *b, void *stream, int32_t *n_failed_backward) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_fb_batch_sync: null argument");
    const hipStream_t st = (hipStream_t)stream;
    if (b->n > 0) {
      AASR_HIP(hipMemcpyAsync(b->result.data(), b->d_result.p, b->result.size() * sizeof(FbResult), hipMemcpyDeviceToHost, st));
      if (!b->occ.empty())
        AASR_HIP(hipMemcpyAsync(b->occ.data(), b->d_occ.p, b->occ.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      if (!b->trocc.empty())
        AASR_HIP(hipMemcpyAsync(b->trocc.data(), b->d_trocc.p, b->trocc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipStreamSynchronize(st));
    }
    b->synced = true;
    b->sync_stream = st;
    int failed = 0;
    for (const FbResult &r : b->result) failed += r.status == FB_FAILED_BACKWARD;
    if (n_failed_backward) *n_failed_backward = failed;
  });
}

aasr_status aasr_fb_batch_result(const aasr_fb_batch *b, int32_t u, int32_t *status, double *backward_total,
                                 double *forward_total, int32_t *attempts, double *pdf_occ, double *tr_occ) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n) raise(AASR_ERR_INVALID, "aasr_fb_batch_result: bad argument");
    const FbResult &r = b->result[(size_t)u];
    const FbUttDev &d = b->utt[(size_t)u];
    if (status) *status = r.status;
    if (backward_total) *backward_total = r.backward_total;
    if (forward_total) *forward_total = r.forward_total;
    if (attempts) *attempts = r.attempts;
    if (pdf_occ) {
      if (!b->opt.want_pdf_occ) raise(AASR_ERR_INVALID, "aasr_fb_batch_result: the batch was created without pdf occupancies");
      if (b->opt.device_occ)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_result: the batch keeps its pdf occupancies on the device (device_occ); "
                                "use aasr_fb_batch_entries_dev");
      if (r.status == FB_OK) std::copy(b->occ.begin() + d.occ, b->occ.begin() + d.occ + (int64_t)d.T * d.net.n_pdf, pdf_occ);
    }
    if (tr_occ) {
      if (!b->opt.want_tr_occ) raise(AASR_ERR_INVALID, "aasr_fb_batch_result: the batch was created without transition occupancies");
      if (r.status == FB_OK) std::copy(b->trocc.begin() + d.trocc, b->trocc.begin() + d.trocc + d.net.n_tr, tr_occ);
    }
  });
}

aasr_status aasr_fb_batch_path(aasr_fb_batch *b, int32_t u, int32_t *arcs) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n || !arcs) raise(AASR_ERR_INVALID, "aasr_fb_batch_path: bad argument");
    if (!b->opt.want_path) raise(AASR_ERR_INVALID, "aasr_fb_batch_path: the batch was created without want_path");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fb_batch_path: call aasr_fb_batch_sync first");
    if (b->result[(size_t)u].status != FB_OK)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_path: utterance %d did not run (status %d)", u, b->result[(size_t)u].status);
    // d_path is never initialised: an utterance that failed keeps stale arcs in its slice.  The status check above keeps
    // them from the caller, and the range check below holds whatever the device wrote.
    if (!b->path_fetched) {  // every utterance's path in one copy, on the stream of the sync
      if (!b->path.empty()) {
        AASR_HIP(hipMemcpyAsync(b->path.data(), b->d_path.p, b->path.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b->sync_stream));
        AASR_HIP(hipStreamSynchronize(b->sync_stream));
      }
      b->path_fetched = true;
    }
    const FbUttDev &d = b->utt[(size_t)u];
    const int32_t n_em = d.net.n_em;
    for (int32_t t = 0; t < d.T; t++) {
      const int32_t a = b->path[(size_t)d.path + t];
      if (a < 0 || a >= n_em) raise(AASR_ERR_INVALID, "aasr_fb_batch_path: utterance %d has arc %d at frame %d", u, a, t);
      arcs[t] = a;
    }
  });
}

aasr_status aasr_fb_batch_entries_dev(aasr_fb_batch *b, int32_t n_states, const int64_t *row0, void *stream, int64_t *cnt,
                                      const int32_t **d_rows, const double **d_weights) {
  return guarded([&] {
    if (!b || n_states < 0 || (b->n > 0 && !row0) || !cnt || !d_rows || !d_weights)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: bad argument");
    if (!b->opt.want_pdf_occ || !b->opt.device_occ)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: the batch was created without device_occ");
    const hipStream_t st = (hipStream_t)stream;
    *d_rows = nullptr;
    *d_weights = nullptr;
    b->e_built = b->e_sums_fetched = false;
    b->s_built = b->f_built = false;  // (the frame-major entries index e_utt as their call left it)
    b->e_utt.clear();
    b->e_pairs.clear();
    b->e_index.assign((size_t)b->n, -1);
    // the utterances that ran, and their (pdf, utterance) pairs ordered by global pdf, then by utterance
    std::vector<std::pair<int32_t, FbEntryPair>> keyed;
    int64_t sums = 0;
    int32_t max_T = 0;
    for (int u = 0; u < b->n; u++) {
      if (b->result[(size_t)u].status != FB_OK) continue;
      const FbUttDev &d = b->utt[(size_t)u];
      const aasr_hmmnet &h = *b->nets[(size_t)u];
      if (row0[u] < 0 || row0[u] + d.T > (int64_t)INT32_MAX)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: utterance %d has frame rows %lld .. %lld, outside 0 .. 2^31", u,
              (long long)row0[u], (long long)(row0[u] + d.T));
      b->e_index[(size_t)u] = (int32_t)b->e_utt.size();
      for (int32_t j = 0; j < (int32_t)h.pdfs.size(); j++) {
        if (h.pdfs[(size_t)j] < 0 || h.pdfs[(size_t)j] >= n_states)
          raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: utterance %d uses pdf %d, the model has %d", u, h.pdfs[(size_t)j],
                n_states);
        keyed.push_back({h.pdfs[(size_t)j], FbEntryPair{(int32_t)b->e_utt.size(), j}});
      }
      b->e_utt.push_back(FbEntryUtt{d.occ, sums, row0[u], d.T, d.net.n_pdf});
      sums += d.T;
      max_T = std::max(max_T, d.T);
    }
    std::stable_sort(keyed.begin(), keyed.end(),
                     [](const std::pair<int32_t, FbEntryPair> &a, const std::pair<int32_t, FbEntryPair> &c) { return a.first < c.first; });
    for (const auto &k : keyed) b->e_pairs.push_back(k.second);
    const int32_t n_utt = (int32_t)b->e_utt.size(), n_pairs = (int32_t)b->e_pairs.size();
    std::fill(cnt, cnt + (size_t)n_states + 1, (int64_t)0);
    std::fill(b->entries_shape, b->entries_shape + 5, 0);
    b->entries_shape[1] = n_utt;
    b->e_out.assign((size_t)n_pairs + 1, 0);
    b->e_sums.assign((size_t)sums, 0.0);
    b->e_stream = st;
    if (n_pairs == 0) {
      b->e_built = b->s_built = true;
      return;
    }
    b->d_e_utt.ensure((size_t)n_utt);
    b->d_e_pairs.ensure((size_t)n_pairs);
    b->d_e_counts.ensure((size_t)n_pairs);
    b->d_e_out.ensure((size_t)n_pairs + 1);
    b->d_e_sums.ensure((size_t)sums);
    AASR_HIP(hipMemcpyAsync(b->d_e_utt.p, b->e_utt.data(), (size_t)n_utt * sizeof(FbEntryUtt), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(b->d_e_pairs.p, b->e_pairs.data(), (size_t)n_pairs * sizeof(FbEntryPair), hipMemcpyHostToDevice, st));
    fb_frame_sums_launch(b->d_e_utt.p, n_utt, max_T, b->d_occ.p, b->d_e_sums.p, st);
    fb_entry_counts_launch(b->d_e_utt.p, b->d_e_pairs.p, n_pairs, b->d_occ.p, b->d_e_counts.p, st);
    // the one fetch and the one wait of the call: the entries of every pair
    b->e_counts.assign((size_t)n_pairs, 0);
    AASR_HIP(hipMemcpyAsync(b->e_counts.data(), b->d_e_counts.p, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
    for (int32_t q = 0; q < n_pairs; q++) {
      if (b->e_counts[(size_t)q] < 0 || b->e_counts[(size_t)q] > b->e_utt[(size_t)b->e_pairs[(size_t)q].utt].T)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: pair %d reports %d entries", q, b->e_counts[(size_t)q]);
      b->e_out[(size_t)q + 1] = b->e_out[(size_t)q] + b->e_counts[(size_t)q];
      cnt[(size_t)keyed[(size_t)q].first + 1] += b->e_counts[(size_t)q];
    }
    for (int32_t s = 0; s < n_states; s++) cnt[(size_t)s + 1] += cnt[(size_t)s];
    const int64_t total = b->e_out[(size_t)n_pairs];
    if (total > (int64_t)INT32_MAX) raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_dev: more than 2^31 entries in one batch");
    b->d_e_rows.ensure((size_t)std::max<int64_t>(1, total));
    b->d_e_weights.ensure((size_t)std::max<int64_t>(1, total));
    AASR_HIP(hipMemcpyAsync(b->d_e_out.p, b->e_out.data(), b->e_out.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    fb_entry_fill_launch(b->d_e_utt.p, b->d_e_pairs.p, n_pairs, b->d_occ.p, b->d_e_sums.p, b->d_e_out.p, b->d_e_rows.p,
                         b->d_e_weights.p, st);
    b->entries_shape[0] = (int32_t)total;
    b->entries_shape[2] = ((max_T + FBE_THREADS - 1) / FBE_THREADS) * n_utt;
    b->entries_shape[3] = b->entries_shape[4] = (n_pairs + FBE_THREADS - 1) / FBE_THREADS;
    b->e_built = b->s_built = true;
    *d_rows = b->d_e_rows.p;
    *d_weights = b->d_e_weights.p;
  });
}

aasr_status aasr_fb_batch_entries_host(aasr_fb_batch *b, int32_t *rows, double *weights) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_host: null argument");
    if (!b->e_built) raise(AASR_ERR_INVALID, "aasr_fb_batch_entries_host: call aasr_fb_batch_entries_dev first");
    const size_t total = (size_t)b->e_out.back();
    if (total == 0) return;
    if (rows) AASR_HIP(hipMemcpyAsync(rows, b->d_e_rows.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, b->e_stream));
    if (weights) AASR_HIP(hipMemcpyAsync(weights, b->d_e_weights.p, total * sizeof(double), hipMemcpyDeviceToHost, b->e_stream));
    AASR_HIP(hipStreamSynchronize(b->e_stream));
  });
}

aasr_status aasr_fb_batch_frame_sums(aasr_fb_batch *b, int32_t u, double *sums) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n || !sums) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_sums: bad argument");
    if (!b->s_built) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_sums: call aasr_fb_batch_entries_dev first");
    const int32_t e = b->e_index[(size_t)u];
    if (e < 0) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_sums: utterance %d did not run (status %d)", u, b->result[(size_t)u].status);
    if (!b->e_sums_fetched) {  // every covered utterance's sums in one copy, on the stream that computed them
      if (!b->e_sums.empty()) {
        AASR_HIP(hipMemcpyAsync(b->e_sums.data(), b->d_e_sums.p, b->e_sums.size() * sizeof(double), hipMemcpyDeviceToHost, b->e_stream));
        AASR_HIP(hipStreamSynchronize(b->e_stream));
      }
      b->e_sums_fetched = true;
    }
    const FbEntryUtt &eu = b->e_utt[(size_t)e];
    std::copy(b->e_sums.begin() + eu.sums, b->e_sums.begin() + eu.sums + eu.T, sums);
  });
}

aasr_status aasr_fb_batch_frame_entries_dev(aasr_fb_batch *b, int32_t n_states, const int64_t *row0, int64_t n_rows,
                                            void *stream, int64_t *n_entries, const int64_t **d_off, const int32_t **d_pdf,
                                            const double **d_weight) {
  return guarded([&] {
    if (!b || n_states < 0 || n_rows < 0 || (b->n > 0 && !row0) || !n_entries || !d_off || !d_pdf || !d_weight)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: bad argument");
    if (!b->opt.want_pdf_occ || !b->opt.device_occ)
      raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: the batch was created without device_occ");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: call aasr_fb_batch_sync first");
    if (n_rows >= (int64_t)INT32_MAX) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: more than 2^31 frame rows");
    const hipStream_t st = (hipStream_t)stream;
    *n_entries = 0;
    *d_off = nullptr;
    *d_pdf = nullptr;
    *d_weight = nullptr;
    // the pdf-major entries go: both calls keep the covered utterances and their frame sums in the same members
    b->e_built = b->e_sums_fetched = b->s_built = b->f_built = false;
    b->e_utt.clear();
    b->e_index.assign((size_t)b->n, -1);
    b->f_pdf_at.clear();
    b->f_pdfs.clear();
    std::fill(b->frame_entries_shape, b->frame_entries_shape + 5, 0);
    int64_t sums = 0, bound = 0;
    int32_t max_T = 0;
    std::vector<std::pair<int64_t, int64_t>> windows;  // the utterances' rows must not overlap: a row has one lane
    for (int u = 0; u < b->n; u++) {
      if (b->result[(size_t)u].status != FB_OK) continue;
      const FbUttDev &d = b->utt[(size_t)u];
      const aasr_hmmnet &h = *b->nets[(size_t)u];
      if (row0[u] < 0 || row0[u] + d.T > n_rows)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: utterance %d has frame rows %lld .. %lld of %lld", u,
              (long long)row0[u], (long long)(row0[u] + d.T), (long long)n_rows);
      for (int32_t pdf : h.pdfs)
        if (pdf < 0 || pdf >= n_states)
          raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: utterance %d uses pdf %d, the model has %d", u, pdf, n_states);
      windows.push_back({row0[u], row0[u] + d.T});
      b->e_index[(size_t)u] = (int32_t)b->e_utt.size();
      b->e_utt.push_back(FbEntryUtt{d.occ, sums, row0[u], d.T, d.net.n_pdf});
      b->f_pdf_at.push_back((int64_t)b->f_pdfs.size());
      b->f_pdfs.insert(b->f_pdfs.end(), h.pdfs.begin(), h.pdfs.end());
      sums += d.T;
      bound += (int64_t)d.T * d.net.n_pdf;
      max_T = std::max(max_T, d.T);
    }
    std::sort(windows.begin(), windows.end());
    for (size_t i = 1; i < windows.size(); i++)
      if (windows[i].first < windows[i - 1].second)
        raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: two utterances share frame row %lld", (long long)windows[i].first);
    const int32_t n_utt = (int32_t)b->e_utt.size();
    b->e_sums.assign((size_t)sums, 0.0);
    b->e_stream = st;
    b->f_total = 0;
    b->f_rows = n_rows;
    b->frame_entries_shape[1] = n_utt;
    b->d_f_counts.ensure((size_t)n_rows + 1);
    b->d_f_off.ensure((size_t)n_rows + 1);
    const int64_t scan_blocks = fb_frame_scan_blocks(n_rows);
    b->d_f_block_sums.ensure((size_t)scan_blocks + 1);
    AASR_HIP(hipMemsetAsync(b->d_f_counts.p, 0, ((size_t)n_rows + 1) * sizeof(int32_t), st));
    if (n_utt > 0) {
      b->d_e_utt.ensure((size_t)n_utt);
      b->d_e_sums.ensure((size_t)sums);
      b->d_f_pdf_at.ensure((size_t)n_utt);
      b->d_f_pdfs.ensure(std::max<size_t>(1, b->f_pdfs.size()));
      AASR_HIP(hipMemcpyAsync(b->d_e_utt.p, b->e_utt.data(), (size_t)n_utt * sizeof(FbEntryUtt), hipMemcpyHostToDevice, st));
      AASR_HIP(hipMemcpyAsync(b->d_f_pdf_at.p, b->f_pdf_at.data(), (size_t)n_utt * sizeof(int64_t), hipMemcpyHostToDevice, st));
      if (!b->f_pdfs.empty())
        AASR_HIP(hipMemcpyAsync(b->d_f_pdfs.p, b->f_pdfs.data(), b->f_pdfs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      fb_frame_sums_launch(b->d_e_utt.p, n_utt, max_T, b->d_occ.p, b->d_e_sums.p, st);
      fb_frame_counts_launch(b->d_e_utt.p, n_utt, max_T, b->d_occ.p, b->d_f_counts.p, st);
    }
    fb_frame_offsets_launch(b->d_f_counts.p, n_rows, b->d_f_block_sums.p, b->d_f_off.p, st);
    // the one fetch and the one wait of the call: the number of entries
    int64_t total = 0;
    AASR_HIP(hipMemcpyAsync(&total, b->d_f_off.p + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
    if (total < 0 || total > bound) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: the frames report %lld entries", (long long)total);
    if (total > (int64_t)INT32_MAX) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_dev: more than 2^31 entries in one batch");
    b->d_f_pdf.ensure((size_t)std::max<int64_t>(1, total));
    b->d_f_weight.ensure((size_t)std::max<int64_t>(1, total));
    if (total > 0)
      fb_frame_fill_launch(b->d_e_utt.p, b->d_f_pdf_at.p, b->d_f_pdfs.p, n_utt, max_T, b->d_occ.p, b->d_e_sums.p, b->d_f_off.p,
                           b->d_f_pdf.p, b->d_f_weight.p, st);
    b->f_total = total;
    b->frame_entries_shape[0] = (int32_t)total;
    b->frame_entries_shape[2] = ((max_T + FBF_THREADS - 1) / FBF_THREADS) * n_utt;
    b->frame_entries_shape[3] = (int32_t)scan_blocks;
    b->frame_entries_shape[4] = total > 0 ? b->frame_entries_shape[2] : 0;
    b->f_built = b->s_built = true;
    *n_entries = total;
    *d_off = b->d_f_off.p;
    *d_pdf = b->d_f_pdf.p;
    *d_weight = b->d_f_weight.p;
  });
}

aasr_status aasr_fb_batch_frame_entries_host(aasr_fb_batch *b, int64_t *off, int32_t *pdf, double *weight) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_host: null argument");
    if (!b->f_built) raise(AASR_ERR_INVALID, "aasr_fb_batch_frame_entries_host: call aasr_fb_batch_frame_entries_dev first");
    const size_t total = (size_t)b->f_total;
    if (off) AASR_HIP(hipMemcpyAsync(off, b->d_f_off.p, ((size_t)b->f_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, b->e_stream));
    if (pdf && total) AASR_HIP(hipMemcpyAsync(pdf, b->d_f_pdf.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, b->e_stream));
    if (weight && total) AASR_HIP(hipMemcpyAsync(weight, b->d_f_weight.p, total * sizeof(double), hipMemcpyDeviceToHost, b->e_stream));
    AASR_HIP(hipStreamSynchronize(b->e_stream));
  });
}

void aasr_debug_fb_frame_entries_shape(const aasr_fb_batch *b, int32_t *out) {
  if (!b || !out) return;
  std::copy(b->frame_entries_shape, b->frame_entries_shape + 5, out);
}

void aasr_debug_fb_entries_shape(const aasr_fb_batch *b, int32_t *out) {
  if (!b || !out) return;
  std::copy(b->entries_shape, b->entries_shape + 5, out);
}

}  // extern "C"

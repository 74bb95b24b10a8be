// fst_search.cc -- the handles of the FST decoder (aasr_fstnet_*, aasr_fst_durations_*, aasr_fst_batch_*): the network
// and the duration table of a batch on the device, one launch of k_fst_search over its utterances (fst_search.h), the
// results and, on request, every final token with its words read back through the history table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"
#include "fst_conf.h"
#include "fst_net.h"
#include "fst_search.h"

using namespace aasr;

struct aasr_fst_batch {
  aasr_fst_options opt{};  // capacities resolved
  const aasr_fstnet *net = nullptr;
  int32_t n = 0, D = 0, cap_tok = 0, cap_words = 0, n_pdf_table = 0;
  std::vector<int32_t> T;
  std::vector<int64_t> row0;
  std::vector<FstResult> result;
  std::vector<int32_t> res_words;
  std::vector<int32_t> dur_slot;
  bool synced = false, launched = false;
  hipStream_t sync_stream = nullptr;
  DevBuf<int32_t> d_net_i, d_T, d_dur_slot, d_tok_i, d_cand_i, d_res_words;
  DevBuf<int64_t> d_row0;
  DevBuf<float> d_net_f, d_dur_table, d_tok_f, d_cand_f, d_decode;
  DevBuf<unsigned long long> d_u64;
  DevBuf<FstResult> d_result;
  int32_t decode_bytes = 0;
  int64_t bytes = 0;
  FstParams p{};
};

namespace {

int32_t pow2_at_least(int64_t v) {
  int64_t p = 16;
  while (p < v && p < (1ll << 30)) p <<= 1;
  return (int32_t)p;
}

}  // namespace

namespace aasr {

const FstParams &fst_batch_params(const aasr_fst_batch *b) { return b->p; }

void fst_decode_table(int32_t lnabytes, std::vector<float> &dec) {  // LnaReaderCircular.cc:180-198, the division in double
  dec.resize(lnabytes == 2 ? 65536 : 256);
  for (size_t i = 0; i < dec.size(); i++) dec[i] = lnabytes == 2 ? (float)((double)(int)i / -1820.0) : (float)((double)(int)i / -24.0);
}

// the n tokens of utterance u by descending log-probability, their words read back through the history table
void fst_tokens_read(const char *who, const FstParams &p, int32_t u, int32_t n, hipStream_t st, int32_t *node, float *logprob,
                     int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words) {
  word_begin[0] = 0;
  if (n == 0) return;
  const size_t ct = (size_t)p.cap_tok, ch = (size_t)p.cap_hist;
  std::vector<int32_t> tn((size_t)n), td((size_t)n), th((size_t)n);
  std::vector<float> tl((size_t)n);
  std::vector<unsigned long long> hk(ch);
  AASR_HIP(hipMemcpyAsync(tn.data(), p.t_node + (size_t)u * ct, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  AASR_HIP(hipMemcpyAsync(td.data(), p.t_dur + (size_t)u * ct, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  AASR_HIP(hipMemcpyAsync(th.data(), p.t_hist + (size_t)u * ct, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  AASR_HIP(hipMemcpyAsync(tl.data(), p.t_lp + (size_t)u * ct, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  AASR_HIP(hipMemcpyAsync(hk.data(), p.h_key + (size_t)u * ch, ch * 8, hipMemcpyDeviceToHost, st));
  AASR_HIP(hipStreamSynchronize(st));
  // descending log-probability, the earlier token first among equals (the order of the reference's list)
  std::vector<int32_t> order((size_t)n);
  for (int32_t i = 0; i < n; i++) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return tl[(size_t)x] > tl[(size_t)y]; });
  int32_t at = 0;
  std::vector<int32_t> chain;
  for (int32_t j = 0; j < n; j++) {
    const int32_t i = order[(size_t)j];
    node[j] = tn[(size_t)i];
    logprob[j] = tl[(size_t)i];
    dur[j] = td[(size_t)i];
    chain.clear();
    for (int64_t h = th[(size_t)i]; h != 0;) {
      if (h < 0 || h > (int64_t)ch || hk[(size_t)h - 1] == ~0ull || chain.size() > (size_t)p.cap_words)
        raise(AASR_ERR_INVALID, "%s: utterance %d has a broken history chain", who, u);
      chain.push_back((int32_t)(uint32_t)hk[(size_t)h - 1]);
      h = (int64_t)(hk[(size_t)h - 1] >> 32);
    }
    if (words) {
      if (at + (int32_t)chain.size() > cap_words) raise(AASR_ERR_INVALID, "%s: room for %d words", who, cap_words);
      std::copy(chain.rbegin(), chain.rend(), words + at);
    }
    at += (int32_t)chain.size();
    word_begin[j + 1] = at;
  }
}

}  // namespace aasr

extern "C" {

aasr_status aasr_fstnet_create_from_file(const char *path, aasr_fstnet **out) {
  return guarded([&] {
    if (!path || !out) raise(AASR_ERR_INVALID, "aasr_fstnet_create_from_file: null argument");
    *out = nullptr;
    std::unique_ptr<aasr_fstnet> n(new aasr_fstnet());
    fst_net_read(path, *n);
    *out = n.release();
  });
}

void aasr_fstnet_destroy(aasr_fstnet *net) { delete net; }
int32_t aasr_fstnet_num_nodes(const aasr_fstnet *net) { return net ? (int32_t)net->node_pdf.size() : -1; }
int32_t aasr_fstnet_num_arcs(const aasr_fstnet *net) { return net ? (int32_t)net->arc_tgt.size() : -1; }
int32_t aasr_fstnet_num_symbols(const aasr_fstnet *net) { return net ? (int32_t)net->symbols.size() : -1; }
int32_t aasr_fstnet_initial(const aasr_fstnet *net) { return net ? net->initial : -1; }
int32_t aasr_fstnet_max_pdf(const aasr_fstnet *net) { return net ? net->max_pdf : -1; }
const char *aasr_fstnet_symbol(const aasr_fstnet *net, int32_t id) {
  return net && id >= 0 && id < (int32_t)net->symbols.size() ? net->symbols[(size_t)id].c_str() : nullptr;
}

aasr_status aasr_fstnet_arrays(const aasr_fstnet *net, int32_t *arc_begin, int32_t *arc_tgt, float *arc_logprob,
                               int32_t *arc_word, int32_t *node_pdf, int32_t *node_end) {
  return guarded([&] {
    if (!net) raise(AASR_ERR_INVALID, "aasr_fstnet_arrays: null argument");
    if (arc_begin) std::copy(net->arc_begin.begin(), net->arc_begin.end(), arc_begin);
    if (arc_tgt) std::copy(net->arc_tgt.begin(), net->arc_tgt.end(), arc_tgt);
    if (arc_logprob) std::copy(net->arc_lp.begin(), net->arc_lp.end(), arc_logprob);
    if (arc_word) std::copy(net->arc_word.begin(), net->arc_word.end(), arc_word);
    if (node_pdf) std::copy(net->node_pdf.begin(), net->node_pdf.end(), node_pdf);
    if (node_end) std::copy(net->node_end.begin(), net->node_end.end(), node_end);
  });
}

void aasr_fst_default_options(aasr_fst_options *o) {
  if (!o) return;
  *o = aasr_fst_options();
  o->beam = 2600.0f;  // FstSearch_tmpl.hh:19-22
  o->token_limit = 5000;
  o->duration_scale = 3.0f;
  o->transition_scale = 1.0f;
}

aasr_status aasr_fst_durations_read(const char *path, aasr_fst_durations **out) {
  return guarded([&] {
    if (!path || !out) raise(AASR_ERR_INVALID, "aasr_fst_durations_read: null argument");
    *out = nullptr;
    std::unique_ptr<aasr_fst_durations> d(new aasr_fst_durations());
    fst_durations_read(path, *d);
    *out = d.release();
  });
}

void aasr_fst_durations_destroy(aasr_fst_durations *dur) { delete dur; }
int32_t aasr_fst_durations_num_states(const aasr_fst_durations *dur) { return dur ? dur->n : -1; }
float aasr_fst_durations_logprob(const aasr_fst_durations *dur, int32_t dur_by_state, int32_t pdf, int32_t d) {
  return fst_duration_logprob(dur, dur_by_state != 0, pdf, d);
}

aasr_status aasr_fst_batch_create(const aasr_fstnet *net, const aasr_fst_durations *dur, const aasr_fst_options *opt,
                                  int32_t n_utt, const int32_t *n_frames, aasr_fst_batch **out) {
  return guarded([&] {
    if (!net || !opt || !out || n_utt < 0 || (n_utt > 0 && !n_frames)) raise(AASR_ERR_INVALID, "aasr_fst_batch_create: null argument");
    *out = nullptr;
    if (!(opt->beam >= 0) || !std::isfinite(opt->beam)) raise(AASR_ERR_INVALID, "aasr_fst_batch_create: the beam must be finite and not negative");
    if (opt->token_limit < 0) raise(AASR_ERR_INVALID, "aasr_fst_batch_create: the token limit must not be negative");
    if (!std::isfinite(opt->duration_scale) || !std::isfinite(opt->transition_scale))
      raise(AASR_ERR_INVALID, "aasr_fst_batch_create: the scales must be finite");
    if (opt->cap_candidates < 0 || opt->cap_recomb < 0 || opt->cap_history < 0)
      raise(AASR_ERR_INVALID, "aasr_fst_batch_create: negative capacity");
    int32_t D = 0;
    for (int u = 0; u < n_utt; u++) {
      if (n_frames[u] < 0) raise(AASR_ERR_INVALID, "aasr_fst_batch_create: utterance %d has %d frames", u, n_frames[u]);
      D = std::max(D, n_frames[u]);
    }
    require_device();
    std::unique_ptr<aasr_fst_batch> b(new aasr_fst_batch());
    b->net = net;
    b->n = n_utt;
    b->D = D;
    b->T.assign(n_frames, n_frames + n_utt);
    b->opt = *opt;
    // capacities: a frame's candidates are at most (limit + 1) tokens x the largest out-degree; the default stops at eight
    // times the network's arcs (at least 65536), beyond which a rerun doubles it.  The recombination table holds one entry
    // per kept candidate at the most: twice the candidates keeps it half empty.  The history table grows by at most one entry
    // per word-carrying candidate kept: frames x tokens / 4 between 2^12 and 2^20 entries.
    const int64_t K = (int64_t)opt->token_limit + 1;
    const int64_t n_arcs = (int64_t)net->arc_tgt.size();
    if (b->opt.cap_candidates == 0)
      b->opt.cap_candidates = (int32_t)std::max<int64_t>(16, std::min<int64_t>(K * std::max(1, net->max_degree), std::max<int64_t>(65536, 8 * n_arcs)));
    if (b->opt.cap_recomb == 0) b->opt.cap_recomb = pow2_at_least(2 * (int64_t)b->opt.cap_candidates);
    if (b->opt.cap_history == 0)
      b->opt.cap_history = pow2_at_least(std::min<int64_t>(1 << 20, std::max<int64_t>(1 << 12, (int64_t)D * std::min<int64_t>(K, b->opt.cap_candidates) / 4)));
    if ((b->opt.cap_recomb & (b->opt.cap_recomb - 1)) || (b->opt.cap_history & (b->opt.cap_history - 1)))
      raise(AASR_ERR_INVALID, "aasr_fst_batch_create: the table capacities must be powers of two");
    b->cap_tok = (int32_t)std::min<int64_t>(K, b->opt.cap_candidates);
    b->cap_words = D + 1;
    // network
    const size_t nn = net->node_pdf.size(), na = net->arc_tgt.size();
    std::vector<int32_t> ni;
    ni.insert(ni.end(), net->arc_begin.begin(), net->arc_begin.end());
    ni.insert(ni.end(), net->node_pdf.begin(), net->node_pdf.end());
    ni.insert(ni.end(), net->node_end.begin(), net->node_end.end());
    ni.insert(ni.end(), net->arc_tgt.begin(), net->arc_tgt.end());
    ni.insert(ni.end(), net->arc_word.begin(), net->arc_word.end());
    b->d_net_i.upload(ni.data(), ni.size());
    std::vector<float> nf(net->arc_lp);
    if (nf.empty()) nf.push_back(0);
    b->d_net_f.upload(nf.data(), nf.size());
    // durations: the table covers the pdfs the network can name
    std::vector<float> table;
    b->n_pdf_table = net->max_pdf + 1;
    if (dur) {
      fst_dur_table(dur, opt->dur_by_state != 0, b->n_pdf_table, D, b->dur_slot, table);
      if (b->dur_slot.empty()) b->dur_slot.push_back(-1);
      if (table.empty()) table.push_back(0);
      b->d_dur_slot.upload(b->dur_slot.data(), b->dur_slot.size());
      b->d_dur_table.upload(table.data(), table.size());
    }
    const size_t nu = (size_t)std::max(1, n_utt);
    const size_t ct = (size_t)b->cap_tok, cc = (size_t)b->opt.cap_candidates, cr = (size_t)b->opt.cap_recomb, ch = (size_t)b->opt.cap_history;
    b->d_T.upload(b->T.empty() ? &D : b->T.data(), nu);
    b->d_row0.alloc(nu);
    b->d_tok_i.alloc(nu * (4 * ct + 1));
    b->d_tok_f.alloc(nu * ct);
    b->d_cand_i.alloc(nu * 5 * cc);
    b->d_cand_f.alloc(nu * cc);
    b->d_u64.alloc(nu * (cc + 2 * cr + ch));
    b->d_res_words.alloc(nu * (size_t)b->cap_words);
    b->d_result.alloc(nu);
    b->result.assign((size_t)n_utt, FstResult{});
    b->res_words.assign(nu * (size_t)b->cap_words, 0);
    b->bytes = (int64_t)(ni.size() * 4 + nf.size() * 4 + table.size() * 4 + b->dur_slot.size() * 4 +
                         nu * ((4 * ct + 1) * 4 + ct * 4 + 6 * cc * 4 + (cc + 2 * cr + ch) * 8 + (size_t)b->cap_words * 4 + sizeof(FstResult) + 16));
    FstParams &p = b->p;
    p.arc_begin = b->d_net_i.p;
    p.node_pdf = p.arc_begin + nn + 1;
    p.node_end = p.node_pdf + nn;
    p.arc_tgt = p.node_end + nn;
    p.arc_word = p.arc_tgt + na;
    p.arc_lp = b->d_net_f.p;
    p.initial = net->initial;
    p.n_frames = b->d_T.p;
    p.row0 = b->d_row0.p;
    p.dur_slot = dur ? b->d_dur_slot.p : nullptr;
    p.dur_table = dur ? b->d_dur_table.p : nullptr;
    p.D = D;
    p.beam = opt->beam;
    p.duration_scale = opt->duration_scale;
    p.transition_scale = opt->transition_scale;
    p.token_limit = opt->token_limit;
    p.cap_tok = b->cap_tok;
    p.cap_cand = b->opt.cap_candidates;
    p.cap_recomb = b->opt.cap_recomb;
    p.cap_hist = b->opt.cap_history;
    p.cap_words = b->cap_words;
    p.t_node = b->d_tok_i.p;
    p.t_dur = p.t_node + nu * ct;
    p.t_hist = p.t_dur + nu * ct;
    p.t_off = p.t_hist + nu * ct;
    p.t_lp = b->d_tok_f.p;
    p.c_lp = b->d_cand_f.p;
    p.c_tok = b->d_cand_i.p;
    p.c_node = p.c_tok + nu * cc;
    p.c_dur = p.c_node + nu * cc;
    p.c_hist = p.c_dur + nu * cc;
    p.c_slot = p.c_hist + nu * cc;
    p.w_key = b->d_u64.p;
    p.r_key = p.w_key + nu * cc;
    p.r_val = p.r_key + nu * cr;
    p.h_key = p.r_val + nu * cr;
    p.res_words = b->d_res_words.p;
    p.result = b->d_result.p;
    *out = b.release();
  });
}

void aasr_fst_batch_destroy(aasr_fst_batch *b) { delete b; }
int64_t aasr_fst_batch_device_bytes(const aasr_fst_batch *b) { return b ? b->bytes : -1; }
void aasr_fst_batch_options(const aasr_fst_batch *b, aasr_fst_options *out) {
  if (b && out) *out = b->opt;
}

aasr_status aasr_fst_batch_dev(aasr_fst_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                               const int64_t *row0, void *stream) {
  return guarded([&] {
    if (!b || (b->n > 0 && !row0)) raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: null argument");
    if (lnabytes != 1 && lnabytes != 2 && lnabytes != 4) raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: lnabytes %d is not 1, 2 or 4", lnabytes);
    if (n_models < 1) raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: %d models", n_models);
    if (b->net->max_pdf >= n_models)
      raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: the network names pdf %d, the acoustics have %d models", b->net->max_pdf, n_models);
    const hipStream_t st = (hipStream_t)stream;
    b->synced = false;
    b->row0.assign(row0, row0 + b->n);
    for (int u = 0; u < b->n; u++) {
      if (row0[u] < 0 || row0[u] + b->T[(size_t)u] > n_rows)
        raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: utterance %d reads rows %lld .. %lld of %lld", u, (long long)row0[u],
              (long long)(row0[u] + b->T[(size_t)u]), (long long)n_rows);
    }
    if (b->n == 0) return;
    if (!d_lna && n_rows > 0) raise(AASR_ERR_INVALID, "aasr_fst_batch_dev: null acoustics");
    if (lnabytes != 4 && b->decode_bytes != lnabytes) {
      std::vector<float> dec;
      fst_decode_table(lnabytes, dec);
      b->d_decode.upload(dec.data(), dec.size());
      b->decode_bytes = lnabytes;
    }
    AASR_HIP(hipMemcpyAsync(b->d_row0.p, b->row0.data(), b->row0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    FstParams p = b->p;
    p.lna = (const uint8_t *)d_lna;
    p.decode = b->d_decode.p;
    p.lnabytes = lnabytes;
    p.n_models = n_models;
    fst_search_launch(p, b->n, st);
    AASR_HIP(hipGetLastError());
    b->launched = true;  // (row0 is the batch's own copy: nothing of the caller's is read after this call returns)
  });
}

aasr_status aasr_fst_batch_sync(aasr_fst_batch *b, void *stream, int32_t *n_overflow) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_fst_batch_sync: null argument");
    if (!b->launched && b->n > 0) raise(AASR_ERR_INVALID, "aasr_fst_batch_sync: call aasr_fst_batch_dev first");
    const hipStream_t st = (hipStream_t)stream;
    if (b->n > 0) {
      AASR_HIP(hipMemcpyAsync(b->result.data(), b->d_result.p, b->result.size() * sizeof(FstResult), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(b->res_words.data(), b->d_res_words.p, b->res_words.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipStreamSynchronize(st));
    }
    b->synced = true;
    b->sync_stream = st;
    int over = 0;
    for (const FstResult &r : b->result) over += r.status >= FST_OVERFLOW_CANDIDATES;
    if (n_overflow) *n_overflow = over;
  });
}

aasr_status aasr_fst_batch_result(const aasr_fst_batch *b, int32_t u, int32_t *status, float *logprob, float *best_logprob,
                                  float *best_final_logprob, int32_t *n_words, int32_t *words, int32_t cap_words,
                                  int32_t *n_tokens) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n) raise(AASR_ERR_INVALID, "aasr_fst_batch_result: bad argument");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fst_batch_result: call aasr_fst_batch_sync first");
    const FstResult &r = b->result[(size_t)u];
    if (r.n_words < 0 || r.n_words > b->cap_words) raise(AASR_ERR_INVALID, "aasr_fst_batch_result: utterance %d reports %d words", u, r.n_words);
    if (status) *status = r.status;
    if (logprob) *logprob = r.logprob;
    if (best_logprob) *best_logprob = r.best_lp;
    if (best_final_logprob) *best_final_logprob = r.best_final_lp;
    if (n_words) *n_words = r.n_words;
    if (n_tokens) *n_tokens = r.n_tokens;
    if (words) {
      if (cap_words < r.n_words) raise(AASR_ERR_INVALID, "aasr_fst_batch_result: %d words, room for %d", r.n_words, cap_words);
      const int32_t *w = b->res_words.data() + (size_t)u * (size_t)b->cap_words;
      for (int32_t i = 0; i < r.n_words; i++) {
        if (w[i] < 0 || w[i] >= (int32_t)b->net->symbols.size()) raise(AASR_ERR_INVALID, "aasr_fst_batch_result: utterance %d has word id %d", u, w[i]);
        words[i] = w[i];
      }
    }
  });
}

aasr_status aasr_fst_batch_tokens(aasr_fst_batch *b, int32_t u, int32_t cap_tokens, int32_t *node, float *logprob, int32_t *dur,
                                  int32_t *word_begin, int32_t cap_words, int32_t *words) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n || !node || !logprob || !dur || !word_begin) raise(AASR_ERR_INVALID, "aasr_fst_batch_tokens: bad argument");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fst_batch_tokens: call aasr_fst_batch_sync first");
    const FstResult &r = b->result[(size_t)u];
    const int32_t n = r.n_tokens;
    if (n < 0 || n > b->cap_tok) raise(AASR_ERR_INVALID, "aasr_fst_batch_tokens: utterance %d reports %d tokens", u, n);
    if (cap_tokens < n) raise(AASR_ERR_INVALID, "aasr_fst_batch_tokens: %d tokens, room for %d", n, cap_tokens);
    fst_tokens_read("aasr_fst_batch_tokens", b->p, u, n, b->sync_stream, node, logprob, dur, word_begin, cap_words, words);
  });
}

}  // extern "C"

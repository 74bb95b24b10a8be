// fst_conf.cc -- the confidence handle of the FST decoder (aasr_fst_conf_batch_*): one aasr_fst_batch per network, the
// frame-best pass and the token records on the device (fst_conf.h), and the reference's scalar formulas with the edit
// distance on the host (decoder/src/FstConfidence.cc restated; include/aasr.h states them).  Floating-point contraction
// is off in this unit: every float operation of the formulas is rounded on its own, as the reference's are.
#pragma STDC FP_CONTRACT OFF
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "fst_conf.h"
#include "fst_net.h"

using namespace aasr;

struct aasr_fst_conf_batch {
  aasr_fst_conf_options opt{};
  const aasr_fstnet *net[2] = {nullptr, nullptr};
  aasr_fst_batch *inner[2] = {nullptr, nullptr};  // grammar, phone loop
  int32_t n = 0;
  int64_t total = 0;
  std::vector<int32_t> T;
  std::vector<int64_t> frame_off, row0;
  std::vector<FstConfRecord> rec[2];
  std::vector<float> sum;
  std::vector<aasr_fst_conf_result> result;
  std::vector<std::string> text[2];
  bool synced = false, launched = false, frame_best_done = false;
  DevBuf<int64_t> d_frame_off, d_row0;
  DevBuf<float> d_frame_best, d_sum, d_decode;
  DevBuf<FstConfRecord> d_rec[2];
  int32_t decode_bytes = 0;
  ~aasr_fst_conf_batch() {
    aasr_fst_batch_destroy(inner[0]);
    aasr_fst_batch_destroy(inner[1]);
  }
};

namespace {

void ok(aasr_status s) {
  if (s != AASR_OK) raise(s, "%s", last_error().c_str());
}

std::string remove_junk(const char *s, size_t n) {  // spaces and repeats of the last kept byte go; a space does not end a run
  std::string out;
  char prev = ' ';
  for (size_t i = 0; i < n; i++) {
    if (s[i] == ' ' || s[i] == prev) continue;
    prev = s[i];
    out += s[i];
  }
  return out;
}

// Levenshtein distance over bytes, two rows
int32_t edit_distance(const std::string &a, const std::string &b) {
  std::vector<int32_t> prev(b.size() + 1), cur(b.size() + 1);
  for (size_t j = 0; j <= b.size(); j++) prev[j] = (int32_t)j;
  for (size_t i = 0; i < a.size(); i++) {
    cur[0] = (int32_t)i + 1;
    for (size_t j = 0; j < b.size(); j++) cur[j + 1] = std::min(std::min(cur[j], prev[j + 1]) + 1, prev[j] + (a[i] != b[j]));
    prev.swap(cur);
  }
  return prev[b.size()];
}

// FstConfidence::grammar_token_and_best_acu_confidence and the two result_and_confidence; r holds the raw inputs
void formulas(aasr_fst_conf_result &r, int32_t n_words, const std::string &grammar, const std::string *ploop) {
  const float frames = (float)r.frames;
  r.best_acu_conf = 1.5f - 0.25f * (-r.best_final_logprob + r.best_acu_score) / frames;
  if (n_words == 0)
    r.token_conf = FSTC_NONE;
  else
    r.token_conf = std::max(0.0f, std::min(1.0f, 0.2f - 5.0f * (-r.best_final_logprob + r.best_different_logprob) / frames));
  if (!ploop) {
    r.ploop_conf = r.edit_conf = 0.0f;
    r.confidence = (float)(0.5 * (r.token_conf + r.best_acu_conf));
    return;
  }
  r.ploop_conf = std::min(1.0f, 1.0f - 0.25f * (-r.grammar_logprob + r.ploop_logprob) / frames);
  const std::string cg = remove_junk(grammar.data(), grammar.size()), cp = remove_junk(ploop->data(), ploop->size());
  r.edit_conf = std::max(0.0f, 1.0f - float(edit_distance(cg, cp)) / (float)cg.size());
  r.confidence = (std::min(1.0f, r.ploop_conf) + 20.0f * std::min(1.0f, r.token_conf) + 5.0f * std::min(1.0f, r.edit_conf) +
                  std::min(1.0f, r.best_acu_conf)) / 27.0f;
}

void check_dev_args(const aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows, const int64_t *row0,
                    const char *who) {
  if (!b || (b->n > 0 && !row0)) raise(AASR_ERR_INVALID, "%s: null argument", who);
  if (lnabytes != 1 && lnabytes != 2 && lnabytes != 4) raise(AASR_ERR_INVALID, "%s: lnabytes %d is not 1, 2 or 4", who, lnabytes);
  if (n_models < 1) raise(AASR_ERR_INVALID, "%s: %d models", who, n_models);
  if ((uintptr_t)d_lna % (uintptr_t)lnabytes) raise(AASR_ERR_INVALID, "%s: the acoustics are not aligned to %d bytes", who, lnabytes);
  for (int u = 0; u < b->n; u++) {
    if (row0[u] < 0 || row0[u] + b->T[(size_t)u] > n_rows)
      raise(AASR_ERR_INVALID, "%s: utterance %d reads rows %lld .. %lld of %lld", who, u, (long long)row0[u],
            (long long)(row0[u] + b->T[(size_t)u]), (long long)n_rows);
  }
  if (b->n > 0 && !d_lna && n_rows > 0) raise(AASR_ERR_INVALID, "%s: null acoustics", who);
}

void queue_frame_best(aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, const int64_t *row0, hipStream_t st) {
  if (b->n == 0) return;
  if (lnabytes != 4 && b->decode_bytes != lnabytes) {
    std::vector<float> dec;
    fst_decode_table(lnabytes, dec);
    b->d_decode.upload(dec.data(), dec.size());
    b->decode_bytes = lnabytes;
  }
  b->row0.assign(row0, row0 + b->n);
  AASR_HIP(hipMemcpyAsync(b->d_row0.p, b->row0.data(), b->row0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  FstFrameBestParams p{};
  p.lna = (const uint8_t *)d_lna;
  p.decode = b->d_decode.p;
  p.lnabytes = lnabytes;
  p.n_models = n_models;
  p.n_utt = b->n;
  p.row0 = b->d_row0.p;
  p.frame_off = b->d_frame_off.p;
  p.frame_best = b->d_frame_best.p;
  p.sum = b->d_sum.p;
  fst_frame_best_launch(p, b->total, st);
  AASR_HIP(hipGetLastError());
  b->frame_best_done = true;
}

}  // namespace

namespace aasr {

void fst_conf_check_options(const aasr_fst_options &o, const char *who, const char *which) {
  if (!(o.beam >= 0) || !std::isfinite(o.beam)) raise(AASR_ERR_INVALID, "%s: the %s beam must be finite and not negative", who, which);
  if (o.token_limit < 0) raise(AASR_ERR_INVALID, "%s: the %s token limit must not be negative", who, which);
  if (!std::isfinite(o.duration_scale) || !std::isfinite(o.transition_scale)) raise(AASR_ERR_INVALID, "%s: the %s scales must be finite", who, which);
  if (o.cap_candidates < 0 || o.cap_recomb < 0 || o.cap_history < 0) raise(AASR_ERR_INVALID, "%s: negative %s capacity", who, which);
}

// a phone loop puts a symbol on every phone: far more of its candidates carry a word than a grammar's, so its derived
// history table holds frames x tokens entries (aasr_fst_batch_create: a quarter of that), between 2^12 and 2^21
int32_t fst_conf_phone_history(const aasr_fst_options &phone, int64_t longest) {
  int64_t K = (int64_t)phone.token_limit + 1;
  if (phone.cap_candidates > 0) K = std::min<int64_t>(K, phone.cap_candidates);
  int64_t cap = 1 << 12;
  while (cap < longest * K && cap < (1 << 21)) cap <<= 1;
  return (int32_t)cap;
}

bool fst_conf_finish(aasr_fst_conf_result &r, const int32_t status[2], const float logprob[2], const FstConfRecord &g, bool phone_loop,
                     float sum, const std::string &grammar, const std::string &ploop, const char *who, int32_t u) {
  r.grammar_status = status[0];
  r.phone_status = status[1];
  if (status[0] >= AASR_FST_OVERFLOW_CANDIDATES || status[1] >= AASR_FST_OVERFLOW_CANDIDATES) return true;
  if (g.has_final && std::memcmp(&g.best_final_lp, &logprob[0], sizeof(float)) != 0)
    raise(AASR_ERR_INVALID, "%s: utterance %d: the token record's best end-node token is not the search's", who, u);
  r.valid = 1;
  r.no_final = !g.has_final;
  r.grammar_logprob = logprob[0];
  r.ploop_logprob = logprob[1];
  r.best_final_logprob = g.best_final_lp;  // (-9999999.9f without an end-node token)
  r.best_different_logprob = g.best_different_lp;
  r.best_acu_score = phone_loop ? sum : 0.0f;
  formulas(r, g.has_final ? g.best_final_n_words : 0, grammar, phone_loop ? &ploop : nullptr);
  return false;
}

}  // namespace aasr

extern "C" {

void aasr_fst_conf_default_options(aasr_fst_conf_options *o) {
  if (!o) return;
  *o = aasr_fst_conf_options();
  aasr_fst_default_options(&o->grammar);
  aasr_fst_default_options(&o->phone);
}

aasr_status aasr_fst_conf_batch_create(const aasr_fstnet *grammar_net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                                       const aasr_fst_conf_options *opt, int32_t n_utt, const int32_t *n_frames,
                                       aasr_fst_conf_batch **out) {
  return guarded([&] {
    if (!opt || !out || n_utt < 0 || (n_utt > 0 && !n_frames)) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_create: null argument");
    *out = nullptr;
    if (!grammar_net) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_create: no grammar network");
    if (opt->phone_loop && !phone_net) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_create: phone_loop without a phone-loop network");
    fst_conf_check_options(opt->grammar, "aasr_fst_conf_batch_create", "grammar");
    fst_conf_check_options(opt->phone, "aasr_fst_conf_batch_create", "phone");
    for (int u = 0; u < n_utt; u++)
      if (n_frames[u] < 0) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_create: utterance %d has %d frames", u, n_frames[u]);
    require_device();
    std::unique_ptr<aasr_fst_conf_batch> b(new aasr_fst_conf_batch());
    b->opt = *opt;
    b->n = n_utt;
    b->T.assign(n_frames, n_frames + n_utt);
    b->net[0] = grammar_net;
    b->net[1] = opt->phone_loop ? phone_net : nullptr;
    ok(aasr_fst_batch_create(grammar_net, dur, &opt->grammar, n_utt, n_frames, &b->inner[0]));
    aasr_fst_batch_options(b->inner[0], &b->opt.grammar);
    if (opt->phone_loop) {
      aasr_fst_options phone = opt->phone;
      int64_t D = 0;
      for (int u = 0; u < n_utt; u++) D = std::max<int64_t>(D, n_frames[u]);
      if (phone.cap_history == 0) phone.cap_history = fst_conf_phone_history(phone, D);
      ok(aasr_fst_batch_create(phone_net, dur, &phone, n_utt, n_frames, &b->inner[1]));
      aasr_fst_batch_options(b->inner[1], &b->opt.phone);
    }
    b->frame_off.assign((size_t)n_utt + 1, 0);
    for (int u = 0; u < n_utt; u++) b->frame_off[(size_t)u + 1] = b->frame_off[(size_t)u] + n_frames[u];
    b->total = b->frame_off[(size_t)n_utt];
    const size_t nu = (size_t)std::max(1, n_utt);
    b->d_frame_off.upload(b->frame_off.data(), b->frame_off.size());
    b->d_row0.alloc(nu);
    b->d_frame_best.alloc((size_t)std::max<int64_t>(1, b->total));
    b->d_sum.alloc(nu);
    b->d_rec[0].alloc(nu);
    b->d_rec[1].alloc(nu);
    b->sum.assign((size_t)n_utt, 0.0f);
    b->rec[0].assign((size_t)n_utt, FstConfRecord{});
    b->rec[1].assign((size_t)n_utt, FstConfRecord{});
    b->result.assign((size_t)n_utt, aasr_fst_conf_result{});
    b->text[0].assign((size_t)n_utt, std::string());
    b->text[1].assign((size_t)n_utt, std::string());
    *out = b.release();
  });
}

void aasr_fst_conf_batch_destroy(aasr_fst_conf_batch *b) { delete b; }
void aasr_fst_conf_batch_options(const aasr_fst_conf_batch *b, aasr_fst_conf_options *out) {
  if (b && out) *out = b->opt;
}
aasr_fst_batch *aasr_fst_conf_batch_grammar(aasr_fst_conf_batch *b) { return b ? b->inner[0] : nullptr; }
aasr_fst_batch *aasr_fst_conf_batch_phone(aasr_fst_conf_batch *b) { return b ? b->inner[1] : nullptr; }

aasr_status aasr_fst_conf_batch_frame_best_dev(aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models,
                                               int64_t n_rows, const int64_t *row0, void *stream) {
  return guarded([&] {
    check_dev_args(b, d_lna, lnabytes, n_models, n_rows, row0, "aasr_fst_conf_batch_frame_best_dev");
    queue_frame_best(b, d_lna, lnabytes, n_models, row0, (hipStream_t)stream);
  });
}

aasr_status aasr_fst_conf_batch_dev(aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                                    const int64_t *row0, void *stream) {
  return guarded([&] {
    check_dev_args(b, d_lna, lnabytes, n_models, n_rows, row0, "aasr_fst_conf_batch_dev");
    const hipStream_t st = (hipStream_t)stream;
    b->synced = false;
    ok(aasr_fst_batch_dev(b->inner[0], d_lna, lnabytes, n_models, n_rows, row0, stream));
    if (b->inner[1]) ok(aasr_fst_batch_dev(b->inner[1], d_lna, lnabytes, n_models, n_rows, row0, stream));
    if (b->inner[1]) queue_frame_best(b, d_lna, lnabytes, n_models, row0, st);  // (plain FstConfidence never uses the sum)
    for (int k = 0; k < 2; k++)
      if (b->inner[k]) fst_conf_tokens_launch(fst_batch_params(b->inner[k]), b->d_rec[k].p, b->n, st);
    AASR_HIP(hipGetLastError());
    b->launched = true;
  });
}

aasr_status aasr_fst_conf_batch_sync(aasr_fst_conf_batch *b, void *stream, int32_t *n_overflow) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_sync: null argument");
    if (!b->launched && b->n > 0) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_sync: call aasr_fst_conf_batch_dev first");
    const hipStream_t st = (hipStream_t)stream;
    if (b->n > 0) {
      for (int k = 0; k < 2; k++)
        if (b->inner[k])
          AASR_HIP(hipMemcpyAsync(b->rec[k].data(), b->d_rec[k].p, b->rec[k].size() * sizeof(FstConfRecord), hipMemcpyDeviceToHost, st));
      if (b->inner[1]) AASR_HIP(hipMemcpyAsync(b->sum.data(), b->d_sum.p, b->sum.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    int32_t over[2] = {0, 0};
    for (int k = 0; k < 2; k++)
      if (b->inner[k]) ok(aasr_fst_batch_sync(b->inner[k], stream, &over[k]));  // (waits for the stream)
    int32_t n_over = 0;
    std::vector<int32_t> words;
    for (int32_t u = 0; u < b->n; u++) {
      aasr_fst_conf_result r{};
      r.frames = b->T[(size_t)u];
      int32_t status[2] = {AASR_FST_OK, AASR_FST_OK};
      float logprob[2] = {-1.0f, -1.0f};
      for (int k = 0; k < 2; k++) {
        b->text[k][(size_t)u].clear();
        if (!b->inner[k]) continue;
        int32_t nw = 0;
        words.assign((size_t)r.frames + 1, 0);
        ok(aasr_fst_batch_result(b->inner[k], u, &status[k], &logprob[k], nullptr, nullptr, &nw, words.data(), (int32_t)words.size(), nullptr));
        std::string &t = b->text[k][(size_t)u];
        for (int32_t i = 0; i < nw; i++) {
          if (i) t += ' ';
          t += b->net[k]->symbols[(size_t)words[(size_t)i]];
        }
      }
      if (fst_conf_finish(r, status, logprob, b->rec[0][(size_t)u], b->inner[1] != nullptr, b->sum[(size_t)u], b->text[0][(size_t)u],
                          b->text[1][(size_t)u], "aasr_fst_conf_batch_sync", u))
        n_over++;
      b->result[(size_t)u] = r;
    }
    b->synced = true;
    if (n_overflow) *n_overflow = n_over;
  });
}

aasr_status aasr_fst_conf_batch_result(const aasr_fst_conf_batch *b, int32_t u, aasr_fst_conf_result *out) {
  return guarded([&] {
    if (!b || !out || u < 0 || u >= b->n) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_result: bad argument");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_result: call aasr_fst_conf_batch_sync first");
    const aasr_fst_conf_result &r = b->result[(size_t)u];
    *out = r;
    if (b->opt.verbose && r.valid && b->inner[1]) {  // FstConfidenceWithPhoneLoop::result_and_confidence's verbose block
      fprintf(stderr, "%s:\n\tToken: %.4f\n", b->text[0][(size_t)u].c_str(), r.token_conf);
      fprintf(stderr, "\tPloop: %.4f\n", r.ploop_conf);
      fprintf(stderr, "\tEdit: %.4f\n", r.edit_conf);
      fprintf(stderr, "\tBacu: %.4f\n", r.best_acu_conf);
      fprintf(stderr, "\tTotal: %.4f\n\n", r.confidence);
    }
  });
}

aasr_status aasr_fst_conf_batch_record(const aasr_fst_conf_batch *b, int32_t u, int32_t phone, int32_t *has_final, int32_t *n_words,
                                       int32_t *has_different, float *best_final_logprob, float *best_different_logprob) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n || (phone != 0 && phone != 1) || !b->inner[phone]) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_record: bad argument");
    if (!b->synced) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_record: call aasr_fst_conf_batch_sync first");
    const FstConfRecord &r = b->rec[phone][(size_t)u];
    if (has_final) *has_final = r.has_final;
    if (n_words) *n_words = r.best_final_n_words;
    if (has_different) *has_different = r.has_different;
    if (best_final_logprob) *best_final_logprob = r.best_final_lp;
    if (best_different_logprob) *best_different_logprob = r.best_different_lp;
  });
}

aasr_status aasr_fst_conf_batch_frame_best(aasr_fst_conf_batch *b, int32_t u, void *stream, float *best, int32_t cap, float *sum) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_frame_best: bad argument");
    if (!b->frame_best_done) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_frame_best: no frame-best pass was queued");
    const int32_t T = b->T[(size_t)u];
    if (best && cap < T) raise(AASR_ERR_INVALID, "aasr_fst_conf_batch_frame_best: %d frames, room for %d", T, cap);
    const hipStream_t st = (hipStream_t)stream;
    if (best && T > 0)
      AASR_HIP(hipMemcpyAsync(best, b->d_frame_best.p + b->frame_off[(size_t)u], (size_t)T * sizeof(float), hipMemcpyDeviceToHost, st));
    if (sum) AASR_HIP(hipMemcpyAsync(sum, b->d_sum.p + u, sizeof(float), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
  });
}

int32_t aasr_fst_conf_remove_junk(const char *s, int32_t n, char *out, int32_t cap) {
  if (n < 0 || (n > 0 && !s)) return -1;
  const std::string c = remove_junk(s, (size_t)n);
  if ((int32_t)c.size() > cap || (c.size() > 0 && !out)) return -1;
  std::copy(c.begin(), c.end(), out);
  return (int32_t)c.size();
}

int32_t aasr_fst_conf_edit_distance(const char *a, int32_t na, const char *b, int32_t nb) {
  if (na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) return -1;
  return edit_distance(std::string(a ? a : "", (size_t)na), std::string(b ? b : "", (size_t)nb));
}

void aasr_fst_conf_formulas(aasr_fst_conf_result *r, int32_t n_words, const char *grammar, int32_t n_grammar, const char *ploop,
                            int32_t n_ploop) {
  if (!r) return;
  const std::string g(grammar ? grammar : "", (size_t)std::max(0, n_grammar)), p(ploop ? ploop : "", (size_t)std::max(0, n_ploop));
  formulas(*r, n_words, g, ploop ? &p : nullptr);
}

}  // extern "C"

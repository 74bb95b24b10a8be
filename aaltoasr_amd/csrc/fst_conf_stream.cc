// fst_conf_stream.cc -- the handle of the confidence on streaming sessions (aasr_fst_conf_stream_*): per network the
// buffers of a batch of n_sessions utterances of max_frames frames (an aasr_fst_batch, as aasr_fst_stream holds one; the
// phone loop's with fst_conf.cc's larger history table), the sessions' records of both searches, the token records, the
// carried sums, and one launch of k_fst_conf_chunk per feed (fst_conf_stream.h).  The host counts every session's fed
// frames, so that a feed can be refused before anything is queued; the formulas run in fst_conf.cc (fst_conf_finish: one
// copy, floating-point contraction off there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "fst_conf_stream.h"
#include "fst_net.h"

using namespace aasr;

struct aasr_fst_conf_stream {
  aasr_fst_conf_options opt{};
  const aasr_fstnet *net[2] = {nullptr, nullptr};
  aasr_fst_batch *inner[2] = {nullptr, nullptr};  // grammar, phone loop
  int32_t n = 0, max_frames = 0, cap_words = 0;
  // per session, on the host: reset and not fed since; the frames fed (whatever the searches' statuses); the acoustics'
  // width and model count of the session's feeds
  std::vector<uint8_t> fresh;
  std::vector<int32_t> count, fed_bytes, fed_models;
  // what the last sync fetched, and what it made of it
  std::vector<FstSessionState> state[2];
  std::vector<FstResult> search[2];
  std::vector<int32_t> res_words[2], part_words[2];
  std::vector<FstConfRecord> rec[2];
  std::vector<float> sum;
  std::vector<int32_t> sum_frames;
  std::vector<aasr_fst_conf_result> result;
  std::vector<std::string> text[2];
  bool synced = true;  // nothing queued since the last sync
  hipStream_t sync_stream = nullptr;
  std::deque<std::vector<FstFeed>> pending;  // the feeds' orders, kept until the sync that follows their copies
  DevBuf<FstSessionState> d_state[2];
  DevBuf<int32_t> d_part_words[2];
  DevBuf<FstConfRecord> d_rec[2];
  DevBuf<FstFeed> d_feed;
  DevBuf<float> d_sum;
  DevBuf<int32_t> d_sum_frames;
  DevBuf<float> d_decode1, d_decode2;
  int64_t bytes = 0;
  ~aasr_fst_conf_stream() {
    aasr_fst_batch_destroy(inner[0]);
    aasr_fst_batch_destroy(inner[1]);
  }
};

namespace {

void ok(aasr_status s) {
  if (s != AASR_OK) raise(s, "%s", last_error().c_str());
}

void mark_fresh(aasr_fst_conf_stream *s, int32_t u) {
  s->fresh[(size_t)u] = 1;
  s->count[(size_t)u] = 0;
  s->fed_bytes[(size_t)u] = s->fed_models[(size_t)u] = 0;  // (no frames yet: the first ones set the width)
}

bool initial_is_end(const aasr_fstnet *net) { return net->node_end[(size_t)net->initial] != 0; }

// the search of a session that was not fed yet, as k_fst_conf_chunk leaves it after no frame
FstResult start_result(const aasr_fstnet *net) {
  const bool end = initial_is_end(net);
  FstResult r;
  r.status = FST_OK;
  r.n_tokens = 1;
  r.n_words = 0;
  r.logprob = end ? 0.0f : -1.0f;
  r.best_lp = 0.0f;
  r.best_final_lp = end ? 0.0f : FSTC_NONE;
  return r;
}

FstConfRecord start_record(const aasr_fstnet *net) {
  const bool end = initial_is_end(net);
  FstConfRecord r{};
  r.has_final = end;
  r.best_final_lp = end ? 0.0f : FSTC_NONE;
  r.best_different_lp = FSTC_NONE;
  return r;
}

// session u's confidence from what the sync fetched (a fresh session: from the start state, zero frames)
void finish(aasr_fst_conf_stream *s, int32_t u) {
  const size_t i = (size_t)u;
  const bool fresh = s->fresh[i];
  aasr_fst_conf_result r{};
  r.frames = fresh ? 0 : s->count[i];
  int32_t status[2] = {AASR_FST_OK, AASR_FST_OK};
  float logprob[2] = {-1.0f, -1.0f};
  for (int k = 0; k < 2; k++) {
    std::string &t = s->text[k][i];
    t.clear();
    if (!s->inner[k]) continue;
    const FstResult sr = fresh ? start_result(s->net[k]) : s->search[k][i];
    status[k] = sr.status;
    logprob[k] = sr.logprob;
    if (sr.n_words < 0 || sr.n_words > s->cap_words) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_sync: session %d reports %d words", u, sr.n_words);
    const int32_t *w = s->res_words[k].data() + i * (size_t)s->cap_words;
    const int32_t n_sym = (int32_t)s->net[k]->symbols.size();
    for (int32_t j = 0; j < sr.n_words; j++) {
      if (w[j] < 0 || w[j] >= n_sym) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_sync: session %d has word id %d", u, w[j]);
      if (j) t += ' ';
      t += s->net[k]->symbols[(size_t)w[j]];
    }
  }
  if (!fresh && s->inner[1] && s->sum_frames[i] != r.frames)
    raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_sync: session %d was fed %d frames, its sum covers %d", u, r.frames, s->sum_frames[i]);
  const FstConfRecord g = fresh ? start_record(s->net[0]) : s->rec[0][i];
  fst_conf_finish(r, status, logprob, g, s->inner[1] != nullptr, fresh ? 0.0f : s->sum[i], s->text[0][i], s->text[1][i],
                  "aasr_fst_conf_stream_sync", u);
  s->result[i] = r;
}

const char *const WHO_FEED = "aasr_fst_conf_stream_feed_dev";

}  // namespace

extern "C" {

aasr_status aasr_fst_conf_stream_create(const aasr_fstnet *grammar_net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                                        const aasr_fst_conf_options *opt, int32_t n_sessions, int32_t max_frames,
                                        aasr_fst_conf_stream **out) {
  return guarded([&] {
    if (!opt || !out) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_create: null argument");
    *out = nullptr;
    if (!grammar_net) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_create: no grammar network");
    if (opt->phone_loop && !phone_net) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_create: phone_loop without a phone-loop network");
    if (n_sessions < 1) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_create: %d sessions", n_sessions);
    if (max_frames < 1) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_create: max_frames %d", max_frames);
    fst_conf_check_options(opt->grammar, "aasr_fst_conf_stream_create", "grammar");
    fst_conf_check_options(opt->phone, "aasr_fst_conf_stream_create", "phone");
    require_device();
    std::unique_ptr<aasr_fst_conf_stream> s(new aasr_fst_conf_stream());
    s->opt = *opt;
    s->n = n_sessions;
    s->max_frames = max_frames;
    s->cap_words = max_frames + 1;
    s->net[0] = grammar_net;
    s->net[1] = opt->phone_loop ? phone_net : nullptr;
    // per network the buffers of a batch whose every utterance has max_frames frames (aasr_fst_stream_create)
    const std::vector<int32_t> T((size_t)n_sessions, max_frames);
    ok(aasr_fst_batch_create(grammar_net, dur, &opt->grammar, n_sessions, T.data(), &s->inner[0]));
    aasr_fst_batch_options(s->inner[0], &s->opt.grammar);
    if (opt->phone_loop) {
      aasr_fst_options phone = opt->phone;
      if (phone.cap_history == 0) phone.cap_history = fst_conf_phone_history(phone, max_frames);
      ok(aasr_fst_batch_create(phone_net, dur, &phone, n_sessions, T.data(), &s->inner[1]));
      aasr_fst_batch_options(s->inner[1], &s->opt.phone);
    }
    const size_t nu = (size_t)n_sessions, nw = nu * (size_t)s->cap_words;
    s->fresh.assign(nu, 1);
    s->count.assign(nu, 0);
    s->fed_bytes.assign(nu, 0);
    s->fed_models.assign(nu, 0);
    s->sum.assign(nu, 0.0f);
    s->sum_frames.assign(nu, 0);
    s->result.assign(nu, aasr_fst_conf_result{});
    FstSessionState start{};
    start.n_act = 1;
    start.fresh = 1;
    s->bytes = (int64_t)(nu * sizeof(FstFeed));
    for (int k = 0; k < 2; k++) {
      s->text[k].assign(nu, std::string());
      if (!s->inner[k]) continue;
      s->state[k].assign(nu, start);
      s->search[k].assign(nu, FstResult{});
      s->res_words[k].assign(nw, 0);
      s->part_words[k].assign(nw, 0);
      s->rec[k].assign(nu, FstConfRecord{});
      s->d_state[k].upload(s->state[k].data(), nu);
      s->d_part_words[k].alloc(nw);
      s->d_rec[k].upload(s->rec[k].data(), nu);
      s->bytes += aasr_fst_batch_device_bytes(s->inner[k]) + (int64_t)(nu * (sizeof(FstSessionState) + sizeof(FstConfRecord)) + nw * 4);
    }
    s->d_feed.alloc(nu);
    if (s->inner[1]) {
      s->d_sum.upload(s->sum.data(), nu);
      s->d_sum_frames.upload(s->sum_frames.data(), nu);
      s->bytes += (int64_t)(nu * 8);
    }
    for (int32_t u = 0; u < n_sessions; u++) finish(s.get(), u);
    *out = s.release();
  });
}

void aasr_fst_conf_stream_destroy(aasr_fst_conf_stream *s) { delete s; }
int64_t aasr_fst_conf_stream_device_bytes(const aasr_fst_conf_stream *s) { return s ? s->bytes : -1; }
void aasr_fst_conf_stream_options(const aasr_fst_conf_stream *s, aasr_fst_conf_options *out) {
  if (s && out) *out = s->opt;
}

aasr_status aasr_fst_conf_stream_reset(aasr_fst_conf_stream *s, int32_t u) {
  return guarded([&] {
    if (!s) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_reset: null argument");
    if (u < -1 || u >= s->n) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_reset: session %d of %d", u, s->n);
    for (int32_t v = 0; v < s->n; v++)
      if (u == -1 || u == v) {
        mark_fresh(s, v);
        finish(s, v);
      }
  });
}

aasr_status aasr_fst_conf_stream_feed_dev(aasr_fst_conf_stream *s, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                                          const int64_t *row0, const int32_t *n_new, void *stream) {
  return guarded([&] {
    if (!s || !row0 || !n_new) raise(AASR_ERR_INVALID, "%s: null argument", WHO_FEED);
    if (lnabytes != 1 && lnabytes != 2 && lnabytes != 4) raise(AASR_ERR_INVALID, "%s: lnabytes %d is not 1, 2 or 4", WHO_FEED, lnabytes);
    if (n_models < 1) raise(AASR_ERR_INVALID, "%s: %d models", WHO_FEED, n_models);
    if ((uintptr_t)d_lna % (uintptr_t)lnabytes) raise(AASR_ERR_INVALID, "%s: the acoustics are not aligned to %d bytes", WHO_FEED, lnabytes);
    for (int k = 0; k < 2; k++)
      if (s->net[k] && s->net[k]->max_pdf >= n_models)
        raise(AASR_ERR_INVALID, "%s: the %s network names pdf %d, the acoustics have %d models", WHO_FEED, k ? "phone-loop" : "grammar",
              s->net[k]->max_pdf, n_models);
    // every refusal comes before anything is queued or counted
    bool any_rows = false;
    for (int32_t u = 0; u < s->n; u++) {
      const size_t i = (size_t)u;
      if (n_new[u] < 0) raise(AASR_ERR_INVALID, "%s: session %d is fed %d frames", WHO_FEED, u, n_new[u]);
      const int64_t before = s->fresh[i] ? 0 : s->count[i];
      if (before + n_new[u] > s->max_frames)
        raise(AASR_ERR_INVALID, "%s: session %d would reach %lld frames, max_frames is %d", WHO_FEED, u, (long long)(before + n_new[u]),
              s->max_frames);
      if (n_new[u] == 0) continue;
      any_rows = true;
      if (!s->fresh[i] && s->fed_bytes[i] != 0 && (s->fed_bytes[i] != lnabytes || s->fed_models[i] != n_models))
        raise(AASR_ERR_INVALID, "%s: session %d was fed %d models of %d bytes, now %d of %d", WHO_FEED, u, s->fed_models[i], s->fed_bytes[i],
              n_models, lnabytes);
      if (row0[u] < 0 || row0[u] > n_rows || n_new[u] > n_rows - row0[u])
        raise(AASR_ERR_INVALID, "%s: session %d reads rows %lld .. %lld of %lld", WHO_FEED, u, (long long)row0[u],
              (long long)(row0[u] + n_new[u]), (long long)n_rows);
    }
    if (any_rows && !d_lna) raise(AASR_ERR_INVALID, "%s: null acoustics", WHO_FEED);
    const hipStream_t st = (hipStream_t)stream;
    DevBuf<float> &dec = lnabytes == 1 ? s->d_decode1 : s->d_decode2;
    if (lnabytes != 4 && !dec.p) {  // (one table per width, built once: none is replaced under a queued launch)
      std::vector<float> table;
      fst_decode_table(lnabytes, table);
      dec.upload(table.data(), table.size());
    }
    s->pending.emplace_back((size_t)s->n);
    std::vector<FstFeed> &feed = s->pending.back();
    for (int32_t u = 0; u < s->n; u++) {
      const size_t i = (size_t)u;
      feed[i].row0 = n_new[u] > 0 ? row0[u] : 0;
      feed[i].n_new = n_new[u];
      feed[i].fresh = s->fresh[i];
    }
    AASR_HIP(hipMemcpyAsync(s->d_feed.p, feed.data(), feed.size() * sizeof(FstFeed), hipMemcpyHostToDevice, st));
    FstParams p[2];
    FstStreamParams q[2];
    for (int k = 0; k < 2; k++) {
      p[k] = fst_batch_params(s->inner[k] ? s->inner[k] : s->inner[0]);  // (without a phone loop role 1 does not exist)
      p[k].lna = (const uint8_t *)d_lna;
      p[k].decode = lnabytes == 4 ? nullptr : dec.p;
      p[k].lnabytes = lnabytes;
      p[k].n_models = n_models;
      q[k].state = s->d_state[k].p;
      q[k].feed = s->d_feed.p;
      q[k].part_words = s->d_part_words[k].p;
    }
    FstConfStreamParams c{};
    c.rec[0] = s->d_rec[0].p;
    c.rec[1] = s->d_rec[1].p;
    c.sum = s->d_sum.p;
    c.sum_frames = s->d_sum_frames.p;
    fst_conf_stream_launch(p[0], q[0], p[1], q[1], c, s->n, s->inner[1] != nullptr, st);
    AASR_HIP(hipGetLastError());
    for (int32_t u = 0; u < s->n; u++) {
      const size_t i = (size_t)u;
      s->count[i] = (s->fresh[i] ? 0 : s->count[i]) + n_new[u];
      s->fresh[i] = 0;
      if (n_new[u] > 0) {
        s->fed_bytes[i] = lnabytes;
        s->fed_models[i] = n_models;
      }
    }
    s->synced = false;
  });
}

aasr_status aasr_fst_conf_stream_sync(aasr_fst_conf_stream *s, void *stream) {
  return guarded([&] {
    if (!s) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_sync: null argument");
    const hipStream_t st = (hipStream_t)stream;
    const size_t nu = (size_t)s->n;
    for (int k = 0; k < 2; k++) {
      if (!s->inner[k]) continue;
      const FstParams &p = fst_batch_params(s->inner[k]);
      AASR_HIP(hipMemcpyAsync(s->state[k].data(), s->d_state[k].p, nu * sizeof(FstSessionState), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(s->search[k].data(), p.result, nu * sizeof(FstResult), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(s->res_words[k].data(), p.res_words, s->res_words[k].size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(s->part_words[k].data(), s->d_part_words[k].p, s->part_words[k].size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(s->rec[k].data(), s->d_rec[k].p, nu * sizeof(FstConfRecord), hipMemcpyDeviceToHost, st));
    }
    if (s->inner[1]) {
      AASR_HIP(hipMemcpyAsync(s->sum.data(), s->d_sum.p, nu * sizeof(float), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(s->sum_frames.data(), s->d_sum_frames.p, nu * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    AASR_HIP(hipStreamSynchronize(st));
    s->pending.clear();
    s->synced = true;
    s->sync_stream = st;
    for (int32_t u = 0; u < s->n; u++) finish(s, u);
  });
}

aasr_status aasr_fst_conf_stream_result(const aasr_fst_conf_stream *s, int32_t u, aasr_fst_conf_result *out) {
  return guarded([&] {
    if (!s || !out || u < 0 || u >= s->n) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_result: bad argument");
    if (!s->fresh[(size_t)u] && !s->synced) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_result: call aasr_fst_conf_stream_sync first");
    const aasr_fst_conf_result &r = s->result[(size_t)u];
    *out = r;
    if (s->opt.verbose && r.valid && s->inner[1]) {  // FstConfidenceWithPhoneLoop::result_and_confidence's verbose block
      fprintf(stderr, "%s:\n\tToken: %.4f\n", s->text[0][(size_t)u].c_str(), r.token_conf);
      fprintf(stderr, "\tPloop: %.4f\n", r.ploop_conf);
      fprintf(stderr, "\tEdit: %.4f\n", r.edit_conf);
      fprintf(stderr, "\tBacu: %.4f\n", r.best_acu_conf);
      fprintf(stderr, "\tTotal: %.4f\n\n", r.confidence);
    }
  });
}

aasr_status aasr_fst_conf_stream_search_result(const aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t *status,
                                               int32_t *frames_done, float *logprob, float *best_logprob, float *best_final_logprob,
                                               int32_t *n_words, int32_t *words, int32_t cap_words, int32_t *n_partial_words,
                                               int32_t *partial_words, int32_t cap_partial, int32_t *n_tokens) {
  return guarded([&] {
    const char *who = "aasr_fst_conf_stream_search_result";
    if (!s || u < 0 || u >= s->n || (phone != 0 && phone != 1) || !s->inner[phone]) raise(AASR_ERR_INVALID, "%s: bad argument", who);
    const size_t i = (size_t)u;
    const bool fresh = s->fresh[i];
    if (!fresh && !s->synced) raise(AASR_ERR_INVALID, "%s: call aasr_fst_conf_stream_sync first", who);
    const FstResult r = fresh ? start_result(s->net[phone]) : s->search[phone][i];
    const int32_t np = fresh ? 0 : s->state[phone][i].n_partial;
    if (r.n_words < 0 || r.n_words > s->cap_words || np < 0 || np > s->cap_words)
      raise(AASR_ERR_INVALID, "%s: session %d reports %d and %d words", who, u, r.n_words, np);
    if (status) *status = r.status;
    if (frames_done) *frames_done = fresh ? 0 : s->state[phone][i].frames_done;
    if (logprob) *logprob = r.logprob;
    if (best_logprob) *best_logprob = r.best_lp;
    if (best_final_logprob) *best_final_logprob = r.best_final_lp;
    if (n_words) *n_words = r.n_words;
    if (n_partial_words) *n_partial_words = np;
    if (n_tokens) *n_tokens = r.n_tokens;
    const int32_t n_sym = (int32_t)s->net[phone]->symbols.size();
    auto copy = [&](const std::vector<int32_t> &from, int32_t n, int32_t *to, int32_t cap, const char *what) {
      if (!to) return;
      if (cap < n) raise(AASR_ERR_INVALID, "%s: %d %swords, room for %d", who, n, what, cap);
      const int32_t *w = from.data() + i * (size_t)s->cap_words;
      for (int32_t k = 0; k < n; k++) {
        if (w[k] < 0 || w[k] >= n_sym) raise(AASR_ERR_INVALID, "%s: session %d has word id %d", who, u, w[k]);
        to[k] = w[k];
      }
    };
    copy(s->res_words[phone], r.n_words, words, cap_words, "");
    copy(s->part_words[phone], np, partial_words, cap_partial, "partial ");
  });
}

aasr_status aasr_fst_conf_stream_tokens(aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t cap_tokens, int32_t *node,
                                        float *logprob, int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words) {
  return guarded([&] {
    const char *who = "aasr_fst_conf_stream_tokens";
    if (!s || u < 0 || u >= s->n || (phone != 0 && phone != 1) || !s->inner[phone] || !node || !logprob || !dur || !word_begin)
      raise(AASR_ERR_INVALID, "%s: bad argument", who);
    const size_t i = (size_t)u;
    if (s->fresh[i]) {
      if (cap_tokens < 1) raise(AASR_ERR_INVALID, "%s: 1 token, room for %d", who, cap_tokens);
      node[0] = s->net[phone]->initial;
      logprob[0] = 0.0f;
      dur[0] = 0;
      word_begin[0] = word_begin[1] = 0;
      return;
    }
    if (!s->synced) raise(AASR_ERR_INVALID, "%s: call aasr_fst_conf_stream_sync first", who);
    const FstParams &p = fst_batch_params(s->inner[phone]);
    const int32_t n = s->search[phone][i].n_tokens;
    if (n < 0 || n > p.cap_tok) raise(AASR_ERR_INVALID, "%s: session %d reports %d tokens", who, u, n);
    if (cap_tokens < n) raise(AASR_ERR_INVALID, "%s: %d tokens, room for %d", who, n, cap_tokens);
    fst_tokens_read(who, p, u, n, s->sync_stream, node, logprob, dur, word_begin, cap_words, words);
  });
}

aasr_status aasr_fst_conf_stream_record(const aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t *has_final, int32_t *n_words,
                                        int32_t *has_different, float *best_final_logprob, float *best_different_logprob) {
  return guarded([&] {
    if (!s || u < 0 || u >= s->n || (phone != 0 && phone != 1) || !s->inner[phone]) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_record: bad argument");
    const size_t i = (size_t)u;
    if (!s->fresh[i] && !s->synced) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_record: call aasr_fst_conf_stream_sync first");
    const FstConfRecord r = s->fresh[i] ? start_record(s->net[phone]) : s->rec[phone][i];
    if (has_final) *has_final = r.has_final;
    if (n_words) *n_words = r.best_final_n_words;
    if (has_different) *has_different = r.has_different;
    if (best_final_logprob) *best_final_logprob = r.best_final_lp;
    if (best_different_logprob) *best_different_logprob = r.best_different_lp;
  });
}

aasr_status aasr_fst_conf_stream_best_acu(const aasr_fst_conf_stream *s, int32_t u, float *sum, int32_t *frames) {
  return guarded([&] {
    if (!s || u < 0 || u >= s->n) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_best_acu: bad argument");
    if (!s->inner[1]) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_best_acu: no phone loop, the sum is not carried");
    const size_t i = (size_t)u;
    if (!s->fresh[i] && !s->synced) raise(AASR_ERR_INVALID, "aasr_fst_conf_stream_best_acu: call aasr_fst_conf_stream_sync first");
    if (sum) *sum = s->fresh[i] ? 0.0f : s->sum[i];
    if (frames) *frames = s->fresh[i] ? 0 : s->sum_frames[i];
  });
}

}  // extern "C"

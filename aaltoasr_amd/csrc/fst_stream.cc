// fst_stream.cc -- the handle of the FST decoder's streaming sessions (aasr_fst_stream_*): the buffers of a batch of
// n_sessions utterances of max_frames frames (an aasr_fst_batch, so capacities, network and duration table are derived
// exactly as a batch derives them), the sessions' records, and one launch of k_fst_search_chunk per feed (fst_stream.h).
// The host keeps its own count of every session's frames so that a feed can be refused before anything is queued.
#include <hip/hip_runtime.h>

#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "fst_conf.h"
#include "fst_net.h"
#include "fst_stream.h"

using namespace aasr;

struct aasr_fst_stream {
  const aasr_fstnet *net = nullptr;
  aasr_fst_batch *inner = nullptr;
  int32_t n = 0, max_frames = 0, cap_words = 0;
  // per session, on the host: reset and not fed since (answers come from the start state); the frames counted here; the
  // status last seen at a sync; the acoustics' width and model count of the session's feeds
  std::vector<uint8_t> fresh;
  std::vector<int32_t> count, seen_status, fed_bytes, fed_models;
  // what the last sync fetched
  std::vector<FstSessionState> state;
  std::vector<FstResult> result;
  std::vector<int32_t> res_words, part_words;
  bool synced = true;  // nothing queued since the last sync
  hipStream_t sync_stream = nullptr;
  std::deque<std::vector<FstFeed>> pending;  // the feeds' orders, kept until the sync that follows their copies
  DevBuf<FstSessionState> d_state;
  DevBuf<FstFeed> d_feed;
  DevBuf<int32_t> d_part_words;
  DevBuf<float> d_decode1, d_decode2;
  int64_t bytes = 0;
  ~aasr_fst_stream() { aasr_fst_batch_destroy(inner); }
};

namespace {

void mark_fresh(aasr_fst_stream *s, int32_t u) {
  s->fresh[(size_t)u] = 1;
  s->count[(size_t)u] = 0;
  s->seen_status[(size_t)u] = FST_OK;
  s->fed_bytes[(size_t)u] = s->fed_models[(size_t)u] = 0;  // (no frames yet: the first ones set the width)
}

bool initial_is_end(const aasr_fstnet *net) { return net->node_end[(size_t)net->initial] != 0; }

}  // namespace

extern "C" {

aasr_status aasr_fst_stream_create(const aasr_fstnet *net, const aasr_fst_durations *dur, const aasr_fst_options *opt,
                                   int32_t n_sessions, int32_t max_frames, aasr_fst_stream **out) {
  return guarded([&] {
    if (!net || !opt || !out) raise(AASR_ERR_INVALID, "aasr_fst_stream_create: null argument");
    *out = nullptr;
    if (n_sessions < 1) raise(AASR_ERR_INVALID, "aasr_fst_stream_create: %d sessions", n_sessions);
    if (max_frames < 1) raise(AASR_ERR_INVALID, "aasr_fst_stream_create: max_frames %d", max_frames);
    std::unique_ptr<aasr_fst_stream> s(new aasr_fst_stream());
    s->net = net;
    s->n = n_sessions;
    s->max_frames = max_frames;
    // the buffers of a batch whose every utterance has max_frames frames: the same capacity rules, the duration table
    // for d = 0 ... max_frames (a duration cannot exceed the frames elapsed), max_frames + 1 words per result
    const std::vector<int32_t> T((size_t)n_sessions, max_frames);
    const aasr_status st = aasr_fst_batch_create(net, dur, opt, n_sessions, T.data(), &s->inner);
    if (st != AASR_OK) {
      const std::string why = aasr_last_error();
      raise(st, "aasr_fst_stream_create: %s", why.c_str());
    }
    s->cap_words = max_frames + 1;
    const size_t nu = (size_t)n_sessions;
    s->fresh.assign(nu, 1);
    s->count.assign(nu, 0);
    s->seen_status.assign(nu, FST_OK);
    s->fed_bytes.assign(nu, 0);
    s->fed_models.assign(nu, 0);
    FstSessionState start{};
    start.n_act = 1;
    start.fresh = 1;
    s->state.assign(nu, start);
    s->result.assign(nu, FstResult{});
    s->res_words.assign(nu * (size_t)s->cap_words, 0);
    s->part_words.assign(nu * (size_t)s->cap_words, 0);
    s->d_state.upload(s->state.data(), nu);
    s->d_feed.alloc(nu);
    s->d_part_words.alloc(nu * (size_t)s->cap_words);
    s->bytes = aasr_fst_batch_device_bytes(s->inner) +
               (int64_t)(nu * (sizeof(FstSessionState) + sizeof(FstFeed) + (size_t)s->cap_words * 4));
    *out = s.release();
  });
}

void aasr_fst_stream_destroy(aasr_fst_stream *s) { delete s; }
int64_t aasr_fst_stream_device_bytes(const aasr_fst_stream *s) { return s ? s->bytes : -1; }
void aasr_fst_stream_options(const aasr_fst_stream *s, aasr_fst_options *out) {
  if (s && out) aasr_fst_batch_options(s->inner, out);
}

aasr_status aasr_fst_stream_reset(aasr_fst_stream *s, int32_t u) {
  return guarded([&] {
    if (!s) raise(AASR_ERR_INVALID, "aasr_fst_stream_reset: null argument");
    if (u < -1 || u >= s->n) raise(AASR_ERR_INVALID, "aasr_fst_stream_reset: session %d of %d", u, s->n);
    for (int32_t v = 0; v < s->n; v++)
      if (u == -1 || u == v) mark_fresh(s, v);
  });
}

aasr_status aasr_fst_stream_feed_dev(aasr_fst_stream *s, const void *d_lna, int32_t lnabytes, int32_t n_models,
                                     int64_t n_rows, const int64_t *row0, const int32_t *n_new, void *stream) {
  return guarded([&] {
    if (!s || !row0 || !n_new) raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: null argument");
    if (lnabytes != 1 && lnabytes != 2 && lnabytes != 4) raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: lnabytes %d is not 1, 2 or 4", lnabytes);
    if (n_models < 1) raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: %d models", n_models);
    if (s->net->max_pdf >= n_models)
      raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: the network names pdf %d, the acoustics have %d models", s->net->max_pdf, n_models);
    // every refusal comes before anything is queued or counted
    bool any_rows = false;
    for (int32_t u = 0; u < s->n; u++) {
      const size_t i = (size_t)u;
      if (n_new[u] < 0) raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: session %d is fed %d frames", u, n_new[u]);
      const bool counted = s->fresh[i] || s->seen_status[i] == FST_OK;  // (a sticky session skips its frames)
      const int64_t before = s->fresh[i] ? 0 : s->count[i];
      if (counted && before + n_new[u] > s->max_frames)
        raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: session %d would reach %lld frames, max_frames is %d", u,
              (long long)(before + n_new[u]), s->max_frames);
      if (n_new[u] == 0) continue;
      any_rows = true;
      if (!s->fresh[i] && s->fed_bytes[i] != 0 && (s->fed_bytes[i] != lnabytes || s->fed_models[i] != n_models))
        raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: session %d was fed %d models of %d bytes, now %d of %d", u, s->fed_models[i],
              s->fed_bytes[i], n_models, lnabytes);
      if (row0[u] < 0 || row0[u] > n_rows || n_new[u] > n_rows - row0[u])
        raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: session %d reads rows %lld .. %lld of %lld", u, (long long)row0[u],
              (long long)(row0[u] + n_new[u]), (long long)n_rows);
    }
    if (any_rows && !d_lna) raise(AASR_ERR_INVALID, "aasr_fst_stream_feed_dev: null acoustics");
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
    FstParams p = fst_batch_params(s->inner);
    p.lna = (const uint8_t *)d_lna;
    p.decode = lnabytes == 4 ? nullptr : dec.p;
    p.lnabytes = lnabytes;
    p.n_models = n_models;
    FstStreamParams q;
    q.state = s->d_state.p;
    q.feed = s->d_feed.p;
    q.part_words = s->d_part_words.p;
    fst_stream_launch(p, q, s->n, st);
    AASR_HIP(hipGetLastError());
    for (int32_t u = 0; u < s->n; u++) {
      const size_t i = (size_t)u;
      if (s->fresh[i]) {
        s->fresh[i] = 0;
        s->count[i] = n_new[u];
      } else if (s->seen_status[i] == FST_OK) {
        s->count[i] += n_new[u];
      }
      if (n_new[u] > 0) {
        s->fed_bytes[i] = lnabytes;
        s->fed_models[i] = n_models;
      }
    }
    s->synced = false;
  });
}

aasr_status aasr_fst_stream_sync(aasr_fst_stream *s, void *stream) {
  return guarded([&] {
    if (!s) raise(AASR_ERR_INVALID, "aasr_fst_stream_sync: null argument");
    const hipStream_t st = (hipStream_t)stream;
    const FstParams &p = fst_batch_params(s->inner);
    AASR_HIP(hipMemcpyAsync(s->state.data(), s->d_state.p, s->state.size() * sizeof(FstSessionState), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(s->result.data(), p.result, s->result.size() * sizeof(FstResult), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(s->res_words.data(), p.res_words, s->res_words.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(s->part_words.data(), s->d_part_words.p, s->part_words.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
    s->pending.clear();
    s->synced = true;
    s->sync_stream = st;
    for (int32_t u = 0; u < s->n; u++) {  // the device's word on every session that is not waiting for its first feed
      const size_t i = (size_t)u;
      if (s->fresh[i]) continue;
      s->count[i] = s->state[i].frames_done;
      s->seen_status[i] = s->state[i].status;
    }
  });
}

aasr_status aasr_fst_stream_result(const aasr_fst_stream *s, int32_t u, int32_t *status, int32_t *frames_done, float *logprob,
                                   float *best_logprob, float *best_final_logprob, int32_t *n_words, int32_t *words,
                                   int32_t cap_words, int32_t *n_partial_words, int32_t *partial_words, int32_t cap_partial,
                                   int32_t *n_tokens) {
  return guarded([&] {
    if (!s || u < 0 || u >= s->n) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: bad argument");
    const size_t i = (size_t)u;
    if (s->fresh[i]) {  // the start state, as k_fst_search_chunk leaves it after no frame
      const bool end = initial_is_end(s->net);
      if (status) *status = FST_OK;
      if (frames_done) *frames_done = 0;
      if (logprob) *logprob = end ? 0.0f : -1.0f;
      if (best_logprob) *best_logprob = 0.0f;
      if (best_final_logprob) *best_final_logprob = end ? 0.0f : -9999999.9f;
      if (n_words) *n_words = 0;
      if (n_partial_words) *n_partial_words = 0;
      if (n_tokens) *n_tokens = 1;
      return;
    }
    if (!s->synced) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: call aasr_fst_stream_sync first");
    const FstResult &r = s->result[i];
    const int32_t np = s->state[i].n_partial;
    if (r.n_words < 0 || r.n_words > s->cap_words || np < 0 || np > s->cap_words)
      raise(AASR_ERR_INVALID, "aasr_fst_stream_result: session %d reports %d and %d words", u, r.n_words, np);
    if (status) *status = r.status;
    if (frames_done) *frames_done = s->state[i].frames_done;
    if (logprob) *logprob = r.logprob;
    if (best_logprob) *best_logprob = r.best_lp;
    if (best_final_logprob) *best_final_logprob = r.best_final_lp;
    if (n_words) *n_words = r.n_words;
    if (n_partial_words) *n_partial_words = np;
    if (n_tokens) *n_tokens = r.n_tokens;
    const int32_t n_sym = (int32_t)s->net->symbols.size();
    if (words) {
      if (cap_words < r.n_words) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: %d words, room for %d", r.n_words, cap_words);
      const int32_t *w = s->res_words.data() + i * (size_t)s->cap_words;
      for (int32_t k = 0; k < r.n_words; k++) {
        if (w[k] < 0 || w[k] >= n_sym) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: session %d has word id %d", u, w[k]);
        words[k] = w[k];
      }
    }
    if (partial_words) {
      if (cap_partial < np) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: %d partial words, room for %d", np, cap_partial);
      const int32_t *w = s->part_words.data() + i * (size_t)s->cap_words;
      for (int32_t k = 0; k < np; k++) {
        if (w[k] < 0 || w[k] >= n_sym) raise(AASR_ERR_INVALID, "aasr_fst_stream_result: session %d has word id %d", u, w[k]);
        partial_words[k] = w[k];
      }
    }
  });
}

aasr_status aasr_fst_stream_tokens(aasr_fst_stream *s, int32_t u, int32_t cap_tokens, int32_t *node, float *logprob,
                                   int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words) {
  return guarded([&] {
    if (!s || u < 0 || u >= s->n || !node || !logprob || !dur || !word_begin) raise(AASR_ERR_INVALID, "aasr_fst_stream_tokens: bad argument");
    const size_t i = (size_t)u;
    if (s->fresh[i]) {
      if (cap_tokens < 1) raise(AASR_ERR_INVALID, "aasr_fst_stream_tokens: 1 token, room for %d", cap_tokens);
      node[0] = s->net->initial;
      logprob[0] = 0.0f;
      dur[0] = 0;
      word_begin[0] = word_begin[1] = 0;
      return;
    }
    if (!s->synced) raise(AASR_ERR_INVALID, "aasr_fst_stream_tokens: call aasr_fst_stream_sync first");
    const FstParams &p = fst_batch_params(s->inner);
    const int32_t n = s->result[i].n_tokens;
    if (n < 0 || n > p.cap_tok) raise(AASR_ERR_INVALID, "aasr_fst_stream_tokens: session %d reports %d tokens", u, n);
    if (cap_tokens < n) raise(AASR_ERR_INVALID, "aasr_fst_stream_tokens: %d tokens, room for %d", n, cap_tokens);
    fst_tokens_read("aasr_fst_stream_tokens", p, u, n, s->sync_stream, node, logprob, dur, word_begin, cap_words, words);
  });
}

}  // extern "C"

// fst_live.cc -- the live driver of the FST decoder (aasr_run_fst_live, the fst_stream tool): headerless PCM16 from a
// descriptor that is still being written, words while it arrives.  The samples are read as the adapter's stream mode
// reads them (aku/FeatureGenerator.cc, stream_read_until: frame t is computable when the samples cover frame t + halo_r
// + 1; at the end of input, the frames up to aasr_feat_eof_frame).  Per chunk of chunk_frames frames: the feature
// chain for exactly those frames over the samples so far, ONE score + LNA step (aasr_gmm_score_lna_dev, normalised, as
// fst_decode's engine mode runs it per group) and one feed of a one-session aasr_fst_stream that reads the step's
// device buffer in place -- no LNA value leaves the device.  aasr_run_fst_live_confidence is the same loop over a
// one-session aasr_fst_conf_stream (fst_stream --confidence): a confidence behind every log-probability it prints.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "feat.h"
#include "gmm.h"
#include "recipe_pass.h"

using namespace aasr;

namespace {

const char *const STATUS[] = {"OK", "NO_TOKENS", "OVERFLOW_CANDIDATES", "OVERFLOW_RECOMB", "OVERFLOW_HISTORY"};

void ok(aasr_status s) {
  if (s != AASR_OK) raise(s, "%s", last_error().c_str());
}

// the one live session: an aasr_fst_stream, or with conf an aasr_fst_conf_stream whose grammar search answers for it
struct Session {
  aasr_fst_stream *s = nullptr;
  aasr_fst_conf_stream *c = nullptr;
  ~Session() {
    aasr_fst_stream_destroy(s);
    aasr_fst_conf_stream_destroy(c);
  }
  void feed(const void *d_lna, int lnabytes, int n_models, int32_t n, hipStream_t stream) {
    const int64_t row0 = 0;
    if (c)
      ok(aasr_fst_conf_stream_feed_dev(c, d_lna, lnabytes, n_models, n, &row0, &n, stream));
    else
      ok(aasr_fst_stream_feed_dev(s, d_lna, lnabytes, n_models, n, &row0, &n, stream));
  }
  // after a sync: the search's answers (any pointer may be NULL) and, with conf, the confidence's
  void fetch(hipStream_t stream, int32_t *status, int32_t *frames, float *logprob, float *best, int32_t *n_words, std::vector<int32_t> *words,
             int32_t *n_partial, std::vector<int32_t> *partial, aasr_fst_conf_result *conf) {
    int32_t *w = words ? words->data() : nullptr, *pw = partial ? partial->data() : nullptr;
    const int32_t cw = words ? (int32_t)words->size() : 0, cp = partial ? (int32_t)partial->size() : 0;
    if (c) {
      ok(aasr_fst_conf_stream_sync(c, stream));
      ok(aasr_fst_conf_stream_search_result(c, 0, 0, status, frames, logprob, best, nullptr, n_words, w, cw, n_partial, pw, cp, nullptr));
      ok(aasr_fst_conf_stream_result(c, 0, conf));
    } else {
      ok(aasr_fst_stream_sync(s, stream));
      ok(aasr_fst_stream_result(s, 0, status, frames, logprob, best, nullptr, n_words, w, cw, n_partial, pw, cp, nullptr));
    }
  }
};

// the descriptor's samples, appended to pcm as they arrive
struct SampleReader {
  int fd;
  bool big_endian, eof = false;
  bool have_odd = false;
  unsigned char odd = 0;
  std::vector<unsigned char> raw;
  // blocks until at least one more byte is there (or the end); appends the whole samples
  void read_some(std::vector<int16_t> &pcm) {
    raw.resize(1 << 16);
    ssize_t got;
    do {
      got = read(fd, raw.data(), raw.size());
    } while (got < 0 && errno == EINTR);
    if (got < 0) raise(AASR_ERR_IO, "fst_stream: read error on the input: %s", strerror(errno));
    if (got == 0) {
      eof = true;  // (a trailing odd byte is no sample)
      return;
    }
    size_t i = 0;
    const size_t n = (size_t)got;
    auto sample = [&](unsigned char a, unsigned char b) {
      const unsigned lo = big_endian ? b : a, hi = big_endian ? a : b;
      pcm.push_back((int16_t)(lo | (hi << 8)));
    };
    if (have_odd) {
      sample(odd, raw[0]);
      have_odd = false;
      i = 1;
    }
    for (; i + 1 < n; i += 2) sample(raw[i], raw[i + 1]);
    if (i < n) {
      odd = raw[i];
      have_odd = true;
    }
  }
};

aasr_status run_live(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                     const aasr_fst_live_options *opt, const aasr_fst_live_confidence_options *conf, aasr_run_stats *stats,
                     const char *who);

}  // namespace

extern "C" {

void aasr_fst_live_default_options(aasr_fst_live_options *o) {
  if (!o) return;
  *o = aasr_fst_live_options();
  aasr_fst_default_options(&o->fst);
  o->lnabytes = 2;
  o->chunk_frames = 16;
  o->max_frames = 7500;
}

aasr_status aasr_run_fst_live(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur,
                              const aasr_fst_live_options *opt, aasr_run_stats *stats) {
  if (!opt) return guarded([&] { raise(AASR_ERR_INVALID, "aasr_run_fst_live: null argument"); });
  return run_live(feat, gmm, net, nullptr, dur, opt, nullptr, stats, "aasr_run_fst_live");
}

void aasr_fst_live_confidence_default_options(aasr_fst_live_confidence_options *o) {
  if (!o) return;
  *o = aasr_fst_live_confidence_options();
  aasr_fst_live_default_options(&o->live);
  aasr_fst_default_options(&o->phone);
}

aasr_status aasr_run_fst_live_confidence(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net,
                                         const aasr_fst_durations *dur, const aasr_fst_live_confidence_options *opt,
                                         aasr_run_stats *stats) {
  if (!opt) return guarded([&] { raise(AASR_ERR_INVALID, "aasr_run_fst_live_confidence: null argument"); });
  return run_live(feat, gmm, net, phone_net, dur, &opt->live, opt, stats, "aasr_run_fst_live_confidence");
}

}  // extern "C"

namespace {

aasr_status run_live(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                     const aasr_fst_live_options *opt, const aasr_fst_live_confidence_options *conf, aasr_run_stats *stats,
                     const char *who) {
  return guarded([&] {
    if (!feat || !gmm || !net || !opt) raise(AASR_ERR_INVALID, "%s: null argument", who);
    if (conf && conf->phone_loop && !phone_net) raise(AASR_ERR_INVALID, "%s: phone_loop without a phone-loop network", who);
    if (conf && !conf->phone_loop) phone_net = nullptr;
    if (opt->lnabytes != 2 && opt->lnabytes != 4) raise(AASR_ERR_INVALID, "Invalid number of LNA bytes");
    if (opt->chunk_frames < 1) raise(AASR_ERR_INVALID, "fst_stream: a chunk must hold at least 1 frame");
    if (opt->max_frames < 1) raise(AASR_ERR_INVALID, "fst_stream: max_frames must be at least 1");
    if (aasr_feat_input_is_features(feat)) raise(AASR_ERR_INVALID, "fst_stream: the feature configuration reads features, not audio");
    check_feature_dim(gmm, feat);
    const int n_models = aasr_gmm_num_states(gmm);
    if (aasr_fstnet_max_pdf(net) >= n_models)
      raise(AASR_ERR_INVALID, "fst_stream: the network names pdf %d, the model has %d states", aasr_fstnet_max_pdf(net), n_models);
    if (phone_net && aasr_fstnet_max_pdf(phone_net) >= n_models)
      raise(AASR_ERR_INVALID, "fst_stream: the phone-loop network names pdf %d, the model has %d states", aasr_fstnet_max_pdf(phone_net), n_models);
    require_device();
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t stream = nullptr;
    AASR_HIP(hipStreamCreate(&stream));
    std::unique_ptr<void, void (*)(void *)> stream_guard((void *)stream, [](void *s) { (void)hipStreamDestroy((hipStream_t)s); });

    const int chunk = (int)std::min<int64_t>(opt->chunk_frames, opt->max_frames), dim = aasr_feat_dim(feat), lnabytes = opt->lnabytes;
    int halo_l = 0, halo_r = 0;
    aasr_feat_halo(feat, &halo_l, &halo_r);
    // the samples of max_frames frames and their look-ahead, with room for what one read can bring beyond them
    const double adv = (double)aasr_feat_sample_rate(feat) / (double)aasr_feat_frame_rate(feat);
    const size_t cap_pcm = (size_t)(((double)opt->max_frames + halo_r + 16) * adv) + (size_t)(8 * adv) + (1 << 16);
    Session g;
    if (conf) {
      aasr_fst_conf_options co;
      aasr_fst_conf_default_options(&co);
      co.grammar = opt->fst;
      co.phone = conf->phone;
      co.phone_loop = phone_net != nullptr;
      co.verbose = 0;
      ok(aasr_fst_conf_stream_create(net, phone_net, dur, &co, 1, opt->max_frames, &g.c));
    } else {
      ok(aasr_fst_stream_create(net, dur, &opt->fst, 1, opt->max_frames, &g.s));
    }
    DevBuf<int16_t> d_pcm;
    DevBuf<float> d_fea, d_scratch;
    DevBuf<uint8_t> d_lna;
    d_pcm.alloc(cap_pcm);
    d_fea.alloc((size_t)chunk * (size_t)dim);
    d_scratch.alloc((size_t)std::max<int64_t>(1, aasr_gmm_score_scratch_floats(gmm, chunk)));
    d_lna.alloc((size_t)chunk * (size_t)n_models * (size_t)lnabytes + 16);

    SampleReader in{opt->in_fd, feat->mods[0].endian == 2};
    std::vector<int16_t> pcm;
    size_t uploaded = 0;
    int32_t done = 0;  // frames fed
    std::vector<int32_t> words((size_t)opt->max_frames + 1), partial((size_t)opt->max_frames + 1), printed;
    bool printed_any = false;
    for (;;) {
      // samples until the chunk's last frame is computable, or to the end of the input
      while (!in.eof && aasr_feat_eof_frame(feat, (int64_t)pcm.size()) - 1 < (int64_t)done + chunk - 1 + halo_r + 1) {
        in.read_some(pcm);
        if (pcm.size() > cap_pcm) raise(AASR_ERR_INVALID, "fst_stream: the input is longer than --max-frames %d frames", opt->max_frames);
      }
      const int eof_frame = aasr_feat_eof_frame(feat, (int64_t)pcm.size());
      if (in.eof && eof_frame < 1) raise(AASR_ERR_SHORT_AUDIO, "audio shorter than frame");
      const int computable = in.eof ? eof_frame : eof_frame - 1 - halo_r;
      const int n = std::min(chunk, computable - done);
      if (n > 0) {
        if (pcm.size() > uploaded) {
          AASR_HIP(hipStreamSynchronize(stream));
          AASR_HIP(hipMemcpy(d_pcm.p + uploaded, pcm.data() + uploaded, (pcm.size() - uploaded) * sizeof(int16_t), hipMemcpyHostToDevice));
          uploaded = pcm.size();
        }
        UttBatch ub;
        ub.n_utts = 1;
        ub.frame_off = {0, n};
        ub.pcm_off = {0, (int64_t)uploaded};
        ub.first = {done};
        feat_run_batch(feat, d_pcm.p, ub, (int)feat->mods.size() - 1, d_fea.p, nullptr, stream);
        ok(aasr_gmm_score_lna_dev(gmm, d_fea.p, n, 1, lnabytes, d_scratch.p, d_lna.p, stream));
        g.feed(d_lna.p, lnabytes, n_models, n, stream);
        done += n;
        if (opt->partial) {  // a line whenever the best token's words are not the ones printed last
          int32_t status = 0, frames = 0, np = 0;
          float best = 0;
          aasr_fst_conf_result cr{};
          g.fetch(stream, &status, &frames, nullptr, &best, nullptr, nullptr, &np, &partial, &cr);
          const std::vector<int32_t> now(partial.begin(), partial.begin() + np);
          if (status == AASR_FST_OK && (!printed_any ? !now.empty() : now != printed)) {
            printf("%d %.9g", frames, (double)best);
            if (conf) printf(" %.9g", (double)cr.confidence);
            for (int32_t w : now) printf(" %s", aasr_fstnet_symbol(net, w));
            printf("\n");
            fflush(stdout);
            printed = now;
            printed_any = true;
          }
        }
      }
      if (in.eof && done >= eof_frame) break;
    }
    int32_t status = 0, n_words = 0;
    float logprob = -1;
    aasr_fst_conf_result cr{};
    g.fetch(stream, &status, nullptr, &logprob, nullptr, &n_words, &words, nullptr, nullptr, &cr);
    printf("- %.9g", (double)logprob);
    if (conf) printf(" %.9g", (double)cr.confidence);
    for (int32_t i = 0; i < n_words; i++) printf(" %s", aasr_fstnet_symbol(net, words[(size_t)i]));
    if (conf && status == AASR_FST_OK) status = cr.phone_status;  // (the grammar's status first, as fst_decode --confidence)
    if (status != AASR_FST_OK) printf(" %s", STATUS[status]);
    printf("\n");
    fflush(stdout);
    if (opt->info > 0) fprintf(stderr, "fst_stream: %d frames in chunks of %d\n", done, chunk);
    if (stats) fill_run_stats(stats, 1, done, t0, 0.0);
  });
}

}  // namespace

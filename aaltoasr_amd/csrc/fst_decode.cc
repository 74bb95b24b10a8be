// fst_decode.cc -- the recipe driver of the FST decoder (aasr_run_fst_decode_recipe), beside network_pass.cc on the shared
// recipe pass (recipe_pass.h): groups of utterances, per group one feature launch set per stretch of equal speaker
// settings, ONE score + LNA step over the group's frames (aasr_gmm_score_lna_dev: what the phone_probs driver runs per
// block) and one search launch (aasr_fst_batch_*) that reads the step's device buffer in place -- the LNA values of
// engine mode never leave the device.  With lna_files the recipe's lna= files are uploaded instead.
// aasr_run_fst_confidence_recipe is the same loop with a confidence batch (aasr_fst_conf_batch_*) per group: the group's
// LNA device buffer feeds the grammar search, the phone-loop search and the frame-best pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
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

struct Line {
  int32_t status = 0;
  float logprob = -1;
  std::vector<int32_t> words;
  aasr_fst_conf_result conf{};  // --confidence
};

struct BatchGuard {
  aasr_fst_batch *b = nullptr;
  ~BatchGuard() { aasr_fst_batch_destroy(b); }
};
struct ConfBatchGuard {
  aasr_fst_conf_batch *b = nullptr;
  ~ConfBatchGuard() { aasr_fst_conf_batch_destroy(b); }
};

void ok(aasr_status s) {
  if (s != AASR_OK) raise(s, "%s", last_error().c_str());
}

// one launch over the utterances `which`; -> how many of them overflowed a capacity
int32_t run_batch(const aasr_fstnet *net, const aasr_fst_durations *dur, const aasr_fst_options &opt, const std::vector<int32_t> &frames,
                  const std::vector<int64_t> &row0_all, const std::vector<size_t> &which, const uint8_t *d_lna, int64_t n_rows,
                  int lnabytes, int n_models, hipStream_t stream, std::vector<Line> &out, aasr_fst_options *resolved) {
  std::vector<int32_t> T;
  std::vector<int64_t> row0;
  for (size_t i : which) {
    T.push_back(frames[i]);
    row0.push_back(row0_all[i]);
  }
  BatchGuard g;
  int32_t over = 0;
  ok(aasr_fst_batch_create(net, dur, &opt, (int32_t)which.size(), T.data(), &g.b));
  ok(aasr_fst_batch_dev(g.b, d_lna, lnabytes, n_models, n_rows, row0.data(), stream));
  ok(aasr_fst_batch_sync(g.b, stream, &over));
  aasr_fst_batch_options(g.b, resolved);
  for (size_t k = 0; k < which.size(); k++) {
    Line &l = out[which[k]];
    int32_t n = 0;
    l.words.assign((size_t)T[k] + 1, 0);
    ok(aasr_fst_batch_result(g.b, (int32_t)k, &l.status, &l.logprob, nullptr, nullptr, &n, l.words.data(), (int32_t)l.words.size(), nullptr));
    l.words.resize((size_t)n);
  }
  return over;
}

// the same over a confidence batch; at info >= 1 the reference's verbose block per utterance on stderr
int32_t run_conf_batch(const aasr_fstnet *net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur, const aasr_fst_conf_options &opt,
                       const std::vector<int32_t> &frames, const std::vector<int64_t> &row0_all, const std::vector<size_t> &which,
                       const uint8_t *d_lna, int64_t n_rows, int lnabytes, int n_models, hipStream_t stream, std::vector<Line> &out,
                       aasr_fst_conf_options *resolved) {
  std::vector<int32_t> T;
  std::vector<int64_t> row0;
  for (size_t i : which) {
    T.push_back(frames[i]);
    row0.push_back(row0_all[i]);
  }
  ConfBatchGuard g;
  int32_t over = 0;
  ok(aasr_fst_conf_batch_create(net, phone_net, dur, &opt, (int32_t)which.size(), T.data(), &g.b));
  ok(aasr_fst_conf_batch_dev(g.b, d_lna, lnabytes, n_models, n_rows, row0.data(), stream));
  ok(aasr_fst_conf_batch_sync(g.b, stream, &over));
  aasr_fst_conf_batch_options(g.b, resolved);
  for (size_t k = 0; k < which.size(); k++) {
    Line &l = out[which[k]];
    int32_t n = 0;
    l.words.assign((size_t)T[k] + 1, 0);
    ok(aasr_fst_batch_result(aasr_fst_conf_batch_grammar(g.b), (int32_t)k, &l.status, &l.logprob, nullptr, nullptr, &n, l.words.data(),
                             (int32_t)l.words.size(), nullptr));
    l.words.resize((size_t)n);
    ok(aasr_fst_conf_batch_result(g.b, (int32_t)k, &l.conf));
  }
  return over;
}

void double_capacities(aasr_fst_options &o) {
  o.cap_candidates *= 2;
  o.cap_recomb *= 2;
  o.cap_history *= 2;
}

aasr_status run_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur, const char *recipe_path,
                       const aasr_fst_decode_options *opt, const aasr_fstnet *phone_net, const aasr_fst_confidence_options *conf,
                       aasr_run_stats *stats);

}  // namespace

extern "C" {

void aasr_fst_confidence_default_options(aasr_fst_confidence_options *o) {
  if (!o) return;
  *o = aasr_fst_confidence_options();
  aasr_fst_decode_default_options(&o->decode);
  aasr_fst_default_options(&o->phone);
}

aasr_status aasr_run_fst_confidence_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net,
                                           const aasr_fst_durations *dur, const char *recipe_path,
                                           const aasr_fst_confidence_options *opt, aasr_run_stats *stats) {
  if (!opt) return guarded([&] { raise(AASR_ERR_INVALID, "aasr_run_fst_confidence_recipe: null argument"); });
  return run_recipe(feat, gmm, net, dur, recipe_path, &opt->decode, phone_net, opt, stats);
}

aasr_status aasr_run_fst_decode_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur,
                                       const char *recipe_path, const aasr_fst_decode_options *opt, aasr_run_stats *stats) {
  return run_recipe(feat, gmm, net, dur, recipe_path, opt, nullptr, nullptr, stats);
}

void aasr_fst_decode_default_options(aasr_fst_decode_options *o) {
  if (!o) return;
  *o = aasr_fst_decode_options();
  aasr_fst_default_options(&o->fst);
  o->lnabytes = 2;
  o->group = 256;
}

}  // extern "C"

namespace {

aasr_status run_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur, const char *recipe_path,
                       const aasr_fst_decode_options *opt, const aasr_fstnet *phone_net, const aasr_fst_confidence_options *conf,
                       aasr_run_stats *stats) {
  return guarded([&] {
    if (!net || !recipe_path || !opt || !opt->out) raise(AASR_ERR_INVALID, "aasr_run_fst_decode_recipe: null argument");
    const bool engine = !opt->lna_files;
    if (engine && (!feat || !gmm)) raise(AASR_ERR_INVALID, "aasr_run_fst_decode_recipe: engine mode needs a feature chain and a model");
    if (!engine && opt->speakers) raise(AASR_ERR_INVALID, "fst_decode: a speaker configuration belongs to engine mode");
    if (engine && opt->lnabytes != 2 && opt->lnabytes != 4) raise(AASR_ERR_INVALID, "Invalid number of LNA bytes");
    if (opt->group < 1) raise(AASR_ERR_INVALID, "fst_decode: the group must hold at least 1 utterance");
    if (conf && conf->phone_loop && !phone_net) raise(AASR_ERR_INVALID, "fst_decode: a phone loop without a phone-loop network");
    const int32_t max_pdf = std::max(aasr_fstnet_max_pdf(net), conf && conf->phone_loop ? aasr_fstnet_max_pdf(phone_net) : -1);
    aasr_fst_conf_options copt;
    aasr_fst_conf_default_options(&copt);
    if (conf) {
      copt.grammar = opt->fst;
      copt.phone = conf->phone;
      copt.phone_loop = conf->phone_loop;
      copt.verbose = opt->info > 0;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, false);
    for (const RecipeInfo &u : infos) {
      if (engine && u.audio_path.empty()) raise(AASR_ERR_INVALID, "fst_decode: a recipe line without audio=");
      if (!engine && u.lna_path.empty()) raise(AASR_ERR_INVALID, "fst_decode: --lna-files and a recipe line without lna=");
    }
    if (engine) {
      check_feature_dim(gmm, feat);
      if (max_pdf >= aasr_gmm_num_states(gmm))
        raise(AASR_ERR_INVALID, "fst_decode: the network names pdf %d, the model has %d states", max_pdf, aasr_gmm_num_states(gmm));
    }
    require_device();
    const bool to_stdout = strcmp(opt->out, "-") == 0;
    FILE *out = to_stdout ? stdout : fopen(opt->out, "w");
    if (!out) raise(AASR_ERR_IO, "could not open %s for writing", opt->out);
    struct Close {
      FILE *f;
      bool keep;
      ~Close() {
        if (f && !keep) fclose(f);
      }
    } closer{out, to_stdout};
    hipStream_t stream = nullptr;
    AASR_HIP(hipStreamCreate(&stream));
    std::unique_ptr<void, void (*)(void *)> stream_guard((void *)stream, [](void *s) { (void)hipStreamDestroy((hipStream_t)s); });
    // -S: a change of feature parameters waits for the features queued with the old ones
    struct Unhook {
      aasr_spkc *s;
      ~Unhook() {
        if (s) spkc_set_before_change(s, nullptr);
      }
    } unhook{opt->speakers};
    if (opt->speakers) spkc_set_before_change(opt->speakers, [&]() { (void)hipStreamSynchronize(stream); });

    DevBuf<int16_t> d_pcm;
    DevBuf<float> d_fea, d_scratch;
    DevBuf<uint8_t> d_lna;
    int64_t total_frames = 0;
    double device_seconds = 0;
    const float frame_rate = engine ? aasr_feat_frame_rate(feat) : 0;
    for (size_t g0 = 0; g0 < infos.size(); g0 += (size_t)opt->group) {
      const size_t g1 = std::min(infos.size(), g0 + (size_t)opt->group), n = g1 - g0;
      std::vector<int32_t> frames(n);
      std::vector<int64_t> row0(n + 1, 0);
      int lnabytes = opt->lnabytes, n_models = engine ? aasr_gmm_num_states(gmm) : 0;
      auto td = std::chrono::steady_clock::now();  // from the group's first upload to its last result
      if (engine) {
        // the group's input and frame ranges, then its samples in one device buffer
        std::vector<std::vector<int16_t>> audio(n);
        std::vector<int32_t> first(n);
        std::vector<int64_t> pcm_off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
          const RecipeInfo &u = infos[g0 + i];
          announce(u, opt->info, (int)(g0 + i), (int)infos.size());
          audio[i] = load_utterance_input(feat, u);
          int last;
          frame_range(u, frame_rate, &first[i], &last);
          const int eof = aasr_feat_eof_frame(feat, (int64_t)audio[i].size());
          if (eof < 1) raise(AASR_ERR_SHORT_AUDIO, "audio shorter than frame");
          const int stop = last > 0 ? std::min(last, eof) : eof;
          frames[i] = std::max(0, stop - first[i]);
          row0[i + 1] = row0[i] + frames[i];
          pcm_off[i + 1] = pcm_off[i] + (int64_t)audio[i].size();
        }
        td = std::chrono::steady_clock::now();
        const int64_t F = row0[n];
        const int dim = aasr_feat_dim(feat);
        AASR_HIP(hipStreamSynchronize(stream));  // (growing a buffer frees the old one)
        d_pcm.ensure((size_t)std::max<int64_t>(1, pcm_off[n]));
        d_fea.ensure((size_t)std::max<int64_t>(1, F * dim));
        d_scratch.ensure((size_t)std::max<int64_t>(1, aasr_gmm_score_scratch_floats(gmm, F)));
        d_lna.ensure((size_t)std::max<int64_t>(1, F * n_models * lnabytes));
        for (size_t i = 0; i < n; i++)
          if (!audio[i].empty())
            AASR_HIP(hipMemcpyAsync(d_pcm.p + pcm_off[i], audio[i].data(), audio[i].size() * sizeof(int16_t), hipMemcpyHostToDevice, stream));
        // features: one launch set per stretch of utterances with the same speaker settings (the whole group without -S)
        for (size_t a = 0; a < n;) {
          size_t e = a + 1;
          if (opt->speakers) {
            const RecipeInfo &ua = infos[g0 + a];
            while (e < n && infos[g0 + e].speaker_id == ua.speaker_id && infos[g0 + e].utterance_id == ua.utterance_id) e++;
            apply_speaker(opt->speakers, ua);  // aku/phone_probs.cc:191-196
          } else {
            e = n;
          }
          UttBatch ub;
          ub.n_utts = (int32_t)(e - a);
          for (size_t i = a; i <= e; i++) {
            ub.frame_off.push_back(row0[i] - row0[a]);
            ub.pcm_off.push_back(pcm_off[i] - pcm_off[a]);
          }
          ub.first.assign(first.begin() + (long)a, first.begin() + (long)e);
          if (row0[e] > row0[a])
            feat_run_batch(feat, d_pcm.p + pcm_off[a], ub, (int)feat->mods.size() - 1, d_fea.p + row0[a] * dim, nullptr, stream);
          a = e;
        }
        // one score + LNA step over the group; its output is the search's input, in place
        ok(aasr_gmm_score_lna_dev(gmm, d_fea.p, F, 1, lnabytes, d_scratch.p, d_lna.p, stream));
        AASR_HIP(hipStreamSynchronize(stream));  // (the samples are read from the group's host buffers)
      } else {
        std::vector<uint8_t> all;
        for (size_t i = 0; i < n; i++) {
          const std::string &name = infos[g0 + i].lna_path;
          std::ifstream in(name, std::ios::binary);
          if (!in) raise(AASR_ERR_IO, "could not open %s", name.c_str());
          const std::vector<uint8_t> image((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
          if (image.size() < 5) raise(AASR_ERR_INVALID, "fst_decode: %s is no LNA file", name.c_str());
          const int models = (image[0] << 24) | (image[1] << 16) | (image[2] << 8) | image[3], bytes = image[4];
          if (models <= 0) raise(AASR_ERR_INVALID, "LnaReaderCircular::open(): invalid number of states %d (%s)", models, name.c_str());
          if (bytes != 1 && bytes != 2 && bytes != 4)
            raise(AASR_ERR_INVALID, "LnaReaderCircular::open(): invalid LNA byte number %d (%s)", bytes, name.c_str());
          if (i == 0) {
            lnabytes = bytes;
            n_models = models;
          } else if (bytes != lnabytes || models != n_models) {
            raise(AASR_ERR_INVALID, "fst_decode: %s has %d models of %d bytes, the files before it in its group %d of %d", name.c_str(),
                  models, bytes, n_models, lnabytes);
          }
          const size_t row = (size_t)models * (size_t)bytes;
          frames[i] = (int32_t)((image.size() - 5) / row);  // (a partial last frame is the reader's end of file)
          row0[i + 1] = row0[i] + frames[i];
          all.insert(all.end(), image.begin() + 5, image.begin() + 5 + (long)((size_t)frames[i] * row));
        }
        if (max_pdf >= n_models)
          raise(AASR_ERR_INVALID, "fst_decode: the network names pdf %d, the acoustics have %d models", max_pdf, n_models);
        d_lna.ensure(std::max<size_t>(16, all.size()));
        if (!all.empty()) AASR_HIP(hipMemcpy(d_lna.p, all.data(), all.size(), hipMemcpyHostToDevice));
      }
      std::vector<Line> result(n);
      std::vector<size_t> which(n);
      for (size_t i = 0; i < n; i++) which[i] = i;
      if (conf) {
        aasr_fst_conf_options resolved;
        if (run_conf_batch(net, phone_net, dur, copt, frames, row0, which, d_lna.p, row0[n], lnabytes, n_models, stream, result, &resolved) > 0) {
          which.clear();
          for (size_t i = 0; i < n; i++)
            if (!result[i].conf.valid) which.push_back(i);
          double_capacities(resolved.grammar);
          double_capacities(resolved.phone);
          fprintf(stderr, "fst_decode: %zu utterances overflowed a capacity, running them again with twice as much\n", which.size());
          aasr_fst_conf_options again;
          run_conf_batch(net, phone_net, dur, resolved, frames, row0, which, d_lna.p, row0[n], lnabytes, n_models, stream, result, &again);
        }
      } else {
        aasr_fst_options resolved;
        if (run_batch(net, dur, opt->fst, frames, row0, which, d_lna.p, row0[n], lnabytes, n_models, stream, result, &resolved) > 0) {
          which.clear();
          for (size_t i = 0; i < n; i++)
            if (result[i].status >= AASR_FST_OVERFLOW_CANDIDATES) which.push_back(i);
          double_capacities(resolved);
          fprintf(stderr, "fst_decode: %zu utterances overflowed a capacity, running them again with twice as much\n", which.size());
          aasr_fst_options again;
          run_batch(net, dur, resolved, frames, row0, which, d_lna.p, row0[n], lnabytes, n_models, stream, result, &again);
        }
      }
      device_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count();
      total_frames += row0[n];
      for (size_t i = 0; i < n; i++) {
        const RecipeInfo &u = infos[g0 + i];
        fprintf(out, "%s %.9g", engine ? u.audio_path.c_str() : u.lna_path.c_str(), (double)result[i].logprob);
        if (conf) fprintf(out, " %.9g", (double)result[i].conf.confidence);
        for (int32_t w : result[i].words) fprintf(out, " %s", aasr_fstnet_symbol(net, w));
        const int32_t status = result[i].status != AASR_FST_OK || !conf ? result[i].status : result[i].conf.phone_status;
        if (status != AASR_FST_OK) fprintf(out, " %s", STATUS[status]);
        fprintf(out, "\n");
      }
      fflush(out);
    }
    if (stats) fill_run_stats(stats, (int64_t)infos.size(), total_frames, t0, device_seconds);
  });
}

}  // namespace

// logl.cc -- the log-likelihood of a recipe (aku/logl.cc): per utterance the sum of the frame log-likelihoods along
// a .phn state segmentation (seg_loglik.hip; logl.cc's transtat is an unset global, so no transition terms enter), or
// with -H / -D the forward total of the forward-backward pass over the utterance's HMM network (hmmnet_fb.hip) on the
// state log-likelihood rows of the model's scoring entry.  The recipe pass is the shared one (recipe_pass.h), the
// network step the network drivers' (network_pass.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "network_pass.h"
#include "phn_line.h"
#include "recipe_pass.h"
#include "stats.h"

using namespace aasr;

namespace {

constexpr int64_t PHN_GROUP_FRAMES = (int64_t)1 << 18;

// logl.cc:71-80
void print_file_line(const RecipeInfo &u, int info, double ll) {
  if (info <= 0) return;
  fprintf(stdout, "Log likelihood for file %s", u.audio_path.c_str());
  if (u.start_time || u.end_time) fprintf(stdout, " (%.2f-%.2f)", u.start_time, u.end_time);
  fprintf(stdout, ": %f\n", ll);
}

}  // namespace

extern "C" {

void aasr_logl_default_options(aasr_logl_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->ac_scale = 1;
}

aasr_status aasr_run_logl_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                 const aasr_logl_options *opt, double *total_log_likelihood, aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || !total_log_likelihood)
      raise(AASR_ERR_INVALID, "aasr_run_logl_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    if (opt->mpv) raise(AASR_ERR_UNSUPPORTED, "logl: --mpv (multipath Viterbi) is not supported");
    aasr_spkc *spk = opt->speakers;
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, true);
    refuse_line_limits(infos, "logl");
    check_feature_dim(gmm, feat);
    check_stats_model(gmm, "logl");
    const bool nets = opt->hmmnet || opt->den_hmmnet;
    const TopoTables tt(topo);
    const float fr = aasr_feat_frame_rate(feat);
    GroupStager stager(feat, spk);
    const hipStream_t stream = stager.stream;
    double total = 0;
    int64_t num_frames = 0;

    if (!nets) {
      aasr_segll *h = nullptr;
      {
        const aasr_status cs = aasr_segll_create(gmm, &h);
        if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
      }
      std::unique_ptr<aasr_segll, void (*)(aasr_segll *)> hguard(h, aasr_segll_destroy);
      const int phn_flags = opt->snl ? PHN_STATE_NUM_LABELS : 0;
      DevBuf<double> d_ll;
      std::vector<double> ll;
      size_t next = 0;
      while (next < infos.size()) {
        const size_t group_first = next;
        std::vector<std::vector<int16_t>> audio;
        std::vector<int32_t> start, rows, pdfs;
        std::vector<char> ok;
        int64_t rows_total = 0;
        while (next < infos.size() && audio.size() < 1024 && (audio.empty() || rows_total < PHN_GROUP_FRAMES)) {
          const RecipeInfo &u = infos[next++];
          audio.push_back(load_utterance_input(feat, u));
          int first, last;
          frame_range(u, fr, &first, &last);
          const Segmentation seg =
              read_segmentation(topo, tt, (opt->ophn ? u.alignment_path : u.transcript_path).c_str(), fr, first, last,
                                aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), false, phn_flags);
          if (!seg.initialized) {  // logl.cc:210-216
            fprintf(stderr, "Could not initialize the utterance for PhnReader.");
            fprintf(stderr, "Current file was: %s\n", u.audio_path.c_str());
            audio.back().clear();
          }
          ok.push_back(seg.initialized);
          start.push_back(seg.start_frame);
          rows.push_back((int32_t)seg.pdf.size());
          pdfs.insert(pdfs.end(), seg.pdf.begin(), seg.pdf.end());
          rows_total += (int64_t)seg.pdf.size();
        }
        stager.stage(audio, start, rows, [&](size_t i) { apply_speaker(spk, infos[group_first + i]); });
        if (rows_total > 0) {
          check_stats_model(gmm, "logl");  // (a speaker's cmllr block would have reached the model by now)
          d_ll.ensure((size_t)rows_total);
          if (aasr_segll_score_dev(h, stager.d_x.p, rows_total, pdfs.data(), d_ll.p, stream) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
          ll.resize((size_t)rows_total);
          AASR_HIP(hipMemcpyAsync(ll.data(), d_ll.p, ll.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
          AASR_HIP(hipStreamSynchronize(stream));
        }
        size_t row = 0;
        for (size_t i = 0; i < audio.size(); i++) {
          if (!ok[i]) continue;
          double cur = 0;  // the frames in order, safe_log(1 * state_likelihood) each (logl.cc:57-60)
          for (int32_t f = 0; f < rows[i]; f++) cur += ll[row + (size_t)f];
          row += (size_t)rows[i];
          print_file_line(infos[group_first + i], opt->info, cur);
          total += cur;
        }
        num_frames += rows_total;
      }
      *total_log_likelihood = total;
      fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, 0);
      return;
    }

    // ---- HMM networks ----
    aasr_fb_options fo;
    network_fb_options(&fo, opt->fw_beam, opt->bw_beam, opt->ac_scale_given != 0, opt->ac_scale, opt->vit != 0);
    StageTimers tm;
    tm.on = getenv("AASR_RECIPE_TIMING") != nullptr;
    const int S = aasr_gmm_num_states(gmm);
    const bool f64 = aasr_gmm_get_precision(gmm) == AASR_PREC_F64;
    NetworkCache net_cache(topo, S);
    GroupScores scores;
    size_t next = 0;
    while (next < infos.size()) {
      double t = now_s();
      const size_t group_first = next;
      NetworkGroup g;
      while (next < infos.size() && g.size() < 1024 &&
             (g.size() == 0 || (g.rows_total < NETWORK_GROUP_FRAMES && g.rows_total * S < NETWORK_GROUP_SCORES))) {
        const RecipeInfo &u = infos[next++];
        g.add(feat, net_cache, u, opt->den_hmmnet ? u.den_hmmnet_path : u.hmmnet_path, fr);
      }
      tm.host += now_s() - t;
      t = now_s();
      stager.stage(g.audio, g.start, g.rows, [&](size_t i) { apply_speaker(spk, infos[group_first + i]); });
      if (tm.on) AASR_HIP(hipStreamSynchronize(stream));
      tm.feat += now_s() - t;
      check_stats_model(gmm, "logl");
      const void *d_scores = nullptr;
      const FbBatchPtr b = run_network_group(fo, gmm, stager, g, scores, f64, &d_scores, &tm);
      for (size_t i = 0; i < g.size(); i++) {
        const RecipeInfo &u = infos[group_first + i];
        double fw = 0;
        if (!report_network_outcome(b.get(), i, fo, RetryMessages::BAUM_WELCH, u, &fw)) continue;
        print_file_line(u, opt->info, fw);
        total += fw;
      }
      num_frames += g.rows_total;
    }
    if (tm.on)
      fprintf(stderr, "logl timing: input and networks %.3f s, features %.3f s, scoring %.3f s, forward-backward %.3f s\n",
              tm.host, tm.feat, tm.score, tm.fb);
    *total_log_likelihood = total;
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, 0);
  });
}

}  // extern "C"

// network_pass.cc -- the forward-backward step of the network drivers (network_pass.h).
#include "network_pass.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

#include "feat.h"
#include "gmm.h"
#include "hmmnet.h"
#include "hmmnet_fb.h"

namespace aasr {

const aasr_hmmnet *NetworkCache::get(const std::string &path) {
  auto it = nets.find(path);
  if (it == nets.end()) {
    aasr_hmmnet *net = nullptr;
    const aasr_status rs = aasr_hmmnet_read(topo, path.c_str(), &net);
    if (rs != AASR_OK) raise(rs, "%s", last_error().c_str());
    it = nets.emplace(path, std::unique_ptr<aasr_hmmnet, void (*)(aasr_hmmnet *)>(net, aasr_hmmnet_destroy)).first;
  }
  for (int32_t pdf : it->second->pdfs)
    if (pdf >= num_states)
      raise(AASR_ERR_INVALID, "%s: state %d is not below the model's %d states", path.c_str(), pdf, num_states);
  return it->second.get();
}

void network_frame_range(const RecipeInfo &info, float frame_rate, int eof_frame, int *first, int *rows) {
  int last;
  frame_range(info, frame_rate, first, &last);
  const int end = last > 0 ? std::min(last, eof_frame) : eof_frame;
  if (end - *first < 1)
    raise(AASR_ERR_INVALID, "HmmNetBaumWelch: no frames for %s (frames %d to %d)", info.audio_path.c_str(), *first, end);
  if (end - *first == 1) fprintf(stderr, "HmmNetBaumWelch: Warning: Single frame utterance\n");
  *rows = end - *first;
}

const void *GroupScores::score(aasr_gmm *gmm, const double *d_x, int64_t n_rows, bool f64, hipStream_t stream) {
  const int S = aasr_gmm_num_states(gmm), D = aasr_gmm_dim(gmm);
  if (f64) {
    d_scores64.ensure((size_t)n_rows * S);
    if (aasr_gmm_score_f64_dev(gmm, d_x, n_rows, d_scores64.p, stream) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    return d_scores64.p;
  }
  // the scoring entry of the default mode takes float frames
  x64.resize((size_t)n_rows * D);
  AASR_HIP(hipMemcpyAsync(x64.data(), d_x, x64.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  AASR_HIP(hipStreamSynchronize(stream));
  x32.assign(x64.begin(), x64.end());
  d_x32.ensure(x32.size());
  d_scores32.ensure((size_t)n_rows * S);
  AASR_HIP(hipMemcpyAsync(d_x32.p, x32.data(), x32.size() * sizeof(float), hipMemcpyHostToDevice, stream));
  if (aasr_gmm_score_dev(gmm, d_x32.p, n_rows, d_scores32.p, stream) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  return d_scores32.p;
}

void network_fb_options(aasr_fb_options *fo, double fw_beam, double bw_beam, bool ac_scale_given, double ac_scale,
                        bool viterbi) {
  aasr_fb_default_options(fo);
  if (fw_beam > 0) fo->fw_beam = fw_beam;  // set_pruning_thresholds: 0 keeps the default
  if (bw_beam > 0) fo->bw_beam = bw_beam;
  if (ac_scale_given) fo->ac_scale = ac_scale;
  fo->mode = viterbi ? AASR_FB_VITERBI : AASR_FB_BAUM_WELCH;
}

void NetworkGroup::add(aasr_feat *feat, NetworkCache &cache, const RecipeInfo &info, const std::string &net_path,
                       float frame_rate) {
  audio.push_back(load_utterance_input(feat, info));
  // Recipe::Info::init_hmmnet_files (Recipe.cc:198-231)
  if (net_path.empty()) raise(AASR_ERR_INVALID, "Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe.");
  nets.push_back(cache.get(net_path));
  int first, n;
  network_frame_range(info, frame_rate, aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), &first, &n);
  start.push_back(first);
  rows.push_back(n);
  row0.push_back(rows_total);
  rows_total += n;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

FbBatchPtr run_network_group(const aasr_fb_options &fo, aasr_gmm *gmm, const GroupStager &stager, const NetworkGroup &g,
                             GroupScores &scores, bool f64, const void **d_scores, StageTimers *timers) {
  const hipStream_t stream = stager.stream;
  const int S = aasr_gmm_num_states(gmm);
  double t = now_s();
  *d_scores = scores.score(gmm, stager.d_x.p, g.rows_total, f64, stream);
  if (timers && timers->on) AASR_HIP(hipStreamSynchronize(stream));
  if (timers) timers->score += now_s() - t;
  t = now_s();
  aasr_fb_batch *b = nullptr;
  if (aasr_fb_batch_create(&fo, (int32_t)g.size(), g.nets.data(), g.rows.data(), &b) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  FbBatchPtr batch(b, aasr_fb_batch_destroy);
  int32_t failed = 0;
  for (int attempt = 1; attempt <= fo.max_attempts; attempt++) {
    if (aasr_fb_batch_dev(b, *d_scores, S, g.rows_total, f64 ? 1 : 0, g.row0.data(), attempt, stream) != AASR_OK ||
        aasr_fb_batch_sync(b, stream, &failed) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    if (failed == 0) break;
  }
  if (timers) timers->fb += now_s() - t;
  return batch;
}

bool report_network_outcome(const aasr_fb_batch *b, size_t i, const aasr_fb_options &fo, RetryMessages style,
                            const RecipeInfo &info, double *forward_total) {
  int32_t status = 0, attempts = 0;
  if (aasr_fb_batch_result(b, (int32_t)i, &status, nullptr, forward_total, &attempts, nullptr, nullptr) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  const bool gave_up = status == FB_FAILED_BACKWARD;
  if (style == RetryMessages::SEGMENTATOR) {
    if (attempts > 1 || gave_up) fprintf(stderr, "Could not initialize the utterance segmentation.\n");
    for (int k = 2; k <= attempts; k++) fprintf(stderr, "Increasing beam to %.1f\n", k * fo.bw_beam);
    if (gave_up) fprintf(stderr, "Giving up for this file\n");
  } else {
    for (int k = 2; k <= attempts; k++)
      fprintf(stderr, "Warning: Backward phase failed, increasing beam to %.1f\n", k * fo.bw_beam);
    if (gave_up) {
      fprintf(stderr, "Could not run Baum-Welch for file %s\n", info.audio_path.c_str());
      fprintf(stderr, "The HMM network may be incorrect or initial beam too low.\n");
    }
  }
  if (gave_up) return false;
  if (status != FB_OK) raise(AASR_ERR_INVALID, "No paths survived to the end of the network!");
  return true;
}

void check_frame_sums(aasr_fb_batch *b, size_t i, const NetworkGroup &g, const RecipeInfo &info, double *max_dev) {
  std::vector<double> sums((size_t)g.rows[i]);
  if (aasr_fb_batch_frame_sums(b, (int32_t)i, sums.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  for (int32_t f = 0; f < g.rows[i]; f++) {
    const double dev = std::fabs(1 - sums[(size_t)f]);
    if (dev > 0.02) {
      fprintf(stderr, "Warning: Sum of PDF probabilities is %g at frame %i\n", sums[(size_t)f], g.start[i] + f);
      if (sums[(size_t)f] < 0.01)  // (the reference exits here)
        raise(AASR_ERR_INVALID, "HmmNetBaumWelch: the sum of PDF probabilities is %g at frame %d of %s", sums[(size_t)f],
              g.start[i] + f, info.audio_path.c_str());
    }
    *max_dev = std::max(*max_dev, dev);
  }
}

}  // namespace aasr

// vtln.cc -- VTLN warp-factor estimation (aku/vtln.cc) over a recipe: per speaker a grid of warp factors, per grid
// point the utterances' features under that factor on the device and the log-likelihood of their .phn segmentations
// (seg_loglik.hip), summed per speaker on the host in the reference's order; the best factor of every speaker goes to
// the module and the speaker configuration, which writes the speaker file.  The grid arithmetic and the summary text
// are exported on their own (aasr_vtln_grid, aasr_vtln_summary_text).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "phn_line.h"
#include "recipe_pass.h"
#include "stats.h"

using namespace aasr;

namespace {

constexpr int64_t VTLN_GROUP_FRAMES = (int64_t)1 << 18;  // x the grid's size doubles of device and host memory
int64_t g_group_frames = VTLN_GROUP_FRAMES;

struct SpeakerStats {
  float center = 1;
  std::vector<float> warp_factors;
  std::vector<double> log_likelihoods;
};

// the module's warp factor as VtlnModule::get_warp_factor of the adapters reads it: the parameter block's "%g" text
float module_warp_factor(const aasr_feat *feat, const char *module) {
  char *text = nullptr;
  int64_t len = 0;
  if (aasr_feat_get_parameters(feat, module, &text, &len) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  const std::string t(text, (size_t)len);
  aasr_free(text);
  float wf = 1.0f;
  const size_t at = t.find("warp_factor");
  if (at != std::string::npos) wf = (float)strtod(t.c_str() + at + strlen("warp_factor"), nullptr);
  return wf;
}

std::string summary_text(const std::map<std::string, SpeakerStats> &speakers) {
  std::string out;
  char buf[128];
  for (const auto &kv : speakers) {
    out += "[" + kv.first + "]\n";
    for (size_t i = 0; i < kv.second.warp_factors.size(); i++) {
      snprintf(buf, sizeof buf, "%.3f: %.3f\n", kv.second.warp_factors[i], kv.second.log_likelihoods[i]);
      out += buf;
    }
    out += "\n";
  }
  return out;
}

}  // namespace

extern "C" {

void aasr_vtln_default_options(aasr_vtln_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->grid_size = 21;
  o->grid_rad = 0.1f;
}

void aasr_vtln_grid(const aasr_vtln_options *opt, float *start_out, float *step_out, int32_t *size_out) {
  if (!opt) return;
  float grid_start = opt->grid_rad;
  int grid_size = std::max(opt->grid_size, 1);
  float grid_step = 2 * grid_start / std::max(grid_size - 1, 1);
  if (opt->relative) {
    if (!opt->grid_rad_given) grid_start = 0.03;
    if (!opt->grid_size_given) grid_size = 5;
    grid_step = 2 * grid_start / std::max(grid_size - 1, 1);
  }
  grid_start = -grid_start;
  if (start_out) *start_out = grid_start;
  if (step_out) *step_out = grid_step;
  if (size_out) *size_out = grid_size;
}

aasr_status aasr_vtln_summary_text(const char *const *speakers, int32_t n_speakers, const int32_t *counts,
                                   const float *warps, const double *logliks, char **text, int64_t *len) {
  return guarded([&] {
    if (n_speakers < 0 || !text || !len || (n_speakers > 0 && (!speakers || !counts)))
      raise(AASR_ERR_INVALID, "aasr_vtln_summary_text: bad argument");
    std::map<std::string, SpeakerStats> m;
    size_t at = 0;
    for (int i = 0; i < n_speakers; i++) {
      if (!speakers[i] || counts[i] < 0 || (counts[i] > 0 && (!warps || !logliks)))
        raise(AASR_ERR_INVALID, "aasr_vtln_summary_text: bad argument");
      SpeakerStats &s = m[speakers[i]];
      s.warp_factors.insert(s.warp_factors.end(), warps + at, warps + at + counts[i]);
      s.log_likelihoods.insert(s.log_likelihoods.end(), logliks + at, logliks + at + counts[i]);
      at += (size_t)counts[i];
    }
    const std::string t = summary_text(m);
    char *out = (char *)malloc(t.size() + 1);
    if (!out) raise(AASR_ERR_INVALID, "aasr_vtln_summary_text: out of memory");
    memcpy(out, t.c_str(), t.size() + 1);
    *text = out;
    *len = (int64_t)t.size();
  });
}

void aasr_debug_vtln_set_group_frames(int64_t frames) { g_group_frames = frames > 0 ? frames : VTLN_GROUP_FRAMES; }

aasr_status aasr_run_vtln_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                 const aasr_vtln_options *opt, aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || !opt->speakers || !opt->module)
      raise(AASR_ERR_INVALID, "aasr_run_vtln_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    aasr_spkc *spk = opt->speakers;
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, true);
    refuse_line_limits(infos, "vtln");
    {  // dynamic_cast<VtlnModule *>(fea_gen.module(name)): an unknown name is the generator's message
      const char *type = nullptr;
      for (int i = 0; i < aasr_feat_num_modules(feat); i++)
        if (!strcmp(aasr_feat_module_name(feat, i), opt->module)) type = aasr_feat_module_type(feat, i);
      if (!type) raise(AASR_ERR_INVALID, "unknown module requested: %s", opt->module);
      if (strcmp(type, "vtln")) raise(AASR_ERR_INVALID, "Module %s is not a VTLN module", opt->module);
    }
    float grid_start, grid_step;
    int32_t grid_size;
    aasr_vtln_grid(opt, &grid_start, &grid_step, &grid_size);
    check_feature_dim(gmm, feat);
    for (const RecipeInfo &u : infos)
      if (u.speaker_id.empty()) raise(AASR_ERR_INVALID, "Speaker ID is missing");
    aasr_segll *h = nullptr;
    {
      const aasr_status cs = aasr_segll_create(gmm, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_segll, void (*)(aasr_segll *)> hguard(h, aasr_segll_destroy);
    const TopoTables tt(topo);
    const float fr = aasr_feat_frame_rate(feat);
    const int phn_flags = (opt->snl ? PHN_STATE_NUM_LABELS : 0) | (opt->rsamp ? PHN_RELATIVE_SAMPLES : 0);
    GroupStager stager(feat, spk);
    const hipStream_t stream = stager.stream;
    DevBuf<double> d_ll;
    std::vector<double> ll;
    std::map<std::string, SpeakerStats> speaker_stats;
    // the warp last written to the module, and the configuration's change count then: what an utterance with the
    // same settings need not write again (its features stay in flight with the previous one's)
    std::string module_text;
    int64_t module_changes = -1;
    int64_t num_frames = 0;

    // set_speaker (aku/vtln.cc:47-86) -> the index of the grid point's warp factor in the speaker's list
    auto set_speaker = [&](const RecipeInfo &u, int grid_iter) -> int {
      apply_speaker(spk, u);
      check_stats_model(gmm, "vtln");  // (a speaker's cmllr block would have reached the model by now)
      auto it = speaker_stats.find(u.speaker_id);
      if (it == speaker_stats.end()) {
        SpeakerStats s;
        s.center = opt->relative ? module_warp_factor(feat, opt->module) : 1;
        it = speaker_stats.emplace(u.speaker_id, s).first;
      }
      SpeakerStats &s = it->second;
      const float new_warp = s.center + grid_start + grid_iter * grid_step;
      // VtlnModule::set_warp_factor of the adapters: the parameter block, "%.9g" so that the float arrives bit for bit
      char buf[96];
      snprintf(buf, sizeof buf, "{\n  warp_factor %.9g\n}\n", (double)new_warp);
      const int64_t changes = aasr_spkc_num_changes(spk);
      if (changes != module_changes || module_text != buf) {
        AASR_HIP(hipStreamSynchronize(stream));  // the features queued with the old tables
        if (aasr_feat_set_parameters(feat, opt->module, buf) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        module_text = buf;
        module_changes = changes;
      }
      size_t i = 0;
      for (; i < s.warp_factors.size(); i++)
        if (fabs(new_warp - s.warp_factors[i]) < 1e-10) break;
      if (i == s.warp_factors.size()) {
        s.warp_factors.push_back(new_warp);
        s.log_likelihoods.push_back(0);
      }
      return (int)i;
    };

    size_t next = 0;
    while (next < infos.size()) {
      // host side first: audio and segmentation, the -i messages in recipe order
      const size_t group_first = next;
      std::vector<std::vector<int16_t>> audio;
      std::vector<int32_t> start, rows, pdfs;
      int64_t rows_total = 0;
      while (next < infos.size() && audio.size() < 1024 && (audio.empty() || rows_total < g_group_frames)) {
        const RecipeInfo &u = infos[next++];
        announce(u, opt->info);
        audio.push_back(load_utterance_input(feat, u));
        int first, last;
        frame_range(u, fr, &first, &last);
        const Segmentation seg =
            read_segmentation(topo, tt, (opt->ophn ? u.alignment_path : u.transcript_path).c_str(), fr, first, last,
                              aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), false, phn_flags);
        if (!seg.initialized) audio.back().clear();  // (no line: next_frame gives no frame, vtln.cc:97-99)
        start.push_back(seg.start_frame);
        rows.push_back((int32_t)seg.pdf.size());
        pdfs.insert(pdfs.end(), seg.pdf.begin(), seg.pdf.end());
        rows_total += (int64_t)seg.pdf.size();
      }
      const size_t n_utts = audio.size();
      d_ll.ensure((size_t)std::max<int64_t>(1, rows_total) * grid_size);
      // per grid point the group's features under its warp factors and their log-likelihoods into row `grid_iter`
      std::vector<int> warp_index((size_t)grid_size * n_utts);
      for (int grid_iter = 0; grid_iter < grid_size; grid_iter++) {
        stager.stage(audio, start, rows, [&](size_t i) {
          warp_index[(size_t)grid_iter * n_utts + i] = set_speaker(infos[group_first + i], grid_iter);
        });
        if (rows_total > 0 &&
            aasr_segll_score_dev(h, stager.d_x.p, rows_total, pdfs.data(), d_ll.p + (size_t)grid_iter * rows_total, stream) !=
                AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      }
      if (rows_total == 0) continue;
      ll.resize((size_t)rows_total * grid_size);
      AASR_HIP(hipMemcpyAsync(ll.data(), d_ll.p, ll.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
      AASR_HIP(hipStreamSynchronize(stream));
      // compute_vtln_log_likelihoods (aku/vtln.cc:93-114): per utterance the grid points one after the other, per
      // grid point the frames in order, each added to the speaker's running total for that warp factor
      size_t row = 0;
      for (size_t i = 0; i < n_utts; i++) {
        SpeakerStats &s = speaker_stats[infos[group_first + i].speaker_id];
        for (int grid_iter = 0; grid_iter < grid_size; grid_iter++) {
          double &total = s.log_likelihoods[(size_t)warp_index[(size_t)grid_iter * n_utts + i]];
          const double *v = &ll[(size_t)grid_iter * rows_total + row];
          for (int32_t f = 0; f < rows[i]; f++) total += v[f];
        }
        row += (size_t)rows[i];
      }
      num_frames += rows_total;
    }

    // find_best_warp_factors (aku/vtln.cc:131-151): the first strict maximum, speakers in the order of their ids
    AASR_HIP(hipStreamSynchronize(stream));
    for (const auto &kv : speaker_stats) {
      const SpeakerStats &s = kv.second;
      float best_wf = s.warp_factors[0];
      double best_ll = s.log_likelihoods[0];
      for (size_t i = 1; i < s.warp_factors.size(); i++)
        if (s.log_likelihoods[i] > best_ll) {
          best_ll = s.log_likelihoods[i];
          best_wf = s.warp_factors[i];
        }
      if (aasr_spkc_set_speaker(spk, kv.first.c_str()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      char buf[96];
      snprintf(buf, sizeof buf, "{\n  warp_factor %.9g\n}\n", (double)best_wf);
      if (aasr_feat_set_parameters(feat, opt->module, buf) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    if (opt->savesum) {
      const std::string t = summary_text(speaker_stats);
      write_text_file(opt->savesum, t.data(), t.size());
    }
    if (opt->out) {
      std::set<std::string> updated;
      for (const auto &kv : speaker_stats) updated.insert(kv.first);
      write_speaker_file_for_batch(spk, updated, opt->num_batches, opt->batch_index, opt->out);
    }
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, 0);
  });
}

}  // extern "C"

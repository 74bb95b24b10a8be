// dur_est.cc -- state duration models from state-numbered .phn files: aku/dur_est.cc's main (:142-218), collect_dur_stats
// (:33-44), write_dur_histograms (:46-55), estimate_gamma_models (:62-120) and write_gamma_models (:122-140) on the
// project's .phn line reader (phn_line.h) and topology handle.  Host only: nothing here touches the device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"
#include "phn_line.h"
#include "recipe_pass.h"

using namespace aasr;

namespace {

// PhnReader's line counting on top of next_phn_line (PhnReader.cc:296-297): no line after last_line
struct DurReader {
  FILE *f;
  float spf;
  int first_frame = 0, last_frame = 0, last_line = 0, line_no = 0;
  bool next(PhnLine *phn) {
    if (last_line > 0 && line_no >= last_line) return false;
    return next_phn_line(f, spf, first_frame, last_frame, &line_no, phn);
  }
};

// negative_gamma_loglikelihood (:57-60)
double negative_gamma_loglikelihood(double a, double mean_log, double log_mean) {
  return a * (1 + log_mean - log(a)) + lgamma(a) + (1 - a) * mean_log;
}

// estimate_gamma_models (:62-120), operation for operation
bool estimate_gamma(const int32_t *hist, int n, double *a_out, double *b_out) {
  double count, mean, var;
  double mean_log, log_mean;
  count = std::accumulate(hist, hist + n, 0);
  if (count < 2) return false;
  mean = 0;
  for (int i = 0; i < n; i++) mean += (i + 1) * hist[i];
  mean /= (double)count;
  var = 0;
  for (int i = 0; i < n; i++) var += (i + 1 - mean) * (i + 1 - mean) * hist[i];
  var = std::max(var / ((double)count - 1), 0.25);
  log_mean = log(mean);
  mean_log = 0;
  for (int i = 0; i < n; i++) mean_log += log(i + 1) * hist[i];
  mean_log /= (double)count;
  // the maximum likelihood solution by golden-section search
  double x1, x2, x1v, x2v;
  double a, b, r;
  r = (sqrt(5) - 1) / 2;
  a = 1;
  b = 2 * std::max(mean * mean / var, 1.5) - 1;
  x1 = a + (1 - r) * (b - a);
  x2 = a + r * (b - 1);  // (b - 1, as the reference has it; a is 1 here)
  x1v = negative_gamma_loglikelihood(x1, mean_log, log_mean);
  x2v = negative_gamma_loglikelihood(x2, mean_log, log_mean);
  while (b - a > 0.01) {
    if (x2v > x1v) {
      b = x2;
      x2 = x1;
      x2v = x1v;
      x1 = a + (1 - r) * (b - a);
      x1v = negative_gamma_loglikelihood(x1, mean_log, log_mean);
    } else {
      a = x1;
      x1 = x2;
      x1v = x2v;
      x2 = b - (1 - r) * (b - a);
      x2v = negative_gamma_loglikelihood(x2, mean_log, log_mean);
    }
  }
  *a_out = (a + b) / 2;
  *b_out = mean / *a_out;
  return true;
}

}  // namespace

extern "C" {

void aasr_dur_est_default_options(aasr_dur_est_options *o) {
  if (!o) return;
  *o = aasr_dur_est_options();
  o->maxdur = 100;
  o->mincount = 10;
}

int32_t aasr_dur_est_fit_gamma(const int32_t *hist, int32_t n, double *a, double *b) {
  if (!hist || n < 0 || !a || !b) return 0;
  return estimate_gamma(hist, n, a, b) ? 1 : 0;
}

aasr_status aasr_run_dur_est(const char *ph_path, const char *recipe_path, const aasr_dur_est_options *opt) {
  return guarded([&] {
    if (!ph_path || !recipe_path || !opt) raise(AASR_ERR_INVALID, "aasr_run_dur_est: null argument");
    aasr_topo *topo = nullptr;
    {
      const aasr_status st = aasr_topo_create_from_ph(ph_path, &topo);
      if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_topo, void (*)(aasr_topo *)> tguard(topo, aasr_topo_destroy);
    const int num_states = aasr_topo_num_states(topo);
    const int max_dur = opt->maxdur;
    if (max_dur < 1) raise(AASR_ERR_INVALID, "dur_est: --maxdur must be at least 1 (is %d)", max_dur);
    std::vector<std::vector<int32_t>> dur_table((size_t)num_states, std::vector<int32_t>((size_t)max_dur, 0));
    // dur_est reads its recipe whole, with cluster_speakers = false (:176)
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, 0, 0, false);
    const float frame_rate = 125;  // Recipe::Info::init_phn_files without a feature generator (Recipe.cc:158)
    for (const RecipeInfo &u : infos) {
      if (opt->info > 0) fprintf(stderr, "Processing file: %s\n", u.audio_path.c_str());
      const std::string &path = opt->ophn ? u.alignment_path : u.transcript_path;
      FILE *f = fopen(path.c_str(), "r");
      if (!f) raise(AASR_ERR_IO, "PhnReader::open(): could not open %s", path.c_str());
      std::unique_ptr<FILE, int (*)(FILE *)> fguard(f, fclose);
      DurReader rd{f, 16000 / frame_rate};
      PhnLine phn;
      if (u.start_time > 0 || u.end_time > 0) {  // set_frame_limits (PhnReader.cc:101-124)
        rd.first_frame = (int)(u.start_time * frame_rate);
        rd.last_frame = (int)(u.end_time * frame_rate);
        phn_skip_to_first_frame(f, rd.spf, rd.first_frame, rd.last_frame, &rd.line_no);
      }
      if (u.start_line > 0 || u.end_line > 0) {  // set_line_limits (:82-99): start_line lines are consumed
        rd.last_line = u.end_line;
        while (rd.line_no < u.start_line)
          if (!rd.next(&phn)) break;  // (the reference loops for ever here)
      }
      if (!rd.next(&phn)) {  // init_utterance_segmentation (:127-134) takes one line
        fprintf(stderr, "Could not initialize the utterance for PhnReader.");
        fprintf(stderr, "Current file was: %s\n", u.transcript_path.c_str());
        continue;
      }
      while (rd.next(&phn)) {
        if (phn.state == -1) raise(AASR_ERR_INVALID, "Collecting duration statistics requires phn files with state numbers!");
        const int hmm = aasr_topo_hmm_index(topo, phn.label.c_str());
        if (hmm < 0) raise(AASR_ERR_INVALID, "HmmSet::hmm_index(): unknown hmm '%s'", phn.label.c_str());
        const int ns = aasr_topo_hmm_num_states(topo, hmm);
        if (phn.state < 0 || phn.state >= ns)
          raise(AASR_ERR_INVALID, "dur_est: %s line %d: state %d of hmm '%s', which has %d", path.c_str(), rd.line_no, phn.state,
                phn.label.c_str(), ns);
        std::vector<int32_t> states((size_t)ns);
        if (aasr_topo_hmm_states(topo, hmm, states.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", last_error().c_str());
        const int state_index = states[(size_t)phn.state];
        if (state_index < opt->skip) continue;
        int num_frames = phn.end - phn.start;
        if (num_frames > max_dur) num_frames = max_dur;
        if (num_frames <= 0 || state_index >= num_states)  // (the reference's assert, and its tables' bounds)
          raise(AASR_ERR_INVALID, "dur_est: %s line %d: a duration of %d frames for state %d", path.c_str(), rd.line_no, num_frames,
                state_index);
        dur_table[(size_t)state_index][(size_t)num_frames - 1]++;
      }
    }
    if (opt->hist) {  // write_dur_histograms
      std::string text;
      for (int i = std::max(0, opt->skip); i < num_states; i++) {
        text += std::to_string(i) + " ";
        for (int32_t c : dur_table[(size_t)i]) text += std::to_string(c) + " ";
        text += "\n";
      }
      write_text_file(opt->hist, text.data(), text.size());
    }
    if (opt->gamma) {  // write_gamma_models
      std::string text = "4\n" + std::to_string(num_states) + "\n";
      char line[128];
      for (int i = 0; i < num_states; i++) {
        double a = 0, b = 0;
        const std::vector<int32_t> &h = dur_table[(size_t)i];
        bool ok = !(i < opt->skip || std::accumulate(h.begin(), h.end(), 0) < opt->mincount);
        if (ok && !estimate_gamma(h.data(), (int)h.size(), &a, &b)) {
          if (opt->info > 0) fprintf(stderr, "Warning: Needs at least 2 points for estimating gamma models\n");
          ok = false;
        }
        if (!ok) {
          if (opt->info > 0) fprintf(stderr, "Warning: No duration model for state %i\n", i);
          a = b = 0;
        }
        snprintf(line, sizeof line, "%d %.4f %.4f\n", i, a, b);
        text += line;
      }
      write_text_file(opt->gamma, text.data(), text.size());
    }
  });
}

}  // extern "C"

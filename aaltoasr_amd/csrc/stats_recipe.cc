// stats_recipe.cc -- the stats main loop over a recipe (aku/stats.cc:73-170, 540-620, 740-795) on the statistics
// handle (stats.cc): aasr_run_stats_recipe over .phn segmentations, or with aasr_run_stats_networks_recipe Baum-Welch
// over the recipe's HMM networks (network_pass.h; hmmnet_fb.hip, fb_entries.hip, stats_weighted.hip), with -a the
// alignment files of the best paths.  The segmentation reader is recipe_pass.cc's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "hmmnet.h"
#include "network_pass.h"
#include "recipe_pass.h"
#include "stats.h"

using namespace aasr;

namespace {

double safe_log(double x) { return x < 1e-50 ? std::log(1e-50) : std::log(x); }

// ---- Baum-Welch over the recipe's HMM networks (aku/stats.cc with -H) ----------------------------

// HmmNetBaumWelch::next_frame's label of an emitting arc (:763-768): the arc's label without its '#' end marks
// (LatticeLabel::remove_end_marks) -- the transition index, then the ";..." part the reader kept -- and, where that
// splits at ';' into three or more fields (mixture;state;phone;...), "phone.state"
std::string alignment_label(const aasr_hmmnet &net, int32_t arc) {
  std::string label = std::to_string(net.em_tr[(size_t)arc]);
  for (char c : net.em_label[(size_t)arc])
    if (c != '#') label += c;
  std::vector<std::string> fields;
  size_t at = 0;
  for (;;) {
    const size_t stop = label.find(';', at);
    fields.push_back(label.substr(at, stop == std::string::npos ? std::string::npos : stop - at));
    if (stop == std::string::npos) break;
    at = stop + 1;
  }
  return fields.size() >= 3 ? fields[2] + "." + fields[1] : label;
}

// The alignment file of one utterance as simple_train writes it (aku/stats.cc:116-131, 179-188): runs of one label text,
// "start end label" in samples; the last line ends one frame past the range (the reference's own "+1": next_frame has
// stepped once more before it returned false).  cache: the network's labels, filled as they are asked for.
std::string alignment_text(const aasr_hmmnet &net, std::vector<std::string> &cache, const std::vector<int32_t> &path, int first_frame,
                           int frame_mult) {
  cache.resize(net.em_src.size());
  std::string text;
  char head[64];
  int cur_start = -1;
  const std::string *cur = nullptr;
  auto put = [&](int end) {
    snprintf(head, sizeof head, "%d %d ", cur_start * frame_mult, end * frame_mult);
    text += head;
    text += *cur;
    text += '\n';
  };
  for (size_t t = 0; t < path.size(); t++) {
    std::string &label = cache[(size_t)path[t]];
    if (label.empty()) label = alignment_label(net, path[t]);
    const int frame = first_frame + (int)t;
    if (cur_start < 0) {
      cur_start = frame;
      cur = &label;
    } else if (*cur != label) {
      put(frame);
      cur_start = frame;
      cur = &label;
    }
  }
  if (cur_start >= 0) put(first_frame + (int)path.size() + 1);
  return text;
}

// The network mode of aasr_run_stats_recipe: per group the network step (network_pass.h), then the occupancies as
// weighted entries into the accumulation.  -> total_ll, num_frames of the utterances that ran
void run_stats_networks(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const std::vector<RecipeInfo> &infos,
                        const aasr_stats_options *opt, const aasr_stats_network_options *nopt, aasr_stats *h,
                        GroupStager &stager, double *total_ll, int64_t *num_frames) {
  const hipStream_t stream = stager.stream;
  const bool accumulate = !opt->no_train, transitions = opt->transitions != 0;
  StageTimers tm;
  tm.on = getenv("AASR_RECIPE_TIMING") != nullptr;
  aasr_fb_options fo;
  network_fb_options(&fo, nopt->fw_beam, nopt->bw_beam, nopt->ac_scale_given != 0, nopt->ac_scale, nopt->viterbi != 0);
  fo.want_pdf_occ = 1;
  fo.device_occ = 1;
  fo.want_tr_occ = transitions ? 1 : 0;
  fo.want_path = nopt->alignment ? 1 : 0;
  std::map<const aasr_hmmnet *, std::vector<std::string>> labels;  // per network, per emitting arc ("" until asked for)
  std::vector<int32_t> path;
  const int frame_mult = (int)(16000 / aasr_feat_frame_rate(feat));  // print_alignment_line (aku/stats.cc:59-70)
  const int S = aasr_gmm_num_states(gmm);
  const bool f64 = aasr_gmm_get_precision(gmm) == AASR_PREC_F64;
  const float fr = aasr_feat_frame_rate(feat);
  NetworkCache net_cache(topo, S);
  GroupScores scores;
  std::vector<int64_t> cnt((size_t)S + 1);
  std::vector<double> tr_occ;
  double max_dev = 0;  // max |1 - s_t| over the run
  int64_t entries = 0;
  size_t next = 0;
  while (next < infos.size()) {
    double t = now_s();
    const size_t group_first = next;
    NetworkGroup g;
    std::vector<char> align_open;  // with -a: the utterance's alignment file could be opened
    while (next < infos.size() && g.size() < 1024 &&
           (g.size() == 0 || (g.rows_total < NETWORK_GROUP_FRAMES && g.rows_total * S < NETWORK_GROUP_SCORES))) {
      const RecipeInfo &u = infos[next++];
      announce(u, opt->info);
      if (nopt->alignment) {  // aku/stats.cc:565-572: the file exists, empty, before the utterance is looked at
        FILE *af = fopen(u.alignment_path.c_str(), "w");
        if (!af) fprintf(stderr, "Could not open alignment file %s\n", u.alignment_path.c_str());
        else fclose(af);
        align_open.push_back(af != nullptr);
      }
      g.add(feat, net_cache, u, u.hmmnet_path, fr);
    }
    tm.host += now_s() - t;
    t = now_s();
    stager.stage(g.audio, g.start, g.rows, [&](size_t i) {
      if (!opt->speakers) return;
      apply_speaker(opt->speakers, infos[group_first + i], opt->uttadap != 0);
      check_stats_model(gmm);
    });
    if (tm.on) AASR_HIP(hipStreamSynchronize(stream));
    tm.feat += now_s() - t;
    const void *d_scores = nullptr;
    const FbBatchPtr batch = run_network_group(fo, gmm, stager, g, scores, f64, &d_scores, &tm);
    aasr_fb_batch *b = batch.get();
    t = now_s();
    const int32_t *d_rows = nullptr;
    const double *d_weights = nullptr;
    if (aasr_fb_batch_entries_dev(b, S, g.row0.data(), stream, cnt.data(), &d_rows, &d_weights) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    entries += cnt[(size_t)S];
    tm.fb += now_s() - t;
    t = now_s();
    // the messages in recipe order, the frame sums and the alignment files
    std::vector<char> ran(g.size(), 0);
    for (size_t i = 0; i < g.size(); i++) {
      const RecipeInfo &u = infos[group_first + i];
      if (!report_network_outcome(b, i, fo, RetryMessages::SEGMENTATOR, u)) continue;
      ran[i] = 1;
      check_frame_sums(b, i, g, u, &max_dev);
      if (nopt->alignment && align_open[i]) {
        path.resize((size_t)g.rows[i]);
        if (aasr_fb_batch_path(b, (int32_t)i, path.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        const std::string text = alignment_text(*g.nets[i], labels[g.nets[i]], path, g.start[i], frame_mult);
        write_text_file(u.alignment_path.c_str(), text.data(), text.size());
      }
    }
    if (accumulate && cnt[(size_t)S] > 0 &&
        aasr_stats_accumulate_weighted_dev(h, stager.d_x.p, g.rows_total, cnt.data(), d_rows, d_weights, stream) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    for (size_t i = 0; i < g.size(); i++) {
      if (!ran[i]) continue;
      const aasr_hmmnet &net = *g.nets[i];
      double fw = 0;
      tr_occ.assign(std::max<size_t>(1, net.trs.size()), 0.0);
      if (aasr_fb_batch_result(b, (int32_t)i, nullptr, nullptr, &fw, nullptr, nullptr, transitions ? tr_occ.data() : nullptr) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (accumulate && transitions)
        for (size_t k = 0; k < net.trs.size(); k++) {
          if (net.trs[k] < 0 || (size_t)net.trs[k] >= h->tr_count.size())
            raise(AASR_ERR_INVALID, "%s: transition %d is not one of the model's %zu", infos[group_first + i].hmmnet_path.c_str(),
                  net.trs[k], h->tr_count.size());
          h->tr_count[(size_t)net.trs[k]] += tr_occ[k];
        }
      fprintf(stderr, "  %g\n", fw);  // simple_train: the segmentator's total log-likelihood
      *total_ll += fw;
      *num_frames += g.rows[i];
    }
    // the batch owns the entries that the accumulation reads: it goes when the stream is done with them
    AASR_HIP(hipStreamSynchronize(stream));
    tm.acc += now_s() - t;
  }
  if (opt->info > 0) {
    fprintf(stderr, "Largest |1 - sum of PDF probabilities| of a frame: %g\n", max_dev);
    fprintf(stderr, "Weighted entries: %lld over %lld frames\n", (long long)entries, (long long)*num_frames);
  }
  if (tm.on)
    fprintf(stderr,
            "stats timing: input and networks %.3f s, features %.3f s, scoring %.3f s, forward-backward and entries %.3f s, "
            "accumulation %.3f s\n",
            tm.host, tm.feat, tm.score, tm.fb, tm.acc);
}

}  // namespace

static aasr_status run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                    const aasr_stats_options *opt, const aasr_stats_network_options *nopt,
                                    aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || (!opt->no_train && !opt->out))
      raise(AASR_ERR_INVALID, "%s: null argument", nopt ? "aasr_run_stats_networks_recipe" : "aasr_run_stats_recipe");
    const auto t0 = std::chrono::steady_clock::now();
    check_feature_dim(gmm, feat);
    if (nopt && opt->full_stats)
      raise(AASR_ERR_UNSUPPORTED, "stats: --full-stats is not supported with --networks (full second moments are collected over .phn files only)");
    if (nopt && nopt->alignment && opt->ophn) raise(AASR_ERR_INVALID, "Can not read and write to output PHNs");  // aku/stats.cc:516-517
    if (nopt && nopt->alignment && !nopt->viterbi)
      raise(AASR_ERR_UNSUPPORTED, "stats: alignment output needs the Viterbi mode (-M vit): under Baum-Welch no single arc belongs to a frame");
    if (nopt && opt->ophn)
      raise(AASR_ERR_UNSUPPORTED, "stats: -O is not supported with --networks (a network line has no segmentation to choose)");
    // stats reads its recipe with cluster_speakers = false (aku/stats.cc:422-424)
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, false);
    refuse_line_limits(infos, "stats");
    aasr_stats *h = nullptr;
    {  // (a model the accumulation kernel has no shape for keeps its AASR_ERR_UNSUPPORTED)
      const aasr_status cs = opt->full_stats && !opt->no_train ? aasr_stats_create_full(gmm, topo, &h) : aasr_stats_create(gmm, topo, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_stats, void (*)(aasr_stats *)> hguard(h, aasr_stats_destroy);
    const TopoTables tt(topo);
    const float fr = aasr_feat_frame_rate(feat);
    const bool accumulate = !opt->no_train, transitions = opt->transitions != 0;
    GroupStager stager(feat, opt->speakers);
    const hipStream_t stream = stager.stream;
    DevBuf<double> d_ll;
    double total_ll = 0;
    int64_t num_frames = 0;
    // groups of utterances accumulated in one launch; their frames stay on the device
    const int64_t max_group_frames = (int64_t)1 << 20;
    size_t next = 0;
    if (nopt) {
      run_stats_networks(feat, gmm, topo, infos, opt, nopt, h, stager, &total_ll, &num_frames);
      next = infos.size();
    }
    while (next < infos.size()) {
      // host side first: audio and segmentation, the -i messages in recipe order
      const size_t group_first = next;
      std::vector<std::vector<int16_t>> audio;
      std::vector<Segmentation> segs;
      std::vector<int32_t> start, rows, pdfs;
      int64_t rows_total = 0;
      while (next < infos.size() && audio.size() < 1024 && rows_total < max_group_frames) {
        const RecipeInfo &u = infos[next++];
        announce(u, opt->info);
        audio.push_back(load_utterance_input(feat, u));
        int first, last;
        frame_range(u, fr, &first, &last);
        segs.push_back(read_segmentation(topo, tt, (opt->ophn ? u.alignment_path : u.transcript_path).c_str(), fr, first,
                                         last, aasr_feat_eof_frame(feat, (int64_t)audio.back().size()), transitions));
        const Segmentation &seg = segs.back();
        if (!seg.initialized) {
          fprintf(stderr, "Could not initialize the utterance segmentation.\n");
          fprintf(stderr, "Giving up for this file\n");
          audio.back().clear();  // no frames; kept in the group for its speaker settings (stats.cc:560-565 run first)
        }
        start.push_back(seg.start_frame);
        rows.push_back((int32_t)seg.pdf.size());
        pdfs.insert(pdfs.end(), seg.pdf.begin(), seg.pdf.end());
        rows_total += (int64_t)seg.pdf.size();
      }
      d_ll.ensure((size_t)std::max<int64_t>(1, rows_total));
      // features of the group into one device buffer, speaker configuration per utterance
      stager.stage(audio, start, rows, [&](size_t i) {
        if (!opt->speakers) return;
        apply_speaker(opt->speakers, infos[group_first + i], opt->uttadap != 0);
        check_stats_model(gmm);
      });
      if (accumulate && transitions)
        for (const Segmentation &seg : segs)
          if (aasr_stats_add_transitions(h, seg.tr.data(), (int64_t)seg.tr.size()) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      if (rows_total == 0) continue;
      if (aasr_stats_accumulate_dev(h, stager.d_x.p, rows_total, pdfs.data(), d_ll.p, stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      // the .lls figure in frame order: state likelihoods, then the transition taken (stats.cc:130-160)
      std::vector<double> ll((size_t)rows_total);
      AASR_HIP(hipMemcpyAsync(ll.data(), d_ll.p, ll.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
      AASR_HIP(hipStreamSynchronize(stream));
      size_t row = 0;
      for (const Segmentation &seg : segs)
        for (size_t f = 0; f < seg.pdf.size(); f++) {
          total_ll += ll[row++];  // safe_log(1.0 * state_likelihood): the kernel's safe_log(total)
          if (!(transitions && accumulate) || seg.tr[f] < 0) continue;
          const int t = seg.tr[f], s = h->tr_source[(size_t)t];
          total_ll += safe_log(1.0 * tt.probs[(size_t)s][(size_t)(t - tt.tr_base[(size_t)s])]);
        }
      num_frames += rows_total;
    }
    if (opt->info > 0) {
      fprintf(stderr, "Finished collecting statistics (%i/%i)\n", opt->batch_index, opt->num_batches);
      fprintf(stderr, "Total num log likelihood: %g\n", total_ll);
    }
    const std::string out = opt->out ? opt->out : "";
    if (accumulate) {
      if (aasr_stats_fetch(h, stream) != AASR_OK || aasr_stats_write(h, out.c_str()) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    if (opt->out) {
      const aasr_status st = aasr_stats_write_lls((out + ".lls").c_str(), total_ll, num_frames);
      if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    }
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, 0);
  });
}

extern "C" {

void aasr_stats_default_options(aasr_stats_options *o) {
  if (o) memset(o, 0, sizeof *o);
}

aasr_status aasr_run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                  const aasr_stats_options *opt, aasr_run_stats *stats) {
  return run_stats_recipe(feat, gmm, topo, recipe_path, opt, nullptr, stats);
}

void aasr_stats_network_default_options(aasr_stats_network_options *o) {
  if (o) memset(o, 0, sizeof *o);
  if (o) o->ac_scale = 1;
}

aasr_status aasr_run_stats_networks_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                           const aasr_stats_options *opt, const aasr_stats_network_options *net,
                                           aasr_run_stats *stats) {
  aasr_stats_network_options defaults;
  aasr_stats_network_default_options(&defaults);
  return run_stats_recipe(feat, gmm, topo, recipe_path, opt, net ? net : &defaults, stats);
}

}  // extern "C"

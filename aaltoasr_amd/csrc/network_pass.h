// network_pass.h -- the forward-backward step over a recipe's HMM networks that the network drivers share (logl -H / -D,
// stats --networks, mllr --networks): per line the network and its frame range, per staged group the state scores, one
// forward-backward batch with its retries, per utterance the messages and the frame-sum check.  When a group is full,
// which network of a line goes in and what a tool does with an utterance that ran stay in its driver.  Internal, not
// exported.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "recipe_pass.h"

namespace aasr {

// A group's frames and its score buffer (rows x states) at most, where a driver cuts by them
constexpr int64_t NETWORK_GROUP_FRAMES = (int64_t)1 << 18;
constexpr int64_t NETWORK_GROUP_SCORES = (int64_t)1 << 27;

// The recipe's HMM networks (hmmnet.h), each file read once: Recipe::Info::init_hmmnet_files (Recipe.cc:198-231).  A
// network with a state the model does not have is refused.
struct NetworkCache {
  const aasr_topo *topo;
  int32_t num_states;
  std::map<std::string, std::unique_ptr<aasr_hmmnet, void (*)(aasr_hmmnet *)>> nets;
  NetworkCache(const aasr_topo *topo_, int32_t num_states_) : topo(topo_), num_states(num_states_) {}
  const aasr_hmmnet *get(const std::string &path);
};

// The frames of a network line (Recipe.cc:223-228, HmmNetBaumWelch::generate_features): first .. last, or to the last
// frame of the audio; a limit past the audio is cut to it.  No frames is an error, one frame the reference's warning.
void network_frame_range(const RecipeInfo &info, float frame_rate, int eof_frame, int *first, int *rows);

// State log-likelihood rows of a staged group from the model's scoring entry in the model's precision mode: double
// rows under AASR_PREC_F64, float rows (from float frames, as that entry takes them) otherwise.
struct GroupScores {
  DevBuf<double> d_scores64;
  DevBuf<float> d_scores32, d_x32;
  std::vector<double> x64;
  std::vector<float> x32;
  // -> the rows [n_rows x states] on the device, queued on `stream`
  const void *score(aasr_gmm *gmm, const double *d_x, int64_t n_rows, bool f64, hipStream_t stream);
};

// set_pruning_thresholds, set_acoustic_scaling and the mode of a tool's command line on top of the defaults: a beam of
// 0 keeps the default, the scale applies only when it was given.  The want_* flags stay the caller's.
void network_fb_options(aasr_fb_options *fo, double fw_beam, double bw_beam, bool ac_scale_given, double ac_scale,
                        bool viterbi);

// The utterances of a group: what GroupStager::stage and the forward-backward batch take of them.
struct NetworkGroup {
  std::vector<std::vector<int16_t>> audio;
  std::vector<int32_t> start, rows;
  std::vector<const aasr_hmmnet *> nets;
  std::vector<int64_t> row0;  // the frame row of every utterance's first frame
  int64_t rows_total = 0;
  size_t size() const { return nets.size(); }
  // The line's input, its network net_path (hmmnet_path, or den_hmmnet_path for logl -D; empty: init_hmmnet_files'
  // error) and its frame range
  void add(aasr_feat *feat, NetworkCache &cache, const RecipeInfo &info, const std::string &net_path, float frame_rate);
};

// Seconds per stage of a network driver (AASR_RECIPE_TIMING: `on` makes the stages wait for the stream)
struct StageTimers {
  bool on = false;
  double host = 0, feat = 0, score = 0, fb = 0, acc = 0;
};
double now_s();

typedef std::unique_ptr<aasr_fb_batch, void (*)(aasr_fb_batch *)> FbBatchPtr;

// The step for a group whose frames stager holds: state scores, the batch, attempt 1 and, with 2x ... max_attempts x
// the backward beam, new launches over the utterances whose backward pass failed (aku/logl.cc:183-199, stats.cc:79-102,
// mllr.cc:87-102).  -> the batch, synced; *d_scores: the score rows [rows_total x states] it ran on
FbBatchPtr run_network_group(const aasr_fb_options &fo, aasr_gmm *gmm, const GroupStager &stager, const NetworkGroup &g,
                             GroupScores &scores, bool f64, const void **d_scores, StageTimers *timers = nullptr);

// How a tool words its retries: simple_train's segmentator (aku/stats.cc:79-102) or the Baum-Welch loop of logl and
// mllr (aku/logl.cc:183-199, mllr.cc:87-102)
enum class RetryMessages { SEGMENTATOR, BAUM_WELCH };
// Utterance i of a synced batch: its retry messages on stderr, then false with the give-up message when its backward
// pass never succeeded, true when it ran (*forward_total: get_total_log_likelihood); any other status raises "No paths
// survived to the end of the network!"
bool report_network_outcome(const aasr_fb_batch *b, size_t i, const aasr_fb_options &fo, RetryMessages style,
                            const RecipeInfo &info, double *forward_total = nullptr);

// HmmNetBaumWelch::next_frame's sanity check (:772-779) on utterance i's frame sums s_t, after the batch's entries were
// made: the reference's warning beyond |1 - s_t| = 0.02, an error where it exits (s_t < 0.01); *max_dev: the largest
// |1 - s_t| so far
void check_frame_sums(aasr_fb_batch *b, size_t i, const NetworkGroup &g, const RecipeInfo &info, double *max_dev);

}  // namespace aasr

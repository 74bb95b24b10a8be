// recipe_pass.h -- the pass over a recipe that the training drivers share (stats.cc, mllr.cc, lda.cc; align.cc takes
// the recipe reader, the frame range and the message): read the recipe, per line load the input and the .phn
// segmentation, stage a group of utterances' frames in one device buffer.  What a tool does with the staged frames,
// how it cuts its groups and when it talks to the speaker configuration stays in its driver.  Internal, not exported.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "common.h"
#include "pipeline.h"

namespace aasr {

// Recipe::read of the file: "could not open recipe %s" or the lines of this batch
std::vector<RecipeInfo> read_recipe_file(const char *path, int num_batches, int batch_index, bool cluster_speakers);
// "<tool>: recipe line limits (start-line / end-line) are not supported" for the first line that has one
void refuse_line_limits(const std::vector<RecipeInfo> &infos, const char *tool);
// "gaussian dimension is %d but feature dimension is %d"
void check_feature_dim(const aasr_gmm *gmm, const aasr_feat *feat);
// FeatureGenerator::open(audio_path): the feature file of a pre module or the audio file, in the engine's input units
std::vector<int16_t> load_utterance_input(const aasr_feat *feat, const RecipeInfo &info);
// the line's start-time / end-time in frames (Recipe.cc:170-172); 0, 0 without either
void frame_range(const RecipeInfo &info, float frame_rate, int *first, int *last);
// "Processing file: <audio>[ (index+1/total)][ (start-end)]" on stderr at info_level > 0; index < 0: no (i/n)
void announce(const RecipeInfo &info, int info_level, int index = -1, int total = 0);

// What the segmentation reader needs of the topology: per HMM its states, per state its transitions' target offsets
// and the global index of its first transition (HmmSet::read_ph numbers transitions state by state, HmmSet.cc:319-328).
struct TopoTables {
  std::vector<std::vector<int32_t>> hmm_states;
  std::vector<std::vector<int32_t>> offsets;
  std::vector<std::vector<double>> probs;
  std::vector<int32_t> tr_base;
  int32_t n_transitions = 0;
  explicit TopoTables(const aasr_topo *topo);
};

struct Segmentation {
  bool initialized = false;  // init_utterance_segmentation succeeded
  int32_t start_frame = 0;   // frame of pdf[0]
  std::vector<int32_t> pdf;  // per frame
  std::vector<int32_t> tr;   // per frame: global transition index, -1: none; empty unless transitions were asked for
};

// PhnReader::next_frame (aku/PhnReader.cc:138-292), driven as stats.cc:simple_train drives it: frames until the
// reader's end, the frame loop leaving at eof_frame (< 0: no limit) after next_frame has run for it.  phn_flags: the
// reader's state_num_labels and relative_sample_numbers (phn_line.h), neither by default.  With state-number labels
// the line's number is the state (and pdf) index itself; transitions are refused with them (the reader's "first out
// transition" guess, PhnReader.cc:234-243, is not built).
Segmentation read_segmentation(const aasr_topo *topo, const TopoTables &tt, const char *path, float frame_rate,
                               int first_frame, int last_frame, int eof_frame, bool want_transitions, int phn_flags = 0);
// The state sequence of a recipe line as mllr and lda take it (aku/mllr.cc:111-115, lda.cc:212-218): the line's frame
// range, no transitions; a segmentation that cannot be initialised is reported on stderr and has no frames.
Segmentation read_state_sequence(const aasr_topo *topo, const TopoTables &tt, const RecipeInfo &info, bool ophn,
                                 float frame_rate, int eof_frame);

// A line's speaker and, when asked for, its utterance (where it has an id) in the speaker configuration, as the tools
// do per line before its features are made; nothing without a configuration
void apply_speaker(aasr_spkc *spk, const RecipeInfo &u, bool utterance = true);

// The frames of a group of utterances in one device buffer: the stream, the group's input and its frames [rows x dim]
// of module `target` (< 0: the chain's output).  With a speaker configuration, a change that rewrites feature
// parameters waits for the features queued with the old ones; utterances whose settings stay the same stay in flight
// together.
struct GroupStager {
  aasr_feat *feat;
  aasr_spkc *speakers;
  int target, dim;
  hipStream_t stream = nullptr;
  std::unique_ptr<void, void (*)(void *)> stream_guard;
  DevBuf<int16_t> d_pcm;
  DevBuf<double> d_x;
  GroupStager(aasr_feat *feat, aasr_spkc *speakers, int target = -1);
  ~GroupStager();
  // Queues utterance i's input audio[i] and its frames start[i] ... start[i] + rows[i] into d_x, row after row;
  // before_utterance(i) runs first (the tool's speaker settings).  An utterance without rows queues nothing.
  // The group's audio stays the caller's until the stream has been waited for.  -> the group's rows
  int64_t stage(const std::vector<std::vector<int16_t>> &audio, const std::vector<int32_t> &start,
                const std::vector<int32_t> &rows, const std::function<void(size_t)> &before_utterance);
};

// The speaker file an adaptation tool writes (aku/mllr.cc:318-332, vtln.cc:269-286): every entry of the configuration,
// or with batches (num_batches > 1) the speakers the batch has seen, "default" from batch 1 only, and no utterances.
void write_speaker_file_for_batch(aasr_spkc *speakers, std::set<std::string> seen, int num_batches, int batch_index,
                                  const char *path);

void fill_run_stats(aasr_run_stats *stats, int64_t utterances, int64_t frames,
                    std::chrono::steady_clock::time_point t0, double seconds_device);
// "could not open %s for writing" / "write error on %s"
void write_text_file(const char *path, const char *data, size_t len);

}  // namespace aasr

// recipe_pass.cc -- the recipe pass of the training drivers (recipe_pass.h).
#include "recipe_pass.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>

#include "feat.h"
#include "gmm.h"
#include "phn_line.h"

namespace aasr {

std::vector<RecipeInfo> read_recipe_file(const char *path, int num_batches, int batch_index, bool cluster_speakers) {
  std::ifstream rin(path);
  if (!rin) raise(AASR_ERR_IO, "could not open recipe %s", path);
  std::stringstream ss;
  ss << rin.rdbuf();
  return recipe_read(ss.str(), num_batches, batch_index, cluster_speakers);
}

void refuse_line_limits(const std::vector<RecipeInfo> &infos, const char *tool) {
  for (const RecipeInfo &u : infos)
    if (u.start_line > 0 || u.end_line > 0)
      raise(AASR_ERR_UNSUPPORTED, "%s: recipe line limits (start-line / end-line) are not supported", tool);
}

void check_feature_dim(const aasr_gmm *gmm, const aasr_feat *feat) {
  if (aasr_gmm_dim(gmm) != aasr_feat_dim(feat))
    raise(AASR_ERR_INVALID, "gaussian dimension is %d but feature dimension is %d", aasr_gmm_dim(gmm), aasr_feat_dim(feat));
}

std::vector<int16_t> load_utterance_input(const aasr_feat *feat, const RecipeInfo &info) {
  int16_t *pcm = nullptr;
  int64_t n_samples = 0;
  int32_t rate = 0;
  if (aasr_feat_input_is_features(feat)) {  // a pre module: feacat's feature file, in the engine's input units
    std::ifstream in(info.audio_path, std::ios::binary);
    if (!in) raise(AASR_ERR_IO, "could not open %s", info.audio_path.c_str());
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (aasr_audio_decode(feat, bytes.data(), (int64_t)bytes.size(), &pcm, &n_samples, &rate) != AASR_OK)
      raise(AASR_ERR_IO, "%s: %s", info.audio_path.c_str(), aasr_last_error());
  } else if (aasr_audio_read(feat, info.audio_path.c_str(), &pcm, &n_samples, &rate) != AASR_OK) {
    raise(AASR_ERR_IO, "%s", aasr_last_error());
  }
  std::vector<int16_t> out(pcm, pcm + n_samples);
  aasr_free(pcm);
  return out;
}

void frame_range(const RecipeInfo &info, float frame_rate, int *first, int *last) {
  *first = *last = 0;
  if (info.start_time > 0 || info.end_time > 0) {
    *first = (int)(info.start_time * frame_rate);
    *last = (int)(info.end_time * frame_rate);
  }
}

void announce(const RecipeInfo &info, int info_level, int index, int total) {
  if (info_level <= 0) return;
  fprintf(stderr, "Processing file: %s", info.audio_path.c_str());
  if (index >= 0) fprintf(stderr, " (%d/%d)", index + 1, total);
  if (info.start_time || info.end_time) fprintf(stderr, " (%.2f-%.2f)", info.start_time, info.end_time);
  fprintf(stderr, "\n");
}

TopoTables::TopoTables(const aasr_topo *topo) {
  const int H = aasr_topo_num_hmms(topo), S = aasr_topo_num_states(topo);
  hmm_states.resize((size_t)std::max(0, H));
  for (int h = 0; h < H; h++) {
    hmm_states[(size_t)h].resize((size_t)std::max(0, aasr_topo_hmm_num_states(topo, h)));
    if (aasr_topo_hmm_states(topo, h, hmm_states[(size_t)h].data()) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  }
  offsets.resize((size_t)std::max(0, S));
  probs.resize((size_t)std::max(0, S));
  for (int s = 0; s < S; s++) {
    const int n = aasr_topo_state_num_transitions(topo, s);
    offsets[(size_t)s].resize((size_t)n);
    probs[(size_t)s].resize((size_t)n);
    if (aasr_topo_state_transitions(topo, s, offsets[(size_t)s].data(), probs[(size_t)s].data()) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    tr_base.push_back(n_transitions);
    n_transitions += n;
  }
}

Segmentation read_segmentation(const aasr_topo *topo, const TopoTables &tt, const char *path, float frame_rate,
                               int first_frame, int last_frame, int eof_frame, bool want_transitions, int phn_flags) {
  const bool snl = (phn_flags & PHN_STATE_NUM_LABELS) != 0;
  if (snl && want_transitions)
    raise(AASR_ERR_UNSUPPORTED, "PhnReader: transitions are not collected from phn files with state number labels");
  FILE *f = fopen(path, "r");
  if (!f) raise(AASR_ERR_IO, "PhnReader::open(): could not open %s", path);
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
  const float spf = 16000 / frame_rate;
  int line_no = 0;
  if (first_frame > 0 || last_frame > 0) phn_skip_to_first_frame(f, spf, first_frame, last_frame, &line_no, phn_flags);
  Segmentation seg;
  PhnLine cur;
  if (!next_phn_line(f, spf, first_frame, last_frame, &line_no, &cur, phn_flags)) return seg;
  seg.initialized = true;
  int frame = -1;
  bool eof_flag = false;
  while (!eof_flag) {
    frame = frame == -1 ? cur.start : frame + 1;
    int state;
    if (snl) {  // PhnReader.cc:164-167: the number is the state's index (the reference does not look whether it exists)
      state = cur.state;
      if (state < 0 || state >= (int)tt.offsets.size())
        raise(AASR_ERR_INVALID, "%s: state %d does not exist", path, state);
    } else {
      if (cur.state < 0) raise(AASR_ERR_INVALID, "PhnReader::next_frame(): A state segmented phn file is required");
      const int h = aasr_topo_hmm_index(topo, cur.label.c_str());
      if (h < 0) raise(AASR_ERR_INVALID, "Unknown HMM in transcription: '%s' in %s", cur.label.c_str(), path);
      const std::vector<int32_t> &states = tt.hmm_states[(size_t)h];
      if (cur.state >= (int)states.size())
        raise(AASR_ERR_INVALID, "%s: state %d of HMM %s does not exist", path, cur.state, cur.label.c_str());
      state = states[(size_t)cur.state];
    }
    bool new_phn_loaded = false;
    const PhnLine prev = cur;
    while (frame + 1 >= cur.end) {
      if (!next_phn_line(f, spf, first_frame, last_frame, &line_no, &cur, phn_flags)) {
        eof_flag = true;
        break;
      }
      new_phn_loaded = true;
    }
    int transition = -1;
    if (want_transitions && !eof_flag) {
      const std::vector<int32_t> &off = tt.offsets[(size_t)state];
      int found = -1;
      if (new_phn_loaded) {
        const int cur_state = prev.state;
        const int n_states = (int)tt.hmm_states[(size_t)aasr_topo_hmm_index(topo, prev.label.c_str())].size();
        for (size_t i = 0; i < off.size(); i++) {
          const int next_state = off[i] + cur_state;
          if ((next_state >= n_states && cur.state == 0) || (off[i] != 0 && next_state == cur.state)) {
            found = (int)i;
            break;
          }
        }
      } else {
        for (size_t i = 0; i < off.size(); i++)
          if (off[i] == 0) {
            found = (int)i;
            break;
          }
      }
      if (found < 0) raise(AASR_ERR_INVALID, "PhnReader::next_frame(): Correct transition was not found");
      transition = tt.tr_base[(size_t)state] + found;
    }
    if (eof_frame >= 0 && frame >= eof_frame) break;  // EOF in FeatureGenerator (stats.cc:105-112)
    if (seg.pdf.empty()) seg.start_frame = frame;
    seg.pdf.push_back(state);  // legacy .ph: a state's emission pdf is the state itself
    if (want_transitions) seg.tr.push_back(transition);
  }
  return seg;
}

Segmentation read_state_sequence(const aasr_topo *topo, const TopoTables &tt, const RecipeInfo &info, bool ophn,
                                 float frame_rate, int eof_frame) {
  int first, last;
  frame_range(info, frame_rate, &first, &last);
  Segmentation seg;
  try {
    seg = read_segmentation(topo, tt, (ophn ? info.alignment_path : info.transcript_path).c_str(), frame_rate, first, last,
                            eof_frame, false);
  } catch (const Error &e) {  // (a file that does not open included: these two tools report every failure as invalid)
    raise(AASR_ERR_INVALID, "%s", e.msg.c_str());
  }
  if (!seg.initialized) {
    fprintf(stderr, "Could not initialize the utterance for PhnReader.");
    fprintf(stderr, "Current file was: %s\n", info.audio_path.c_str());
  }
  return seg;
}

void apply_speaker(aasr_spkc *spk, const RecipeInfo &u, bool utterance) {
  if (!spk) return;
  if (aasr_spkc_set_speaker(spk, u.speaker_id.c_str()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  if (utterance && !u.utterance_id.empty() && aasr_spkc_set_utterance(spk, u.utterance_id.c_str()) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
}

GroupStager::GroupStager(aasr_feat *feat_, aasr_spkc *speakers_, int target_)
    : feat(feat_), speakers(speakers_), target(target_),
      dim(target_ < 0 ? aasr_feat_dim(feat_) : feat_->mods[(size_t)target_].dim), stream_guard(nullptr, [](void *s) {
        if (s) (void)hipStreamDestroy((hipStream_t)s);
      }) {
  AASR_HIP(hipStreamCreate(&stream));
  stream_guard.reset((void *)stream);
  if (speakers) {
    const hipStream_t st = stream;
    spkc_set_before_change(speakers, [st]() { AASR_HIP(hipStreamSynchronize(st)); });
  }
}

GroupStager::~GroupStager() {
  if (speakers) spkc_set_before_change(speakers, nullptr);
}

int64_t GroupStager::stage(const std::vector<std::vector<int16_t>> &audio, const std::vector<int32_t> &start,
                           const std::vector<int32_t> &rows, const std::function<void(size_t)> &before_utterance) {
  int64_t rows_total = 0;
  size_t samples = 1;
  for (size_t i = 0; i < audio.size(); i++) {
    rows_total += rows[i];
    samples += audio[i].size();
  }
  d_x.ensure((size_t)std::max<int64_t>(1, rows_total) * dim);
  if (samples > d_pcm.n) {  // (the buffer may still be read by the previous group's features)
    AASR_HIP(hipStreamSynchronize(stream));
    d_pcm.alloc(samples);
  }
  size_t pcm_at = 0;
  int64_t row = 0;
  for (size_t i = 0; i < audio.size(); i++) {
    before_utterance(i);
    const std::vector<int16_t> &a = audio[i];
    const int32_t n = rows[i];
    if (n <= 0) continue;
    if (!a.empty())
      AASR_HIP(hipMemcpyAsync(d_pcm.p + pcm_at, a.data(), a.size() * sizeof(int16_t), hipMemcpyHostToDevice, stream));
    double *out = d_x.p + (size_t)row * dim;
    if (target < 0) {  // the exported call: the chain's output, its argument checks, every failure as invalid
      if (aasr_feat_run_f64_dev(feat, d_pcm.p + pcm_at, (int64_t)a.size(), start[i], n, out, stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    } else {
      UttBatch b;
      b.n_utts = 1;
      b.frame_off = {0, n};
      b.pcm_off = {0, (int64_t)a.size()};
      b.first = {start[i]};
      feat_run_batch(feat, d_pcm.p + pcm_at, b, target, nullptr, out, stream);
    }
    pcm_at += a.size();
    row += n;
  }
  return rows_total;
}

void write_speaker_file_for_batch(aasr_spkc *speakers, std::set<std::string> seen, int num_batches, int batch_index,
                                  const char *path) {
  std::vector<const char *> sp;
  int32_t n_sp = -1, n_ut = -1;
  if (num_batches > 1) {
    if (batch_index == 1) seen.insert("default");
    for (const std::string &s : seen) sp.push_back(s.c_str());
    n_sp = (int32_t)sp.size();
    n_ut = 0;
  }
  char *text = nullptr;
  int64_t len = 0;
  if (aasr_spkc_write_text(speakers, sp.data(), n_sp, nullptr, n_ut, &text, &len) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  std::unique_ptr<char, void (*)(void *)> tguard(text, free);
  write_text_file(path, text, (size_t)len);
}

void fill_run_stats(aasr_run_stats *stats, int64_t utterances, int64_t frames,
                    std::chrono::steady_clock::time_point t0, double seconds_device) {
  if (!stats) return;
  stats->utterances = utterances;
  stats->frames = frames;
  stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  stats->seconds_device = seconds_device;
  stats->seconds_copy_out = 0;
}

void write_text_file(const char *path, const char *data, size_t len) {
  std::ofstream of(path, std::ios::binary);
  if (!of) raise(AASR_ERR_IO, "could not open %s for writing", path);
  of.write(data, (std::streamsize)len);
  if (!of) raise(AASR_ERR_IO, "write error on %s", path);
}

}  // namespace aasr

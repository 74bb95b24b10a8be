// align.h -- the forced aligner's device-side layout, shared by the Viterbi kernel
// (align_viterbi.hip) and its host driver (align.cc).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

enum { ALIGN_ACTIVE = 0, ALIGN_OK = 1, ALIGN_GAVE_UP = 2, ALIGN_ERROR = 3 };

// What one utterance reads: its transcription (the HMM states in order, and per transcript line
// the number of states it adds -- 0 for lines that add none), its score rows and its frame limits.
struct AlignUttDev {
  int64_t pos_begin;   // first entry in tr_state
  int64_t line_begin;  // first entry in line_states
  int64_t row0;        // score row of feature frame start_frame
  int64_t out_begin;   // first entry in the committed-position output
  int64_t cells_begin; // first cell of this utterance's lattice ring (swins x width)
  int64_t meta_begin;  // first entry of the ring's per-frame ranges (3 x swins) and of the path (swins)
  int32_t n_pos, n_lines;
  int32_t start_frame; // first feature frame (PhnReader::first_frame)
  int32_t end_frame;   // (int)(end_time * frame_rate), 0: to the end of the audio
  int32_t eof_frame;   // first frame the feature reader reports as past the end
  int32_t n_out;       // capacity of the output: frames that can be committed
};

// The search state of one utterance between window steps (aku/Viterbi.hh members and the locals
// of align.cc:viterbi_align), kept in device memory.
struct AlignRun {
  double acc;        // m_accumulated_log_prob
  double fin;        // m_final_log_prob
  double beam;       // curr_beam of align.cc (the search uses it as float)
  float best;        // m_best_log_prob
  int32_t sbeam;     // curr_sbeam
  int32_t bestpos;   // m_best_position, absolute transcription position
  int32_t status;    // ALIGN_*
  int32_t fresh;     // 1: the next step starts the utterance from scratch
  int32_t n_fail;    // how many times the forced end was missed (each one doubled the beams)
  int32_t wstart;    // window_start_frame: absolute frame of lattice frame 0
  int32_t cur;       // m_current_frame, relative to wstart
  int32_t ffr;       // m_feature_frame
  int32_t base;      // absolute transcription position of lattice position 0
  int32_t loaded;    // absolute end of the transcription read so far
  int32_t line;      // next unread transcript line
  int32_t tr_eof;    // the transcript has been read to its end
  int32_t lim;       // m_last_position, relative to base
  int32_t committed; // frames committed to the output
  int32_t error;     // nonzero: why the search stopped (ALIGN_ERROR)
};

struct AlignParams {
  const int32_t *tr_state;     // HMM state of each transcription position
  const int32_t *line_states;  // states added per transcript line
  const int32_t *in_begin;     // per transcription position: its incoming transitions [begin, end)
  const int32_t *in_delta;     // source = target - delta, sources ascending, then transition order
  const float *in_logp;        // (float)safe_log(prob) of each incoming transition
  const void *scores;          // state log-likelihood rows (float, or double when f64)
  int64_t pitch;               // elements between consecutive rows
  int32_t f64;
  int32_t swins, width, max_off;
  int32_t target;              // (int)(swins * (1 - overlap))
  int32_t force_end;
  double maxbeam;
  const AlignUttDev *utt;
  AlignRun *run;
  float *cells;                // lattice ring: log-probabilities
  uint8_t *back;               // lattice ring: source delta per cell
  int32_t *meta;               // lattice ring: (origin, start, end) per frame slot
  int32_t *path;               // traceback scratch, swins per utterance
  int32_t *out;                // committed absolute positions, one per frame
};

void align_launch(const AlignParams &p, int32_t n_utt, int32_t windows, hipStream_t stream);

}  // namespace aasr

// phn_line.h -- .phn lines as aku/PhnReader.cc reads them for align and stats (the rules of
// PhnReader.cc:294-400; state-number labels and relative sample numbers are the two flags below):
//   "label[,more labels] [comment]"                      -- no times
//   "start end label[.state][,more labels] [comment]"    -- sample numbers at 16 kHz, when the line
//                                                           starts with a digit
// Fields end at one blank or tab, the blanks after it are skipped, and the last field allowed takes
// the rest of the line.  Only the first label names the HMM.  The state number is what follows the
// first '.', and the label loses that '.' and the one character after it.  Defined in align.cc.
#pragma once
#include <cstdio>
#include <string>

namespace aasr {

struct PhnLine {
  int start = -1, end = -1, state = -1;
  std::string label, comment;
};

// PhnReader's modes (the values of AASR_PHN_* in aasr.h).  State-number labels: the first field after the times is
// atoi'd into `state` and `label` stays empty.  Relative sample numbers: start and end of a timed line are shifted by
// first_frame before they are clipped, and phn_skip_to_first_frame skips nothing.
constexpr int PHN_STATE_NUM_LABELS = 1, PHN_RELATIVE_SAMPLES = 2;

// One entry; false at the end of the file or at a timed line that starts at or after last_frame
// (> 0).  Times are clipped to [first_frame, last_frame] as PhnReader::set_frame_limits leaves them.
bool next_phn_line(FILE *f, float samples_per_frame, int first_frame, int last_frame, int *line_no, PhnLine *phn,
                   int flags = 0);

// PhnReader::set_frame_limits: skips the lines that end at or before first_frame (the file is left
// at the first line that does not)
void phn_skip_to_first_frame(FILE *f, float samples_per_frame, int first_frame, int last_frame, int *line_no,
                             int flags = 0);

}  // namespace aasr

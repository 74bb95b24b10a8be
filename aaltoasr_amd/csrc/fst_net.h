// fst_net.h -- the search network and the duration tables of the FST decoder, host side (fst_net.cc).
//
// The network is the reference's Fst::read (decoder/src/Fst.cc:10-103) restated: "#FSTBasic MaxPlus" text, `I n`,
// `F n`, `T src tgt [pdf [sym [logprob]]]`.  The pdf index moves from the arc to its TARGET node (a node whose pdf is
// still -1 takes the mention, a different later mention is "Conflicting emission_pdf_indices"), the node count grows to
// the largest index mentioned, arcs keep file order within their node.  Symbols are bytes (the reference works in
// ISO-8859-15; nothing is decoded), `,` is "no symbol".  Kept messages: unknown header, too few fields, too many fields
// for I / F, weird number of fields for T, weird type indicator, conflicting pdf.  Two things the reference leaves
// undefined are defined here: a `T` line of three fields mentions pdf -1 (the reference reads a field that is not
// there), and a network without an `I` line, or with a negative node index, is refused.
//
// Duration tables (FstAcoustics::duration_read, FstAcoustics.cc:60-89): version 4, num_states, `id a b` per state.  The
// reference resize(num_states)s both tables and then push_back()s the values: entries [0, n) are zero, the file's values
// sit at [n, 2n), so with pdf indices below n -- every real model -- duration_logprob returns 0 and the search adds
// duration_scale * 0.0f.  That is the DEFAULT indexing here (parity with the reference is the contract);
// by_state = 1 indexes the tables as was evidently meant ([0, n)).  A pdf index past the tables (where the reference
// reads out of bounds) has no duration model: 0.
//
// For a > 0 the term is (a-1)*logf(d) - d/b + (-a*logf(b) - lgammaf(a)) in float (FstAcoustics.cc:91-101).  The device
// never evaluates logf / lgammaf: fst_dur_table builds, on the host and with exactly that expression, dur_lp[k][d] for
// the pdfs k with a > 0 and d = 0 ... D (D the longest utterance of the batch; d = 0 is a token that leaves the initial
// node's pdf before any self-loop), and the kernel looks the value up -- the device adds the very floats the reference adds.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct aasr_fstnet {
  std::vector<int32_t> arc_begin;  // nodes + 1
  std::vector<int32_t> arc_tgt, arc_word;  // arc_word: symbol id, -1: none
  std::vector<float> arc_lp;
  std::vector<int32_t> node_pdf, node_end;
  int32_t initial = -1;
  int32_t max_pdf = -1, max_degree = 0;
  std::vector<std::string> symbols;
};

struct aasr_fst_durations {
  int32_t n = 0;             // states in the file
  std::vector<float> a, b;   // the file's values, [0, n)
};

namespace aasr {

// throws Error (AASR_ERR_IO: cannot open; AASR_ERR_INVALID: the reference's messages)
void fst_net_read(const char *path, aasr_fstnet &net);
void fst_durations_read(const char *path, aasr_fst_durations &dur);
// duration_logprob under either indexing
float fst_duration_logprob(const aasr_fst_durations *dur, bool by_state, int32_t pdf, int32_t d);
// slot[pdf] (n_pdf entries): the row of the pdf in table, -1: no duration model; table: rows x (D + 1) floats
void fst_dur_table(const aasr_fst_durations *dur, bool by_state, int32_t n_pdf, int32_t D, std::vector<int32_t> &slot,
                   std::vector<float> &table);

}  // namespace aasr

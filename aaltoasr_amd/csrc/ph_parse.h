// ph_parse.h -- the one reader of the legacy PHONE topology files (.ph) with their transitions,
// shared by the aku::HmmSet adapter (csrc/aku/HmmSet.cc) and the aligner's topology handle
// (csrc/align.cc).  Rules of aku/HmmSet.cc:208-329: per phone "index states label", the two
// dummy states' numbers, one pdf index per real state, then per source (dummies included)
// "source n" and n "target prob" pairs.  States are tied by their pdf: the first phone that
// mentions a pdf defines that state's transitions (target 1 = the dummy final state, stored as the
// offset that leaves the HMM, i.e. +1 past its last state into the next HMM), later mentions are
// only checked.
#pragma once
#include <istream>
#include <string>
#include <vector>

#include "aku/str.hh"

namespace aasr {

struct PhTransition {
  int source;         // pdf (= state) index of the source
  int target_offset;  // relative to the source's position in its HMM
  double prob;
};

// Reads the part after the "PHONE" word.  on_hmm(label, states) is called once per phone when its
// header has been read, on_state(s, pdf) for each of its real states as the pdf index is read;
// read_error() throws the caller's read error.  state_info[pdf] receives the transitions of each
// pdf in file order.
template <class OnHmm, class OnState, class ReadErrorFn>
void parse_legacy_ph(std::istream &in, OnHmm on_hmm, OnState on_state, ReadErrorFn read_error,
                     std::vector<std::vector<PhTransition>> &state_info) {
  std::string label;
  int phonemes = 0;
  in >> phonemes;
  for (int h = 0; h < phonemes; h++) {
    int index = 0, states = 0;
    in >> index >> states >> label;
    if (!in) read_error();
    states -= 2;  // the dummy entry / exit states
    on_hmm(label, states);
    std::vector<int> hmm_states(states > 0 ? (size_t)states : 0);
    int dummy, pdf;
    std::vector<bool> load_transitions;
    in >> dummy >> dummy;
    for (int s = 0; s < states; s++) {
      in >> pdf;
      // (the reference indexes with whatever it read: a negative or garbage index is a read error here)
      if (!in || pdf < 0 || pdf > (1 << 24)) read_error();
      if (pdf >= (int)state_info.size()) state_info.resize((size_t)pdf + 1);
      hmm_states[(size_t)s] = pdf;
      on_state(s, pdf);
      load_transitions.push_back(state_info[(size_t)pdf].empty());
    }
    for (int s = -2; s < states; s++) {
      int transitions = 0, source = 0;
      in >> source >> transitions;
      source -= 2;
      if (source >= states)
        throw str::fmt(128, "HmmSet::read_legacy_ph: Invalid source state number %i (only %i states)", source,
                       states);
      for (int t = 0; t < transitions; t++) {
        int target;
        double prob;
        in >> target >> prob;
        if (prob <= 0)
          throw str::fmt(128,
                         "HmmSet::read_legacy_ph: Phone %i (%s) transition from %i to %i has nonpositive "
                         "probability %f.",
                         index, label.c_str(), source, target, prob);
        if (source >= 0 && load_transitions[(size_t)source]) {
          if (target == 1) {
            target = states - source;  // the sink
          } else {
            target -= 2;
            if (target > states)
              throw str::fmt(128, "HmmSet::read_legacy_ph: Invalid target state number %i (only %i states)",
                             source, states);
            target -= source;  // relative
          }
          state_info[(size_t)hmm_states[(size_t)source]].push_back(PhTransition{hmm_states[(size_t)source], target, prob});
        }
      }
      if (source >= 0 && !load_transitions[(size_t)source])
        for (const PhTransition &tr : state_info[(size_t)hmm_states[(size_t)source]])
          if (source + tr.target_offset > states)
            throw str::fmt(128,
                           "HmmSet::read_legacy_ph: Invalid target state number %i on existing state %i (only "
                           "%i states)",
                           source, hmm_states[(size_t)source], states);
    }
  }
}

}  // namespace aasr

// hmmnet.h -- an HMM network (the text FST of aku/HmmNetBaumWelch.cc:65-163) as flat arrays for the
// forward-backward kernel (hmmnet_fb.hip).  The reader is host only; hmmnet_fb.cc packs these arrays
// into the device blobs that hmmnet_fb.h describes.
//
// Emitting arcs are numbered in source-node order (CSR em_begin), each source's arcs in file order.
// Epsilon arcs are numbered the same way (eo_begin).  The other groupings are index lists into those
// numberings, ascending within a group, so every segmented sum of the kernel has one fixed order.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/aasr.h"

struct aasr_hmmnet {
  int32_t n_nodes = 0, initial = -1, final_node = -1;
  // emitting arcs, by source
  std::vector<int32_t> em_begin;   // [n_nodes + 1]
  std::vector<int32_t> em_src, em_tgt, em_pdf, em_tr, em_slot, em_trslot, em_self;
  std::vector<double> em_logp, em_static;
  std::vector<std::string> em_label;  // the ";..." higher-level labels, text only
  std::vector<int32_t> in_begin, in_arcs;    // emitting arcs by target node
  std::vector<int32_t> pdfs, pdf_begin, pdf_arcs;   // distinct pdfs ascending, their arcs
  std::vector<int32_t> trs, tr_begin, tr_arcs;      // distinct transition indices ascending, their arcs
  // epsilon arcs, by source
  std::vector<int32_t> eo_begin;   // [n_nodes + 1]
  std::vector<int32_t> ep_src, ep_tgt;
  std::vector<double> ep_score;
  std::vector<int32_t> ei_begin, ei_arcs;    // epsilon arcs by target node
  // nodes with epsilon out-arcs grouped by height (longest epsilon path leaving the node), and nodes with
  // epsilon in-arcs grouped by depth (longest epsilon path entering it): a level reads only finished levels
  std::vector<int32_t> bl_begin, bl_nodes;
  std::vector<int32_t> fl_begin, fl_nodes;
};

namespace aasr {
// HmmNetBaumWelch::read_fst + check_network_structure + the topological-order check, raising the
// reference's messages.  tr_source / tr_prob: per global transition index (HmmSet::read_ph order).
void hmmnet_parse(FILE *file, const std::vector<int32_t> &tr_source, const std::vector<double> &tr_prob,
                  aasr_hmmnet *net);
}  // namespace aasr

// hmmnet.cc -- the HMM network reader (hmmnet.h): HmmNetBaumWelch::read_fst (aku/HmmNetBaumWelch.cc:65-163),
// check_network_structure (:536-617) and the topological-order check of :165-289, with the reference's
// messages, and the flat arrays the forward-backward kernel reads.  The logical-arc hierarchy (parent_arc,
// fix_parent_arcs) is not built: only --mpv reads it.  Host only.
#include "hmmnet.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stack>

#include "aku/str.hh"
#include "common.h"
#include "recipe_pass.h"

using namespace aasr;
using aku::str::read_line;
using aku::str::split;
using aku::str::str2float;
using aku::str::str2long;

namespace {

struct RawArc {
  int source, target, tr_index;  // tr_index < 0: epsilon
  std::string label;
  double score;
};

// groups 0 .. n-1 of the items by key[item]: begin[n + 1] and the items of each group ascending
void group_by(const std::vector<int32_t> &key, int32_t n, std::vector<int32_t> *begin, std::vector<int32_t> *items) {
  begin->assign((size_t)n + 1, 0);
  for (int32_t k : key) (*begin)[(size_t)k + 1]++;
  for (int32_t i = 0; i < n; i++) (*begin)[(size_t)i + 1] += (*begin)[(size_t)i];
  items->assign(key.size(), 0);
  std::vector<int32_t> fill(begin->begin(), begin->end() - 1);
  for (size_t a = 0; a < key.size(); a++) (*items)[(size_t)fill[(size_t)key[a]]++] = (int32_t)a;
}

// nodes with rank > 0 grouped by rank, ascending node numbers within a level
void levels(const std::vector<int32_t> &rank, std::vector<int32_t> *begin, std::vector<int32_t> *nodes) {
  const int32_t top = rank.empty() ? 0 : *std::max_element(rank.begin(), rank.end());
  begin->assign(1, 0);
  nodes->clear();
  for (int32_t l = 1; l <= top; l++) {
    for (size_t n = 0; n < rank.size(); n++)
      if (rank[n] == l) nodes->push_back((int32_t)n);
    begin->push_back((int32_t)nodes->size());
  }
}

}  // namespace

namespace aasr {

void hmmnet_parse(FILE *file, const std::vector<int32_t> &tr_source, const std::vector<double> &tr_prob,
                  aasr_hmmnet *net) {
  long initial = -1, final_node = -1;
  std::string line;
  std::vector<std::string> fields;
  bool ok = true;
  std::vector<RawArc> arcs;
  int n_nodes = 0;
  while (read_line(&line, file, true)) {
    split(&line, " \t", true, &fields);
    if (fields.empty()) continue;
    if (fields[0] == "#FSTBinary") throw std::string("FSTBinary format not supported");
    if (fields[0] == "I") {
      if (initial != -1) throw std::string("Initial node redefined: ") + line;
      if (fields.size() != 2)
        ok = false;
      else
        initial = str2long(&fields[1], &ok);
      if (!ok || initial < 0) throw std::string("Invalid initial node specification: ") + line;
    } else if (fields[0] == "F") {
      if (final_node != -1) throw std::string("Final node redefined: ") + line;
      if (fields.size() != 2)
        ok = false;
      else
        final_node = str2long(&fields[1], &ok);
      if (!ok || final_node < 0) throw std::string("Invalid final node specification: ") + line;
    } else if (fields[0] == "T") {
      long source = -1, target = -1;
      std::string in_label, out_label;
      double score = 0;  // loglikelihoods.one()
      if (fields.size() < 3 || fields.size() > 6) {
        ok = false;
      } else {
        source = str2long(&fields[1], &ok);
        target = str2long(&fields[2], &ok);
        if (fields.size() > 3) {
          if (fields[3] != ",") in_label = fields[3];
          if (fields[3].size() > 0 && fields[3][0] != '#' && fields.size() > 4)
            if (fields[4] != ",") out_label = fields[4];
          if (fields.size() > 5) score = str2float(&fields[5], &ok);
        }
      }
      if (!ok || source < 0 || target < 0 || source > (1 << 28) || target > (1 << 28))
        throw std::string("HmmNetBaumWelch: Invalid transition specification: ") + line;
      n_nodes = std::max<long>(n_nodes, std::max(source, target) + 1);
      // LatticeLabel(in, out): "" or "#..." is an epsilon, otherwise the transition index up to the first ';'
      std::string label = in_label;
      if (!out_label.empty()) label += ';' + out_label;
      RawArc a{(int)source, (int)target, -1, "", score};
      if (!label.empty() && label[0] != '#') {
        bool lok = true;
        const size_t n = label.find_first_of(';');
        const std::string head = n == std::string::npos ? label : label.substr(0, n);
        const long idx = str2long(&head, &lok);
        if (!lok) throw std::string("Invalid arc label ") + (n == std::string::npos ? in_label : label);
        if (idx < 0 || idx >= (long)tr_source.size())
          throw aku::str::fmt(256, "HmmNetBaumWelch: transition index %ld of arc label %s is outside the model's %d transitions",
                              idx, label.c_str(), (int)tr_source.size());
        a.tr_index = (int)idx;
        a.label = n == std::string::npos ? "" : label.substr(n);
      }
      arcs.push_back(a);
    }
  }
  if (initial < 0) throw std::string("initial node not specified");
  if (final_node < 0) throw std::string("final node not specified");
  n_nodes = (int)std::max<long>(n_nodes, std::max(initial, final_node) + 1);
  const size_t N = (size_t)n_nodes;

  // check_network_structure
  std::vector<int> n_in(N, 0), n_out(N, 0), self(N, 0);
  for (const RawArc &a : arcs) {
    if (a.tr_index < 0 && a.source == a.target) throw std::string("HmmNetBaumWelch: Epsilon self loops are not allowed");
    n_in[(size_t)a.target]++;
    if (a.source == a.target)
      self[(size_t)a.source] = 1;
    else
      n_out[(size_t)a.source]++;
  }
  for (size_t i = 0; i < N; i++)
    if (n_out[i] > 1 && self[i]) {
      fprintf(stderr, "At node %i:\n", (int)i);
      throw std::string("HmmNetBaumWelch: Self transitions and multiple out transitions can not be combined");
    }
  if (n_in[(size_t)initial] > 0) throw std::string("HmmNetBaumWelch: Initial node may not have in arcs!");
  if (n_out[(size_t)final_node] + self[(size_t)final_node] > 0)
    throw std::string("HmmNetBaumWelch: Final node may not have out arcs!");

  // the topological order of :165-289: a node is activated when all its in-arcs but the self loop are done
  std::vector<std::vector<int>> out_arcs(N);
  for (size_t a = 0; a < arcs.size(); a++) out_arcs[(size_t)arcs[a].source].push_back((int)a);
  {
    std::stack<int> active;
    std::vector<int> visits(N, 0);
    long processed = 0;
    active.push((int)initial);
    while (!active.empty()) {
      const int cur = active.top();
      active.pop();
      if (++processed > (long)N) throw std::string("Error in creating logical arcs for the search network");
      for (int a : out_arcs[(size_t)cur]) {
        const int t = arcs[(size_t)a].target;
        if (t == cur) continue;
        if (++visits[(size_t)t] + self[(size_t)t] >= n_in[(size_t)t]) active.push(t);
      }
    }
    if (processed < (long)N) {
      fprintf(stderr, "Creating topological ordering: %i nodes processed, out of %i\n", (int)processed, (int)N);
      throw std::string("Failed to create a topological order of the nodes");
    }
  }

  // flat arrays
  aasr_hmmnet &h = *net;
  h = aasr_hmmnet();
  h.n_nodes = n_nodes;
  h.initial = (int32_t)initial;
  h.final_node = (int32_t)final_node;
  h.em_begin.assign(N + 1, 0);
  h.eo_begin.assign(N + 1, 0);
  for (size_t n = 0; n < N; n++) {
    for (int ai : out_arcs[n]) {
      const RawArc &a = arcs[(size_t)ai];
      if (a.tr_index < 0) {
        h.ep_src.push_back(a.source);
        h.ep_tgt.push_back(a.target);
        h.ep_score.push_back(a.score);
      } else {
        h.em_src.push_back(a.source);
        h.em_tgt.push_back(a.target);
        h.em_tr.push_back(a.tr_index);
        h.em_pdf.push_back(tr_source[(size_t)a.tr_index]);
        const double p = tr_prob[(size_t)a.tr_index];
        h.em_logp.push_back(std::log(p));
        h.em_static.push_back(a.score);
        h.em_self.push_back(a.source == a.target);
        h.em_label.push_back(a.label);
      }
    }
    h.em_begin[n + 1] = (int32_t)h.em_src.size();
    h.eo_begin[n + 1] = (int32_t)h.ep_src.size();
  }
  group_by(h.em_tgt, n_nodes, &h.in_begin, &h.in_arcs);
  group_by(h.ep_tgt, n_nodes, &h.ei_begin, &h.ei_arcs);
  auto distinct = [](const std::vector<int32_t> &v, std::vector<int32_t> *values, std::vector<int32_t> *slot) {
    *values = v;
    std::sort(values->begin(), values->end());
    values->erase(std::unique(values->begin(), values->end()), values->end());
    slot->resize(v.size());
    for (size_t a = 0; a < v.size(); a++)
      (*slot)[a] = (int32_t)(std::lower_bound(values->begin(), values->end(), v[a]) - values->begin());
  };
  distinct(h.em_pdf, &h.pdfs, &h.em_slot);
  distinct(h.em_tr, &h.trs, &h.em_trslot);
  group_by(h.em_slot, (int32_t)h.pdfs.size(), &h.pdf_begin, &h.pdf_arcs);
  group_by(h.em_trslot, (int32_t)h.trs.size(), &h.tr_begin, &h.tr_arcs);
  // epsilon levels: the subgraph is acyclic (the order above exists), so a fixed point is reached in at most N sweeps
  std::vector<int32_t> height(N, 0), depth(N, 0);
  for (bool changed = true; changed;) {
    changed = false;
    for (size_t e = 0; e < h.ep_src.size(); e++) {
      const size_t s = (size_t)h.ep_src[e], t = (size_t)h.ep_tgt[e];
      if (height[s] < height[t] + 1) height[s] = height[t] + 1, changed = true;
      if (depth[t] < depth[s] + 1) depth[t] = depth[s] + 1, changed = true;
    }
  }
  levels(height, &h.bl_begin, &h.bl_nodes);
  levels(depth, &h.fl_begin, &h.fl_nodes);
}

}  // namespace aasr

extern "C" {

aasr_status aasr_hmmnet_read(const aasr_topo *topo, const char *path, aasr_hmmnet **out) {
  return guarded([&] {
    if (!topo || !path || !out) raise(AASR_ERR_INVALID, "aasr_hmmnet_read: null argument");
    *out = nullptr;
    const TopoTables tt(topo);
    std::vector<int32_t> tr_source;
    std::vector<double> tr_prob;
    for (size_t s = 0; s < tt.probs.size(); s++)
      for (double p : tt.probs[s]) {
        tr_source.push_back((int32_t)s);
        tr_prob.push_back(p);
      }
    FILE *fp = fopen(path, "r");
    if (!fp) raise(AASR_ERR_IO, "HmmNetBaumWelch::open: Could not open file `%s'.", path);
    std::unique_ptr<FILE, int (*)(FILE *)> guard(fp, fclose);
    std::unique_ptr<aasr_hmmnet> net(new aasr_hmmnet());
    hmmnet_parse(fp, tr_source, tr_prob, net.get());
    *out = net.release();
  });
}

void aasr_hmmnet_destroy(aasr_hmmnet *net) { delete net; }

aasr_status aasr_hmmnet_counts(const aasr_hmmnet *h, int32_t *counts) {
  return guarded([&] {
    if (!h || !counts) raise(AASR_ERR_INVALID, "aasr_hmmnet_counts: null argument");
    const int32_t c[AASR_HMMNET_NUM_COUNTS] = {h->n_nodes, (int32_t)h->em_src.size(), (int32_t)h->ep_src.size(),
                                               (int32_t)h->bl_begin.size() - 1, (int32_t)h->fl_begin.size() - 1,
                                               (int32_t)h->pdfs.size(), (int32_t)h->trs.size(), h->initial, h->final_node};
    std::copy(c, c + AASR_HMMNET_NUM_COUNTS, counts);
  });
}

aasr_status aasr_hmmnet_array(const aasr_hmmnet *h, int32_t which, void *out, int64_t capacity, int64_t *count) {
  return guarded([&] {
    if (!h || !count) raise(AASR_ERR_INVALID, "aasr_hmmnet_array: null argument");
    const std::vector<int32_t> *iv[] = {&h->em_begin, &h->em_src,   &h->em_tgt,   &h->em_pdf,  &h->em_tr,    &h->em_self,
                                        &h->in_begin, &h->in_arcs,  &h->pdfs,     &h->pdf_begin, &h->pdf_arcs, &h->trs,
                                        &h->tr_begin, &h->tr_arcs,  &h->eo_begin, &h->ep_src,  &h->ep_tgt,   &h->ei_begin,
                                        &h->ei_arcs,  &h->bl_begin, &h->bl_nodes, &h->fl_begin, &h->fl_nodes};
    const std::vector<double> *dv[] = {&h->em_logp, &h->em_static, &h->ep_score};
    const int n_i = (int)(sizeof iv / sizeof iv[0]), n_d = (int)(sizeof dv / sizeof dv[0]);
    if (which >= 0 && which < n_i) {
      *count = (int64_t)iv[which]->size();
      if (out && capacity >= *count) std::copy(iv[which]->begin(), iv[which]->end(), (int32_t *)out);
    } else if (which >= 100 && which < 100 + n_d) {
      *count = (int64_t)dv[which - 100]->size();
      if (out && capacity >= *count) std::copy(dv[which - 100]->begin(), dv[which - 100]->end(), (double *)out);
    } else {
      raise(AASR_ERR_INVALID, "aasr_hmmnet_array: no array %d", which);
    }
  });
}

const char *aasr_hmmnet_arc_label(const aasr_hmmnet *h, int32_t arc) {
  if (!h || arc < 0 || arc >= (int32_t)h->em_label.size()) return nullptr;
  return h->em_label[(size_t)arc].c_str();
}

}  // extern "C"

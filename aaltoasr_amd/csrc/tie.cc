// tie.cc -- decision-tree state tying (aku/tie.cc over aku/PhonePool.cc): the labels, the rule file, the context
// phones and their trees on the host; the candidates' sums and likelihood gains on the device (tie_split.hip, layout:
// tie.h); the basebind and model writers; and the tie main loop over a recipe (aasr_run_tie_recipe).
//
// The host decides which candidates exist (occupancies are integer frame counts, so the --count test, the "smaller
// side" rule and the skip of a member set already tried are exact), the device returns a gain per candidate, and the
// host picks the winner with the reference's comparisons in the reference's order.  Trees are independent: every
// round evaluates the open cluster of every tree in one launch sequence.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "aku/str.hh"
#include "common.h"
#include "feat.h"
#include "phn_line.h"
#include "recipe_pass.h"
#include "scatter.h"
#include "tie.h"

using namespace aasr;

namespace {

// ---- labels (PhonePool::center_phone, fill_left_contexts, fill_right_contexts) ---------------------------------

std::string center_phone(const std::string &label) {
  const int pos1 = (int)label.find_last_of('-');
  const int pos2 = (int)label.find_first_of('+');
  std::string temp;
  if (pos1 >= 0 && pos2 >= 0) {
    if (pos2 > pos1 + 1) temp = label.substr((size_t)pos1 + 1, (size_t)(pos2 - pos1 - 1));
  } else if (pos1 >= 0) {
    temp = label.substr((size_t)pos1 + 1);
  } else if (pos2 >= 0) {
    temp = label.substr(0, (size_t)pos2);
  } else {
    temp = label;
  }
  if (temp.empty()) throw std::string("PhonePool: Invalid phone label") + label;
  return temp;
}

// nearest context first: "x-a-b+c" gives a, x
std::vector<std::string> left_contexts(const std::string &label) {
  std::vector<std::string> far_first;
  int cur = 0, next;
  while ((next = (int)label.find('-', (size_t)cur + 1)) >= cur) {
    far_first.push_back(label.substr((size_t)cur, (size_t)(next - cur)));
    cur = next + 1;
  }
  return std::vector<std::string>(far_first.rbegin(), far_first.rend());
}

std::vector<std::string> right_contexts(const std::string &label) {
  std::vector<std::string> out;
  int cur = (int)label.find('+'), next;
  if (cur > 0) {
    cur++;
    while ((next = (int)label.find('+', (size_t)cur + 1)) >= cur) {
      out.push_back(label.substr((size_t)cur, (size_t)(next - cur)));
      cur = next + 1;
    }
    out.push_back(label.substr((size_t)cur));
  }
  return out;
}

struct Rule {
  std::string name;
  std::set<std::string> phones;
};

struct Applied {
  int rule, context;
  bool answer;
};

struct ContextPhone {
  std::string label, center;
  int state = 0;
  std::vector<std::string> left, right;
};

struct Cluster {
  std::vector<int> members;                 // classes, ascending
  std::vector<std::vector<Applied>> rules;  // one ordered set while splitting; merging appends the other cluster's
  double occ = 0;
  int state_index = -1;
};

struct Phone {
  std::string label;
  std::vector<std::map<std::string, int>> cp;  // per state: label -> class
  int max_left = 0, max_right = 0;
  std::vector<std::vector<Cluster>> clusters;  // per state, in the reference's vector order
};

bool rule_answer(const ContextPhone &p, const Rule &rule, int context) {
  if (context < 0) {
    if (context < -(int)p.left.size()) return false;
    return rule.phones.count(p.left[(size_t)(-context - 1)]) > 0;
  }
  if (context > 0) {
    if (context > (int)p.right.size()) return false;
    return rule.phones.count(p.right[(size_t)(context - 1)]) > 0;
  }
  throw std::string("PhonePool::ContextPhone::rule_answer: Invalid context index 0");
}

int safe_tolower(int c) { return tolower(c); }

// PhonePool::load_decision_tree_rules
std::vector<Rule> read_rules(const char *path) {
  FILE *fp = fopen(path, "r");
  if (!fp) raise(AASR_ERR_IO, "could not open %s", path);
  std::unique_ptr<FILE, int (*)(FILE *)> guard(fp, fclose);
  std::vector<Rule> rules;
  std::string line;
  std::vector<std::string> fields;
  while (aku::str::read_line(&line, fp, true)) {
    fields.clear();
    aku::str::split(&line, " \t", true, &fields, 3);
    if (fields.empty()) continue;
    if (fields.size() < 2) throw std::string("PhonePool::load_decision_tree_rules: Invalid rule line:\n") + line;
    std::transform(fields[1].begin(), fields[1].end(), fields[1].begin(), safe_tolower);
    if (fields[1] != "context") throw std::string("PhonePool::load_decision_tree_rules: Invalid rule type ") + fields[1];
    Rule r;
    r.name = fields[0];
    std::vector<std::string> phones;
    if (fields.size() > 2) aku::str::split(&fields[2], ", ", true, &phones);
    if (phones.empty()) throw std::string("PhonePool::load_decision_tree_rules: No phones in the context rule:\n") + line;
    r.phones.insert(phones.begin(), phones.end());
    rules.push_back(r);
  }
  return rules;
}

// a candidate of a split: the rule, the context index, which answer's members form the new set (the smaller side)
struct SplitCand {
  int rule, context;
  bool first_answer;
  std::vector<int> set;  // ascending
  double gain = 0;
};
struct SplitQuery {
  int tree;
  const Cluster *cl;
  std::vector<SplitCand> cands;
};
struct Tree {
  Phone *phone;
  int state;
  int cursor = 0;
  int ctx_start = 0, ctx_end = 0;
};

}  // namespace

struct aasr_tie {
  int D = 0;
  int64_t E = 0, EP = 0;
  std::vector<Rule> rules;
  std::map<std::string, Phone> phones;
  std::set<std::string> contexts;
  std::vector<ContextPhone> classes;
  std::map<std::pair<std::string, int>, int> class_index;
  std::vector<double> occ;  // per class, once statistics are set
  bool have_occ = false, have_stats = false, split_done = false;
  DevBuf<double> rows;  // [classes x EP]
  // scratch of a batch
  DevBuf<double> sums, ld_gamma, gain;
  DevBuf<int32_t> d_idx;
  DevBuf<uint32_t> d_mask;
  DevBuf<TieJob> d_jobs;
  DevBuf<TieItem> d_items;
  DevBuf<TieSide> d_sides;
  DevBuf<TieCand> d_cands;
  int32_t last_shape[4] = {0, 0, 0, 0};  // work items of hop 1 and hop 2, sides, candidates of the last batch
  int rounds_split = 0, rounds_merge = 0;
};

namespace {

// ---- a batch on the device ---------------------------------------------------------------------------------

struct Batch {
  std::vector<TieJob> jobs[2];  // hop 1 reads the context phones' rows, hop 2 the sums of hop 1
  std::vector<int32_t> idx;
  std::vector<uint32_t> mask;
  std::vector<TieSide> sides;
  std::vector<TieCand> cands;
  int32_t n_out = 0;  // rows of the sums

  // -> the job's first output row; its masks are zero
  int add_job(int hop, const int32_t *list, int n_k, int n_rows) {
    TieJob j;
    j.idx0 = (int32_t)idx.size();
    j.n_k = n_k;
    j.mask0 = (int32_t)mask.size();
    j.wpr = (n_k + 31) / 32;
    j.n_rows = n_rows;
    j.out0 = n_out;
    idx.insert(idx.end(), list, list + n_k);
    mask.resize(mask.size() + (size_t)j.wpr * n_rows, 0u);
    n_out += n_rows;
    jobs[hop].push_back(j);
    return j.out0;
  }
  void set_bit(int hop, int row, int k) {  // of the last job of the hop
    const TieJob &j = jobs[hop].back();
    mask[(size_t)j.mask0 + (size_t)row * j.wpr + (size_t)(k >> 5)] |= 1u << (k & 31);
  }
  int add_side(int op, int a, int b) {
    sides.push_back(TieSide{a, b, op, 0});
    return (int)sides.size() - 1;
  }
};

void run_batch(aasr_tie *h, const Batch &b, std::vector<double> *gains, std::vector<double> *sums_out) {
  require_device();
  if (!h->have_stats) raise(AASR_ERR_INVALID, "tie: no statistics set");
  const int ET = (int)(h->EP / 16);
  if ((int64_t)b.idx.size() > INT32_MAX || (int64_t)b.mask.size() > INT32_MAX)
    raise(AASR_ERR_UNSUPPORTED, "tie: a batch of more than 2^31 list entries");
  h->sums.ensure((size_t)std::max(1, b.n_out) * h->EP);
  h->d_idx.ensure(std::max<size_t>(1, b.idx.size()));
  h->d_mask.ensure(std::max<size_t>(1, b.mask.size()));
  if (!b.idx.empty()) AASR_HIP(hipMemcpy(h->d_idx.p, b.idx.data(), b.idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!b.mask.empty()) AASR_HIP(hipMemcpy(h->d_mask.p, b.mask.data(), b.mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  for (int hop = 0; hop < 2; hop++) {
    const std::vector<TieJob> &jobs = b.jobs[hop];
    std::vector<TieItem> items;
    for (size_t j = 0; j < jobs.size(); j++)
      for (int rt = 0; rt < (jobs[j].n_rows + 15) / 16; rt++)
        for (int ct = 0; ct < ET; ct += TIE_NE) items.push_back(TieItem{(int32_t)j, rt, ct, 0});
    h->last_shape[hop] = (int32_t)items.size();
    if (items.empty()) continue;
    h->d_jobs.ensure(jobs.size());
    h->d_items.ensure(items.size());
    AASR_HIP(hipMemcpy(h->d_jobs.p, jobs.data(), jobs.size() * sizeof(TieJob), hipMemcpyHostToDevice));
    AASR_HIP(hipMemcpy(h->d_items.p, items.data(), items.size() * sizeof(TieItem), hipMemcpyHostToDevice));
    tie_masked_sum_launch(h->D, hop == 0 ? h->rows.p : h->sums.p, h->d_idx.p, h->d_mask.p, h->d_jobs.p, h->d_items.p,
                          (int)items.size(), h->sums.p, nullptr);
    AASR_HIP(hipStreamSynchronize(nullptr));  // the next hop reuses the job and item buffers
  }
  h->last_shape[2] = (int32_t)b.sides.size();
  h->last_shape[3] = (int32_t)b.cands.size();
  if (!b.cands.empty()) {
    h->d_sides.ensure(b.sides.size());
    h->d_cands.ensure(b.cands.size());
    h->ld_gamma.ensure(2 * b.sides.size());
    h->gain.ensure(b.cands.size());
    AASR_HIP(hipMemcpy(h->d_sides.p, b.sides.data(), b.sides.size() * sizeof(TieSide), hipMemcpyHostToDevice));
    AASR_HIP(hipMemcpy(h->d_cands.p, b.cands.data(), b.cands.size() * sizeof(TieCand), hipMemcpyHostToDevice));
    tie_logdet_launch(h->D, h->sums.p, h->d_sides.p, (int)b.sides.size(), h->ld_gamma.p, nullptr);
    tie_gain_launch(h->ld_gamma.p, h->d_cands.p, (int)b.cands.size(), h->gain.p, nullptr);
  }
  if (gains) {
    gains->resize(b.cands.size());
    if (!b.cands.empty()) AASR_HIP(hipMemcpy(gains->data(), h->gain.p, b.cands.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (sums_out) {
    sums_out->resize((size_t)b.n_out * h->EP);
    if (b.n_out > 0) AASR_HIP(hipMemcpy(sums_out->data(), h->sums.p, sums_out->size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  AASR_HIP(hipDeviceSynchronize());
}

// the label of class c at context index i, or nullptr
const std::string *context_at(const ContextPhone &p, int i) {
  if (i < 0) return -i <= (int)p.left.size() ? &p.left[(size_t)(-i - 1)] : nullptr;
  return i <= (int)p.right.size() ? &p.right[(size_t)(i - 1)] : nullptr;
}

// The split candidates' gains.  hops 1: members -> parent and candidates.  hops 2: members -> parent and the sums
// per (context index, label), then label sums -> the rules' yes sets; the other half is parent - yes.
void device_split_gains(aasr_tie *h, std::vector<SplitQuery> &queries, int hops) {
  Batch b;
  std::vector<std::vector<int>> yes_row(queries.size());
  std::vector<int> parent_row(queries.size());
  if (hops == 1) {
    for (size_t q = 0; q < queries.size(); q++) {
      const std::vector<int> &mem = queries[q].cl->members;
      const std::vector<SplitCand> &cs = queries[q].cands;
      parent_row[q] = b.add_job(0, mem.data(), (int)mem.size(), 1 + (int)cs.size());
      for (int k = 0; k < (int)mem.size(); k++) b.set_bit(0, 0, k);
      for (size_t c = 0; c < cs.size(); c++) {
        size_t at = 0;  // both ascending
        for (int k = 0; k < (int)mem.size() && at < cs[c].set.size(); k++)
          if (mem[(size_t)k] == cs[c].set[at]) {
            b.set_bit(0, 1 + (int)c, k);
            at++;
          }
        yes_row[q].push_back(parent_row[q] + 1 + (int)c);
      }
    }
  } else {
    // hop 1: per query the parent and a one-hot row per (context index, label)
    struct Pos {
      int context;
      std::vector<std::string> labels;  // ascending
      std::vector<int32_t> rows;        // their sums
      std::vector<size_t> cands;
    };
    std::vector<std::vector<Pos>> pos(queries.size());
    for (size_t q = 0; q < queries.size(); q++) {
      const std::vector<int> &mem = queries[q].cl->members;
      const std::vector<SplitCand> &cs = queries[q].cands;
      std::map<int, Pos> by_ctx;
      for (size_t c = 0; c < cs.size(); c++) {
        Pos &p = by_ctx[cs[c].context];
        p.context = cs[c].context;
        p.cands.push_back(c);
      }
      int n_rows = 1;
      for (auto &kv : by_ctx) {
        std::set<std::string> ls;
        for (int m : mem)
          if (const std::string *l = context_at(h->classes[(size_t)m], kv.first)) ls.insert(*l);
        kv.second.labels.assign(ls.begin(), ls.end());
        n_rows += (int)ls.size();
      }
      parent_row[q] = b.add_job(0, mem.data(), (int)mem.size(), n_rows);
      for (int k = 0; k < (int)mem.size(); k++) b.set_bit(0, 0, k);
      int row = 1;
      for (auto &kv : by_ctx) {
        Pos &p = kv.second;
        for (int k = 0; k < (int)mem.size(); k++)
          if (const std::string *l = context_at(h->classes[(size_t)mem[(size_t)k]], p.context))
            b.set_bit(0, row + (int)(std::lower_bound(p.labels.begin(), p.labels.end(), *l) - p.labels.begin()), k);
        for (size_t l = 0; l < p.labels.size(); l++) p.rows.push_back(parent_row[q] + row + (int)l);
        row += (int)p.labels.size();
        pos[q].push_back(p);
      }
    }
    // hop 2: per (query, context index) the rules' phone sets as masks over the label sums
    for (size_t q = 0; q < queries.size(); q++) {
      const std::vector<SplitCand> &cs = queries[q].cands;
      yes_row[q].assign(cs.size(), -1);
      for (const Pos &p : pos[q]) {
        const int out0 = b.add_job(1, p.rows.data(), (int)p.rows.size(), (int)p.cands.size());
        for (size_t r = 0; r < p.cands.size(); r++) {
          const Rule &rule = h->rules[(size_t)cs[p.cands[r]].rule];
          for (size_t l = 0; l < p.labels.size(); l++)
            if (rule.phones.count(p.labels[l])) b.set_bit(1, (int)r, (int)l);
          yes_row[q][p.cands[r]] = out0 + (int)r;
        }
      }
    }
  }
  for (size_t q = 0; q < queries.size(); q++) {
    const int ps = b.add_side(TIE_SIDE_ROW, parent_row[q], 0);
    const std::vector<int> &mem = queries[q].cl->members;
    // An even cluster can be offered one split twice: a set and, from another rule, its complement.  The reference
    // computes both halves the same way both times, so its two gains differ by the order of one subtraction at most,
    // and which of them wins is rounding.  Here the second offer takes the first one's sides in the first one's order:
    // the two gains are the same number, the strict comparison keeps the first, whatever the hop plan.
    std::map<std::vector<int>, std::pair<int, int>> sides_of;
    std::vector<int> rest_set;
    for (size_t c = 0; c < queries[q].cands.size(); c++) {
      const SplitCand &cd = queries[q].cands[c];
      rest_set.clear();
      if (2 * cd.set.size() == mem.size())
        std::set_difference(mem.begin(), mem.end(), cd.set.begin(), cd.set.end(), std::back_inserter(rest_set));
      const auto twin = rest_set.empty() ? sides_of.end() : sides_of.find(rest_set);
      if (twin != sides_of.end()) {
        b.cands.push_back(TieCand{ps, twin->second.first, twin->second.second, 0});
        continue;
      }
      const int direct = b.add_side(TIE_SIDE_ROW, yes_row[q][c], 0);
      const int rest = b.add_side(TIE_SIDE_SUB, parent_row[q], yes_row[q][c]);
      // one hop sums the new set itself; two hops sum the rule's yes set, which is the new set when the answer is true
      const bool direct_is_child1 = hops == 1 || cd.first_answer;
      const int child1 = direct_is_child1 ? direct : rest, child2 = direct_is_child1 ? rest : direct;
      b.cands.push_back(TieCand{ps, child1, child2, 0});
      if (2 * cd.set.size() == mem.size()) sides_of[cd.set] = {child1, child2};
    }
  }
  std::vector<double> gains;
  run_batch(h, b, &gains, nullptr);
  size_t at = 0;
  for (SplitQuery &q : queries)
    for (SplitCand &c : q.cands) c.gain = gains[at++];
}

typedef std::function<void(std::vector<SplitQuery> &)> SplitEvaluator;

std::vector<Tree> make_trees(aasr_tie *h, int max_context) {
  std::vector<Tree> trees;
  for (auto &kv : h->phones) {
    Phone &ph = kv.second;
    ph.max_left = ph.max_right = 0;
    for (const auto &st : ph.cp)
      for (const auto &cp : st) {
        ph.max_left = std::max(ph.max_left, (int)h->classes[(size_t)cp.second].left.size());
        ph.max_right = std::max(ph.max_right, (int)h->classes[(size_t)cp.second].right.size());
      }
    for (int s = 0; s < (int)ph.cp.size(); s++) {
      Tree t;
      t.phone = &ph;
      t.state = s;
      t.ctx_start = max_context > 0 ? -std::min(ph.max_left, max_context) : -ph.max_left;
      t.ctx_end = max_context > 0 ? std::min(ph.max_right, max_context) : ph.max_right;
      trees.push_back(t);
    }
  }
  return trees;
}

// rule_answer for the search, by numbers: the context labels get ids, a rule is a 0/1 table over them
struct AnswerTables {
  std::vector<std::vector<int>> left, right;  // per class: label ids, nearest first
  std::vector<std::vector<char>> has;         // per rule: per label id
  explicit AnswerTables(const aasr_tie *h) {
    std::map<std::string, int> id;
    auto of = [&](const std::string &l) { return id.emplace(l, (int)id.size()).first->second; };
    for (const ContextPhone &p : h->classes) {
      left.emplace_back();
      right.emplace_back();
      for (const std::string &l : p.left) left.back().push_back(of(l));
      for (const std::string &l : p.right) right.back().push_back(of(l));
    }
    for (const Rule &r : h->rules) {
      has.emplace_back(id.size(), 0);
      for (const std::string &l : r.phones) {
        auto it = id.find(l);
        if (it != id.end()) has.back()[(size_t)it->second] = 1;
      }
    }
  }
  bool answer(int cls, int rule, int context) const {
    const std::vector<int> &c = context < 0 ? left[(size_t)cls] : right[(size_t)cls];
    const int k = (context < 0 ? -context : context) - 1;
    return k < (int)c.size() && has[(size_t)rule][(size_t)c[(size_t)k]];
  }
};

// the candidates of PhonePool::apply_best_splitting_rule that reach compute_log_likelihood_gain, in its order
std::vector<SplitCand> split_candidates(const aasr_tie *h, const AnswerTables &at, const Cluster &cl, int ctx_start, int ctx_end,
                                        double min_occ) {
  std::vector<SplitCand> out;
  std::vector<uint64_t> hashes;  // of the sets tried, to tell most of them apart without walking them
  std::vector<char> ans(cl.members.size());
  for (int r = 0; r < (int)h->rules.size(); r++)
    for (int i = ctx_start; i <= ctx_end; i++) {
      if (i == 0) continue;
      double c1 = 0;
      int n_yes = 0;
      for (size_t k = 0; k < cl.members.size(); k++) {
        ans[k] = at.answer(cl.members[k], r, i);
        if (ans[k]) {
          c1 += h->occ[(size_t)cl.members[k]];
          n_yes++;
        }
      }
      const double c2 = cl.occ - c1;
      if (c1 < min_occ || c2 < min_occ) continue;
      SplitCand c;
      c.rule = r;
      c.context = i;
      c.first_answer = n_yes <= (int)cl.members.size() / 2;
      uint64_t hash = 1469598103934665603ull;
      for (size_t k = 0; k < cl.members.size(); k++)
        if ((bool)ans[k] == c.first_answer) {
          c.set.push_back(cl.members[k]);
          hash = (hash ^ (uint64_t)cl.members[k]) * 1099511628211ull;
        }
      bool seen = false;
      for (size_t o = 0; o < out.size() && !seen; o++) seen = hashes[o] == hash && out[o].set == c.set;
      if (seen) continue;
      hashes.push_back(hash);
      out.push_back(std::move(c));
    }
  return out;
}

// PhonePool::decision_tree_cluster_context_phones: its loop per tree, all trees a round at a time
void split_trees(aasr_tie *h, int min_count, double sgain, int max_context, int info, const SplitEvaluator &evaluate) {
  if (!h->have_occ) raise(AASR_ERR_INVALID, "tie: no statistics set");
  if (h->rules.empty()) raise(AASR_ERR_INVALID, "tie: no rules");
  std::vector<Tree> trees = make_trees(h, max_context);
  const AnswerTables answers(h);
  for (Tree &t : trees) {
    Phone &ph = *t.phone;
    if (t.state == 0) ph.clusters.assign(ph.cp.size(), std::vector<Cluster>());
    Cluster first;
    for (const auto &cp : ph.cp[(size_t)t.state]) first.members.push_back(cp.second);
    std::sort(first.members.begin(), first.members.end());
    for (int m : first.members) first.occ += h->occ[(size_t)m];
    ph.clusters[(size_t)t.state].push_back(first);
  }
  h->rounds_split = 0;
  for (;;) {
    std::vector<SplitQuery> queries;
    for (size_t ti = 0; ti < trees.size(); ti++) {
      Tree &t = trees[ti];
      std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      while (t.cursor < (int)cls.size()) {
        SplitQuery q;
        q.tree = (int)ti;
        q.cl = &cls[(size_t)t.cursor];
        q.cands = split_candidates(h, answers, *q.cl, t.ctx_start, t.ctx_end, (double)min_count);
        if (q.cands.empty()) {
          t.cursor++;  // nothing to try: the cluster stays
          continue;
        }
        queries.push_back(std::move(q));
        break;
      }
    }
    if (queries.empty()) break;
    h->rounds_split++;
    evaluate(queries);
    for (SplitQuery &q : queries) {
      Tree &t = trees[(size_t)q.tree];
      std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      double best = -1;
      const SplitCand *win = nullptr;
      for (const SplitCand &c : q.cands)
        if (c.gain > best && c.gain > sgain) {
          best = c.gain;
          win = &c;
        }
      if (!win) {
        t.cursor++;
        continue;
      }
      Cluster &cl = cls[(size_t)t.cursor];
      Cluster other = cl;  // the rules applied so far go with both halves
      other.members.clear();
      std::set_difference(cl.members.begin(), cl.members.end(), win->set.begin(), win->set.end(),
                          std::back_inserter(other.members));
      cl.members = win->set;
      cl.occ = other.occ = 0;
      for (int m : cl.members) cl.occ += h->occ[(size_t)m];
      for (int m : other.members) other.occ += h->occ[(size_t)m];
      if (cl.rules.empty()) cl.rules.resize(1);
      if (other.rules.empty()) other.rules.resize(1);
      cl.rules[0].push_back(Applied{win->rule, win->context, win->first_answer});
      other.rules[0].push_back(Applied{win->rule, win->context, !win->first_answer});
      if (info > 1) {
        fprintf(stderr, "Applying rule %s:\n", h->rules[(size_t)win->rule].name.c_str());
        fprintf(stderr, "   context index:   %i\n", win->context);
        fprintf(stderr, "   likelihood gain: %.2f\n", best);
        fprintf(stderr, "   cluster counts:  %i + %i\n", (int)cl.occ, (int)other.occ);
      }
      cls.push_back(std::move(other));  // (cl is dead from here: the vector may have moved)
      // the split cluster is looked at again: the cursor stays
    }
  }
  if (info > 0) {
    int total = 0;
    for (const Tree &t : trees) {
      fprintf(stderr, "Processing phone %s, state %i\n", t.phone->label.c_str(), t.state);
      fprintf(stderr, "%i clusters generated\n", (int)t.phone->clusters[(size_t)t.state].size());
      total += (int)t.phone->clusters[(size_t)t.state].size();
    }
    fprintf(stderr, "Total: %i clusters generated\n", total);
  }
  h->split_done = true;
}

// PhonePool::merge_context_phones: the greedy loop per tree with its own cursor, a round of all trees' current
// (c, i > c) pairs in one launch.  Every cluster has a row in the sums; a merged cluster's row is summed again
// from its members at the start of the next round.
void merge_trees(aasr_tie *h, double mloss, int info) {
  if (!h->split_done) raise(AASR_ERR_INVALID, "tie: merge before split");
  std::vector<Tree> trees = make_trees(h, 0);
  std::vector<std::vector<int>> row(trees.size());  // per tree, per cluster: its row of the sums
  std::vector<int> orig(trees.size());
  int n_rows = 0;
  for (size_t ti = 0; ti < trees.size(); ti++) {
    orig[ti] = (int)trees[ti].phone->clusters[(size_t)trees[ti].state].size();
    for (int c = 0; c < orig[ti]; c++) row[ti].push_back(n_rows++);
  }
  // a cluster keeps its row number while the rounds run; every round's batch sums the clusters still in play
  h->rounds_merge = 0;
  for (;;) {
    Batch b;
    std::vector<int> side_of((size_t)n_rows, -1);
    bool any = false;
    for (size_t ti = 0; ti < trees.size(); ti++) {
      Tree &t = trees[ti];
      const std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      while (t.cursor < (int)cls.size() && t.cursor + 1 >= (int)cls.size()) t.cursor++;  // no partner left
      if (t.cursor >= (int)cls.size()) continue;
      any = true;
    }
    if (!any) break;
    // the sums: one job per cluster still in play (rows keep their numbers, so the jobs go in row order)
    std::vector<std::pair<int, const Cluster *>> live;
    for (size_t ti = 0; ti < trees.size(); ti++) {
      const Tree &t = trees[ti];
      const std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      if (t.cursor >= (int)cls.size()) continue;
      for (int c = t.cursor; c < (int)cls.size(); c++) live.push_back({row[ti][(size_t)c], &cls[(size_t)c]});
    }
    std::sort(live.begin(), live.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    std::vector<int> at_row((size_t)n_rows, -1);
    for (const auto &lv : live) {
      at_row[(size_t)lv.first] = b.add_job(0, lv.second->members.data(), (int)lv.second->members.size(), 1);
      for (int k = 0; k < (int)lv.second->members.size(); k++) b.set_bit(0, 0, k);
    }
    for (size_t ti = 0; ti < trees.size(); ti++) {
      const Tree &t = trees[ti];
      const std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      if (t.cursor >= (int)cls.size()) continue;
      auto side = [&](int r) {
        if (side_of[(size_t)r] < 0) side_of[(size_t)r] = b.add_side(TIE_SIDE_ROW, at_row[(size_t)r], 0);
        return side_of[(size_t)r];
      };
      const int rc = row[ti][(size_t)t.cursor];
      for (int i = t.cursor + 1; i < (int)cls.size(); i++) {
        const int ri = row[ti][(size_t)i];
        const int parent = b.add_side(TIE_SIDE_ADD, at_row[(size_t)rc], at_row[(size_t)ri]);
        b.cands.push_back(TieCand{parent, side(rc), side(ri), 0});
      }
    }
    std::vector<double> gains;
    run_batch(h, b, &gains, nullptr);
    h->rounds_merge++;
    size_t at = 0;
    for (size_t ti = 0; ti < trees.size(); ti++) {
      Tree &t = trees[ti];
      std::vector<Cluster> &cls = t.phone->clusters[(size_t)t.state];
      if (t.cursor >= (int)cls.size()) continue;
      double min_loss = 2 * mloss;
      int best_target = -1;
      for (int i = t.cursor + 1; i < (int)cls.size(); i++, at++)
        if (gains[at] < min_loss) {
          min_loss = gains[at];
          best_target = i;
        }
      if (min_loss < mloss && best_target > t.cursor) {
        Cluster &a = cls[(size_t)t.cursor];
        const Cluster &o = cls[(size_t)best_target];
        if (info > 1) {
          fprintf(stderr, "  Merging clusters %i and %i (occupancy counts %i + %i)\n", t.cursor, best_target, (int)a.occ, (int)o.occ);
          fprintf(stderr, "    Loglikelihood loss: %.2f\n", min_loss);
        }
        a.rules.insert(a.rules.end(), o.rules.begin(), o.rules.end());
        std::vector<int> u;
        std::set_union(a.members.begin(), a.members.end(), o.members.begin(), o.members.end(), std::back_inserter(u));
        a.members = u;
        a.occ = a.occ + o.occ;
        cls.erase(cls.begin() + best_target);
        row[ti].erase(row[ti].begin() + best_target);
      } else {
        t.cursor++;
      }
    }
  }
  if (info > 0) {
    int total = 0;
    for (size_t ti = 0; ti < trees.size(); ti++) {
      const int n = (int)trees[ti].phone->clusters[(size_t)trees[ti].state].size();
      fprintf(stderr, "Merging clusters of phone %s, state %i, initially %i clusters\n", trees[ti].phone->label.c_str(),
              trees[ti].state, orig[ti]);
      if (orig[ti] > n) fprintf(stderr, "Merging resulted %i clusters\n", n);
      else fprintf(stderr, "No clusters were merged\n");
      total += n;
    }
    fprintf(stderr, "Total %i clusters after merging\n", total);
  }
}

// ---- the writers -------------------------------------------------------------------------------------------

int number_states(aasr_tie *h) {
  int state_index = 0;
  for (auto &kv : h->phones)
    for (auto &st : kv.second.clusters)
      for (Cluster &c : st) c.state_index = state_index++;
  return state_index;
}

// PhonePool::iterate_context_phones: label, then the tied state of every HMM state
void iterate_context_phones(aasr_tie *h, int max_context,
                            const std::function<void(const std::string &, const std::vector<int> &)> &emit) {
  if (!h->split_done) raise(AASR_ERR_INVALID, "tie: nothing to write before the split");
  for (auto &kv : h->phones) {
    Phone &ph = kv.second;
    const int ns = (int)ph.cp.size();
    if (ph.label[0] == '_' || max_context <= 0) {
      std::vector<int> states;
      for (int s = 0; s < ns; s++) {
        if (ph.clusters[(size_t)s].empty()) raise(AASR_ERR_INVALID, "tie: phone %s state %d has no cluster", ph.label.c_str(), s);
        states.push_back(ph.clusters[(size_t)s][0].state_index);
      }
      emit(ph.label, states);
      continue;
    }
    if (h->contexts.empty()) continue;
    const std::vector<std::string> ctx(h->contexts.begin(), h->contexts.end());
    std::vector<size_t> it((size_t)max_context * 2, 0);
    for (;;) {
      std::string label;
      for (int i = 0; i < max_context; i++) label += ctx[it[(size_t)i]] + "-";
      label += ph.label;
      for (int i = max_context; i < 2 * max_context; i++) label += "+" + ctx[it[(size_t)i]];
      ContextPhone cur;
      cur.label = label;
      cur.left = left_contexts(label);
      cur.right = right_contexts(label);
      std::vector<int> states;
      for (int s = 0; s < ns; s++) {
        const std::vector<Cluster> &cls = ph.clusters[(size_t)s];
        int found = cls.size() == 1 ? 0 : -1;
        for (int i = 0; found < 0 && i < (int)cls.size(); i++)
          for (const std::vector<Applied> &set : cls[(size_t)i].rules) {
            bool fits = true;
            for (const Applied &a : set)
              if (rule_answer(cur, h->rules[(size_t)a.rule], a.context) != a.answer) {
                fits = false;
                break;
              }
            if (fits) {
              found = i;
              break;
            }
          }
        if (found < 0) raise(AASR_ERR_INVALID, "tie: no cluster of phone %s state %d takes %s", ph.label.c_str(), s, label.c_str());
        states.push_back(cls[(size_t)found].state_index);
      }
      emit(label, states);
      int i = 2 * max_context - 1;
      for (; i >= 0 && ++it[(size_t)i] == ctx.size(); i--)
        if (i > 0) it[(size_t)i] = 0;
      if (it[0] == ctx.size()) break;
    }
  }
}

std::string basebind_text(aasr_tie *h, int max_context) {
  number_states(h);
  std::string t;
  iterate_context_phones(h, max_context, [&](const std::string &label, const std::vector<int> &states) {
    t += label + " " + std::to_string(states.size());
    for (int s : states) t += " " + std::to_string(s);
    if (!states.empty()) t += "\n";  // SaveToBasebind::add_state ends the line with the last state
  });
  return t;
}

std::string g6(double v) {  // a double through an ostream of default precision
  char buf[64];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

// the final clusters' sums, [clusters x EP] in state order
std::vector<double> final_sums(aasr_tie *h) {
  Batch b;
  for (auto &kv : h->phones)
    for (auto &st : kv.second.clusters)
      for (Cluster &c : st) {
        b.add_job(0, c.members.data(), (int)c.members.size(), 1);
        for (int k = 0; k < (int)c.members.size(); k++) b.set_bit(0, 0, k);
      }
  std::vector<double> sums;
  run_batch(h, b, nullptr, &sums);
  return sums;
}

// PhonePool::save_model and HmmSet::write_all's three text formats
void write_model(aasr_tie *h, const std::string &base, int max_context) {
  const int n_states = number_states(h);
  const int d = h->D;
  const std::vector<double> sums = final_sums(h);
  std::string mc = std::to_string(n_states) + "\n";
  for (int s = 0; s < n_states; s++) mc += "1 " + std::to_string(s) + " 1\n";
  std::string ph_body;
  int n_hmms = 0;
  iterate_context_phones(h, max_context, [&](const std::string &label, const std::vector<int> &states) {
    const int ns = (int)states.size();
    n_hmms++;
    ph_body += std::to_string(n_hmms) + " " + std::to_string(ns + 2) + " " + label + "\n-1 -2";
    for (int s : states) ph_body += " " + std::to_string(s);
    ph_body += "\n0 1 2 1\n1 0\n";
    for (int s = 0; s < ns; s++) {
      const int next = s + 3 == ns + 2 ? 1 : s + 3;
      ph_body += std::to_string(s + 2) + " 2 " + std::to_string(s + 2) + " " + g6(0.8) + " " + std::to_string(next) + " " + g6(0.2) + "\n";
    }
  });
  const std::string ph = "PHONE\n" + std::to_string(n_hmms) + "\n" + ph_body;
  std::string gk = std::to_string(n_states) + " " + std::to_string(d) + " variable\n";
  std::vector<double> mu((size_t)d);
  for (int s = 0; s < n_states; s++) {
    const double *r = sums.data() + (size_t)s * h->EP;
    const double gamma = r[0];
    gk += "full ";
    for (int i = 0; i < d; i++) {
      mu[(size_t)i] = r[1 + i] / gamma;
      gk += g6(mu[(size_t)i]) + " ";
    }
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) {
        const int a = std::max(i, j), c = std::min(i, j);
        const double v = r[1 + d + a * (a + 1) / 2 + c] / gamma - mu[(size_t)a] * mu[(size_t)c];
        gk += g6(v);
        if (!(i == d - 1 && j == d - 1)) gk += " ";
      }
    gk += "\n";
  }
  write_text_file((base + ".mc").c_str(), mc.data(), mc.size());
  write_text_file((base + ".ph").c_str(), ph.data(), ph.size());
  write_text_file((base + ".gk").c_str(), gk.data(), gk.size());
}

// A context phone's class: its row of the statistics.  A class EXISTS for the pool once it is registered: the recipe
// pass numbers every (label, state) of the .phn files first and registers those the reference would have created.
int find_or_add_class(aasr_tie *h, const std::string &label, int state) {
  if (state < 0) raise(AASR_ERR_INVALID, "PhonePool::Phone::get_context_phone: Invalid state %i", state);
  auto it = h->class_index.find({label, state});
  if (it != h->class_index.end()) return it->second;
  if (h->have_occ) raise(AASR_ERR_INVALID, "tie: no new context phones once the statistics are set");
  ContextPhone cp;
  cp.label = label;
  cp.state = state;
  cp.center = center_phone(label);
  cp.left = left_contexts(label);
  cp.right = right_contexts(label);
  const int cls = (int)h->classes.size();
  h->classes.push_back(cp);
  h->class_index[{label, state}] = cls;
  return cls;
}

// PhonePool::get_context_phone's insertions: the phone, the state's map, the pool's context set
void register_class(aasr_tie *h, int cls) {
  const ContextPhone &cp = h->classes[(size_t)cls];
  Phone &ph = h->phones[cp.center];
  ph.label = cp.center;
  if (cp.state >= (int)ph.cp.size()) ph.cp.resize((size_t)cp.state + 1);
  if (!ph.cp[(size_t)cp.state].insert({cp.label, cls}).second) return;
  for (const std::string &c : cp.left) h->contexts.insert(c);
  for (const std::string &c : cp.right) h->contexts.insert(c);
}

int get_class(aasr_tie *h, const std::string &label, int state) {
  const int cls = find_or_add_class(h, label, state);
  register_class(h, cls);
  return cls;
}

// the E tile offsets of a row's values in a scatter accumulator (scatter.h)
std::vector<int32_t> pack_map(int d) {
  std::vector<int32_t> map;
  auto at = [](int r, int q) { return (int32_t)(((r / 16) * (r / 16 + 1) / 2 + q / 16) * 256 + (r % 16) * 16 + q % 16); };
  map.push_back(at(0, 0));
  for (int i = 0; i < d; i++) map.push_back(at(i + 1, 0));
  for (int i = 0; i < d; i++)
    for (int j = 0; j <= i; j++) map.push_back(at(i + 1, j + 1));
  return map;
}

char *dup_text(const std::string &t, int64_t *len) {
  char *p = (char *)malloc(t.size() + 1);
  if (!p) raise(AASR_ERR_INVALID, "out of memory");
  memcpy(p, t.data(), t.size());
  p[t.size()] = 0;
  if (len) *len = (int64_t)t.size();
  return p;
}

// the first module's frame rate, host only (FeatureGenerator::frame_rate is the first module's)
float configured_frame_rate(const std::string &text) {
  size_t pos = 0;
  while (pos < text.size()) {
    size_t e = text.find('\n', pos);
    if (e == std::string::npos) e = text.size();
    const std::string line = str_clean(text.substr(pos, e - pos), " \t");
    pos = e + 1;
    if (line.empty()) continue;
    if (line != "module") raise(AASR_ERR_INVALID, "expected keyword 'module' in the feature configuration: %s", line.c_str());
    ModuleConfig cfg;
    cfg.read(text, &pos);
    float fr = 125;
    cfg.get("frame_rate", fr);
    return fr;
  }
  raise(AASR_ERR_INVALID, "the feature configuration has no module");
}

}  // namespace

extern "C" {

aasr_status aasr_tie_parse_label(const char *label, char **text, int64_t *len) {
  return guarded([&] {
    if (!label || !text) raise(AASR_ERR_INVALID, "aasr_tie_parse_label: null argument");
    std::string t = center_phone(label) + "\n";
    const std::vector<std::string> l = left_contexts(label), r = right_contexts(label);
    for (size_t i = 0; i < l.size(); i++) t += (i ? "\x1f" : "") + l[i];
    t += "\n";
    for (size_t i = 0; i < r.size(); i++) t += (i ? "\x1f" : "") + r[i];
    *text = dup_text(t, len);
  });
}

aasr_status aasr_tie_create(int32_t dim, const char *rule_path, aasr_tie **out) {
  return guarded([&] {
    if (!out || !rule_path || dim < 1) raise(AASR_ERR_INVALID, "aasr_tie_create: bad argument");
    *out = nullptr;
    if (dim > TIE_MAX_DIM) raise(AASR_ERR_UNSUPPORTED, "tie: no gain kernel for dimension %d (1 ... %d)", dim, TIE_MAX_DIM);
    std::unique_ptr<aasr_tie> h(new aasr_tie());
    h->D = dim;
    h->E = tie_row_values(dim);
    h->EP = tie_row_stride(dim);
    h->rules = read_rules(rule_path);
    *out = h.release();
  });
}

void aasr_tie_destroy(aasr_tie *h) { delete h; }

int32_t aasr_tie_num_rules(const aasr_tie *h) { return h ? (int32_t)h->rules.size() : 0; }
int32_t aasr_tie_num_classes(const aasr_tie *h) { return h ? (int32_t)h->classes.size() : 0; }

aasr_status aasr_tie_rules_text(const aasr_tie *h, char **text, int64_t *len) {
  return guarded([&] {
    if (!h || !text) raise(AASR_ERR_INVALID, "aasr_tie_rules_text: null argument");
    std::string t;
    for (const Rule &r : h->rules) {
      t += r.name;
      for (const std::string &p : r.phones) t += "\x1f" + p;
      t += "\n";
    }
    *text = dup_text(t, len);
  });
}

aasr_status aasr_tie_context_phone(aasr_tie *h, const char *label, int32_t state, int32_t *cls) {
  return guarded([&] {
    if (!h || !label || !cls) raise(AASR_ERR_INVALID, "aasr_tie_context_phone: null argument");
    *cls = get_class(h, label, state);
  });
}

aasr_status aasr_debug_tie_set_occupancy(aasr_tie *h, const double *gamma) {
  return guarded([&] {
    if (!h || !gamma) raise(AASR_ERR_INVALID, "aasr_debug_tie_set_occupancy: null argument");
    h->occ.assign(gamma, gamma + h->classes.size());
    h->have_occ = true;
  });
}

aasr_status aasr_tie_set_stats(aasr_tie *h, const double *gamma, const double *sum_x, const double *sum_xx) {
  return guarded([&] {
    if (!h || !gamma || !sum_x || !sum_xx) raise(AASR_ERR_INVALID, "aasr_tie_set_stats: null argument");
    require_device();
    const size_t C = h->classes.size(), d = (size_t)h->D, tri = d * (d + 1) / 2;
    std::vector<double> rows(std::max<size_t>(1, C) * h->EP, 0.0);
    for (size_t c = 0; c < C; c++) {
      double *r = rows.data() + c * h->EP;
      r[0] = gamma[c];
      std::copy(sum_x + c * d, sum_x + (c + 1) * d, r + 1);
      std::copy(sum_xx + c * tri, sum_xx + (c + 1) * tri, r + 1 + d);
    }
    h->rows.upload(rows.data(), rows.size());
    h->occ.assign(gamma, gamma + C);
    h->have_occ = h->have_stats = true;
  });
}

aasr_status aasr_tie_evaluate(aasr_tie *h, int32_t n_jobs, const int32_t *job_k, const int32_t *job_rows, const int32_t *idx,
                              const uint32_t *mask, double *sums, int32_t n_cands, const int32_t *cands, double *gain) {
  return guarded([&] {
    if (!h || n_jobs < 0 || n_cands < 0 || (n_jobs > 0 && (!job_k || !job_rows)) || (n_cands > 0 && (!cands || !gain)))
      raise(AASR_ERR_INVALID, "aasr_tie_evaluate: bad argument");
    if (!h->have_stats) raise(AASR_ERR_INVALID, "aasr_tie_evaluate: no statistics set");
    Batch b;
    int64_t ia = 0, ma = 0;
    for (int j = 0; j < n_jobs; j++) {
      if (job_k[j] < 0 || job_rows[j] < 0 || (job_k[j] > 0 && !idx) || (job_k[j] > 0 && job_rows[j] > 0 && !mask))
        raise(AASR_ERR_INVALID, "aasr_tie_evaluate: job %d: bad size", j);
      for (int k = 0; k < job_k[j]; k++)
        if (idx[ia + k] < 0 || idx[ia + k] >= (int32_t)h->classes.size())
          raise(AASR_ERR_INVALID, "aasr_tie_evaluate: job %d: member %d out of range", j, idx[ia + k]);
      b.add_job(0, idx ? idx + ia : nullptr, job_k[j], job_rows[j]);
      const int64_t words = (int64_t)((job_k[j] + 31) / 32) * job_rows[j];
      if (words > 0) std::copy(mask + ma, mask + ma + words, b.mask.end() - words);
      ia += job_k[j];
      ma += words;
    }
    std::map<int, int> row_side;
    auto side = [&](int r) {
      auto it = row_side.find(r);
      if (it != row_side.end()) return it->second;
      return row_side[r] = b.add_side(TIE_SIDE_ROW, r, 0);
    };
    for (int c = 0; c < n_cands; c++) {
      const int p = cands[3 * c], a = cands[3 * c + 1], o = cands[3 * c + 2];
      if (p < 0 || p >= b.n_out || a < 0 || a >= b.n_out || o < -1 || o >= b.n_out)
        raise(AASR_ERR_INVALID, "aasr_tie_evaluate: candidate %d: row out of range", c);
      const int s2 = o >= 0 ? side(o) : b.add_side(TIE_SIDE_SUB, p, a);
      b.cands.push_back(TieCand{side(p), side(a), s2, 0});
    }
    std::vector<double> g, s;
    run_batch(h, b, &g, sums ? &s : nullptr);
    if (n_cands > 0) std::copy(g.begin(), g.end(), gain);
    if (sums)
      for (int r = 0; r < b.n_out; r++) std::copy(s.begin() + (int64_t)r * h->EP, s.begin() + (int64_t)r * h->EP + h->E, sums + (int64_t)r * h->E);
  });
}

void aasr_debug_tie_shape(const aasr_tie *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 4; i++) out[i] = h ? h->last_shape[i] : 0;
  out[4] = h ? h->rounds_split : 0;
  out[5] = h ? h->rounds_merge : 0;
}

aasr_status aasr_tie_split(aasr_tie *h, int32_t min_count, double sgain, int32_t max_context, int32_t hops, int32_t info) {
  return guarded([&] {
    if (!h || hops < 1 || hops > 2) raise(AASR_ERR_INVALID, "aasr_tie_split: bad argument");
    require_device();
    if (!h->have_stats) raise(AASR_ERR_INVALID, "tie: no statistics set");
    split_trees(h, min_count, sgain, max_context, info, [&](std::vector<SplitQuery> &q) { device_split_gains(h, q, hops); });
  });
}

aasr_status aasr_debug_tie_split_given(aasr_tie *h, int32_t min_count, double sgain, int32_t max_context, aasr_tie_gain_fn fn,
                                       void *user) {
  return guarded([&] {
    if (!h || !fn) raise(AASR_ERR_INVALID, "aasr_debug_tie_split_given: null argument");
    split_trees(h, min_count, sgain, max_context, 0, [&](std::vector<SplitQuery> &qs) {
      for (SplitQuery &q : qs)
        for (SplitCand &c : q.cands)
          c.gain = fn(user, (int32_t)q.cl->members.size(), q.cl->members.data(), (int32_t)c.set.size(), c.set.data());
    });
  });
}

aasr_status aasr_tie_merge(aasr_tie *h, double mloss, int32_t info) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_tie_merge: null argument");
    require_device();
    merge_trees(h, mloss, info);
  });
}

aasr_status aasr_tie_clusters_text(aasr_tie *h, char **text, int64_t *len) {
  return guarded([&] {
    if (!h || !text) raise(AASR_ERR_INVALID, "aasr_tie_clusters_text: null argument");
    if (!h->split_done) raise(AASR_ERR_INVALID, "tie: no clusters before the split");
    number_states(h);
    std::string t;
    char buf[64];
    for (auto &kv : h->phones)
      for (size_t s = 0; s < kv.second.clusters.size(); s++)
        for (const Cluster &c : kv.second.clusters[s]) {
          snprintf(buf, sizeof buf, "%.17g", c.occ);
          t += kv.first + "\x1f" + std::to_string(s) + "\x1f" + std::to_string(c.state_index) + "\x1f" + buf + "\x1f";
          for (size_t m = 0; m < c.members.size(); m++) t += (m ? "," : "") + std::to_string(c.members[m]);
          t += "\x1f";
          for (size_t r = 0; r < c.rules.size(); r++) {
            if (r) t += "|";
            for (size_t a = 0; a < c.rules[r].size(); a++)
              t += (a ? "," : "") + h->rules[(size_t)c.rules[r][a].rule].name + ":" + std::to_string(c.rules[r][a].context) + ":" +
                   (c.rules[r][a].answer ? "1" : "0");
          }
          t += "\n";
        }
    *text = dup_text(t, len);
  });
}

aasr_status aasr_tie_basebind_text(aasr_tie *h, int32_t max_context, char **text, int64_t *len) {
  return guarded([&] {
    if (!h || !text) raise(AASR_ERR_INVALID, "aasr_tie_basebind_text: null argument");
    *text = dup_text(basebind_text(h, max_context), len);
  });
}

aasr_status aasr_tie_write_basebind(aasr_tie *h, const char *path, int32_t max_context) {
  return guarded([&] {
    if (!h || !path) raise(AASR_ERR_INVALID, "aasr_tie_write_basebind: null argument");
    FILE *fp = fopen(path, "w");
    if (!fp) raise(AASR_ERR_IO, "Could not open file %s for writing.", path);
    std::unique_ptr<FILE, int (*)(FILE *)> guard(fp, fclose);
    const std::string t = basebind_text(h, max_context);
    if (fwrite(t.data(), 1, t.size(), fp) != t.size()) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_tie_write_model(aasr_tie *h, const char *base, int32_t max_context) {
  return guarded([&] {
    if (!h || !base) raise(AASR_ERR_INVALID, "aasr_tie_write_model: null argument");
    require_device();
    write_model(h, base, max_context);
  });
}

void aasr_tie_default_options(aasr_tie_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->count = 100;
  o->context = 1;
  o->hops = 1;
}

}  // extern "C"

// ---- the tie main loop over a recipe ---------------------------------------------------------------------------

extern "C" aasr_status aasr_run_tie_recipe(const char *feat_cfg_text, const char *recipe_path, aasr_tie_options *opt,
                                           aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat_cfg_text || !recipe_path || !opt || !opt->rule) raise(AASR_ERR_INVALID, "aasr_run_tie_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    opt->seconds_scatter = opt->seconds_features = opt->seconds_split = opt->seconds_merge = 0;
    // ---- host only, before the device is opened (tie.cc:137-160)
    if (opt->hmmnet) throw std::string("This feature is currently broken. Fix it?");
    const float fr = configured_frame_rate(feat_cfg_text);
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, 0, 0, false);  // tie.cc:143
    if (!((opt->out != nullptr) ^ (opt->basebind != nullptr))) throw std::string("Specify either --out or --basebind for output");
    if (opt->hops < 1 || opt->hops > 2) raise(AASR_ERR_INVALID, "tie: hops must be 1 or 2");
    refuse_line_limits(infos, "tie");
    const std::vector<Rule> rules = read_rules(opt->rule);
    // the text pass: every (label, state) of the .phn files gets a class, so that the accumulator can be sized and a
    // line without a state number is found before the device is opened.  Which of them exist for the pool is known
    // only with the feature end: collect_phone_stats creates a line's context phone, then meets the end and leaves.
    struct Line {
      int cls, start, end;
    };
    std::unique_ptr<aasr_tie> h(new aasr_tie());
    h->rules = rules;
    std::vector<std::vector<Line>> lines(infos.size());
    for (size_t f = 0; f < infos.size(); f++) {
      const std::string &path = opt->ophn ? infos[f].alignment_path : infos[f].transcript_path;
      FILE *fp = fopen(path.c_str(), "r");
      if (!fp) raise(AASR_ERR_IO, "PhnReader::open(): could not open %s", path.c_str());
      std::unique_ptr<FILE, int (*)(FILE *)> guard(fp, fclose);
      int first, last, line_no = 0;
      frame_range(infos[f], fr, &first, &last);
      const float spf = 16000 / fr;
      if (first > 0 || last > 0) phn_skip_to_first_frame(fp, spf, first, last, &line_no);
      PhnLine phn;
      while (next_phn_line(fp, spf, first, last, &line_no, &phn)) {
        if (phn.state == -1) throw std::string("Context phone tying requires phn files with state numbers!");
        lines[f].push_back(Line{find_or_add_class(h.get(), phn.label, phn.state), phn.start, phn.end});
      }
    }
    const int C = (int)h->classes.size();
    if (C == 0) raise(AASR_ERR_INVALID, "tie: the recipe's .phn files name no context phone");

    // ---- the device
    std::unique_ptr<aasr_feat> feat(feat_create(feat_cfg_text));
    const int D = aasr_feat_dim(feat.get());
    if (D > TIE_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "tie: feature dimension %d: the gain kernel is built for 1 ... %d", D, TIE_MAX_DIM);
    h->D = D;
    h->E = tie_row_values(D);
    h->EP = tie_row_stride(D);
    aasr_spkc *spk = nullptr;
    if (opt->speakers) {
      if (aasr_spkc_create(feat.get(), nullptr, &spk) != AASR_OK || aasr_spkc_read_file(spk, opt->speakers) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    std::unique_ptr<aasr_spkc, void (*)(aasr_spkc *)> spguard(spk, aasr_spkc_destroy);
    aasr_scatter *sc = nullptr;
    {
      const aasr_status cs = aasr_scatter_create(C, D, &sc);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_scatter, void (*)(aasr_scatter *)> scguard(sc, aasr_scatter_destroy);
    int64_t num_frames = 0;
    {
      GroupStager stager(feat.get(), spk, -1);
      const hipStream_t stream = stager.stream;
      hipEvent_t ev[3];
      for (hipEvent_t &e : ev) AASR_HIP(hipEventCreate(&e));
      struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() {
          for (int i = 0; i < 3; i++) (void)hipEventDestroy(e[i]);
        }
      } evguard{ev};
      const int64_t max_group_frames = (int64_t)1 << 18;
      size_t next = 0;
      while (next < infos.size()) {
        const size_t group_first = next;
        std::vector<std::vector<int16_t>> audio;
        std::vector<int32_t> start, rows, cls;
        int64_t rows_total = 0;
        while (next < infos.size() && audio.size() < 1024 && rows_total < max_group_frames) {
          announce(infos[next], opt->info);
          audio.emplace_back();
          audio.back() = load_utterance_input(feat.get(), infos[next]);
          const int eof = aasr_feat_eof_frame(feat.get(), (int64_t)audio.back().size());
          // collect_phone_stats: frames start ... end - 1 of every line; the feature end cuts the line and the file
          const std::vector<Line> &ls = lines[next];
          int lo = -1, hi = -1;
          std::vector<std::pair<int, int>> spans;  // (frame, class)
          for (const Line &l : ls) {
            register_class(h.get(), l.cls);  // frames or not
            bool cut = false;
            for (int fnum = l.start; fnum < l.end; fnum++) {
              if (fnum >= eof) {
                cut = true;
                break;
              }
              spans.push_back({fnum, l.cls});
            }
            if (cut) break;
          }
          for (const auto &sp : spans) {
            lo = lo < 0 ? sp.first : std::min(lo, sp.first);
            hi = std::max(hi, sp.first);
          }
          const int n = lo < 0 ? 0 : hi - lo + 1;
          const size_t base = cls.size();
          cls.resize(base + (size_t)n, -1);
          for (const auto &sp : spans) {
            if (cls[base + (size_t)(sp.first - lo)] != -1)
              raise(AASR_ERR_UNSUPPORTED, "tie: %s: frame %d lies in two .phn lines",
                    (opt->ophn ? infos[next].alignment_path : infos[next].transcript_path).c_str(), sp.first);
            cls[base + (size_t)(sp.first - lo)] = sp.second;
          }
          if (n == 0) audio.back().clear();
          start.push_back(std::max(lo, 0));
          rows.push_back(n);
          rows_total += n;
          num_frames += (int64_t)spans.size();
          next++;
        }
        stager.stage(audio, start, rows, [&](size_t i) {
          if (i == 0) AASR_HIP(hipEventRecord(ev[0], stream));
          apply_speaker(spk, infos[group_first + i]);  // tie.cc:207-212
        });
        AASR_HIP(hipEventRecord(ev[1], stream));
        if (rows_total > 0 && aasr_scatter_accumulate_dev(sc, stager.d_x.p, rows_total, cls.data(), nullptr, stream) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        AASR_HIP(hipEventRecord(ev[2], stream));
        AASR_HIP(hipStreamSynchronize(stream));
        float ms = 0;
        AASR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        opt->seconds_features += ms * 1e-3;
        AASR_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
        opt->seconds_scatter += ms * 1e-3;
      }
    }
    // the sums stay on the device: the accumulator's tiles become the rows of the search
    {
      const std::vector<int32_t> map = pack_map(D);
      DevBuf<int32_t> d_map;
      d_map.upload(map.data(), map.size());
      h->rows.alloc((size_t)C * h->EP);
      tie_pack_launch(scatter_device_accumulator(sc), scatter_class_doubles(D), d_map.p, D, C, h->rows.p, nullptr);
      h->occ.resize((size_t)C);
      AASR_HIP(hipMemcpy2D(h->occ.data(), sizeof(double), h->rows.p, (size_t)h->EP * sizeof(double), sizeof(double), (size_t)C,
                           hipMemcpyDeviceToHost));
      AASR_HIP(hipDeviceSynchronize());
      h->have_occ = h->have_stats = true;
    }
    scguard.reset();
    if (opt->info > 0) {
      size_t n = 0;
      for (const auto &kv : h->phones)
        for (const auto &st : kv.second.cp) n += st.size();
      fprintf(stderr, "%i context dependent phone states in total\n", (int)n);
    }
    const auto t1 = std::chrono::steady_clock::now();
    split_trees(h.get(), opt->count, opt->sgain, opt->context, opt->info,
                [&](std::vector<SplitQuery> &q) { device_split_gains(h.get(), q, opt->hops); });
    const auto t2 = std::chrono::steady_clock::now();
    if (opt->mloss_given) merge_trees(h.get(), opt->mloss, opt->info);
    const auto t3 = std::chrono::steady_clock::now();
    opt->seconds_split = std::chrono::duration<double>(t2 - t1).count();
    opt->seconds_merge = std::chrono::duration<double>(t3 - t2).count();
    if (opt->out) {
      write_model(h.get(), opt->out, opt->context);
    } else {
      FILE *fp = fopen(opt->basebind, "w");
      if (!fp) raise(AASR_ERR_IO, "Could not open file %s for writing.", opt->basebind);
      std::unique_ptr<FILE, int (*)(FILE *)> guard(fp, fclose);
      const std::string t = basebind_text(h.get(), opt->context);
      if (fwrite(t.data(), 1, t.size(), fp) != t.size()) raise(AASR_ERR_IO, "write error on %s", opt->basebind);
    }
    opt->clusters = number_states(h.get());
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, opt->seconds_scatter + opt->seconds_features);
  });
}

// fst_net.cc -- reader of the FST decoder's search network and duration tables (fst_net.h).
#include "fst_net.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "common.h"

namespace aasr {

namespace {

// str::read_line(line, file, true): false at the end of the file
bool read_line(std::string &s, FILE *f) {
  char buf[4096];
  s.clear();
  while (fgets(buf, sizeof buf, f)) {
    s.append(buf);
    if (s[s.size() - 1] == '\n') break;
  }
  if (ferror(f) || s.empty()) return false;
  if (s[s.size() - 1] == '\n') s.erase(s.size() - 1);
  return true;
}

// str::split(line, " ", true): runs of spaces are one delimiter, a trailing delimiter adds an empty field
std::vector<std::string> split(const std::string &str) {
  std::vector<std::string> fields;
  size_t begin = 0, end = 0;
  bool pending = false;
  while (begin < str.size()) {
    pending = false;
    while (end < str.size()) {
      if (str[end] == ' ') {
        pending = true;
        break;
      }
      end++;
    }
    fields.push_back(str.substr(begin, end - begin));
    end++;
    while (end < str.size() && str[end] == ' ') end++;
    begin = end;
  }
  if (pending) fields.push_back("");
  return fields;
}

struct File {
  FILE *f;
  ~File() {
    if (f) fclose(f);
  }
};

}  // namespace

void fst_net_read(const char *path, aasr_fstnet &net) {
  File in{fopen(path, "r")};
  if (!in.f) raise(AASR_ERR_IO, "fst: cannot open %s: %s", path, strerror(errno));
  std::string line;
  read_line(line, in.f);
  if (line != "#FSTBasic MaxPlus") raise(AASR_ERR_INVALID, "Unknown header '%s'.", line.c_str());
  std::vector<int32_t> pdf, end;
  std::vector<std::vector<int32_t>> out;  // arcs of a node, file order
  std::vector<int32_t> tgt, word;
  std::vector<float> lp;
  std::map<std::string, int32_t> sym_id;
  int32_t initial = -1;
  auto grow = [&](int32_t n) {
    if ((int64_t)pdf.size() <= n) {
      pdf.resize((size_t)n + 1, -1);
      end.resize((size_t)n + 1, 0);
      out.resize((size_t)n + 1);
    }
  };
  while (read_line(line, in.f)) {
    const std::vector<std::string> f = split(line);
    if (f.size() < 2) raise(AASR_ERR_INVALID, "Too few fields '%s'.", line.c_str());
    const int32_t first = atoi(f[1].c_str());
    if (first < 0) raise(AASR_ERR_INVALID, "Negative node index '%s'.", line.c_str());
    grow(first);
    if (f[0] == "I") {
      initial = first;
      if (f.size() > 2) raise(AASR_ERR_INVALID, "Too many fields for I: '%s'.", line.c_str());
      continue;
    }
    if (f[0] == "F") {
      end[(size_t)first] = 1;
      if (f.size() > 2) raise(AASR_ERR_INVALID, "Too many fields for F: '%s'.", line.c_str());
      continue;
    }
    if (f[0] != "T") raise(AASR_ERR_INVALID, "Weird type indicator: '%s'.", f[0].c_str());
    if (f.size() < 3 || f.size() > 6) raise(AASR_ERR_INVALID, "Weird number of fields for T: '%s'.", line.c_str());
    const int32_t second = atoi(f[2].c_str());
    if (second < 0) raise(AASR_ERR_INVALID, "Negative node index '%s'.", line.c_str());
    grow(second);
    int32_t w = -1;
    if (f.size() >= 5 && f[4] != ",") {
      auto it = sym_id.find(f[4]);
      if (it == sym_id.end()) {
        it = sym_id.emplace(f[4], (int32_t)net.symbols.size()).first;
        net.symbols.push_back(f[4]);
      }
      w = it->second;
    }
    out[(size_t)first].push_back((int32_t)tgt.size());
    tgt.push_back(second);
    word.push_back(w);
    lp.push_back(f.size() >= 6 ? (float)strtod(f[5].c_str(), nullptr) : 0.0f);
    const int32_t p = f.size() >= 4 ? atoi(f[3].c_str()) : -1;
    if (pdf[(size_t)second] == -1)
      pdf[(size_t)second] = p;
    else if (pdf[(size_t)second] != p)
      raise(AASR_ERR_INVALID, "Conflicting emission_pdf_indices for node %d: %d != %d.", second, pdf[(size_t)second], p);
  }
  if (initial < 0) raise(AASR_ERR_INVALID, "No initial node.");
  const size_t n = pdf.size();
  net.arc_begin.assign(n + 1, 0);
  net.max_degree = 0;
  net.max_pdf = -1;
  for (size_t i = 0; i < n; i++) {
    net.arc_begin[i + 1] = net.arc_begin[i] + (int32_t)out[i].size();
    net.max_degree = std::max(net.max_degree, (int32_t)out[i].size());
    net.max_pdf = std::max(net.max_pdf, pdf[i]);
    for (int32_t a : out[i]) {
      net.arc_tgt.push_back(tgt[(size_t)a]);
      net.arc_word.push_back(word[(size_t)a]);
      net.arc_lp.push_back(lp[(size_t)a]);
    }
  }
  net.node_pdf = pdf;
  net.node_end = end;
  net.initial = initial;
}

void fst_durations_read(const char *path, aasr_fst_durations &dur) {
  std::ifstream in(path);
  if (!in) raise(AASR_ERR_IO, "FstAcoustics: open error (%s)", path);
  int version = 0, n = 0;
  in >> version;
  if (!in || version != 4) raise(AASR_ERR_INVALID, "FstAcoustics: invalid format (%s: version)", path);
  in >> n;
  if (!in || n < 0) raise(AASR_ERR_INVALID, "FstAcoustics: invalid format (%s: number of states)", path);
  dur.n = n;
  dur.a.clear();
  dur.b.clear();
  for (int i = 0; i < n; i++) {
    int id = -1;
    float a = 0, b = 0;
    in >> id;
    if (!in || id != i) raise(AASR_ERR_INVALID, "FstAcoustics: invalid format (%s: state %d)", path, i);
    in >> a >> b;
    if (!in) raise(AASR_ERR_INVALID, "FstAcoustics: invalid format (%s: state %d)", path, i);
    dur.a.push_back(a);
    dur.b.push_back(b);
  }
}

float fst_duration_logprob(const aasr_fst_durations *dur, bool by_state, int32_t pdf, int32_t d) {
  if (!dur || pdf < 0) return 0.0f;
  // the reference's tables: n zeros, then the file's values; by_state: the file's values
  const int32_t at = by_state ? pdf : pdf - dur->n;
  if (at < 0 || at >= dur->n) return 0.0f;
  const float a = dur->a[(size_t)at];
  if (a <= 0) return 0.0f;
  const float b = dur->b[(size_t)at];
  const float const_term = -a * logf(b) - lgammaf(a);
  return (a - 1) * logf((float)d) - d / b + const_term;
}

void fst_dur_table(const aasr_fst_durations *dur, bool by_state, int32_t n_pdf, int32_t D, std::vector<int32_t> &slot,
                   std::vector<float> &table) {
  slot.assign((size_t)std::max(0, n_pdf), -1);
  table.clear();
  if (!dur) return;
  int32_t rows = 0;
  for (int32_t p = 0; p < n_pdf; p++) {
    const int32_t at = by_state ? p : p - dur->n;
    if (at < 0 || at >= dur->n || dur->a[(size_t)at] <= 0) continue;
    slot[(size_t)p] = rows++;
    for (int32_t d = 0; d <= D; d++) table.push_back(fst_duration_logprob(dur, by_state, p, d));
  }
}

}  // namespace aasr

// align.cc -- the forced aligner's host side: the HMM topology handle, transcripts, the batched
// search's driver (aasr_align_batch_*) and the align main loop over a recipe
// (aasr_run_align_recipe, aku/align.cc:171-346).  The search itself is align_viterbi.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "align.h"
#include "aku/str.hh"
#include "common.h"
#include "ph_parse.h"
#include "phn_line.h"
#include "recipe_pass.h"

struct aasr_topo {
  struct Hmm {
    std::string label;
    std::vector<int> states;
  };
  std::vector<Hmm> hmms;
  std::map<std::string, int> index;
  std::vector<std::vector<aasr::PhTransition>> state_info;
  int max_off = 0;
};

using namespace aasr;

extern "C" {

aasr_status aasr_topo_create_from_ph(const char *ph_path, aasr_topo **out) {
  return guarded([&] {
    if (!ph_path || !out) raise(AASR_ERR_INVALID, "aasr_topo_create_from_ph: null argument");
    *out = nullptr;
    std::ifstream in(ph_path);
    if (!in) raise(AASR_ERR_IO, "aasr_topo_create_from_ph: could not open %s", ph_path);
    std::string word;
    in >> word;
    if (word != "PHONE") raise(AASR_ERR_INVALID, "%s: not a PHONE topology file", ph_path);
    std::unique_ptr<aasr_topo> t(new aasr_topo());
    parse_legacy_ph(
        in,
        [&](const std::string &label, int states) {
          if (t->index.count(label)) raise(AASR_ERR_INVALID, "%s: duplicate HMM %s", ph_path, label.c_str());
          if (states < 0) raise(AASR_ERR_INVALID, "%s: HMM %s has %d states", ph_path, label.c_str(), states + 2);
          t->index[label] = (int)t->hmms.size();
          t->hmms.push_back({label, std::vector<int>((size_t)states)});
        },
        [&](int s, int pdf) { t->hmms.back().states[(size_t)s] = pdf; },
        [&] { raise(AASR_ERR_INVALID, "%s: read error", ph_path); }, t->state_info);
    for (const auto &v : t->state_info)
      for (const PhTransition &tr : v) t->max_off = std::max(t->max_off, tr.target_offset);
    *out = t.release();
  });
}

void aasr_topo_destroy(aasr_topo *h) { delete h; }
int32_t aasr_topo_num_hmms(const aasr_topo *h) { return h ? (int32_t)h->hmms.size() : -1; }
int32_t aasr_topo_hmm_index(const aasr_topo *h, const char *label) {
  if (!h || !label) return -1;
  const auto it = h->index.find(label);
  return it == h->index.end() ? -1 : it->second;
}
const char *aasr_topo_hmm_label(const aasr_topo *h, int32_t hmm) {
  if (!h || hmm < 0 || hmm >= (int32_t)h->hmms.size()) return nullptr;
  return h->hmms[(size_t)hmm].label.c_str();
}
int32_t aasr_topo_hmm_num_states(const aasr_topo *h, int32_t hmm) {
  if (!h || hmm < 0 || hmm >= (int32_t)h->hmms.size()) return -1;
  return (int32_t)h->hmms[(size_t)hmm].states.size();
}
aasr_status aasr_topo_hmm_states(const aasr_topo *h, int32_t hmm, int32_t *states) {
  return guarded([&] {
    if (!h || !states || hmm < 0 || hmm >= (int32_t)h->hmms.size())
      raise(AASR_ERR_INVALID, "aasr_topo_hmm_states: bad argument");
    for (size_t s = 0; s < h->hmms[(size_t)hmm].states.size(); s++) states[s] = h->hmms[(size_t)hmm].states[s];
  });
}
int32_t aasr_topo_num_states(const aasr_topo *h) { return h ? (int32_t)h->state_info.size() : -1; }
int32_t aasr_topo_state_num_transitions(const aasr_topo *h, int32_t state) {
  if (!h || state < 0 || state >= (int32_t)h->state_info.size()) return -1;
  return (int32_t)h->state_info[(size_t)state].size();
}
aasr_status aasr_topo_state_transitions(const aasr_topo *h, int32_t state, int32_t *target_offset, double *prob) {
  return guarded([&] {
    if (!h || state < 0 || state >= (int32_t)h->state_info.size())
      raise(AASR_ERR_INVALID, "aasr_topo_state_transitions: bad argument");
    const auto &v = h->state_info[(size_t)state];
    for (size_t k = 0; k < v.size(); k++) {
      if (target_offset) target_offset[k] = v[k].target_offset;
      if (prob) prob[k] = v[k].prob;
    }
  });
}
int32_t aasr_topo_max_offset(const aasr_topo *h) { return h ? h->max_off : -1; }

aasr_status aasr_topo_validate(const aasr_topo *h, const aasr_gmm *gmm) {
  if (!h || !gmm) return fail(AASR_ERR_INVALID, "aasr_topo_validate: null argument");
  return aasr_topo_check_states(h, aasr_gmm_num_states(gmm));
}

aasr_status aasr_topo_check_states(const aasr_topo *h, int32_t S) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_topo_check_states: null argument");
    for (const auto &m : h->hmms) {
      for (int s : m.states)
        if (s >= S)
          raise(AASR_ERR_INVALID, "HMM %s: state %d is not below the model's %d states", m.label.c_str(), s, S);
      for (int s : m.states)
        for (const PhTransition &tr : h->state_info[(size_t)s]) {
          if (tr.target_offset > 255)
            raise(AASR_ERR_INVALID, "HMM %s: transition offset %d exceeds 255", m.label.c_str(), tr.target_offset);
          if (tr.target_offset < 0)
            raise(AASR_ERR_INVALID, "HMM %s: negative transition offset %d", m.label.c_str(), tr.target_offset);
        }
    }
  });
}

void aasr_align_default_options(aasr_align_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->swins = 1000;
  o->beam = 100.0;
  o->sbeam = 100;
  o->maxbeam = 1600.0;
  o->overlap = 0.4f;
}

}  // extern "C"

namespace aasr {

// the fields of a .phn line (phn_line.h)
static std::vector<std::string> phn_fields(const std::string &text, size_t max_fields) {
  std::vector<std::string> out;
  size_t at = 0;
  while (at < text.size()) {
    if (out.size() + 1 == max_fields) {
      out.emplace_back(text, at);
      break;
    }
    const size_t stop = std::min(text.find_first_of(" \t", at), text.size());
    out.emplace_back(text, at, stop - at);
    at = stop + 1;
    if (at < text.size()) at = std::min(text.find_first_not_of(" \t", at), text.size());
  }
  return out;
}

// the next non-empty line of f without its newline; false at the end of the file
static bool phn_next_text(FILE *f, std::string *text) {
  for (;;) {
    if (!aku::str::read_line(text, f)) return false;
    if (!text->empty() && text->back() == '\n') text->pop_back();
    if (!text->empty()) return true;
  }
}

// One transcript entry; false at the end of the file or at a timed line that starts at or after
// last_frame (> 0).  Times are clipped to [first_frame, last_frame] as PhnReader::set_frame_limits
// leaves them.
bool next_phn_line(FILE *f, float samples_per_frame, int first_frame, int last_frame, int *line_no, PhnLine *phn,
                   int flags) {
  std::string text;
  if (!phn_next_text(f, &text)) {
    if (ferror(f)) raise(AASR_ERR_IO, "transcript: read error on line %d", *line_no);
    return false;
  }
  PhnLine e;
  std::string head;
  if (isdigit((unsigned char)text[0])) {
    const std::vector<std::string> fl = phn_fields(text, 4);
    bool ok = fl.size() >= 3, ok_end = true;
    if (ok) {
      const long s0 = aku::str::str2long(&fl[0], &ok), s1 = aku::str::str2long(&fl[1], &ok_end);
      e.start = (int)(s0 / samples_per_frame);
      e.end = (int)(s1 / samples_per_frame);
      ok = ok && ok_end;
      head = fl[2];
      const size_t dot = head.find('.');
      if (dot != std::string::npos) {
        e.state = atoi(head.c_str() + dot + 1);
        head = head.substr(0, dot) + (dot + 2 < head.size() ? head.substr(dot + 2) : std::string());
      }
      if (fl.size() == 4) e.comment = fl[3];
    }
    if (!ok || e.start > e.end)
      raise(AASR_ERR_INVALID, "transcript: invalid start or end time on line %d:\n%s\n", *line_no, text.c_str());
  } else {
    const std::vector<std::string> fl = phn_fields(text, 2);
    head = fl[0];
    if (fl.size() == 2) e.comment = fl[1];
  }
  if ((flags & PHN_RELATIVE_SAMPLES) && e.start >= 0) {  // PhnReader.cc:360-364
    e.start += first_frame;
    e.end += first_frame;
  }
  if (last_frame > 0 && e.start >= last_frame) return false;
  if (last_frame > 0 && e.end >= last_frame) e.end = last_frame;
  if (first_frame > 0 && e.start >= 0 && e.start < first_frame) e.start = first_frame;
  if (flags & PHN_STATE_NUM_LABELS) e.state = atoi(head.c_str());  // :383-386, a state number instead of a label
  else e.label = head.substr(0, std::min(head.find(','), head.size()));
  *phn = e;
  (*line_no)++;
  return true;
}

void phn_skip_to_first_frame(FILE *f, float samples_per_frame, int first_frame, int last_frame, int *line_no, int flags) {
  if (flags & PHN_RELATIVE_SAMPLES) return;  // PhnReader.cc:108
  PhnLine phn;
  long curpos = ftell(f), oldpos = curpos;
  while (next_phn_line(f, samples_per_frame, first_frame, last_frame, line_no, &phn, flags)) {
    oldpos = curpos;
    curpos = ftell(f);
    if (phn.end < 0 || phn.end > first_frame) {
      fseek(f, oldpos, SEEK_SET);
      (*line_no)--;
      return;
    }
  }
}

struct Transcript {
  std::vector<int32_t> line_hmms;      // HMM per line, -1: the line adds none
  std::vector<std::string> comments;   // per line
};

static Transcript read_transcript(const aasr_topo *topo, const char *path, float frame_rate, int first_frame,
                                  int last_frame) {
  FILE *f = fopen(path, "r");
  if (!f) raise(AASR_ERR_IO, "could not open transcript %s", path);
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
  const float spf = 16000 / frame_rate;
  int line_no = 0;
  PhnLine phn;
  if (first_frame > 0 || last_frame > 0) phn_skip_to_first_frame(f, spf, first_frame, last_frame, &line_no);
  Transcript t;
  while (next_phn_line(f, spf, first_frame, last_frame, &line_no, &phn)) {
    if (phn.state == -1 || phn.state == 0) {
      const int h = aasr_topo_hmm_index(topo, phn.label.c_str());
      if (h < 0) raise(AASR_ERR_INVALID, "unknown HMM '%s' in transcript %s", phn.label.c_str(), path);
      t.line_hmms.push_back(h);
    } else {
      t.line_hmms.push_back(-1);
    }
    t.comments.push_back(phn.comment);
  }
  return t;
}

}  // namespace aasr

extern "C" aasr_status aasr_align_read_transcript(const aasr_topo *topo, const char *path, float frame_rate,
                                                  int32_t first_frame, int32_t last_frame, int32_t **line_hmms,
                                                  int32_t *n_lines) {
  return guarded([&] {
    if (!topo || !path || !line_hmms || !n_lines) raise(AASR_ERR_INVALID, "aasr_align_read_transcript: null argument");
    Transcript t = read_transcript(topo, path, frame_rate, first_frame, last_frame);
    *line_hmms = (int32_t *)malloc(std::max<size_t>(1, t.line_hmms.size()) * sizeof(int32_t));
    if (!*line_hmms) raise(AASR_ERR_INVALID, "out of memory");
    std::copy(t.line_hmms.begin(), t.line_hmms.end(), *line_hmms);
    *n_lines = (int32_t)t.line_hmms.size();
  });
}

extern "C" int32_t aasr_align_format_line(float frame_rate, int32_t start, int32_t end, const char *label,
                                          const char *comment, char *buf, int32_t cap) {
  if (!buf || cap <= 0) return -1;
  buf[0] = 0;
  if (start < 0) return 0;
  const int frame_mult = (int)(16000 / frame_rate);  // .phn files assume 16 kHz samples
  const int n = snprintf(buf, (size_t)cap, "%d %d %s %s\n", start * frame_mult, end * frame_mult, label ? label : "",
                         comment ? comment : "");
  return n < cap ? n : -1;
}

// ---- batched search --------------------------------------------------------------------------

struct aasr_align_batch {
  const aasr_topo *topo = nullptr;
  aasr_align_options opt{};
  int32_t n = 0, width = 0, target = 0;
  std::vector<AlignUttDev> utt;
  std::vector<AlignRun> run;
  std::vector<int32_t> out;  // host copy after a sync
  DevBuf<int32_t> d_tr_state, d_lines, d_in_begin, d_in_delta, d_out, d_meta, d_path;
  DevBuf<float> d_in_logp, d_cells;
  DevBuf<uint8_t> d_back;
  DevBuf<AlignUttDev> d_utt;
  DevBuf<AlignRun> d_run;
  int64_t bytes = 0;
};

namespace aasr {

// the widest range a frame can hold: the state beam on both sides of the best position plus the
// largest forward offset, for the largest state beam the retries can reach, capped by the window
static int align_width(const aasr_align_options &o, int max_off) {
  double beam = o.beam;
  int64_t sbeam = o.sbeam;
  for (int k = 0; k < 30 && beam * 2 <= o.maxbeam; k++) {
    beam *= 2;
    sbeam *= 2;
  }
  const int64_t w = std::min<int64_t>(o.swins, 2 * sbeam + 1 + max_off);
  return (int)std::max<int64_t>(1, w);
}

}  // namespace aasr

extern "C" {

aasr_status aasr_align_batch_create(const aasr_topo *topo, const aasr_align_options *opt, int32_t n_utt,
                                    const int32_t *line_off, const int32_t *line_hmms, const int32_t *start_frame,
                                    const int32_t *end_frame, const int32_t *eof_frame, aasr_align_batch **out) {
  return guarded([&] {
    if (!topo || !opt || n_utt < 0 || !out || (n_utt > 0 && (!line_off || !start_frame || !end_frame || !eof_frame)))
      raise(AASR_ERR_INVALID, "aasr_align_batch_create: null argument");
    *out = nullptr;
    if (opt->swins < 1) raise(AASR_ERR_INVALID, "aasr_align_batch_create: swins must be positive");
    // a beam that doubling cannot raise past maxbeam would retry without end
    if (!(opt->beam > 0) || !std::isfinite(opt->beam) || !std::isfinite(opt->maxbeam) || opt->sbeam < 0)
      raise(AASR_ERR_INVALID, "aasr_align_batch_create: beam must be positive and finite, maxbeam finite, sbeam >= 0");
    // a window commits its first `target` frames and moves to path[target]: the path has swins entries, so the
    // target must stay below swins (overlap > 0) and leave a frame to commit (overlap < 1)
    if (!std::isfinite(opt->overlap))
      raise(AASR_ERR_INVALID, "aasr_align_batch_create: overlap must be finite");
    const float kept = 1 - opt->overlap;
    const float commit = opt->swins * kept;  // compared as a float: a wild overlap does not fit an int
    if (!(commit >= 1)) raise(AASR_ERR_INVALID, "aasr_align_batch_create: overlap leaves no frame to commit");
    if ((double)commit >= (double)opt->swins)
      raise(AASR_ERR_INVALID, "aasr_align_batch_create: overlap must be positive (a window of %d frames would commit all)",
            opt->swins);
    const int target = (int)commit;
    if (topo->max_off > 255) raise(AASR_ERR_INVALID, "aasr_align_batch_create: transition offset over 255");
    require_device();
    std::unique_ptr<aasr_align_batch> b(new aasr_align_batch());
    b->topo = topo;
    b->opt = *opt;
    b->n = n_utt;
    b->width = align_width(*opt, topo->max_off);
    if (b->width > 5000)  // LDS: two frames of cells and the new frame's likelihoods
      raise(AASR_ERR_INVALID, "aasr_align_batch_create: lattice width %d (swins / sbeam) exceeds 5000", b->width);
    b->target = target;
    // transcriptions: per position the HMM state
    std::vector<int32_t> tr_state, lines;
    b->utt.resize((size_t)n_utt);
    int64_t out_total = 0;
    for (int u = 0; u < n_utt; u++) {
      AlignUttDev &d = b->utt[(size_t)u];
      d.pos_begin = (int64_t)tr_state.size();
      d.line_begin = (int64_t)lines.size();
      for (int32_t l = line_off[u]; l < line_off[u + 1]; l++) {
        const int h = line_hmms[l];
        if (h >= (int)topo->hmms.size()) raise(AASR_ERR_INVALID, "aasr_align_batch_create: HMM index %d out of range", h);
        if (h < 0) {
          lines.push_back(0);
          continue;
        }
        const auto &states = topo->hmms[(size_t)h].states;
        lines.push_back((int32_t)states.size());
        tr_state.insert(tr_state.end(), states.begin(), states.end());
      }
      d.n_pos = (int32_t)(tr_state.size() - d.pos_begin);
      d.n_lines = (int32_t)(lines.size() - d.line_begin);
      d.start_frame = start_frame[u];
      d.end_frame = end_frame[u];
      d.eof_frame = eof_frame[u];
      d.row0 = 0;
      int stop = d.eof_frame;
      if (d.end_frame > 0) stop = std::min(stop, d.end_frame);
      d.n_out = std::max(0, stop - d.start_frame);
      d.out_begin = out_total;
      out_total += d.n_out;
      d.cells_begin = (int64_t)u * opt->swins * b->width;
      d.meta_begin = (int64_t)u * opt->swins;
    }
    // per transcription position its incoming transitions: sources in ascending position, each
    // source's transitions in .ph order (the order in which the reference pushes them)
    std::vector<std::vector<std::pair<int32_t, float>>> incoming(tr_state.size());
    for (int u = 0; u < n_utt; u++) {
      const AlignUttDev &d = b->utt[(size_t)u];
      for (int q = 0; q < d.n_pos; q++)
        for (const PhTransition &tr : topo->state_info[(size_t)tr_state[(size_t)(d.pos_begin + q)]]) {
          const int p = q + tr.target_offset;
          if (p < d.n_pos)
            incoming[(size_t)(d.pos_begin + p)].push_back(
                {tr.target_offset, (float)(tr.prob < 1e-50 ? std::log(1e-50) : std::log(tr.prob))});
        }
    }
    std::vector<int32_t> in_begin(1, 0), in_delta;
    std::vector<float> in_logp;
    for (const auto &v : incoming) {
      for (const auto &e : v) {
        in_delta.push_back(e.first);
        in_logp.push_back(e.second);
      }
      in_begin.push_back((int32_t)in_delta.size());
    }
    if (tr_state.empty()) tr_state.push_back(0);
    if (lines.empty()) lines.push_back(0);
    if (in_delta.empty()) {
      in_delta.push_back(0);
      in_logp.push_back(0.f);
    }
    b->d_tr_state.upload(tr_state.data(), tr_state.size());
    b->d_lines.upload(lines.data(), lines.size());
    b->d_in_begin.upload(in_begin.data(), in_begin.size());
    b->d_in_delta.upload(in_delta.data(), in_delta.size());
    b->d_in_logp.upload(in_logp.data(), in_logp.size());
    const size_t nu = (size_t)std::max(1, n_utt);
    const size_t cells = nu * (size_t)opt->swins * (size_t)b->width;
    b->d_cells.alloc(cells);
    b->d_back.alloc(cells);
    b->d_meta.alloc(nu * (size_t)opt->swins * 3);
    b->d_path.alloc(nu * (size_t)opt->swins);
    b->d_out.alloc((size_t)std::max<int64_t>(1, out_total));
    b->out.assign((size_t)std::max<int64_t>(1, out_total), -1);
    b->run.assign((size_t)n_utt, AlignRun());
    for (auto &r : b->run) {
      memset(&r, 0, sizeof r);
      r.status = ALIGN_ACTIVE;
      r.fresh = 1;
      r.beam = opt->beam;
      r.sbeam = opt->sbeam;
    }
    b->d_run.alloc(nu);
    if (n_utt) AASR_HIP(hipMemcpy(b->d_run.p, b->run.data(), b->run.size() * sizeof(AlignRun), hipMemcpyHostToDevice));
    b->d_utt.alloc(nu);
    b->bytes = (int64_t)(cells * 5 + nu * opt->swins * 16 + tr_state.size() * 4 + lines.size() * 4 +
                         std::max<int64_t>(1, out_total) * 4 + nu * (sizeof(AlignRun) + sizeof(AlignUttDev)));
    *out = b.release();
  });
}

void aasr_align_batch_destroy(aasr_align_batch *b) { delete b; }

int32_t aasr_align_batch_rows(const aasr_align_batch *b, int32_t u) {
  if (!b || u < 0 || u >= b->n) return -1;
  return std::max(1, b->utt[(size_t)u].n_out);
}

int64_t aasr_align_batch_device_bytes(const aasr_align_batch *b) { return b ? b->bytes : -1; }

aasr_status aasr_align_batch_dev(const aasr_gmm *gmm, aasr_align_batch *b, const void *d_state_loglik, int64_t pitch,
                                 int32_t f64, const int64_t *row0, int32_t windows, void *stream) {
  return guarded([&] {
    if (!gmm || !b || (b->n > 0 && (!d_state_loglik || !row0)) || windows < 1)
      raise(AASR_ERR_INVALID, "aasr_align_batch_dev: bad argument");
    if (pitch < aasr_gmm_num_states(gmm)) raise(AASR_ERR_INVALID, "aasr_align_batch_dev: pitch below the state count");
    const aasr_status st = aasr_topo_validate(b->topo, gmm);
    if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    if (b->n == 0) return;
    for (int u = 0; u < b->n; u++) b->utt[(size_t)u].row0 = row0[u];
    AASR_HIP(hipMemcpyAsync(b->d_utt.p, b->utt.data(), b->utt.size() * sizeof(AlignUttDev), hipMemcpyHostToDevice,
                            (hipStream_t)stream));
    AlignParams p{};
    p.tr_state = b->d_tr_state.p;
    p.line_states = b->d_lines.p;
    p.in_begin = b->d_in_begin.p;
    p.in_delta = b->d_in_delta.p;
    p.in_logp = b->d_in_logp.p;
    p.scores = d_state_loglik;
    p.pitch = pitch;
    p.f64 = f64 ? 1 : 0;
    p.swins = b->opt.swins;
    p.width = b->width;
    p.max_off = b->topo->max_off;
    p.target = b->target;
    p.force_end = b->opt.no_force_end ? 0 : 1;
    p.maxbeam = b->opt.maxbeam;
    p.utt = b->d_utt.p;
    p.run = b->d_run.p;
    p.cells = b->d_cells.p;
    p.back = b->d_back.p;
    p.meta = b->d_meta.p;
    p.path = b->d_path.p;
    p.out = b->d_out.p;
    align_launch(p, b->n, windows, (hipStream_t)stream);
  });
}

aasr_status aasr_align_batch_sync(aasr_align_batch *b, void *stream, int32_t *n_active) {
  return guarded([&] {
    if (!b) raise(AASR_ERR_INVALID, "aasr_align_batch_sync: null argument");
    if (b->n > 0) {
      AASR_HIP(hipMemcpyAsync(b->run.data(), b->d_run.p, b->run.size() * sizeof(AlignRun), hipMemcpyDeviceToHost,
                              (hipStream_t)stream));
      AASR_HIP(hipMemcpyAsync(b->out.data(), b->d_out.p, b->out.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                              (hipStream_t)stream));
      AASR_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    int active = 0;
    for (const AlignRun &r : b->run) active += r.status == ALIGN_ACTIVE;
    if (n_active) *n_active = active;
  });
}

aasr_status aasr_align_batch_result(const aasr_align_batch *b, int32_t u, int32_t *positions, int32_t *n_committed,
                                    double *loglik, int32_t *status, int32_t *n_fail) {
  return guarded([&] {
    if (!b || u < 0 || u >= b->n) raise(AASR_ERR_INVALID, "aasr_align_batch_result: bad argument");
    const AlignRun &r = b->run[(size_t)u];
    const AlignUttDev &d = b->utt[(size_t)u];
    if (positions)
      for (int f = 0; f < r.committed; f++) positions[f] = b->out[(size_t)(d.out_begin + f)];
    if (n_committed) *n_committed = r.committed;
    if (loglik) *loglik = r.acc + r.fin;
    if (status) *status = r.status;
    if (n_fail) *n_fail = r.n_fail;
    if (r.status == ALIGN_ERROR && status == nullptr)
      raise(AASR_ERR_INVALID, "aasr_align_batch_result: utterance %d: search error %d", u, r.error);
  });
}

}  // extern "C"

// ---- the align main loop over a recipe ---------------------------------------------------------

namespace aasr {

// what align adds to a recipe line
struct AlignUtt {
  RecipeInfo info;
  int start_frame = 0, end_frame = 0, eof_frame = 0, rows = 0;
  Transcript tr;
};

// the printing half of align.cc:viterbi_align over the committed positions of one utterance
static void write_alignment(const aasr_topo *topo, const AlignUtt &u, float frame_rate, bool print_all_states,
                            const int32_t *positions, int n_committed, bool finished) {
  std::vector<std::string> label, comment;
  std::vector<char> printed;
  for (size_t l = 0; l < u.tr.line_hmms.size(); l++) {
    const int h = u.tr.line_hmms[l];
    if (h < 0) continue;
    const auto &hmm = topo->hmms[(size_t)h];
    for (size_t s = 0; s < hmm.states.size(); s++) {
      std::string sl = hmm.label;
      if (print_all_states) sl += "." + std::to_string(s);
      if (s == 0) {
        label.push_back(sl);
        comment.push_back(u.tr.comments[l]);
        printed.push_back(0);
      } else {
        label.push_back(print_all_states ? sl : std::string());
        comment.push_back(std::string());
        printed.push_back(print_all_states ? 0 : 1);
      }
    }
  }
  FILE *f = fopen(u.info.alignment_path.c_str(), "w");
  if (!f) raise(AASR_ERR_IO, "could not open %s for writing", u.info.alignment_path.c_str());
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
  char line[4096];
  std::string out;
  int print_start = -1;
  std::string print_label, print_comment;
  auto emit = [&](int start, int end) {
    const int n = aasr_align_format_line(frame_rate, start, end, print_label.c_str(), print_comment.c_str(), line,
                                         (int32_t)sizeof line);
    if (n > 0) out.append(line, (size_t)n);
    else if (n < 0) {
      const int frame_mult = (int)(16000 / frame_rate);
      out += std::to_string(start * frame_mult) + " " + std::to_string(end * frame_mult) + " " + print_label + " " +
             print_comment + "\n";
    }
  };
  for (int fr = 0; fr < n_committed; fr++) {
    const int p = positions[fr];
    if (p < 0 || p >= (int)printed.size()) raise(AASR_ERR_INVALID, "align: position %d out of the transcription", p);
    if (!printed[(size_t)p]) {
      emit(print_start, fr + u.start_frame);
      print_start = fr + u.start_frame;
      print_label = label[(size_t)p];
      print_comment = comment[(size_t)p];
      printed[(size_t)p] = 1;
    }
  }
  if (finished) emit(print_start, u.start_frame + n_committed + 1);
  if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size())
    raise(AASR_ERR_IO, "write error on %s", u.info.alignment_path.c_str());
}

}  // namespace aasr

extern "C" aasr_status aasr_run_align_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                             const char *recipe_path, const aasr_align_options *opt,
                                             aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt) raise(AASR_ERR_INVALID, "aasr_run_align_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    require_device();
    {
      const aasr_status st = aasr_topo_validate(topo, gmm);
      if (st != AASR_OK) raise(st, "%s", last_error().c_str());
    }
    check_feature_dim(gmm, feat);
    // align reads its recipe with cluster_speakers = true (aku/align.cc:237-239)
    std::vector<AlignUtt> utts;
    for (RecipeInfo &info : read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, true)) {
      utts.emplace_back();
      utts.back().info = std::move(info);
    }
    const float fr = aasr_feat_frame_rate(feat);
    const int S = aasr_gmm_num_states(gmm), D = aasr_gmm_dim(gmm);
    const bool f64 = aasr_gmm_get_precision(gmm) == AASR_PREC_F64;
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    hipStream_t stream;
    AASR_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    std::unique_ptr<void, void (*)(void *)> sguard((void *)stream, [](void *s) { (void)hipStreamDestroy((hipStream_t)s); });
    DevBuf<uint8_t> d_scores, d_frames;
    const double orig_beam = opt->beam;
    const int orig_sbeam = opt->sbeam;
    double curr_beam = orig_beam;
    int curr_sbeam = orig_sbeam;
    double sum_data_likelihood = 0.0, prec_buff = 0.0;
    int64_t frames_total = 0;
    // groups of utterances searched together; the score rows of a group stay on the device
    const int64_t max_group_rows_x_states = (int64_t)1 << 28;
    size_t next = 0;
    while (next < utts.size()) {
      // features and scores, utterance by utterance (the speaker configuration changes the model)
      std::vector<size_t> group;
      std::vector<int64_t> row0;
      int64_t rows_total = 0;
      std::vector<double> feats;
      std::vector<float> feats32;
      while (next < utts.size() && group.size() < 256) {
        AlignUtt &u = utts[next];
        const RecipeInfo &info = u.info;
        if (info.start_line > 0 || info.end_line > 0)  // (here, not up front: the groups before this line are written)
          raise(AASR_ERR_UNSUPPORTED, "align: recipe line limits (start-line / end-line) are not supported");
        apply_speaker(opt->speakers, info);
        int16_t *pcm = nullptr;
        int64_t n_samples = 0;
        int32_t rate = 0;
        if (aasr_audio_read(feat, info.audio_path.c_str(), &pcm, &n_samples, &rate) != AASR_OK)
          raise(AASR_ERR_IO, "%s", aasr_last_error());
        std::unique_ptr<int16_t, void (*)(int16_t *)> pguard(pcm, [](int16_t *p) { aasr_free(p); });
        u.eof_frame = aasr_feat_eof_frame(feat, n_samples);
        int first, last;
        frame_range(info, fr, &first, &last);
        u.start_frame = first;
        u.end_frame = (int)(info.end_time * fr);
        u.tr = read_transcript(topo, info.transcript_path.c_str(), fr, first, last);
        int stop = u.eof_frame;
        if (u.end_frame > 0) stop = std::min(stop, u.end_frame);
        u.rows = std::max(1, stop - u.start_frame);
        if (!group.empty() && (rows_total + u.rows) * (int64_t)S > max_group_rows_x_states) break;
        feats.resize((size_t)u.rows * D);
        if (aasr_feat_run_f64(feat, pcm, n_samples, u.start_frame, u.rows, nullptr, feats.data()) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        // the scores go to a buffer that grows with the group; keep what is there
        const size_t need = (size_t)(rows_total + u.rows) * S * esz;
        if (need > d_scores.n) {
          DevBuf<uint8_t> bigger;
          bigger.alloc(std::max(need, d_scores.n * 2));
          if (rows_total)
            AASR_HIP(hipMemcpyAsync(bigger.p, d_scores.p, (size_t)rows_total * S * esz, hipMemcpyDeviceToDevice, stream));
          AASR_HIP(hipStreamSynchronize(stream));
          d_scores = std::move(bigger);
        }
        d_frames.ensure((size_t)u.rows * D * esz);
        if (f64) {
          AASR_HIP(hipMemcpyAsync(d_frames.p, feats.data(), feats.size() * sizeof(double), hipMemcpyHostToDevice, stream));
          if (aasr_gmm_score_f64_dev(gmm, (const double *)d_frames.p, u.rows,
                                     (double *)(d_scores.p + (size_t)rows_total * S * esz), stream) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        } else {
          feats32.assign(feats.begin(), feats.end());
          AASR_HIP(hipMemcpyAsync(d_frames.p, feats32.data(), feats32.size() * sizeof(float), hipMemcpyHostToDevice, stream));
          if (aasr_gmm_score_dev(gmm, (const float *)d_frames.p, u.rows,
                                 (float *)(d_scores.p + (size_t)rows_total * S * esz), stream) != AASR_OK)
            raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        }
        AASR_HIP(hipStreamSynchronize(stream));  // the host buffers are reused for the next utterance
        group.push_back(next);
        row0.push_back(rows_total);
        rows_total += u.rows;
        next++;
      }
      // the search, all utterances of the group at once
      std::vector<int32_t> line_off(1, 0), line_hmms, sf, ef, of;
      for (size_t g : group) {
        const AlignUtt &u = utts[g];
        line_hmms.insert(line_hmms.end(), u.tr.line_hmms.begin(), u.tr.line_hmms.end());
        line_off.push_back((int32_t)line_hmms.size());
        sf.push_back(u.start_frame);
        ef.push_back(u.end_frame);
        of.push_back(u.eof_frame);
      }
      aasr_align_batch *b = nullptr;
      if (aasr_align_batch_create(topo, opt, (int32_t)group.size(), line_off.data(), line_hmms.data(), sf.data(),
                                  ef.data(), of.data(), &b) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      std::unique_ptr<aasr_align_batch, void (*)(aasr_align_batch *)> bguard(b, aasr_align_batch_destroy);
      int32_t active = (int32_t)group.size();
      while (active > 0) {
        if (aasr_align_batch_dev(gmm, b, d_scores.p, S, f64 ? 1 : 0, row0.data(), 1 << 20, stream) != AASR_OK ||
            aasr_align_batch_sync(b, stream, &active) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      }
      // files and diagnostics in recipe order (align.cc:249-327)
      std::vector<int32_t> positions;
      for (size_t k = 0; k < group.size(); k++) {
        const AlignUtt &u = utts[group[k]];
        int32_t n_committed = 0, status = 0, n_fail = 0;
        double ll = 0;
        positions.assign((size_t)std::max(1, u.rows), 0);
        if (aasr_align_batch_result(b, (int32_t)k, positions.data(), &n_committed, &ll, &status, &n_fail) != AASR_OK)
          raise(AASR_ERR_INVALID, "%s", aasr_last_error());
        if (status == ALIGN_ERROR)
          raise(AASR_ERR_INVALID, "align: the search failed on %s (transcription or pruning does not fit the audio)",
                u.info.audio_path.c_str());
        if (curr_beam != orig_beam) {
          std::cerr << "Restoring original beam " << orig_beam << " and original state beam " << orig_sbeam
                    << std::endl;
          curr_beam = orig_beam;
          curr_sbeam = orig_sbeam;
        }
        announce(u.info, opt->info);
        for (int i = 0; i < n_fail; i++) {
          curr_beam *= 2;
          curr_sbeam *= 2;
          std::cerr << "Too low beams, doubling to beam " << curr_beam << " and state beam " << curr_sbeam
                    << std::endl;
          if (curr_beam <= opt->maxbeam)
            announce(u.info, opt->info);
          else
            std::cerr << "Have to stop trying, beam already over max" << std::endl;
        }
        write_alignment(topo, u, fr, !opt->phoseg, positions.data(), n_committed, status == ALIGN_OK);
        if (status == ALIGN_OK) {
          if (opt->info > 1) fprintf(stderr, "File log likelihood: %f\n", ll);
          prec_buff += ll;
          if (fabsl(prec_buff) > 100000) {
            sum_data_likelihood += prec_buff;
            prec_buff = 0;
          }
        }
        sum_data_likelihood += prec_buff;
        if (opt->info > 0) fprintf(stderr, "Total data log likelihood: %f\n", sum_data_likelihood);
        frames_total += n_committed;
      }
    }
    fill_run_stats(stats, (int64_t)utts.size(), frames_total, t0, 0);
  });
}

// estimate.cc -- model re-estimation from statistics dumps (aku/estimate.cc --ml over diagonal pools): the
// estimation handle that reads a model's files and adds the .gks / .mcs / .phs dumps of stats
// (HmmSet::accumulate_*_from_dump, aku/HmmSet.cc:655-765), the ML update (Gaussian / Mixture::estimate_parameters,
// HmmSet::estimate_transition_parameters), the pool edits (delete_gaussians, remove_mixture_components,
// split_gaussians, aku/HmmSet.cc:1058-1350), the writers, the MLLT handle that drives the device passes of
// HmmSet::estimate_mllt (mllt.hip) with its host row solver, and the tool's main (aasr_run_estimate).
// Everything but the MLLT handle is host only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "aku/str.hh"
#include "common.h"
#include "feat.h"
#include "gmm.h"
#include "mllt.h"
#include "ph_parse.h"
#include "pipeline.h"
#include "recipe_pass.h"

using namespace aasr;

namespace {

constexpr int kMlltIter = 7;    // MAX_MLLT_ITER (aku/HmmSet.hh:13)
constexpr int kMlltAIter = 80;  // MAX_MLLT_A_ITER

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// one pool entry: a diagonal Gaussian with its ML accumulator (GaussianAccumulator, aku/Distributions.hh)
struct EstGaussian {
  std::vector<double> mean, var;
  bool has_accum = false;    // start_accumulating has run (the first dump line that names the Gaussian)
  bool accumulated = false;  // a dump carried statistics for it
  int feacount = 0;
  double gamma = 0, aux_gamma = 0;
  std::vector<double> sum_x, sum_xx;  // sum_xx: [dim] or the packed lower triangle, by the handle's mode
};

struct EstMixture {
  std::vector<int> pointers;
  std::vector<double> weights;
  // MixtureAccumulator: sized when the first dump line names the mixture, NOT resized by the pool edits
  bool has_accum = false, accumulated = false;
  std::vector<double> gamma;
  double aux_gamma = 0, mixture_ll = 0;
  void normalize() {
    double sum = 0;
    for (double w : weights) sum += w;
    for (double &w : weights) w /= sum;
  }
  int component_index(int p) const {
    for (size_t i = 0; i < pointers.size(); i++)
      if (pointers[i] == p) return (int)i;
    return -1;
  }
  // Mixture::update_components (aku/Distributions.cc:2447-2463)
  void update_components(const std::vector<int> &cmap) {
    for (int i = 0; i < (int)pointers.size(); i++) {
      if (cmap[(size_t)pointers[(size_t)i]] < 0) {
        pointers.erase(pointers.begin() + i);
        weights.erase(weights.begin() + i);
        i--;
      } else {
        pointers[(size_t)i] = cmap[(size_t)pointers[(size_t)i]];
      }
    }
    normalize();
  }
};

struct EstTransition {
  int source, target;
  double prob;
};

}  // namespace

struct aasr_estimate {
  int dim = 0;
  int mode = 0;  // PDF::StatisticsMode of the first dump (1: diagonal, 3: full second moments), 0: none yet
  double minvar = 0.1, covsmooth = 0;
  std::vector<EstGaussian> pool;
  std::vector<EstMixture> mixtures;
  struct Hmm {
    std::string label;
    std::vector<int> states;
  };
  std::vector<Hmm> hmms;
  int n_states = 0;
  std::vector<std::vector<int>> state_transitions;  // per state: indices into transitions
  std::vector<EstTransition> transitions;
  std::vector<double> trans_accum;  // m_transition_accum's prob; empty before the first .phs
  std::vector<uint8_t> trans_accumulated;
  std::map<std::string, double> sum_statistics;  // the .lls lines, by name
  bool full() const { return (mode & 2) != 0; }
  size_t xx_len() const { return full() ? (size_t)dim * (dim + 1) / 2 : (size_t)dim; }
};

namespace {

// ---- reading the dumps ---------------------------------------------------------------------------

// {Diagonal,Full}StatisticsAccumulator::accumulate_from_dump (aku/Distributions.cc:63-94, 176-206)
void accumulate_gaussian(aasr_estimate *h, EstGaussian &g, std::istream &is) {
  int feacount = 0;
  double gamma = 0, aux_gamma = 0;
  float t = 0;
  is.read((char *)&feacount, sizeof(int));
  is.read((char *)&gamma, sizeof(double));
  is.read((char *)&aux_gamma, sizeof(double));
  if (is.fail()) fprintf(stderr, "Error while reading statistics dump\n");
  if (feacount < 0) raise(AASR_ERR_INVALID, "Invalid statistics dump\n");
  g.feacount += feacount;
  g.gamma += gamma;
  g.aux_gamma += aux_gamma;
  g.accumulated = true;
  for (int i = 0; i < h->dim; i++) {
    is.read((char *)&t, sizeof(float));
    g.sum_x[(size_t)i] += t;
  }
  const size_t n = h->xx_len();
  for (size_t i = 0; i < n; i++) {
    is.read((char *)&t, sizeof(float));
    g.sum_xx[i] += t;
  }
}

void start_gaussian(aasr_estimate *h, EstGaussian &g) {
  g.has_accum = true;
  g.sum_x.assign((size_t)h->dim, 0.0);
  g.sum_xx.assign(h->xx_len(), 0.0);
}

void set_mode(aasr_estimate *h, int mode, const std::string &filename) {
  if (h->mode != 0) return;
  if (mode & ~3)
    raise(AASR_ERR_UNSUPPORTED, "estimate: %s holds discriminative statistics (mode %d); only ML statistics (modes 1 and 3) are supported",
          filename.c_str(), mode);
  h->mode = mode;
}

// HmmSet::accumulate_gk_from_dump (aku/HmmSet.cc:731-765), Gaussian::accumulate_from_dump (Distributions.cc:318-333)
void accumulate_gk(aasr_estimate *h, const std::string &filename) {
  std::ifstream gks(filename.c_str(), std::ifstream::binary);
  if (!gks) raise(AASR_ERR_IO, "HmmSet::accumulate_gk_from_dump(): could not open %s", filename.c_str());
  int num_pdfs = 0, dim = 0, pdf = 0, mode = 0;
  gks.read((char *)&num_pdfs, sizeof(int));
  gks.read((char *)&dim, sizeof(int));
  if (num_pdfs != (int)h->pool.size())
    raise(AASR_ERR_INVALID, "HmmSet::accumulate_gk_from_dump: the number of mixture base distributions in: %s is wrong\n",
          filename.c_str());
  if (dim != h->dim)
    raise(AASR_ERR_INVALID, "HmmSet::accumulate_gk_from_dump: the dimensionality of mixture base distributions in: %s is wrong\n",
          filename.c_str());
  gks.read((char *)&mode, sizeof(int));
  set_mode(h, mode, filename);
  while (gks.good()) {
    gks.read((char *)&pdf, sizeof(int));
    if (gks.eof()) break;
    if (pdf < 0 || pdf >= num_pdfs) raise(AASR_ERR_INVALID, "Invalid statistics dump (wrong pdf index)");
    EstGaussian &g = h->pool[(size_t)pdf];
    int accum_pos = -1;
    gks.read((char *)&accum_pos, sizeof(int));
    if (!g.has_accum) start_gaussian(h, g);
    while (accum_pos >= 0) {
      if (accum_pos != 0) raise(AASR_ERR_INVALID, "Gaussian::accumulate_from_dump:Invalid accumulator position %i", accum_pos);
      accumulate_gaussian(h, g, gks);
      accum_pos = -1;  // (a truncated file ends the Gaussian instead of repeating the last word)
      gks.read((char *)&accum_pos, sizeof(int));
    }
  }
}

// HmmSet::accumulate_mc_from_dump (aku/HmmSet.cc:701-728), Mixture::accumulate_from_dump (Distributions.cc:2211-2245)
void accumulate_mc(aasr_estimate *h, const std::string &filename) {
  std::ifstream mcs(filename.c_str());
  if (!mcs) raise(AASR_ERR_IO, "HmmSet::accumulate_mc_from_dump(): could not open %s", filename.c_str());
  int n = 0, pdf = 0, mode = 0;
  mcs >> n;
  if (n != (int)h->mixtures.size())
    raise(AASR_ERR_INVALID, "HmmSet::accumulate_mc_from_dump: the number of PDFs in: %s is wrong\n", filename.c_str());
  mcs >> mode;
  set_mode(h, mode, filename);
  while (mcs >> pdf) {
    // (the reference indexes with what it read and asserts the sizes)
    if (pdf < 0 || pdf >= n) raise(AASR_ERR_INVALID, "Invalid statistics dump (wrong pdf index)");
    EstMixture &m = h->mixtures[(size_t)pdf];
    int accum_pos = -1;
    mcs >> accum_pos;
    if (!m.has_accum) {
      m.has_accum = true;
      m.gamma.assign(m.pointers.size(), 0.0);
    }
    while (accum_pos >= 0) {
      if (accum_pos != 0) raise(AASR_ERR_INVALID, "Mixture::accumulate_from_dump: Invalid accumulator position %i", accum_pos);
      int pointer = 0, sz = 0;
      double acc = 0;
      mcs >> sz;
      if (sz != (int)m.pointers.size() || sz != (int)m.gamma.size())
        raise(AASR_ERR_INVALID, "Mixture::accumulate_from_dump: mixture %d has %d components in %s, the model %d", pdf, sz,
              filename.c_str(), (int)m.pointers.size());
      for (int i = 0; i < sz; i++) {
        mcs >> pointer >> acc;
        if (pointer != m.pointers[(size_t)i])
          raise(AASR_ERR_INVALID, "Mixture::accumulate_from_dump: component %d of mixture %d is Gaussian %d in %s, the model's is %d", i,
                pdf, pointer, filename.c_str(), m.pointers[(size_t)i]);
        m.gamma[(size_t)i] += acc;
      }
      double aux = 0, ll = 0;
      mcs >> aux >> ll;
      m.aux_gamma += aux;
      m.mixture_ll += ll;
      m.accumulated = true;
      accum_pos = -1;
      mcs >> accum_pos;
    }
  }
}

// HmmSet::accumulate_ph_from_dump (aku/HmmSet.cc:654-698).  The stream is read as the reference reads it: a dump
// lists only the transitions that were accumulated, and once it has run out the loop goes on to the announced count
// with the values of the last line it read.
void accumulate_ph(aasr_estimate *h, const std::string &filename) {
  std::ifstream phs(filename.c_str());
  if (!phs) {
    fprintf(stderr, "HmmSet::accumulate_ph_from_dump(): could not open %s\n", filename.c_str());
    return;
  }
  if (h->trans_accum.empty()) {
    h->trans_accum.assign(h->transitions.size(), 0.0);
    h->trans_accumulated.assign(h->transitions.size(), 0);
  }
  unsigned int num_transitions = 0;
  phs >> num_transitions;
  if (h->trans_accum.size() != num_transitions)
    raise(AASR_ERR_INVALID,
          "HmmSet::accumulate_ph_from_dump: the number of transitions in: %s doesn't match the earlier accumulations\n",
          filename.c_str());
  int source = 0, target = 0, pos;
  double occ = 0;
  for (unsigned int t = 0; t < num_transitions; t++) {
    phs >> source >> target >> occ;
    pos = -1;
    if (phs.eof() && t == 0) break;  // Allow premature EOF here (no transition information)
    for (size_t ts = 0; ts < h->transitions.size(); ts++)
      if (h->transitions[ts].source == source && h->transitions[ts].target == target) {
        pos = (int)ts;
        break;
      }
    if (pos == -1) raise(AASR_ERR_INVALID, "HmmSet::accumulate_ph_from_dump: the transition %i could not be accumulated", (int)t);
    h->trans_accum[(size_t)pos] += occ;
    h->trans_accumulated[(size_t)pos] = 1;
  }
}

// estimate.cc:292-311
void accumulate_lls(aasr_estimate *h, const std::string &filename) {
  std::ifstream lls_file(filename.c_str());
  while (lls_file.good()) {
    char buf[256];
    std::string temp;
    std::vector<std::string> fields;
    lls_file.getline(buf, 256);
    temp.assign(buf);
    aku::str::split(&temp, ":", false, &fields, 2);
    if (fields.size() == 2) {
      const double value = strtod(fields[1].c_str(), NULL);
      if (h->sum_statistics.find(fields[0]) == h->sum_statistics.end()) h->sum_statistics[fields[0]] = value;
      else h->sum_statistics[fields[0]] = h->sum_statistics[fields[0]] + value;
    }
  }
}

// ---- the ML update -------------------------------------------------------------------------------

// Gaussian::estimate_parameters, ML branch (aku/Distributions.cc:502-527, 677-712) for a diagonal Gaussian:
// get_mean_estimate scales by 1 / gamma; the diagonal accumulator divides the second moment by gamma, the full one
// scales it by 1 / gamma before the rank-one update
void estimate_gaussian(aasr_estimate *h, EstGaussian &g) {
  if (!g.accumulated) {
    fprintf(stderr, "Warning: Could not estimate Gaussian parameters due to missing statistics!\n");
    return;
  }
  const int d = h->dim;
  const double inv = 1 / g.gamma;
  std::vector<double> mean((size_t)d), var((size_t)d);
  for (int i = 0; i < d; i++) mean[(size_t)i] = g.sum_x[(size_t)i] * inv;
  for (int i = 0; i < d; i++) {
    if (h->full()) var[(size_t)i] = g.sum_xx[(size_t)i * (i + 1) / 2 + i] * inv - mean[(size_t)i] * mean[(size_t)i];
    else var[(size_t)i] = g.sum_xx[(size_t)i] / g.gamma - mean[(size_t)i] * mean[(size_t)i];
  }
  if (g.feacount > 1)
    for (int i = 0; i < d; i++)
      if (var[(size_t)i] <= 0) fprintf(stderr, "Warning: Variance in dimension %i is %g (%i features)\n", i, var[(size_t)i], g.feacount);
  for (int i = 0; i < d; i++)
    if (var[(size_t)i] < h->minvar) var[(size_t)i] = h->minvar;
  // (covsmooth scales the off-diagonal entries, which a diagonal Gaussian drops)
  g.mean = mean;
  g.var = var;
}

// Mixture::estimate_parameters, ML branch (aku/Distributions.cc:2262-2283)
void estimate_mixture(EstMixture &m) {
  if (!m.accumulated) {
    fprintf(stderr, "Warning: Could not estimate mixture parameters due to missing statistics!\n");
    return;
  }
  double total_gamma = 0;
  for (size_t i = 0; i < m.weights.size(); i++) total_gamma += m.gamma[i];
  for (size_t i = 0; i < m.weights.size(); i++) m.weights[i] = m.gamma[i] / total_gamma;
}

void estimate_mixtures(aasr_estimate *h) {
  // HmmSet::estimate_parameters walks the states; state s emits mixture s
  for (int s = 0; s < h->n_states; s++) {
    if (s >= (int)h->mixtures.size()) raise(AASR_ERR_INVALID, "estimate: state %d has no mixture", s);
    estimate_mixture(h->mixtures[(size_t)s]);
  }
}

// HmmSet::estimate_transition_parameters (aku/HmmSet.cc:781-815): a FLOAT running sum per state, the 0.001 floor,
// the old probabilities for a state without counts
void estimate_transitions(aasr_estimate *h) {
  if (h->trans_accum.empty()) return;  // no .phs was read: nothing to normalise
  for (int s = 0; s < h->n_states; s++) {
    float sum = 0.0;
    const std::vector<int> &st = h->state_transitions[(size_t)s];
    for (int t : st) sum += h->trans_accum[(size_t)t];
    for (int t : st) {
      if (sum > 0.0) {
        double p = h->trans_accum[(size_t)t] / sum;
        if (p < .001) p = .001;
        h->transitions[(size_t)t].prob = p;
      }
    }
  }
}

// ---- the pool edits ------------------------------------------------------------------------------

double gaussian_occupancy(const EstGaussian &g) { return g.accumulated ? g.gamma : -1; }

void delete_marked(aasr_estimate *h, const std::vector<int> &index_map) {
  std::vector<EstGaussian> kept;
  for (size_t i = 0; i < h->pool.size(); i++)
    if (index_map[i] >= 0) kept.push_back(std::move(h->pool[i]));
  h->pool.swap(kept);
}

// HmmSet::delete_gaussians (aku/HmmSet.cc:1057-1142)
int delete_gaussians(aasr_estimate *h, double minocc, std::vector<int> &index_map) {
  const int n = (int)h->pool.size();
  index_map.resize((size_t)n);
  for (int i = 0; i < n; i++) index_map[(size_t)i] = i;
  for (int i = 0; i < n; i++) {
    const double occ = gaussian_occupancy(h->pool[(size_t)i]);
    if (occ < minocc && occ >= 0) {
      for (int j = i + 1; j < n; j++) index_map[(size_t)j]--;
      index_map[(size_t)i] = -1;
    }
  }
  // retain at least one Gaussian for each mixture: the component of the largest weight (the first such)
  for (EstMixture &m : h->mixtures) {
    bool all_deleted = true;
    for (int p : m.pointers)
      if (index_map[(size_t)p] >= 0) {
        all_deleted = false;
        break;
      }
    if (!all_deleted) continue;
    double max_weight = -1;
    int max_index = -1;
    for (size_t i = 0; i < m.pointers.size(); i++)
      if (m.weights[i] > max_weight) {
        max_weight = m.weights[i];
        max_index = m.pointers[i];
      }
    if (max_index < 0) raise(AASR_ERR_INVALID, "estimate: a mixture without components");
    int new_index = 0;
    for (int j = max_index - 1; j >= 0; j--)
      if (index_map[(size_t)j] >= 0) {
        new_index = index_map[(size_t)j] + 1;
        break;
      }
    index_map[(size_t)max_index] = new_index;
    for (int j = max_index + 1; j < n; j++)
      if (index_map[(size_t)j] >= 0) index_map[(size_t)j]++;
  }
  int deleted = 0;
  for (int i = 0; i < n; i++)
    if (index_map[(size_t)i] < 0) deleted++;
  delete_marked(h, index_map);
  for (EstMixture &m : h->mixtures) m.update_components(index_map);
  return deleted;
}

// HmmSet::remove_mixture_components (aku/HmmSet.cc:1145-1210)
int remove_mixture_components(aasr_estimate *h, double min_weight, std::vector<int> &index_map) {
  const int n = (int)h->pool.size();
  std::vector<int> gauss_count((size_t)n, 0);
  for (EstMixture &m : h->mixtures) {
    for (;;) {
      if (m.weights.empty()) raise(AASR_ERR_INVALID, "estimate: --mremove leaves a mixture without components");
      double cur_min_weight = m.weights[0];
      int min_index = 0;
      for (int i = 1; i < (int)m.weights.size(); i++)
        if (m.weights[(size_t)i] < cur_min_weight) {
          cur_min_weight = m.weights[(size_t)i];
          min_index = i;
        }
      if (cur_min_weight > min_weight) break;
      m.pointers.erase(m.pointers.begin() + min_index);
      m.weights.erase(m.weights.begin() + min_index);
      m.normalize();
    }
    for (int p : m.pointers) gauss_count[(size_t)p]++;
  }
  index_map.resize((size_t)n);
  int cur_index = 0;
  for (int i = 0; i < n; i++) index_map[(size_t)i] = gauss_count[(size_t)i] == 0 ? -1 : cur_index++;
  if (cur_index < n) {
    delete_marked(h, index_map);
    for (EstMixture &m : h->mixtures) m.update_components(index_map);
  }
  return n - cur_index;
}

// HmmSet::split_gaussians (aku/HmmSet.cc:1213-1350)
int split_gaussians(aasr_estimate *h, double minocc, int maxg, int numgauss, double splitalpha) {
  int num_splits = 0;
  double mixg_minocc = 0;
  if (minocc < 1.0) minocc = 1.0;
  // PDFPool::get_occ_sorted_gaussians: by falling occupancy; std::sort leaves equal occupancies in any order, here
  // the lower index goes first
  std::vector<int> sorted;
  for (int i = 0; i < (int)h->pool.size(); i++)
    if (h->pool[(size_t)i].accumulated && h->pool[(size_t)i].gamma >= 0) sorted.push_back(i);
  std::stable_sort(sorted.begin(), sorted.end(), [&](int x, int y) { return h->pool[(size_t)x].gamma > h->pool[(size_t)y].gamma; });
  const int P = (int)h->mixtures.size();
  std::vector<double> pdf_occ((size_t)P);
  std::vector<int> occ_limit((size_t)P);
  double sum_occ = 0;
  for (int p = 0; p < P; p++) {
    const EstMixture &m = h->mixtures[(size_t)p];
    // (the reference reads the accumulator of a mixture that never had one)
    if (!m.has_accum) raise(AASR_ERR_INVALID, "estimate: --split needs statistics for every mixture (mixture %d has none)", p);
    double g_occ_sum = 0;
    int gauss_occ_limit = 0;
    for (size_t k = 0; k < m.pointers.size(); k++) {
      const double g_occ = m.gamma[k];  // by position: the accumulator keeps its order through the pool edits
      g_occ_sum += g_occ;
      gauss_occ_limit += (int)floor(g_occ / (minocc / 2.0));
    }
    pdf_occ[(size_t)p] = g_occ_sum;
    occ_limit[(size_t)p] = gauss_occ_limit;
    sum_occ += g_occ_sum;
  }
  if (numgauss > 0) {
    if ((int)h->pool.size() >= numgauss) return 0;
    const double max_rel_error = .001;
    mixg_minocc = 10 * h->dim;
    const double temp = sum_occ / (double)P;
    mixg_minocc = pow(temp, splitalpha) / (temp / mixg_minocc);
    double interval = mixg_minocc;
    bool growing = true;
    for (int i = 0; i < 30; i++) {
      int total_gaussians = 0;
      for (int p = 0; p < P; p++) {
        int num_mix_g = (int)floor(pow(pdf_occ[(size_t)p], splitalpha) / mixg_minocc);
        if (num_mix_g > occ_limit[(size_t)p]) num_mix_g = occ_limit[(size_t)p];
        total_gaussians += std::max(std::min(num_mix_g, maxg), (int)h->mixtures[(size_t)p].pointers.size());
      }
      if (total_gaussians > (1 + max_rel_error) * numgauss) {
        if (growing) {
          mixg_minocc *= 2;
          interval = mixg_minocc / 2.0;
        } else {
          mixg_minocc += interval / 2.0;
        }
      } else if (total_gaussians < numgauss) {
        growing = false;
        mixg_minocc -= interval / 2.0;
      } else {
        break;
      }
      if (!growing) interval /= 2.0;
    }
  }
  for (int gi : sorted) {
    bool split = true;
    std::vector<int> pdf_index;
    for (int p = 0; p < P; p++) {
      const EstMixture &m = h->mixtures[(size_t)p];
      if (m.component_index(gi) >= 0) {
        if ((numgauss > 0 && pow(pdf_occ[(size_t)p], splitalpha) / (m.pointers.size() + 1) < mixg_minocc) ||
            (int)m.pointers.size() >= maxg || h->pool[(size_t)gi].gamma < minocc) {
          split = false;
          break;
        }
        pdf_index.push_back(p);
      }
    }
    if (!split) continue;
    // PDFPool::split_gaussian, DiagonalGaussian::split with perturbation 0.2 (aku/Distributions.cc:1291-1312)
    EstGaussian g2 = h->pool[(size_t)gi];
    EstGaussian &g1 = h->pool[(size_t)gi];
    for (int i = 0; i < h->dim; i++) {
      const double sd = 0.2 * sqrt(g1.var[(size_t)i]);
      g1.mean[(size_t)i] -= sd;
      g2.mean[(size_t)i] += sd;
    }
    const int new_index = (int)h->pool.size();
    h->pool.push_back(std::move(g2));
    for (int p : pdf_index) {
      EstMixture &m = h->mixtures[(size_t)p];
      const int k = m.component_index(gi);
      const double cur_coef = m.weights[(size_t)k];
      m.weights[(size_t)k] = 0.5 * cur_coef;
      m.pointers.push_back(new_index);
      m.weights.push_back(0.5 * cur_coef);
    }
    num_splits++;
  }
  return num_splits;
}

// ---- the writers ---------------------------------------------------------------------------------

// a double through an ostream of default precision: "%g"
std::string G6(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

void write_file(const std::string &path, const std::string &text, const char *who) {
  std::ofstream out(path.c_str());
  if (!out) raise(AASR_ERR_IO, "%s: could not open %s", who, path.c_str());
  out << text;
  out.flush();
  if (!out) raise(AASR_ERR_IO, "%s: error writing file: %s", who, path.c_str());
}

// PDFPool::write_gk (aku/Distributions.cc:2913-2967), DiagonalGaussian::write (:1119-1128)
void write_gk(const aasr_estimate *h, const std::string &path) {
  std::string t = std::to_string(h->pool.size()) + " " + std::to_string(h->dim) + " variable\n";
  for (const EstGaussian &g : h->pool) {
    t += "diag ";
    for (int i = 0; i < h->dim; i++) t += G6(g.mean[(size_t)i]) + " ";
    for (int i = 0; i < h->dim - 1; i++) t += G6(g.var[(size_t)i]) + " ";
    t += G6(g.var[(size_t)h->dim - 1]);
    t += "\n";
  }
  write_file(path, t, "PDFPool::write_gk()");
}

// HmmSet::write_mc (aku/HmmSet.cc:360-370): the count of mixtures, then one line per STATE
void write_mc(const aasr_estimate *h, const std::string &path) {
  std::string t = std::to_string(h->mixtures.size()) + "\n";
  for (int i = 0; i < h->n_states; i++) {
    const EstMixture &m = h->mixtures[(size_t)i];
    t += std::to_string(m.pointers.size());
    for (size_t w = 0; w < m.pointers.size(); w++) t += " " + std::to_string(m.pointers[w]) + " " + G6(m.weights[w]);
    t += "\n";
  }
  write_file(path, t, "HmmSet::write_mc()");
}

// HmmSet::write_legacy_ph (aku/HmmSet.cc:379-425)
void write_ph(const aasr_estimate *h, const std::string &path) {
  std::string t = "PHONE\n" + std::to_string(h->hmms.size()) + "\n";
  for (size_t hi = 0; hi < h->hmms.size(); hi++) {
    const aasr_estimate::Hmm &hmm = h->hmms[hi];
    const int ns = (int)hmm.states.size();
    t += std::to_string(hi + 1) + " " + std::to_string(ns + 2) + " " + hmm.label + "\n";
    t += "-1 -2";
    for (int s : hmm.states) t += " " + std::to_string(s);
    t += "\n0 1 2 1\n1 0\n";
    for (int s = 0; s < ns; s++) {
      const std::vector<int> &tr = h->state_transitions[(size_t)hmm.states[(size_t)s]];
      t += std::to_string(s + 2) + " " + std::to_string(tr.size());
      for (int ti : tr) {
        int target = h->transitions[(size_t)ti].target + 2 + s;
        if (target == ns + 2) target = 1;
        t += " " + std::to_string(target) + " " + G6(h->transitions[(size_t)ti].prob);
      }
      t += "\n";
    }
  }
  write_file(path, t, "HmmSet::write_ph()");
}

}  // namespace

// ---- the estimation handle's C surface -------------------------------------------------------------

extern "C" {

aasr_status aasr_estimate_create(const char *gk, const char *mc, const char *ph, aasr_estimate **out) {
  return guarded([&] {
    if (!gk || !mc || !ph || !out) raise(AASR_ERR_INVALID, "aasr_estimate_create: null argument");
    *out = nullptr;
    std::unique_ptr<aasr_estimate> h(new aasr_estimate());
    // HmmSet::read_all reads the .mc first; the order only decides which missing file is named
    {
      std::ifstream in(mc);
      if (!in) raise(AASR_ERR_IO, "HmmSet::read_mc(): could not open %s", mc);
      int pdfs = 0;
      in >> pdfs;
      if (!in || pdfs < 0) raise(AASR_ERR_INVALID, "HmmSet::read_mc(): bad header in %s", mc);
      h->mixtures.resize((size_t)pdfs);
      for (EstMixture &m : h->mixtures) {  // Mixture::read (aku/Distributions.cc:2418-2434)
        int n = 0;
        in >> n;
        for (int w = 0; w < n; w++) {
          int index = 0;
          double weight = 0;
          in >> index >> weight;
          if (in.fail()) raise(AASR_ERR_INVALID, "Error in reading mixture specifications");
          m.pointers.push_back(index);
          m.weights.push_back(weight);
        }
        m.normalize();
      }
    }
    {
      std::ifstream in(ph);
      if (!in) raise(AASR_ERR_IO, "HmmSet::read_ph(): could not open %s", ph);
      std::string word;
      in >> word;
      if (word != "PHONE") raise(AASR_ERR_INVALID, "HmmSet::read_ph(): not a PHONE file: %s", ph);
      std::vector<std::vector<PhTransition>> state_info;
      parse_legacy_ph(
          in,
          [&](const std::string &label, int states) {
            if (states < 0) raise(AASR_ERR_INVALID, "%s: HMM %s has %d states", ph, label.c_str(), states + 2);
            h->hmms.push_back({label, std::vector<int>((size_t)states)});
          },
          [&](int s, int pdf) { h->hmms.back().states[(size_t)s] = pdf; },
          [&] { raise(AASR_ERR_INVALID, "HmmSet::read_ph(): read error in %s", ph); }, state_info);
      // the states and their transitions, numbered in state order (aku/HmmSet.cc:316-328)
      h->n_states = (int)state_info.size();
      h->state_transitions.resize(state_info.size());
      for (size_t s = 0; s < state_info.size(); s++)
        for (const PhTransition &tr : state_info[s]) {
          h->state_transitions[s].push_back((int)h->transitions.size());
          h->transitions.push_back(EstTransition{(int)s, tr.target_offset, tr.prob});
        }
      if (h->n_states > (int)h->mixtures.size())
        raise(AASR_ERR_INVALID, "%s names state %d but %s has %d mixtures", ph, h->n_states - 1, mc, (int)h->mixtures.size());
    }
    {
      HostModel m;
      read_gk_pool(gk, m);
      if (m.any_full())
        raise(AASR_ERR_UNSUPPORTED, "estimate: only diagonal Gaussians are supported (%s holds full-covariance or subspace Gaussians)", gk);
      h->dim = m.dim;
      h->pool.resize((size_t)m.G);
      for (int64_t g = 0; g < m.G; g++) {
        h->pool[(size_t)g].mean.assign(m.mean.begin() + g * m.dim, m.mean.begin() + (g + 1) * m.dim);
        h->pool[(size_t)g].var.assign(m.var.begin() + g * m.dim, m.var.begin() + (g + 1) * m.dim);
      }
    }
    for (const EstMixture &m : h->mixtures)
      for (int p : m.pointers)
        if (p < 0 || p >= (int)h->pool.size()) raise(AASR_ERR_INVALID, "%s names Gaussian %d, %s has %d", mc, p, gk, (int)h->pool.size());
    *out = h.release();
  });
}

void aasr_estimate_destroy(aasr_estimate *h) { delete h; }

aasr_status aasr_estimate_add_dump(aasr_estimate *h, const char *base, int32_t transitions) {
  return guarded([&] {
    if (!h || !base) raise(AASR_ERR_INVALID, "aasr_estimate_add_dump: null argument");
    const std::string b = base;
    accumulate_gk(h, b + ".gks");
    accumulate_mc(h, b + ".mcs");
    if (transitions) accumulate_ph(h, b + ".phs");
    accumulate_lls(h, b + ".lls");
  });
}

aasr_status aasr_estimate_set_gaussian_parameters(aasr_estimate *h, double minvar, double covsmooth) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_set_gaussian_parameters: null argument");
    h->minvar = minvar;
    h->covsmooth = covsmooth;
  });
}

aasr_status aasr_estimate_transitions(aasr_estimate *h) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_transitions: null argument");
    estimate_transitions(h);
  });
}

aasr_status aasr_estimate_ml(aasr_estimate *h, int32_t pool, int32_t mixtures) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_ml: null argument");
    if (pool)
      for (EstGaussian &g : h->pool) estimate_gaussian(h, g);
    if (mixtures) estimate_mixtures(h);
  });
}

aasr_status aasr_estimate_delete_gaussians(aasr_estimate *h, double minocc, int32_t *index_map, int32_t *n_deleted) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_delete_gaussians: null argument");
    std::vector<int> map;
    const int n = delete_gaussians(h, minocc, map);
    if (index_map) std::copy(map.begin(), map.end(), index_map);
    if (n_deleted) *n_deleted = n;
  });
}

aasr_status aasr_estimate_remove_mixture_components(aasr_estimate *h, double min_weight, int32_t *index_map, int32_t *n_deleted) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_remove_mixture_components: null argument");
    std::vector<int> map;
    const int n = remove_mixture_components(h, min_weight, map);
    if (index_map) std::copy(map.begin(), map.end(), index_map);
    if (n_deleted) *n_deleted = n;
  });
}

aasr_status aasr_estimate_split_gaussians(aasr_estimate *h, double minocc, int32_t maxmixgauss, int32_t numgauss, double splitalpha,
                                          int32_t *n_splits) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_split_gaussians: null argument");
    const int n = split_gaussians(h, minocc, maxmixgauss, numgauss, splitalpha);
    if (n_splits) *n_splits = n;
  });
}

aasr_status aasr_estimate_write_gk(const aasr_estimate *h, const char *path) {
  return guarded([&] {
    if (!h || !path) raise(AASR_ERR_INVALID, "aasr_estimate_write_gk: null argument");
    write_gk(h, path);
  });
}

aasr_status aasr_estimate_write_mc(const aasr_estimate *h, const char *path) {
  return guarded([&] {
    if (!h || !path) raise(AASR_ERR_INVALID, "aasr_estimate_write_mc: null argument");
    write_mc(h, path);
  });
}

aasr_status aasr_estimate_write_ph(const aasr_estimate *h, const char *path) {
  return guarded([&] {
    if (!h || !path) raise(AASR_ERR_INVALID, "aasr_estimate_write_ph: null argument");
    write_ph(h, path);
  });
}

void aasr_estimate_sizes(const aasr_estimate *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 7; i++) out[i] = 0;
  if (!h) return;
  size_t comps = 0;
  for (const EstMixture &m : h->mixtures) comps += m.pointers.size();
  out[0] = (int32_t)h->pool.size();
  out[1] = h->dim;
  out[2] = (int32_t)h->mixtures.size();
  out[3] = (int32_t)comps;
  out[4] = h->n_states;
  out[5] = (int32_t)h->transitions.size();
  out[6] = h->mode;
}

aasr_status aasr_estimate_get_statistics(const aasr_estimate *h, int32_t *accumulated, int32_t *feacount, double *gamma, double *sum_x,
                                         double *sum_xx) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_statistics: null argument");
    const size_t d = (size_t)h->dim, n = h->xx_len();
    for (size_t g = 0; g < h->pool.size(); g++) {
      const EstGaussian &e = h->pool[g];
      if (accumulated) accumulated[g] = e.accumulated ? 1 : 0;
      if (feacount) feacount[g] = e.feacount;
      if (gamma) gamma[g] = e.gamma;
      for (size_t i = 0; sum_x && i < d; i++) sum_x[g * d + i] = e.has_accum ? e.sum_x[i] : 0.0;
      for (size_t i = 0; sum_xx && i < n; i++) sum_xx[g * n + i] = e.has_accum ? e.sum_xx[i] : 0.0;
    }
  });
}

aasr_status aasr_estimate_get_mixture_statistics(const aasr_estimate *h, int32_t *accumulated, int32_t *offsets, double *gamma) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_mixture_statistics: null argument");
    int32_t off = 0;
    for (size_t m = 0; m < h->mixtures.size(); m++) {
      const EstMixture &e = h->mixtures[m];
      if (accumulated) accumulated[m] = e.accumulated ? 1 : 0;
      if (offsets) offsets[m] = off;
      for (size_t k = 0; k < e.pointers.size(); k++, off++)
        if (gamma) gamma[off] = k < e.gamma.size() ? e.gamma[k] : 0.0;
    }
    if (offsets) offsets[h->mixtures.size()] = off;
  });
}

aasr_status aasr_estimate_get_transition_statistics(const aasr_estimate *h, int32_t *accumulated, double *occupancy) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_transition_statistics: null argument");
    for (size_t t = 0; t < h->transitions.size(); t++) {
      if (accumulated) accumulated[t] = h->trans_accum.empty() ? 0 : h->trans_accumulated[t];
      if (occupancy) occupancy[t] = h->trans_accum.empty() ? 0.0 : h->trans_accum[t];
    }
  });
}

aasr_status aasr_estimate_get_gaussians(const aasr_estimate *h, double *mean, double *var) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_gaussians: null argument");
    const size_t d = (size_t)h->dim;
    for (size_t g = 0; g < h->pool.size(); g++) {
      if (mean) std::copy(h->pool[g].mean.begin(), h->pool[g].mean.end(), mean + g * d);
      if (var) std::copy(h->pool[g].var.begin(), h->pool[g].var.end(), var + g * d);
    }
  });
}

aasr_status aasr_estimate_get_mixtures(const aasr_estimate *h, int32_t *offsets, int32_t *index, double *weight) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_mixtures: null argument");
    int32_t off = 0;
    for (size_t m = 0; m < h->mixtures.size(); m++) {
      const EstMixture &e = h->mixtures[m];
      if (offsets) offsets[m] = off;
      for (size_t k = 0; k < e.pointers.size(); k++, off++) {
        if (index) index[off] = e.pointers[k];
        if (weight) weight[off] = e.weights[k];
      }
    }
    if (offsets) offsets[h->mixtures.size()] = off;
  });
}

aasr_status aasr_estimate_get_transitions(const aasr_estimate *h, int32_t *source, int32_t *target, double *prob) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_estimate_get_transitions: null argument");
    for (size_t t = 0; t < h->transitions.size(); t++) {
      if (source) source[t] = h->transitions[t].source;
      if (target) target[t] = h->transitions[t].target;
      if (prob) prob[t] = h->transitions[t].prob;
    }
  });
}

}  // extern "C"

// ---- the MLLT handle -----------------------------------------------------------------------------

struct aasr_mllt {
  int dim = 0, PB = 0, E = 0, ET = 0;
  int64_t G = 0, GP = 0, TS = 0;
  int64_t slab_bytes = MLLT_SLAB_BYTES;
  std::vector<double> gamma, sum_x;
  std::vector<int32_t> ok;
  DevBuf<double> cov, p, var, w, slab, sums;
  std::vector<double> h_p, h_w, h_sums;
  int32_t shape[3] = {0, 0, 0};
  double times[4] = {0, 0, 0, 0};  // seconds: covariance build, variance passes, G passes, host solve
};

namespace {

// p[e][i] = a_ir a_ic, doubled off the diagonal (mllt.h)
void mllt_variances(aasr_mllt *h, const double *A, double *var) {
  const int d = h->dim, IP = 16 * h->PB;
  const auto t0 = std::chrono::steady_clock::now();
  h->h_p.assign((size_t)h->E * IP, 0.0);
  for (int r = 0, e = 0; r < d; r++)
    for (int c = 0; c <= r; c++, e++)
      for (int i = 0; i < d; i++) {
        const double v = A[(size_t)i * d + r] * A[(size_t)i * d + c];
        h->h_p[(size_t)e * IP + i] = r == c ? v : 2 * v;
      }
  AASR_HIP(hipMemcpy(h->p.p, h->h_p.data(), h->h_p.size() * sizeof(double), hipMemcpyHostToDevice));
  mllt_var_launch(d, h->G, h->cov.p, h->p.p, h->var.p, nullptr);
  AASR_HIP(hipMemcpy(var, h->var.p, (size_t)h->G * d * sizeof(double), hipMemcpyDeviceToHost));
  h->times[1] += seconds_since(t0);
}

// sums[i] = sum_g (gamma_g / var_gi) S_g as the packed lower triangle [dim x E]; Gaussians without statistics weigh 0
void mllt_g_sums(aasr_mllt *h, const double *var, double *out) {
  const int d = h->dim, IP = 16 * h->PB;
  const auto t0 = std::chrono::steady_clock::now();
  h->h_w.assign((size_t)h->GP * IP, 0.0);
  for (int64_t g = 0; g < h->G; g++)
    if (h->ok[(size_t)g])
      for (int i = 0; i < d; i++) h->h_w[(size_t)g * IP + i] = h->gamma[(size_t)g] / var[(size_t)g * d + i];
  AASR_HIP(hipMemcpy(h->w.p, h->h_w.data(), h->h_w.size() * sizeof(double), hipMemcpyHostToDevice));
  AASR_HIP(hipMemset(h->sums.p, 0, (size_t)h->TS * sizeof(double)));
  const int64_t NI = h->GP / MLLT_ITEM;
  const int64_t max_items = std::max<int64_t>(1, h->slab_bytes / (h->TS * (int64_t)sizeof(double)));
  h->slab.ensure((size_t)std::min(NI, max_items) * h->TS);
  int launches = 0;
  for (int64_t i0 = 0; i0 < NI; i0 += max_items, launches++)
    mllt_gsum_launch(d, h->GP, h->cov.p, h->w.p, (int)i0, (int)std::min(max_items, NI - i0), h->slab.p, h->sums.p, nullptr);
  h->h_sums.resize((size_t)h->TS);
  AASR_HIP(hipMemcpy(h->h_sums.data(), h->sums.p, h->h_sums.size() * sizeof(double), hipMemcpyDeviceToHost));
  const int64_t EP = (int64_t)16 * h->ET;
  for (int i = 0; i < d; i++)
    for (int e = 0; e < h->E; e++) out[(size_t)i * h->E + e] = h->h_sums[(size_t)(i * EP + e)];
  h->shape[0] = h->PB;
  h->shape[1] = (int32_t)NI;
  h->shape[2] = launches;
  h->times[2] += seconds_since(t0);
}

// the inner loop of HmmSet::estimate_mllt (aku/HmmSet.cc:955-980): the cofactors |det| (A^T)^-1 of the CURRENT A
// once, then every row from them: row_i = G_i^T c_i scaled by sqrt(beta / c_i . row_i)
void mllt_update_rows(int d, const double *g_inv, double beta, int iterations, double *A) {
  std::vector<double> c((size_t)d * d);
  for (int it = 0; it < iterations; it++) {
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) c[(size_t)i * d + j] = A[(size_t)j * d + i];
    double det = 1;
    if (!lu_inverse(c, d, &det)) raise(AASR_ERR_INVALID, "mllt: zero pivot in A (inner iteration %d)", it);
    det = std::fabs(det);
    for (double &v : c) v *= det;
    for (int i = 0; i < d; i++) {
      const double *Gi = g_inv + (size_t)i * d * d, *ci = c.data() + (size_t)i * d;
      double *row = A + (size_t)i * d;
      for (int j = 0; j < d; j++) {
        double s = 0;
        for (int k = 0; k < d; k++) s += Gi[(size_t)k * d + j] * ci[k];
        row[j] = s;
      }
      double dot = 0;
      for (int j = 0; j < d; j++) dot += ci[j] * row[j];
      const double sc = sqrt(beta / dot);
      for (int j = 0; j < d; j++) row[j] *= sc;
    }
  }
}

void floor_variances(const aasr_mllt *h, double minvar, std::vector<double> &var, bool warn) {
  const int d = h->dim;
  for (int64_t g = 0; g < h->G; g++) {
    if (!h->ok[(size_t)g]) continue;
    for (int i = 0; i < d; i++) {
      double &v = var[(size_t)g * d + i];
      if (warn && v <= 0) fprintf(stderr, "Warning: Variance in dimension %i is %g (gamma %g)\n", i, v, h->gamma[(size_t)g]);
      if (v < minvar) v = minvar;
    }
  }
}

// HmmSet::estimate_mllt (aku/HmmSet.cc:841-1031) up to the new means and variances
void mllt_estimate(aasr_mllt *h, double minvar, double *A, double *mean, double *var_out) {
  const int d = h->dim;
  for (int i = 0; i < d; i++)
    for (int j = 0; j < d; j++) A[(size_t)i * d + j] = i == j ? 1.0 : 0.0;
  double beta = 0;
  for (int64_t g = 0; g < h->G; g++)
    if (h->ok[(size_t)g]) beta += h->gamma[(size_t)g];
  std::vector<double> var((size_t)h->G * d), sums((size_t)d * h->E), g_inv((size_t)d * d * d), m((size_t)d * d);
  for (int iter = 0; iter < kMlltIter; iter++) {
    mllt_variances(h, A, var.data());
    floor_variances(h, minvar, var, true);
    mllt_g_sums(h, var.data(), sums.data());
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < d; i++) {
      for (int r = 0, e = 0; r < d; r++)
        for (int c = 0; c <= r; c++, e++) m[(size_t)r * d + c] = m[(size_t)c * d + r] = sums[(size_t)i * h->E + e];
      if (!lu_inverse(m, d, nullptr)) raise(AASR_ERR_INVALID, "mllt: zero pivot in G_%d (singular statistics)", i);
      std::copy(m.begin(), m.end(), g_inv.begin() + (size_t)i * d * d);
    }
    mllt_update_rows(d, g_inv.data(), beta, kMlltAIter, A);
    // normalise by |det A|^(1 / dim)
    std::vector<double> lu(A, A + (size_t)d * d);
    double det = 1;
    if (!lu_inverse(lu, d, &det)) raise(AASR_ERR_INVALID, "mllt: zero pivot in A (iteration %d)", iter);
    const double scale = pow(std::fabs(det), 1 / (double)d);
    const double inv = 1 / scale;
    for (int i = 0; i < d * d; i++) A[i] *= inv;
    h->times[3] += seconds_since(t0);
  }
  mllt_variances(h, A, var.data());
  floor_variances(h, minvar, var, true);
  for (int64_t g = 0; g < h->G; g++) {
    if (!h->ok[(size_t)g]) continue;
    const double inv = 1 / h->gamma[(size_t)g];
    for (int i = 0; i < d; i++) {
      double s = 0;
      for (int j = 0; j < d; j++) s += A[(size_t)i * d + j] * (h->sum_x[(size_t)g * d + j] * inv);
      if (mean) mean[(size_t)g * d + i] = s;
      if (var_out) var_out[(size_t)g * d + i] = var[(size_t)g * d + i];
    }
  }
}

}  // namespace

extern "C" {

aasr_status aasr_mllt_create(int32_t dim, int64_t n_gauss, const double *gamma, const double *sum_x, const double *sum_xx,
                             const int32_t *accumulated, aasr_mllt **out) {
  return guarded([&] {
    if (!out || dim < 1 || n_gauss < 1 || !gamma || !sum_x || !sum_xx) raise(AASR_ERR_INVALID, "aasr_mllt_create: bad argument");
    *out = nullptr;
    if (dim > MLLT_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "mllt: no kernels for dimension %d (1 ... %d)", dim, MLLT_MAX_DIM);
    if (n_gauss > ((int64_t)1 << 24)) raise(AASR_ERR_INVALID, "aasr_mllt_create: more than 2^24 Gaussians");
    require_device();
    std::unique_ptr<aasr_mllt> h(new aasr_mllt());
    h->dim = dim;
    h->PB = mllt_pb(dim);
    h->E = mllt_entries(dim);
    h->ET = mllt_et(dim);
    h->G = n_gauss;
    h->GP = mllt_gp(n_gauss);
    h->TS = mllt_slab_doubles(dim);
    h->gamma.assign(gamma, gamma + n_gauss);
    h->sum_x.assign(sum_x, sum_x + n_gauss * dim);
    h->ok.assign((size_t)n_gauss, 1);
    if (accumulated)
      for (int64_t g = 0; g < n_gauss; g++) h->ok[(size_t)g] = accumulated[g] ? 1 : 0;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t cov_n = (size_t)mllt_cov_rows(dim) * h->GP;
    h->cov.alloc(cov_n);
    AASR_HIP(hipMemset(h->cov.p, 0, cov_n * sizeof(double)));
    {
      DevBuf<double> d_gamma, d_sx, d_m2;
      DevBuf<int32_t> d_ok;
      d_gamma.upload(gamma, (size_t)n_gauss);
      d_sx.upload(sum_x, (size_t)n_gauss * dim);
      d_m2.upload(sum_xx, (size_t)n_gauss * h->E);
      d_ok.upload(h->ok.data(), (size_t)n_gauss);
      mllt_cov_launch(dim, n_gauss, d_gamma.p, d_sx.p, d_m2.p, d_ok.p, h->cov.p, nullptr);
      AASR_HIP(hipDeviceSynchronize());
    }
    h->times[0] = seconds_since(t0);
    h->p.alloc((size_t)h->E * 16 * h->PB);
    h->var.alloc((size_t)n_gauss * dim);
    h->w.alloc((size_t)h->GP * 16 * h->PB);
    h->sums.alloc((size_t)h->TS);
    *out = h.release();
  });
}

void aasr_mllt_destroy(aasr_mllt *h) { delete h; }

aasr_status aasr_mllt_get_covariances(aasr_mllt *h, double *cov) {
  return guarded([&] {
    if (!h || !cov) raise(AASR_ERR_INVALID, "aasr_mllt_get_covariances: null argument");
    std::vector<double> row((size_t)h->GP);
    for (int e = 0; e < h->E; e++) {
      AASR_HIP(hipMemcpy(row.data(), h->cov.p + (size_t)e * h->GP, row.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t g = 0; g < h->G; g++) cov[(size_t)g * h->E + e] = row[(size_t)g];
    }
  });
}

aasr_status aasr_mllt_variances(aasr_mllt *h, const double *A, double *var) {
  return guarded([&] {
    if (!h || !A || !var) raise(AASR_ERR_INVALID, "aasr_mllt_variances: null argument");
    mllt_variances(h, A, var);
  });
}

aasr_status aasr_mllt_g_sums(aasr_mllt *h, const double *var, double *g_sums) {
  return guarded([&] {
    if (!h || !var || !g_sums) raise(AASR_ERR_INVALID, "aasr_mllt_g_sums: null argument");
    mllt_g_sums(h, var, g_sums);
  });
}

aasr_status aasr_mllt_update_rows(int32_t dim, const double *g_inv, double beta, int32_t iterations, double *A) {
  return guarded([&] {
    if (dim < 1 || !g_inv || !A || iterations < 0) raise(AASR_ERR_INVALID, "aasr_mllt_update_rows: bad argument");
    mllt_update_rows(dim, g_inv, beta, iterations, A);
  });
}

aasr_status aasr_mllt_estimate(aasr_mllt *h, double minvar, double *A, double *mean, double *var) {
  return guarded([&] {
    if (!h || !A) raise(AASR_ERR_INVALID, "aasr_mllt_estimate: null argument");
    mllt_estimate(h, minvar, A, mean, var);
  });
}

void aasr_debug_mllt_shape(const aasr_mllt *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 3; i++) out[i] = h ? h->shape[i] : 0;
}

void aasr_debug_mllt_times(const aasr_mllt *h, double *out) {
  if (!out) return;
  for (int i = 0; i < 4; i++) out[i] = h ? h->times[i] : 0;
}

aasr_status aasr_debug_mllt_set_slab_bytes(aasr_mllt *h, int64_t bytes) {
  return guarded([&] {
    if (!h || bytes < 1) raise(AASR_ERR_INVALID, "aasr_debug_mllt_set_slab_bytes: bad argument");
    h->slab_bytes = bytes;
  });
}

}  // extern "C"

// ---- the tool's main -----------------------------------------------------------------------------

namespace {

// the lin_transform module `name` of a configuration text, host only: its configured dim (0: none) and the length of
// its configured matrix (0: none)
void configured_transform(const std::string &text, const std::string &name, int *dim, size_t *matrix_len) {
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
    std::string n, type;
    cfg.get("name", n);
    cfg.get("type", type);
    if (n != name) continue;
    if (type != "lin_transform") raise(AASR_ERR_INVALID, "Module %s is not a transform module", name.c_str());
    *dim = 0;
    cfg.get("dim", *dim);
    std::vector<float> m;
    cfg.get("matrix", m);
    *matrix_len = m.size();
    return;
  }
  raise(AASR_ERR_INVALID, "unknown module requested: %s", name.c_str());
}

std::string read_text(const char *path) {
  std::ifstream in(path);
  if (!in) raise(AASR_ERR_IO, "could not open %s", path);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

}  // namespace

extern "C" {

void aasr_estimate_default_options(aasr_estimate_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->minvar = 0.1;
  o->numgauss = -1;
  o->splitalpha = 1.0;
}

aasr_status aasr_estimate_run_mllt(aasr_estimate *h, const float *old_matrix, float *new_matrix, double *seconds) {
  return guarded([&] {
    if (!h || !new_matrix) raise(AASR_ERR_INVALID, "aasr_estimate_run_mllt: null argument");
    if (!h->full())
      raise(AASR_ERR_INVALID,
            "estimate: --mllt needs full second moments (statistics mode 3, written by stats --mllt); the dumps are mode %d",
            h->mode);
    const int d = h->dim;
    if (d > MLLT_MAX_DIM) raise(AASR_ERR_UNSUPPORTED, "mllt: no kernels for dimension %d (1 ... %d)", d, MLLT_MAX_DIM);
    const size_t G = h->pool.size(), E = (size_t)d * (d + 1) / 2;
    std::vector<double> gamma(G, 0.0), sx(G * d, 0.0), sxx(G * E, 0.0), A((size_t)d * d), mean(G * d), var(G * d);
    std::vector<int32_t> ok(G, 0);
    for (size_t g = 0; g < G; g++) {
      const EstGaussian &e = h->pool[g];
      if (!e.accumulated) continue;  // Gaussian::full_stats_accumulated
      ok[g] = 1;
      gamma[g] = e.gamma;
      std::copy(e.sum_x.begin(), e.sum_x.end(), sx.begin() + g * d);
      std::copy(e.sum_xx.begin(), e.sum_xx.end(), sxx.begin() + g * E);
    }
    aasr_mllt *m = nullptr;
    {
      const aasr_status cs = aasr_mllt_create(d, (int64_t)G, gamma.data(), sx.data(), sxx.data(), ok.data(), &m);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_mllt, void (*)(aasr_mllt *)> guard(m, aasr_mllt_destroy);
    mllt_estimate(m, h->minvar, A.data(), mean.data(), var.data());
    for (size_t g = 0; g < G; g++) {
      if (!ok[g]) continue;
      h->pool[g].mean.assign(mean.begin() + g * d, mean.begin() + (g + 1) * d);
      h->pool[g].var.assign(var.begin() + g * d, var.begin() + (g + 1) * d);
    }
    // the module's matrix: A A_old (an unset matrix is the identity), narrowed to float
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) {
        double s = 0;
        for (int k = 0; k < d; k++) s += A[(size_t)i * d + k] * (old_matrix ? (double)old_matrix[(size_t)k * d + j] : (k == j ? 1.0 : 0.0));
        new_matrix[(size_t)i * d + j] = (float)s;
      }
    // the mixtures as in the ML update (aku/HmmSet.cc:1042-1053)
    estimate_mixtures(h);
    if (seconds) aasr_debug_mllt_times(m, seconds);
  });
}

aasr_status aasr_run_estimate(aasr_estimate_options *opt) {
  return guarded([&] {
    if (!opt || !opt->gk || !opt->mc || !opt->ph || !opt->list || !opt->out) raise(AASR_ERR_INVALID, "aasr_run_estimate: null argument");
    opt->n_deleted = opt->n_removed = opt->n_splits = 0;
    opt->seconds_read = opt->seconds_mllt = 0;
    for (double &s : opt->seconds_mllt_parts) s = 0;
    if (opt->split && !(opt->minocc_set || opt->numgauss_set))
      raise(AASR_ERR_INVALID, "Either --minocc or --numgauss is required with --split");
    if (opt->mllt && !opt->config) raise(AASR_ERR_INVALID, "Must specify configuration file with MLLT");
    aasr_estimate *eh = nullptr;
    {
      const aasr_status cs = aasr_estimate_create(opt->gk, opt->mc, opt->ph, &eh);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_estimate, void (*)(aasr_estimate *)> guard(eh, aasr_estimate_destroy);
    const int d = eh->dim;
    std::string cfg_text;
    if (opt->config) cfg_text = read_text(opt->config);
    if (opt->mllt) {  // before the dumps are read and the device is opened
      int cd = 0;
      size_t ml = 0;
      configured_transform(cfg_text, opt->mllt, &cd, &ml);
      if ((cd > 0 && cd != d) || (ml > 0 && ml != (size_t)d * d))
        raise(AASR_ERR_INVALID, "estimate: the matrix of module %s is not %d x %d, the model's dimension", opt->mllt, d, d);
      if (d > MLLT_MAX_DIM) raise(AASR_ERR_UNSUPPORTED, "mllt: no kernels for dimension %d (1 ... %d)", d, MLLT_MAX_DIM);
    }
    // the list of statistics files (estimate.cc:278-312)
    std::ifstream filelist(opt->list);
    if (!filelist) raise(AASR_ERR_IO, "Could not open %s", opt->list);
    const auto t0 = std::chrono::steady_clock::now();
    std::string stat_file;
    while (filelist >> stat_file && stat_file != " ") {
      const aasr_status s = aasr_estimate_add_dump(eh, stat_file.c_str(), opt->transitions);
      if (s != AASR_OK) raise(s, "%s", last_error().c_str());
    }
    opt->seconds_read = seconds_since(t0);
    if (opt->mllt && !eh->full())
      raise(AASR_ERR_INVALID,
            "estimate: --mllt needs full second moments (statistics mode 3, written by stats --mllt); the dumps are mode %d",
            eh->mode);
    eh->minvar = opt->minvar;
    eh->covsmooth = opt->covsmooth;
    if (opt->transitions) estimate_transitions(eh);
    std::unique_ptr<aasr_feat> feat;
    if (opt->mllt) {
      const auto t1 = std::chrono::steady_clock::now();
      feat.reset(feat_create(cfg_text));
      FeatModule *ltm = &feat->mods[(size_t)feat->by_name.at(opt->mllt)];
      if (ltm->dim != d || ltm->src_dim != d)
        raise(AASR_ERR_INVALID, "estimate: the matrix of module %s is %d x %d, the model's dimension is %d", opt->mllt, ltm->dim,
              ltm->src_dim, d);
      std::vector<float> tr((size_t)d * d);
      const aasr_status s =
          aasr_estimate_run_mllt(eh, ltm->matrix_defined ? ltm->matrix.data() : nullptr, tr.data(), opt->seconds_mllt_parts);
      if (s != AASR_OK) raise(s, "%s", last_error().c_str());
      // LinTransformModule::set_transformation_matrix (FeatureModules.cc:1273-1296): the working and the configured
      // matrix both
      ltm->matrix = tr;
      ltm->orig_matrix = tr;
      ltm->matrix_defined = true;
      ltm->d_matrix.upload(ltm->matrix.data(), ltm->matrix.size());
      opt->seconds_mllt = seconds_since(t1);
    } else {
      for (EstGaussian &g : eh->pool) estimate_gaussian(eh, g);
      if (!opt->no_mixture_update) estimate_mixtures(eh);
    }
    std::vector<int> map;
    if (opt->delete_set) opt->n_deleted = delete_gaussians(eh, opt->delete_minocc, map);
    if (opt->mremove_set) opt->n_removed = remove_mixture_components(eh, opt->mremove, map);
    if (opt->split) opt->n_splits = split_gaussians(eh, opt->minocc, opt->maxmixgauss, opt->numgauss, opt->splitalpha);
    if (opt->no_write) return;
    const std::string out = opt->out;
    write_mc(eh, out + ".mc");
    write_ph(eh, out + ".ph");
    write_gk(eh, out + ".gk");
    if (opt->config) {
      // the configuration goes through the feature handle's writer, which lives on the device
      if (!feat) feat.reset(feat_create(cfg_text));
      const std::string text = feat_write_configuration(feat.get());
      write_text_file((out + ".cfg").c_str(), text.data(), text.size());
    }
    if (opt->savesum) {  // estimate.cc:406-425
      std::ofstream summary_file(opt->savesum, std::ios_base::app);
      if (!summary_file) {
        fprintf(stderr, "Could not open summary file: %s\n", opt->savesum);
      } else {
        summary_file.precision(12);
        summary_file << (opt->base_name ? opt->base_name : opt->gk) << std::endl;
        for (const auto &it : eh->sum_statistics) summary_file << "  " << it.first << ": " << it.second << std::endl;
      }
    }
  });
}

}  // extern "C"

// gmm_centred.cc -- operands of the centred-form kernel: the whole model, the outliers of a model that keeps
// the matrix path (outlier routing), and the per-Gaussian view.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gmm_build.h"

namespace aasr {

// Operands of the centred-form kernel + the conditioning estimate that decides
// whether the matrix-core (expanded form) kernels may be used.
// Centred-form operands of a component subset: rows k of the mixture arrays grouped by `off`
// ([n_states + 1] offsets into `comps`).
// pool = true: `comps` are pool Gaussians with weight 1 (the per-Gaussian view), not mixture components
static void build_centred_tables(const HostModel &m, int dimp, const std::vector<int32_t> &comps,
                                 const std::vector<int32_t> &off, DevBuf<float> &d_recs,
                                 DevBuf<int32_t> &d_off, DevBuf<int32_t> &d_splits, int *max_splits,
                                 bool pool = false) {
  const int D = m.dim;
  // k_gmm_diag_score_centred streams a record as groups of 16 floats, one scalar load each: group q =
  // [mu_hi x 4][mu_lo x 4][p' x 4][C (group 0), pad x 3] of dimensions 4 q .. 4 q + 3; one spare record behind the last
  // (the kernel fetches up to four groups ahead)
  const int rec = 4 * dimp;
  const size_t rows = comps.size();
  const int64_t n_states = (int64_t)off.size() - 1;
  std::vector<float> recs((rows + 1) * rec, 0.0f);
  for (size_t r = 0; r < rows; r++) {
    const size_t k = (size_t)comps[r];
    const int64_t gi = pool ? (int64_t)k : (int64_t)m.mix_idx[k];
    for (int d = 0; d < D; d++) {
      double v = m.var[(size_t)gi * D + d];
      double p = v > 0 ? 1 / v : 0;
      const double mu = m.mean[(size_t)gi * D + d];
      float *gq = &recs[r * rec + (size_t)(d / 4) * 16];
      gq[d % 4] = (float)mu;
      gq[4 + d % 4] = (float)(mu - (double)(float)mu);
      gq[8 + d % 4] = (float)(-0.5 * p * kLog2e);
    }
    double c = diag_log_sqrt_det(&m.var[(size_t)gi * D], D) + (pool ? 0.0 : m.logw(k));
    if (std::isnan(c) || c == INFINITY)
      raise(AASR_ERR_INVALID, "Gaussian %ld has a non-finite constant (precision product overflow)", (long)gi);
    recs[r * rec + 12] = std::isfinite(c) ? (float)(c * kLog2e) : kNullConst;
  }
  d_recs.upload(recs.data(), recs.size());
  d_off.upload(off.data(), off.size());
  // state-range cut table: row R-1 = R+1 boundaries with near-equal row counts
  std::vector<int32_t> table((size_t)CENTRED_MAX_SPLITS * (CENTRED_MAX_SPLITS + 1), 0);
  *max_splits = (int)std::max<int64_t>(1, std::min<int64_t>(CENTRED_MAX_SPLITS, n_states));
  for (int R = 1; R <= *max_splits; R++) {
    int32_t *row = &table[(size_t)(R - 1) * (CENTRED_MAX_SPLITS + 1)];
    int64_t s = 0;
    row[0] = 0;
    for (int i = 1; i < R; i++) {
      int64_t want = (int64_t)((double)rows * i / R);
      while (s < n_states && off[(size_t)s] < want) s++;
      if (s <= row[i - 1]) s = row[i - 1] + 1;
      if (s > n_states) s = n_states;
      row[i] = (int32_t)s;
    }
    row[R] = (int32_t)n_states;
  }
  d_splits.upload(table.data(), table.size());
}

int centred_dimp_for(int D) {
  for (int c : {8, 16, 24, 32, 40, 48, 64})
    if (D <= c) return c;
  return 0;
}

// Conditioning of the expanded form, kappa_g = sum_d p (mu - pivot)^2 per Gaussian (and its 2-norm
// over d, KAPPA2_LIMIT).  A model whose worst Gaussian exceeds a limit is scored entirely in the centred form -- unless the
// offenders are a minority (at most a quarter of the mixture components): then only they are,
// over the states that hold them (outlier routing), and the rest keeps the matrix path.
void find_outliers(aasr_gmm *g) {
  const HostModel &m = g->host;
  const int D = m.dim;
  g->outlier.clear();
  g->hyb_enabled = false;
  g->hyb_states = g->hyb_rows = 0;
  g->hyb_comps.clear();
  g->hyb_tab = aasr::DevBuf<uint32_t>();
  std::vector<double> kap((size_t)m.G), kap2((size_t)m.G);
  double kappa = 0;
  for (int64_t i = 0; i < m.G; i++) {
    double k2 = 0;
    const double k = kappa_terms(&m.mean[(size_t)i * D], &m.var[(size_t)i * D], g->pivot.data(), D, &k2);
    kap[(size_t)i] = k;
    kap2[(size_t)i] = std::sqrt(k2);
    kappa = std::max(kappa, k);
  }
  g->kappa = kappa;
  const int dimp = centred_dimp_for(D);
  static const int routing = AASR_EXPERIMENT_ENV("AASR_OUTLIER_ROUTING") ? atoi(AASR_EXPERIMENT_ENV("AASR_OUTLIER_ROUTING")) : 1;
  // Two passes.  First against the plain TWO-term limits: where only a handful of Gaussians break them, those become the
  // outliers and the whole model keeps the fastest rows (round 6: a Gaussian between the two-term and the three-term
  // limits used to cost its state a three-term section of its own and the model its whole-model two-term rows;
  // in the centred form it costs 1.6 us per 449 280 frames + ~20 us for its state's merge: a read-modify-write of one
  // column of the score matrix touches a line per frame).  "A handful": what the public layout pays for them stays below
  // the gather of a model with engine parts (gmm_score.hip, engine_parts_public: 2.4 ms).  Else against the limits of the
  // three-term / f32 rows, as before.
  const double lim2_f16 = D < 8 ? KAPPA2_LIMIT_F16_LOWDIM : KAPPA2_LIMIT_F16;
  for (int pass = 0; pass < 2; pass++) {
    const double lk = pass == 0 ? KAPPA_LIMIT_F16 : KAPPA_LIMIT, lk2 = pass == 0 ? lim2_f16 : KAPPA2_LIMIT;
    std::vector<uint8_t> bad((size_t)m.G, 0);
    double kappa_in = 0, kappa2_in = 0;
    bool any_bad = false;
    for (int64_t i = 0; i < m.G; i++) {
      bad[(size_t)i] = kap[(size_t)i] > lk || kap2[(size_t)i] > lk2;
      any_bad = any_bad || bad[(size_t)i];
      if (!bad[(size_t)i]) {
        kappa_in = std::max(kappa_in, kap[(size_t)i]);
        kappa2_in = std::max(kappa2_in, kap2[(size_t)i]);
      }
    }
    std::vector<int32_t> comps, off{0}, map;
    if (any_bad)
      for (int64_t s = 0; s < m.S; s++) {
        const size_t before = comps.size();
        for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++)
          if (bad[(size_t)m.mix_idx[k]]) comps.push_back(k);
        if (comps.size() > before) {
          off.push_back((int32_t)comps.size());
          map.push_back((int32_t)s);
        }
      }
    if (pass == 0) {
      if (!any_bad) {   // every Gaussian inside the two-term limits
        g->kappa_matrix = kappa_in;
        g->kappa2_matrix = kappa2_in;
        g->ill_conditioned = false;
        return;
      }
      // (the merge costs ~20 us per state as a pass of its own, nothing where the scoring kernel does it in its close logic:
      // models of up to 65 534 states on the grouped layout, hyb_tab below)
      const double merge_us = (m.S <= 65534 && 8 * (int64_t)map.size() <= m.S) ? 0.0 : 20.0;   // (fused only where such states are sparse)
      if (!dimp || !routing || 1.7 * (double)comps.size() + merge_us * (double)map.size() >= (merge_us > 0 ? 1500.0 : 2400.0) ||
          comps.size() * 4 > m.mix_idx.size())
        continue;
    }
    g->kappa_matrix = kappa_in;
    g->kappa2_matrix = kappa2_in;
    g->ill_conditioned = any_bad;
    if (!g->ill_conditioned || !dimp || !routing) return;
    if (comps.empty() || comps.size() * 4 > m.mix_idx.size()) return;  // not a minority: all centred
    g->outlier = bad;
    g->hyb_enabled = true;
    g->ill_conditioned = false;
    g->hyb_states = (int64_t)map.size();
    g->hyb_rows = (int64_t)comps.size();
    build_centred_tables(m, dimp, comps, off, g->hyb_recs, g->hyb_state_off, g->hyb_splits, &g->hyb_max_splits);
    g->hyb_map.upload(map.data(), map.size());
    g->hyb_comps = comps;
    g->hyb_tab = aasr::DevBuf<uint32_t>();
    if (m.S <= 65534 && (int64_t)map.size() <= 65535) {   // (k_gmm_diag_score_pl<..., HYB>: the merge in the close logic)
      std::vector<int32_t> slot((size_t)m.S, -1);
      for (size_t j = 0; j < map.size(); j++) slot[(size_t)map[j]] = (int32_t)j;
      std::vector<uint32_t> tab((size_t)m.S, 0xffffu);
      uint32_t nxt[2] = {0xffffu, 0xffffu};
      for (int64_t s = m.S - 1; s >= 0; s--) {
        if (slot[(size_t)s] >= 0) nxt[s & 1] = (uint32_t)s | ((uint32_t)slot[(size_t)s] << 16);
        tab[(size_t)s] = nxt[s & 1];
      }
      g->hyb_tab.upload(tab.data(), tab.size());
    }
    g->cl.crow_hyb = aasr::DevBuf<int32_t>();  // rebuilt on the next clustered pass
    return;
  }
}

void gmm_build_centred(aasr_gmm *g) {
  const HostModel &m = g->host;
  g->centred_ok = false;
  const int dimp = centred_dimp_for(m.dim);
  if (!dimp) return;
  g->centred_dimp = dimp;
  std::vector<int32_t> comps(m.mix_idx.size());
  for (size_t k = 0; k < comps.size(); k++) comps[k] = (int32_t)k;
  build_centred_tables(m, dimp, comps, m.mix_off, g->centred_recs, g->centred_state_off, g->centred_splits,
                       &g->centred_max_splits);
  g->centred_ok = true;
}

// the pool's Gaussians as one-record "states" of the centred kernel: the per-Gaussian view of a model
// the expanded form cannot hold
void gmm_build_pool_centred(aasr_gmm *g) {
  if (g->pool_centred_built) return;
  const HostModel &m = g->host;
  const int dimp = centred_dimp_for(m.dim);
  if (!dimp) raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", m.dim);
  std::vector<int32_t> comps((size_t)m.G), off((size_t)m.G + 1);
  for (int64_t i = 0; i < m.G; i++) comps[(size_t)i] = (int32_t)i;
  for (int64_t i = 0; i <= m.G; i++) off[(size_t)i] = (int32_t)i;
  if (!g->centred_dimp) g->centred_dimp = dimp;
  build_centred_tables(m, dimp, comps, off, g->poolc_recs, g->poolc_state_off, g->poolc_splits, &g->poolc_max_splits,
                       true);
  g->pool_centred_built = true;
}

}  // namespace aasr

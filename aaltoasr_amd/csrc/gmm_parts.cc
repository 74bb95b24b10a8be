// gmm_parts.cc -- multi-pivot models (pivot groups) and the planner that splits a model into engine parts.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>

#include "gmm_build.h"

namespace aasr {

// ---------------------------------------------------------------------------
// Multi-pivot models and engine parts.
//
// The expanded form  log2e ll = C + sum_d [p mu'] x' + [-p/2] x'^2  (x' = x - pivot) loses eps * kappa, kappa = sum_d p mu'^2
// (gmm.h, KAPPA_LIMIT_F16): how far a Gaussian's mean lies from the PIVOT in units of its own standard deviation.  One
// pivot for the whole pool -- the mean of the means -- is enough for the BASELINE model (means N(0, 1), variances >= 0.25),
// not for a model fitted to data: the tied states of a trained model partition the feature space, a state's Gaussians
// sit around the state's own centre with variances down to the floor (aku's --minvar), and against the pool's centre
// most of them exceed the two-term limits (synth.fit_model on the bench's own features: 39-57 % of the states qualify
// around one pivot, 91-96 % around 8, 97-99 % around 16).  The pivot is a property of the FRAME OPERAND, and a workgroup
// of the scoring kernel streams one contiguous run of rows past the operand it holds: so the states are sorted into
// PIVOT GROUPS, every group a run of whole tiles expanded around its own pivot, the frame operand gets one image per
// group (k_frame_operand, 320 B per frame and group), and a row cut never straddles two groups (build_split_table_pg).
// The output columns follow the sorted order (every group starts on a whole 128-byte line), consumers read a score row
// through a column map (gmm_engine_colmap); public-layout callers get the columns gathered back (gmm_score.hip, launch_engine_parts_public).
// ---------------------------------------------------------------------------
void build_pg_model(aasr_gmm *g) {
  HostModel &m = g->host;
  const int P = m.n_pg(), D = m.dim;
  if (P < 1 || P > PG_MAX || (int)m.pg_begin.size() != P + 1 || (int64_t)m.pg_pivot.size() != (int64_t)P * D ||
      m.pg_begin[0] != 0 || m.pg_begin[(size_t)P] != m.S || (m.pg_arith != 2 && m.pg_arith != 3 && m.pg_arith != 4))
    raise(AASR_ERR_INVALID, "malformed pivot groups");
  for (int p = 0; p < P; p++)
    if (m.pg_begin[(size_t)p] % 32 != 0 || m.pg_real_end[(size_t)p] <= m.pg_begin[(size_t)p] ||
        m.pg_real_end[(size_t)p] > m.pg_begin[(size_t)p + 1])
      raise(AASR_ERR_INVALID, "malformed pivot group %d", p);
  if (m.n_transforms > 0 || m.any_full() || D + 1 > 64)
    raise(AASR_ERR_UNSUPPORTED, "pivot groups are built for plain diagonal models of up to 63 dimensions");
  g->pivot = m.pg_pivot;
  g->d_pivot.upload(g->pivot.data(), g->pivot.size());
  g->class_models.clear();
  g->class_g2t.clear();
  g->full.ok = false;
  g->ill_conditioned = false;
  g->centred_ok = false;
  // conditioning of every component around its group's pivot
  double kmax = 0, k2max = 0;
  for (int64_t s = 0; s < m.S; s++) {
    const float *pv = &m.pg_pivot[(size_t)m.pg_of_state(s) * D];
    for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) {
      const int64_t gi = m.mix_idx[(size_t)k];
      double k2 = 0;
      const double kk = kappa_terms(&m.mean[(size_t)gi * D], &m.var[(size_t)gi * D], pv, D, &k2);
      kmax = std::max(kmax, kk);
      k2max = std::max(k2max, std::sqrt(k2));
    }
  }
  g->kappa = g->kappa_matrix = kmax;
  g->kappa2_matrix = k2max;
  g->mix = PackedRows();
  g->mix.rows = (int64_t)m.mix_idx.size();
  g->paired = TrackLayout();
  g->tracks = TrackLayout();
  g->f16_bad_state = -1;
  g->f16_state_ok.assign((size_t)m.S, 1);
  gmm_build_tracks(g, true);
  if (!g->paired.ok || (m.pg_arith != 3 ? !g->paired.a16h.p : !g->paired.a16.p))
    raise(AASR_ERR_UNSUPPORTED, "no grouped layout for the pivot groups (state %ld)", (long)g->f16_bad_state);
  g->precision = m.pg_arith != 3 ? AASR_PREC_F16X2 : AASR_PREC_BF16X3;
  g->use_bf16x3 = true;
  g->rows_unbiased = true;
  gmm_probe_f16x2(g);   // marks the states it rejects in f16_state_ok (the planner moves them)
}

namespace {
struct PgLimits { double k, k2; };

// worst conditioning of state s around pivot pv, relative to the limits (<= 1: every component qualifies)
double pg_state_ratio(const HostModel &m, int64_t s, const float *pv, const PgLimits &lim) {
  const int D = m.dim;
  double worst = 0;
  for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) {
    const int64_t gi = m.mix_idx[(size_t)k];
    double k2 = 0;
    const double kk = kappa_terms(&m.mean[(size_t)gi * D], &m.var[(size_t)gi * D], pv, D, &k2);
    worst = std::max(worst, std::max(kk / lim.k, std::sqrt(k2) / lim.k2));
    if (!(worst == worst)) return 1e300;
  }
  return worst;
}

// mean of the means of the Gaussians of `states` (one count per component), as floats
void pg_centre(const HostModel &m, const std::vector<int64_t> &states, std::vector<float> &out) {
  const int D = m.dim;
  std::vector<double> acc((size_t)D, 0.0);
  double n = 0;
  for (int64_t s : states)
    for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) {
      const double *mu = &m.mean[(size_t)m.mix_idx[(size_t)k] * D];
      for (int d = 0; d < D; d++) acc[(size_t)d] += mu[d];
      n += 1;
    }
  out.assign((size_t)D, 0.0f);
  if (n > 0)
    for (int d = 0; d < D; d++) out[(size_t)d] = (float)(acc[(size_t)d] / n);
}

struct PgPlan {
  std::vector<float> pivots;              // [P][D]
  std::vector<std::vector<int64_t>> groups;   // member states, ascending
  std::vector<int64_t> rejected;          // candidates that fit no group
};

// Greedy placement of pivots: start from the centre of all candidates; while states fail, try the centre of the worst
// failing state that qualifies around its OWN centre as a further pivot and keep it when the rows it rescues pay for
// one more image of the frame operand (`rows_per_pivot`).  Every state then goes to the pivot it is best conditioned
// around; group centres are re-fitted once where that loses no state.
PgPlan pg_plan(const HostModel &m, const std::vector<int64_t> &cand, const PgLimits &lim, double rows_per_pivot, int max_groups) {
  const int D = m.dim;
  PgPlan plan;
  if (cand.empty()) return plan;
  const size_t n = cand.size();
  std::vector<float> pv;
  pg_centre(m, cand, pv);
  plan.pivots = pv;
  std::vector<double> best(n);
  std::vector<int> grp(n, 0);
  std::vector<int64_t> comps(n);
  for (size_t i = 0; i < n; i++) {
    best[i] = pg_state_ratio(m, cand[i], pv.data(), lim);
    comps[i] = m.mix_off[cand[i] + 1] - m.mix_off[cand[i]];
  }
  std::vector<uint8_t> tried(n, 0);
  int P = 1;
  while (P < max_groups) {
    // candidates for one more pivot: the centres of the worst failing state and of a few others spread over the failing
    // ones; the one that rescues the most rows is taken
    std::vector<size_t> failing;
    int64_t fail_rows = 0;
    for (size_t i = 0; i < n; i++)
      if (best[i] > 1.0) {
        fail_rows += comps[i];
        if (!tried[i]) failing.push_back(i);
      }
    if (failing.empty()) break;
    std::sort(failing.begin(), failing.end(), [&](size_t a, size_t b) { return best[a] != best[b] ? best[a] > best[b] : a < b; });
    const size_t n_try = std::min<size_t>(8, failing.size());
    std::vector<float> c_best;
    std::vector<double> r_best;
    int64_t rescued_best = -1;
    for (size_t t = 0; t < n_try; t++) {
      const size_t pick = failing[t * failing.size() / n_try];
      std::vector<float> c;
      pg_centre(m, std::vector<int64_t>{cand[pick]}, c);
      if (pg_state_ratio(m, cand[pick], c.data(), lim) > 1.0) {   // fails around its own centre: not for this part
        tried[pick] = 1;
        continue;
      }
      std::vector<double> r(n);
      int64_t rescued = 0;
      for (size_t i = 0; i < n; i++) {
        r[i] = best[i] > 1.0 ? pg_state_ratio(m, cand[i], c.data(), lim) : 2.0;
        if (best[i] > 1.0 && r[i] <= 1.0) rescued += comps[i];
      }
      if (rescued > rescued_best) {
        rescued_best = rescued;
        c_best = c;
        r_best = r;
      }
    }
    tried[failing[0]] = 1;   // (the loop ends: the worst one is never tried twice)
    if (rescued_best < 0) continue;
    // the last failing rows are worth more than their share: they also cost a launch of their own
    const double bonus = rescued_best == fail_rows ? 2.0 : 1.0;
    if ((double)rescued_best * bonus < rows_per_pivot) continue;
    plan.pivots.insert(plan.pivots.end(), c_best.begin(), c_best.end());
    for (size_t i = 0; i < n; i++)
      if (best[i] > 1.0 && r_best[i] < best[i]) { best[i] = r_best[i]; grp[i] = P; }
    P++;
  }
  // re-fit every group's pivot to its members' centre where no member is lost
  for (int p = 0; p < P; p++) {
    std::vector<int64_t> mem;
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; i++)
      if (grp[i] == p && best[i] <= 1.0) { mem.push_back(cand[i]); idx.push_back(i); }
    if (mem.empty()) continue;
    std::vector<float> c;
    pg_centre(m, mem, c);
    std::vector<double> r(mem.size());
    bool ok = true;
    for (size_t j = 0; j < mem.size() && ok; j++) {
      r[j] = pg_state_ratio(m, mem[j], c.data(), lim);
      ok = r[j] <= 1.0;
    }
    if (!ok) continue;
    std::copy(c.begin(), c.end(), plan.pivots.begin() + (size_t)p * D);
    for (size_t j = 0; j < mem.size(); j++) best[idx[j]] = r[j];
  }
  // states that still fail may fit a re-fitted pivot
  for (size_t i = 0; i < n; i++) {
    if (best[i] <= 1.0) continue;
    for (int p = 0; p < P; p++) {
      const double r = pg_state_ratio(m, cand[i], &plan.pivots[(size_t)p * D], lim);
      if (r < best[i]) { best[i] = r; grp[i] = p; }
    }
  }
  std::vector<std::vector<int64_t>> groups((size_t)P);
  for (size_t i = 0; i < n; i++) {
    if (best[i] <= 1.0) groups[(size_t)grp[i]].push_back(cand[i]);
    else plan.rejected.push_back(cand[i]);
  }
  std::vector<float> piv2;
  for (int p = 0; p < P; p++) {
    if (groups[(size_t)p].empty()) continue;
    plan.groups.push_back(groups[(size_t)p]);
    piv2.insert(piv2.end(), plan.pivots.begin() + (size_t)p * D, plan.pivots.begin() + (size_t)(p + 1) * D);
  }
  plan.pivots = piv2;
  return plan;
}

// the states `groups` list (in that order; groups padded to whole lines of 32 columns) as a model of their own
HostModel pg_sub_model(const HostModel &m, const std::vector<std::vector<int64_t>> &groups, std::vector<int32_t> *col_of_state,
                       std::vector<int32_t> *parent_gauss = nullptr) {
  HostModel sm;
  sm.dim = m.dim;
  std::vector<int32_t> gmap((size_t)m.G, -1);
  sm.mix_off.push_back(0);
  auto add_state = [&](int64_t s) {
    if (s >= 0) {
      if (col_of_state) (*col_of_state)[(size_t)s] = (int32_t)sm.S;
      for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) {
        const int32_t gi = m.mix_idx[(size_t)k];
        if (gmap[(size_t)gi] < 0) {
          gmap[(size_t)gi] = (int32_t)sm.G++;
          sm.mean.insert(sm.mean.end(), m.mean.begin() + (size_t)gi * m.dim, m.mean.begin() + (size_t)(gi + 1) * m.dim);
          sm.var.insert(sm.var.end(), m.var.begin() + (size_t)gi * m.dim, m.var.begin() + (size_t)(gi + 1) * m.dim);
        }
        sm.mix_idx.push_back(gmap[(size_t)gi]);
        sm.mix_w.push_back(m.mix_w[(size_t)k]);
      }
    }
    sm.mix_off.push_back((int32_t)sm.mix_idx.size());
    sm.S++;
  };
  for (size_t p = 0; p < groups.size(); p++) {
    sm.pg_begin.push_back((int32_t)sm.S);
    for (int64_t s : groups[p]) add_state(s);
    sm.pg_real_end.push_back((int32_t)sm.S);
    if (p + 1 < groups.size())
      while (sm.S % 32) add_state(-1);   // padding columns: the next group starts on a whole line
  }
  sm.pg_begin.push_back((int32_t)sm.S);
  sm.weights_normalized = true;
  if (parent_gauss) {
    parent_gauss->assign((size_t)sm.G, 0);
    for (int64_t gi = 0; gi < m.G; gi++)
      if (gmap[(size_t)gi] >= 0) (*parent_gauss)[(size_t)gmap[(size_t)gi]] = (int32_t)gi;
  }
  if (sm.G == 0) {   // states without components only: the pool still needs an entry (no row points at it)
    sm.G = 1;
    sm.mean.assign((size_t)m.dim, 0.0);
    sm.var.assign((size_t)m.dim, 1.0);
  }
  return sm;
}
}  // namespace

// Splits the model into engine parts (aasr_gmm::engine_parts) when its own layouts cannot score every state with two
// fp16 terms around the pool's one pivot.
void gmm_plan_engine_parts(aasr_gmm *g) {
  g->engine_parts.clear();
  g->engine_colmap = DevBuf<int32_t>();
  g->engine_colmap_h.clear();
  g->engine_cols = 0;
  g->engine_plan_note.clear();
  std::string &note = g->engine_plan_note;
  auto say = [&](const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    note += buf;
  };
  const HostModel &m = g->host;
  if (g->is_engine_part || m.n_pg() > 0 || m.n_transforms > 0 || m.any_full() || !g->dim_parts.empty() ||
      g->class_routing || m.S < 2 || m.mix_idx.empty())
    return;
  // EXPERIMENT (tools/exp_calib.py): every state into ONE slab-constant part around the pool's pivot, whatever its conditioning
  static const int force_sc = AASR_EXPERIMENT_ENV("AASR_EXP_FORCE_SC") ? atoi(AASR_EXPERIMENT_ENV("AASR_EXP_FORCE_SC")) : 0;
  {
    const TrackLayout &L0 = g->paired.ok ? g->paired : g->tracks;
    // the whole model on two fp16 terms around one pivot: nothing to gain -- unless Gaussians were taken off the matrix
    // path to get there (outlier routing: the centred form costs several rows' time per row; a group's own pivot or the
    // slab-constant layout keeps most of them on the matrix cores)
    if (!force_sc && L0.ok && L0.a16h.p && !g->hyb_enabled && !g->ill_conditioned) return;
  }
  const int D = m.dim;
  const double rows_total = (double)m.mix_idx.size();
  // one more pivot costs what ~400 rows cost per frame (k_frame_operand: 0.05 ms per 449 280 frames and image against
  // 8.5 ms for 50 000 rows, + a row cut more per frame block, + a tile of padding); a row on two terms instead of three
  // saves 0.65 of a row, on three terms instead of the centred form several rows
  // AASR_PG_PIVOT_COST (test hook): the rows one more pivot has to rescue, instead of the cost model's figure
  // (read at every build, not latched: a test sets it for one model)
  const double pivot_cost_env = getenv("AASR_PG_PIVOT_COST") ? atof(getenv("AASR_PG_PIVOT_COST")) : -1.0;
  // (round 6: the second part is the slab-constant layout at 1.2 rows' cost, not three terms at 2: a pivot of the first part
  // has to rescue more rows to pay -- measured on the two fitted models of bench.py, engine path ms at 200 / 400 / 615 / 900 /
  // 1 300 / 2 000 rows per pivot: 10.92 / 10.83 / 10.76 / 10.74 / 10.62-10.71 / 10.76-10.80 and 11.25 / 11.02 / 10.90 / 10.87 /
  // 10.79-10.84 / 10.95: a flat minimum around 1 000)
  const double cost2 = pivot_cost_env >= 0 ? pivot_cost_env : 1000.0;
  const double pivot_cost3_env = getenv("AASR_PG_PIVOT_COST3") ? atof(getenv("AASR_PG_PIVOT_COST3")) : pivot_cost_env;   // (the second part's alone)
  const double cost3 = pivot_cost3_env >= 0 ? pivot_cost3_env : 400.0 / 4.0;
  static const double lim_scale = AASR_EXPERIMENT_ENV("AASR_PG_LIMIT_SCALE") ? atof(AASR_EXPERIMENT_ENV("AASR_PG_LIMIT_SCALE")) : 1.0;   // EXPERIMENT
  const PgLimits lim2{lim_scale * KAPPA_LIMIT_F16, lim_scale * (D < 8 ? KAPPA2_LIMIT_F16_LOWDIM : KAPPA2_LIMIT_F16)};
  // three terms around a group's pivot: the one-pivot form's limits (AASR_PG3_LIMIT_SCALE 1.0).  The round first admitted
  // 1.5 times those, every state probed on the device like the two-term rows -- but the probe's frames lie within 2.5
  // sigma, and on 512 frames of the bench's fitted models scored through the parts the part then showed 1.08e-4 (speech-like)
  // and 9.5e-5 (stationary) on values far below the frame's best; 1.25: 6.7e-5 and 1.62e-4; 1.0: 6.2e-5 and 4.3e-5, and the
  // findings of tools/fuzz_fitted.py on seeds 7 / 109 go from nine to five.  What fails the limits takes the remainder's
  // forms: the stationary model pays 0.46 ms for seven states that move there.
#ifndef AASR_PG3_LIMIT_SCALE
#define AASR_PG3_LIMIT_SCALE 1.0
#endif
  const PgLimits lim3{lim_scale * AASR_PG3_LIMIT_SCALE * KAPPA_LIMIT_SC, lim_scale * AASR_PG3_LIMIT_SCALE * KAPPA2_LIMIT_SC};
  std::vector<int64_t> cand;
  for (int64_t s = 0; s < m.S; s++) cand.push_back(s);
  std::vector<aasr_gmm::EnginePart> parts;
  std::vector<int32_t> colmap((size_t)m.S, -1);
  int64_t col0 = 0;
  int64_t probe_moved = 0;
  auto build_part = [&](const std::vector<std::vector<int64_t>> &groups, const std::vector<float> &pivots, int arith,
                        std::vector<int64_t> *probe_rejects) -> bool {
    std::vector<int32_t> cols((size_t)m.S, -1), pgauss;
    HostModel sm = pg_sub_model(m, groups, &cols, &pgauss);
    sm.pg_pivot = pivots;
    sm.pg_arith = arith;
    auto sub = std::make_unique<aasr_gmm>();
    sub->device = g->device;
    sub->is_engine_part = true;
    sub->parent_gauss = pgauss;
    try {
      gmm_build(sub.get(), sm);
    } catch (const Error &e) {
      if (e.code != AASR_ERR_UNSUPPORTED) throw;
      say("[arith %d, %zu groups: %s] ", arith, groups.size(), e.msg.c_str());
      if (probe_rejects && sub->f16_bad_state >= 0) {   // a state whose rows left the fp16 range: out, try again
        for (int64_t s = 0; s < m.S; s++)
          if (cols[(size_t)s] == (int32_t)sub->f16_bad_state) probe_rejects->push_back(s);
      }
      return false;
    }
    if (probe_rejects) {
      for (int64_t s = 0; s < m.S; s++)
        if (cols[(size_t)s] >= 0 && !sub->f16_state_ok[(size_t)cols[(size_t)s]]) probe_rejects->push_back(s);
      if (!probe_rejects->empty()) return false;
    }
    aasr_gmm::EnginePart part;
    part.col0 = col0;
    part.cols = (sub->S + 31) / 32 * 32;
    part.arith = arith;
    for (const auto &gr : groups) part.states += (int64_t)gr.size();
    for (int64_t s = 0; s < m.S; s++)
      if (cols[(size_t)s] >= 0) colmap[(size_t)s] = (int32_t)(col0 + cols[(size_t)s]);
    col0 += part.cols;
    part.model = std::move(sub);
    parts.push_back(std::move(part));
    return true;
  };
  // a plan's groups and pivots restricted to the states still in `pool` (the attempts after the first: a new plan means new
  // rows, new probe frames and new marginal rejects, and the attempts would run out on a part that is fine)
  auto restrict_plan = [&](const PgPlan &kept, const std::vector<int64_t> &pool) {
    PgPlan plan;
    std::vector<uint8_t> in_pool((size_t)m.S, 0);
    for (int64_t s : pool) in_pool[(size_t)s] = 1;
    for (size_t p = 0; p < kept.groups.size(); p++) {
      std::vector<int64_t> gr;
      for (int64_t s : kept.groups[p])
        if (in_pool[(size_t)s]) gr.push_back(s);
      if (gr.empty()) continue;
      plan.groups.push_back(gr);
      plan.pivots.insert(plan.pivots.end(), kept.pivots.begin() + (size_t)p * D, kept.pivots.begin() + (size_t)(p + 1) * D);
    }
    return plan;
  };
  // part 0: two fp16 terms
  if (!force_sc) {
    std::vector<int64_t> pool = cand, out;
    PgPlan kept0;
    for (int attempt = 0; attempt < 12 && !pool.empty(); attempt++) {
      PgPlan plan = attempt == 0 ? pg_plan(m, pool, lim2, cost2, PG_MAX) : restrict_plan(kept0, pool);
      kept0 = plan;
      say("[two terms, attempt %d: %zu candidates -> %zu groups, %zu rejected] ", attempt, pool.size(), plan.groups.size(),
          plan.rejected.size());
      out.insert(out.end(), plan.rejected.begin(), plan.rejected.end());
      if (plan.groups.empty()) { pool.clear(); break; }
      std::vector<int64_t> rejects;
      if (build_part(plan.groups, plan.pivots, 2, &rejects)) { pool.clear(); break; }
      if (rejects.empty()) {   // no layout at all: these states take the next part
        for (const auto &gr : plan.groups) out.insert(out.end(), gr.begin(), gr.end());
        pool.clear();
        break;
      }
      probe_moved += (int64_t)rejects.size();
      std::vector<uint8_t> rej((size_t)m.S, 0);
      for (int64_t s : rejects) rej[(size_t)s] = 1;
      out.insert(out.end(), rejects.begin(), rejects.end());
      pool.clear();
      for (const auto &gr : plan.groups)
        for (int64_t s : gr)
          if (!rej[(size_t)s]) pool.push_back(s);
      std::sort(pool.begin(), pool.end());
    }
    out.insert(out.end(), pool.begin(), pool.end());   // (what twelve attempts did not settle takes the next part)
    std::sort(out.begin(), out.end());
    cand = out;
  }
  // (states the model's own probe moved are normally rejected here again: the union is what is reported)
  g->f16_probe_moved = std::max(g->f16_probe_moved, probe_moved);
  if (parts.empty() && !force_sc) return;   // nothing qualifies for two terms around any pivot: the model's own paths
  // part 1: two fp16 terms in the slab-constant K layout (TrackLayout::sc): 6 slabs instead of 5 at 39 dimensions, and an
  // error that no longer grows with kappa.  (Round 5 had three bf16 terms here: twice a two-term row's cost, and --
  // tools/exp_calib.py -- no more accurate at the same kappa: the error is the accumulators', not the operands'.)
  if (!cand.empty() && 7 * 8 >= D) {
    std::vector<int64_t> pool = cand, out;
    PgPlan kept;
    for (int attempt = 0; attempt < 12 && !pool.empty(); attempt++) {
      PgPlan plan;
      if (force_sc) {
        plan.groups.push_back(pool);
        pg_centre(m, pool, plan.pivots);
      } else if (attempt == 0) {
        plan = pg_plan(m, pool, lim3, cost3, PG_MAX);
      } else {
        plan = restrict_plan(kept, pool);
      }
      kept = plan;
      say("[slab constants, attempt %d: %zu candidates -> %zu groups, %zu rejected] ", attempt, pool.size(), plan.groups.size(),
          plan.rejected.size());
      out.insert(out.end(), plan.rejected.begin(), plan.rejected.end());
      if (plan.groups.empty()) { pool.clear(); break; }
      std::vector<int64_t> rejects;
      if (build_part(plan.groups, plan.pivots, 4, &rejects)) { pool.clear(); break; }
      std::vector<uint8_t> rej((size_t)m.S, 0);
      for (int64_t s : rejects) rej[(size_t)s] = 1;
      if (rejects.empty())   // no layout at all
        for (const auto &gr : plan.groups)
          for (int64_t s : gr) rej[(size_t)s] = 1;
      probe_moved += (int64_t)rejects.size();
      pool.clear();
      for (const auto &gr : plan.groups)
        for (int64_t s : gr) (rej[(size_t)s] ? out : pool).push_back(s);
      std::sort(pool.begin(), pool.end());
    }
    out.insert(out.end(), pool.begin(), pool.end());   // (what twelve attempts did not settle)
    std::sort(out.begin(), out.end());
    cand = out;
  }
  // part 2: whatever is left, as an ordinary model
  if (!cand.empty()) {
    std::vector<int32_t> cols((size_t)m.S, -1), pgauss;
    HostModel sm = pg_sub_model(m, std::vector<std::vector<int64_t>>{cand}, &cols, &pgauss);
    sm.pg_begin.clear();
    sm.pg_real_end.clear();
    auto sub = std::make_unique<aasr_gmm>();
    sub->device = g->device;
    sub->is_engine_part = true;
    sub->parent_gauss = pgauss;
    gmm_build(sub.get(), sm);
    sub->precision = g->precision;
    sub->use_bf16x3 = g->use_bf16x3;
    // a remainder of two or three states is scored in the centred form as a whole: one launch (5 us per row and 449 280
    // frames: 0.68 ms measured for 128 rows, 0.17 for 32) instead of the matrix kernel + the centred kernel for its outliers
    // + their merge, each with the fixed costs of a launch over every frame block (0.4-0.5 ms whatever the part's size)
    if ((int64_t)sm.mix_idx.size() <= 48 && sub->centred_ok && !sub->ill_conditioned) {
      sub->ill_conditioned = true;
      sub->hyb_enabled = false;
    }
    aasr_gmm::EnginePart part;
    part.col0 = col0;
    part.cols = (sub->S + 31) / 32 * 32;
    part.arith = 0;
    part.states = (int64_t)cand.size();
    for (int64_t s = 0; s < m.S; s++)
      if (cols[(size_t)s] >= 0) colmap[(size_t)s] = (int32_t)(col0 + cols[(size_t)s]);
    col0 += part.cols;
    part.model = std::move(sub);
    parts.push_back(std::move(part));
  }
  for (int64_t s = 0; s < m.S; s++)
    if (colmap[(size_t)s] < 0) raise(AASR_ERR_INVALID, "engine parts: state %ld has no column", (long)s);
  g->engine_parts = std::move(parts);
  g->engine_cols = col0;
  g->engine_colmap_h = colmap;
  g->engine_colmap.upload(colmap.data(), colmap.size());
}

}  // namespace aasr

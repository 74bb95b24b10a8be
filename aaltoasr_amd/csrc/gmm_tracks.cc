// gmm_tracks.cc -- the track layouts of the in-register epilogue: reference exponent, row-cut tables, the
// three-term bf16 and two-term fp16 splits of the rows.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gmm_build.h"

namespace aasr {

// Track layouts for the in-register epilogue (k_gmm_diag_score_tracks).
//
// In a 32x32 MFMA accumulator block lane (n, h) holds, for frame column n, the
// 16 rows {8q + 4h + e : q < 4, e < 4}.  Rows are therefore laid out as two
// "tracks" h = 0/1 of 4-row quads (8 quad positions per track per 64-row
// tile), every state lives on ONE track over consecutive quads (padded to a
// quad with null rows), and each lane sums its own state's components straight
// out of its accumulator registers.  No running maximum is needed: a fixed
// reference 2^ref is folded into the constants, valid as long as every
// component's peak value (c_g + log w) leaves headroom in the f32 exponent.
//
//  grouped  (paired): states 2j / 2j+1 side by side on tracks 0 / 1 over the
//            same quads, so they finish together and results can be written 32
//            consecutive states per frame row.  Used when padding the shorter
//            partner costs <= 25 % extra rows (uniform models: nothing).
//  independent: each state goes to the currently shorter track; the tracks close
//            states independently and results are written per state.  Padding
//            is only the quad round-up.
//
// The reference exponent is chosen per model: as large as the peaks allow (cap
// 72), at least 56 so that components 2^16 below the 1e-50 state floor (2^-166)
// still land in the normal f32 range (v_exp_f32 flushes denormals).
static bool choose_reference(const HostModel &m, const std::vector<uint8_t> &outlier, double *ref_out) {
  const int D = m.dim;
  double max_peak_log2 = -INFINITY;
  for (size_t k = 0; k < m.mix_idx.size(); k++) {
    if (!outlier.empty() && outlier[(size_t)m.mix_idx[k]]) continue;  // scored in the centred form
    double peak = diag_log_sqrt_det(&m.var[(size_t)m.mix_idx[k] * D], D) + m.logw(k);
    if (std::isnan(peak) || peak == INFINITY) return false;
    max_peak_log2 = std::max(max_peak_log2, peak * kLog2e);
  }
  double ref = std::floor(std::min(kRefMax, kPeakMax - max_peak_log2));
  if (!(ref >= kRefMin)) return false;
  *ref_out = ref;
  return true;
}

// Row-split table: the tile range can be cut into R contiguous chunks that
// different workgroups score for the same frames (finer work quanta -> no tail
// round on the 256 CUs).  cand_* list the legal cut points (tile index and the
// number of states each track has closed before it); row R-1 of the table holds
// R+1 entries {tile, closes track 0, closes track 1, 0}.
static void build_split_table(DevBuf<int32_t> &splits, int *max_splits, int64_t tiles,
                              const std::vector<int64_t> &cand_tile, const std::vector<int64_t> &cand_k0,
                              const std::vector<int64_t> &cand_k1) {
  std::vector<int32_t> table((size_t)TRACK_MAX_SPLITS * (TRACK_MAX_SPLITS + 1) * 4, 0);
  *max_splits = 1;
  for (int R = 1; R <= TRACK_MAX_SPLITS; R++) {
    std::vector<size_t> pick{0};
    bool ok = true;
    for (int i = 1; i < R && ok; i++) {
      double want = (double)cand_tile.front() + (double)tiles * i / R;
      size_t best = pick.back();
      double bd = 1e300;
      for (size_t c = pick.back() + 1; c + 1 < cand_tile.size(); c++) {
        double d = std::fabs((double)cand_tile[c] - want);
        if (d < bd) { bd = d; best = c; }
      }
      if (best == pick.back()) ok = false;
      pick.push_back(best);
    }
    if (!ok) break;
    pick.push_back(cand_tile.size() - 1);
    int64_t worst = 0;
    for (int i = 0; i < R; i++) worst = std::max(worst, cand_tile[pick[i + 1]] - cand_tile[pick[i]]);
    if ((double)worst > 1.25 * (double)tiles / R + 1) break;  // too uneven
    int32_t *row = &table[(size_t)(R - 1) * (TRACK_MAX_SPLITS + 1) * 4];
    for (int i = 0; i <= R; i++) {
      row[4 * i] = (int32_t)cand_tile[pick[i]];
      row[4 * i + 1] = (int32_t)cand_k0[pick[i]];
      row[4 * i + 2] = (int32_t)cand_k1[pick[i]];
    }
    *max_splits = R;
  }
  splits.upload(table.data(), table.size());
}

// The same for a multi-pivot layout: every pivot group is a run of whole tiles that starts at a legal cut point
// (cand_pg >= 0 there: the group's index), a cut must not straddle two groups, so the table has rows for R = P ...
// PG_MAX_SPLITS only; the R - P cuts beyond the groups' own go, one at a time, to the group whose pieces are longest.
// Entry [3] of a cut is the pivot group of the piece that starts there.
static void build_split_table_pg(TrackLayout &L, const std::vector<int64_t> &cand_tile, const std::vector<int64_t> &cand_k0,
                                 const std::vector<int64_t> &cand_k1, const std::vector<int> &cand_pg, int P) {
  const int cap = PG_MAX_SPLITS;
  std::vector<int32_t> table((size_t)cap * (cap + 1) * 4, 0);
  std::vector<size_t> gs;   // candidate index where each group starts, + the last candidate
  for (size_t c = 0; c + 1 < cand_tile.size(); c++)
    if (cand_pg[c] >= 0) gs.push_back(c);
  gs.push_back(cand_tile.size() - 1);
  L.max_splits = 0;
  L.split_cap = cap;
  if ((int)gs.size() != P + 1) return;
  for (int R = P; R <= cap; R++) {
    std::vector<int> n((size_t)P, 1);
    bool ok = true;
    for (int extra = 0; extra < R - P && ok; extra++) {
      int best = -1;
      double bl = 0;
      for (int gi = 0; gi < P; gi++) {
        if ((size_t)n[(size_t)gi] >= gs[(size_t)gi + 1] - gs[(size_t)gi]) continue;   // no cut point left inside
        const double len = (double)(cand_tile[gs[(size_t)gi + 1]] - cand_tile[gs[(size_t)gi]]) / n[(size_t)gi];
        if (len > bl) { bl = len; best = gi; }
      }
      if (best < 0) ok = false;
      else n[(size_t)best]++;
    }
    if (!ok) break;
    std::vector<size_t> pick;
    for (int gi = 0; gi < P && ok; gi++) {
      const size_t c0 = gs[(size_t)gi], c1 = gs[(size_t)gi + 1];
      const double t0 = (double)cand_tile[c0], span = (double)(cand_tile[c1] - cand_tile[c0]);
      pick.push_back(c0);
      for (int i = 1; i < n[(size_t)gi] && ok; i++) {
        const double want = t0 + span * i / n[(size_t)gi];
        size_t best = pick.back();
        double bd = 1e300;
        for (size_t c = pick.back() + 1; c < c1; c++) {
          const double d = std::fabs((double)cand_tile[c] - want);
          if (d < bd) { bd = d; best = c; }
        }
        if (best == pick.back()) ok = false;
        pick.push_back(best);
      }
    }
    if (!ok) break;
    pick.push_back(cand_tile.size() - 1);
    int32_t *row = &table[(size_t)(R - 1) * (cap + 1) * 4];
    int cur_pg = 0;
    for (int i = 0; i <= R; i++) {
      if (cand_pg[pick[(size_t)i]] >= 0) cur_pg = cand_pg[pick[(size_t)i]];
      row[4 * i] = (int32_t)cand_tile[pick[(size_t)i]];
      row[4 * i + 1] = (int32_t)cand_k0[pick[(size_t)i]];
      row[4 * i + 2] = (int32_t)cand_k1[pick[(size_t)i]];
      row[4 * i + 3] = cur_pg;
    }
    L.max_splits = R;
  }
  L.splits.upload(table.data(), table.size());
}

// Three-term bf16 split of the coefficient rows for the bf16x3 kernel.  coef64
// is [rows][2*D+1] in the f32 kernel's K order (k = 2d linear, 2d+1 quadratic,
// 2D constant); the split-term kernels put the constant first (k = 0; the f16x2
// form keeps its remainder at k = 1) and the dimensions' pairs behind it.
static void pack_bf16x3(int D, const std::vector<double> &coef64, int64_t tiles, TrackLayout &L) {
  int nk16 = (2 * (D + 1) + 15) / 16;  // KH = 8*nk16 >= D+1
  while (8 * nk16 < D + 1) nk16++;
  static const int inst[] = {1, 2, 3, 4, 5, 6, 8};
  int pick = -1;
  for (int c : inst)
    if (c >= nk16) { pick = c; break; }
  if (pick < 0) return;  // no instance: layout stays f32-only
  nk16 = pick;
  const int KH = 8 * nk16;
  const size_t tile_elems = (size_t)nk16 * 3 * 2 * 64 * 8;
  std::vector<uint16_t> a((size_t)tiles * tile_elems, 0);
  const size_t stride = 2 * (size_t)D + 1;
  for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
    const double *c = &coef64[(size_t)r * stride];
    for (int k = 0; k < 2 * KH; k++) {
      // K order of the split-term kernels: the constant, (f16x2: its remainder,) then coef64's own interleaved order
      const double v = k == 0 ? c[2 * D] : (k >= 2 && k - 2 < 2 * D ? c[k - 2] : 0.0);
      float x = (float)v, b1, b2, b3;
      uint16_t h1 = bf16_rne(x, &b1);
      uint16_t h2 = bf16_rne(x - b1, &b2);
      uint16_t h3 = bf16_rne((x - b1) - b2, &b3);
      const uint16_t hs[3] = {h1, h2, h3};
      for (int sp = 0; sp < 3; sp++) a[split_tile_index(nk16, 3, r, k, sp)] = hs[sp];
    }
  }
  L.a16.upload(a.data(), a.size());
  L.nk16 = nk16;
}

// Two-term fp16 split of the same rows for the f16x2 form (AASR_PREC_F16X2): same K order and tile layout with two
// splits; the constant's remainder after its two terms goes to K slot 1 (the frame operand is 1 in both).
// Covers the tiles [0, tiles) of the layout; rows with
// rs.g < 0 (and every row of a state that is not in `st_ok`, when given) are null rows.  Returns false -- and packs
// nothing -- when a value leaves the fp16 range, or when a frame component clamped at kF16Clamp from the pivot could
// still be visible above the 1e-50 floor for some row (the clamp must never change a result the reference's float
// storage holds); `bad_state` then names the state of the first offending row (-1: no single state to blame).
static bool pack_f16x2(const aasr_gmm *g, const std::vector<RowSpec> &rows, const std::vector<int32_t> &row_state,
                       const std::vector<double> &coef64, int64_t tiles, TrackLayout &L, int64_t *bad_state) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const int nk16 = L.nk16;
  const bool sc = L.sc;
  L.a16h = DevBuf<uint16_t>();
  L.f16tab = DevBuf<float>();
  *bad_state = -1;
  if (nk16 <= 0) return false;
  const int KH = 8 * nk16;
  if (sc ? 7 * nk16 < D : 2 * D + 1 >= 2 * KH) return false;  // no room (plain: no spare slot for the constant's remainder)
  const size_t tile_elems = (size_t)nk16 * 2 * 2 * 64 * 8;
  std::vector<uint16_t> a((size_t)tiles * tile_elems, 0);
  const size_t stride = 2 * (size_t)D + 1;
  auto bits = [](_Float16 h) {
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
  };
  // K slots.  Plain: 0 the constant, 1 its remainder, dimension d: 2 + 2 d (linear), 3 + 2 d (quadratic).  Slab-constant
  // (TrackLayout::sc): slab j = slots 16 j ..: its constant share, the remainder, then dimensions 7 j .. 7 j + 6.
  const int n_cslab = sc ? (D + 6) / 7 : 1;          // slabs that carry a constant
  const int base_slab = sc ? n_cslab - 1 : 0;        // ... and the one with peak + log w + reference (and the null marker)
  auto lin_slot = [&](int d) { return sc ? 16 * (d / 7) + 2 + 2 * (d % 7) : 2 + 2 * d; };
  auto const_slot = [&](int j) { return sc ? 16 * j : 0; };
  // kind of slot k: 0 constant of slab *j, 1 its remainder, 2 linear / 3 quadratic term of dimension *d, 4 unused
  auto slot_kind = [&](int k, int *j, int *d) {
    if (!sc) {
      *j = 0;
      if (k == 0) return 0;
      if (k == 1) return 1;
      *d = (k - 2) / 2;
      return *d < D ? 2 + ((k - 2) & 1) : 4;
    }
    *j = k / 16;
    const int q = k % 16;
    if (*j >= n_cslab) return 4;
    if (q == 0) return 0;
    if (q == 1) return 1;
    *d = 7 * *j + (q - 2) / 2;
    return *d < D ? 2 + (q & 1) : 4;
  };
  // the constants of a row's slabs (log2 units); null / zero-weight rows: the marker only
  std::vector<double> cs((size_t)n_cslab);
  auto slab_constants = [&](const double *c, bool *null_row) {
    std::fill(cs.begin(), cs.end(), 0.0);
    *null_row = !(c[2 * D] > -1.0e29);
    if (*null_row) return;
    if (!sc) {
      cs[0] = c[2 * D];
      return;
    }
    double base = c[2 * D];
    for (int d = 0; d < D; d++) {
      const double lin = c[2 * d], quad = c[2 * d + 1];
      const double h = quad < 0 ? lin * lin / (-4.0 * quad) : 0.0;   // 1/2 p mu'^2 log2e
      cs[(size_t)(d / 7)] -= h;
      base += h;
    }
    cs[(size_t)base_slab] += base;
  };
  // Per-column power-of-two scales: column k of the rows is divided by 2^s_k and the frame operand multiplied by it
  // (exact).  An fp16 `lo` term is a subnormal when its value is below 0.25, and a subnormal carries an ABSOLUTE error
  // of 3e-8 -- multiplied by the other operand: with a variance-floored Gaussian's -p/2 = -7 200 against x'^2 = 0.004
  // that was 1.6e-4 (tools/fuzz_parity.py 3102, iteration 78).  Scaling every column so that its largest coefficient
  // sits at 128 bounds that product: 3e-8 x 128 from a subnormal frame term, 3e-8 x (largest term / 128) from a
  // subnormal coefficient next to a large one.
  const int NG = std::max(1, m.n_pg());   // pivot groups: every group has its own column scales and clamps
  std::vector<double> max_a((size_t)NG * 2 * KH, 0.0);
  for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
    if (rows[(size_t)r].g < 0) continue;
    const double *c = &coef64[(size_t)r * stride];
    bool null_row = false;
    slab_constants(c, &null_row);
    if (null_row) continue;   // zero-weight row: its constant is the null marker
    double *ma = &max_a[(size_t)rows[(size_t)r].pg * 2 * KH];
    for (int k = 0; k < 2 * KH; k++) {
      int j = 0, d = 0;
      const int kind = slot_kind(k, &j, &d);
      double v = 0;
      if (kind == 0) v = std::fabs(cs[(size_t)j]);
      else if (kind == 1) v = std::fabs(cs[(size_t)j]) * 0x1p-22;   // the constant's remainder after two fp16 terms
      else if (kind == 2) v = std::fabs(c[2 * d]);
      else if (kind == 3) v = std::fabs(c[2 * d + 1]);
      ma[(size_t)k] = std::max(ma[(size_t)k], v);
    }
  }
  const int KB = const_slot(base_slab);   // the column that also carries the null rows' marker
  std::vector<int> sk((size_t)NG * 2 * KH, 0);
  std::vector<float> tab((size_t)NG * 3 * KH, 0.0f);   // per group: [2 KH] frame-operand scales 2^s_k, [KH] clamp of |x - pivot|
  for (int gi = 0; gi < NG; gi++) {
    int *skg = &sk[(size_t)gi * 2 * KH];
    float *tabg = &tab[(size_t)gi * 3 * KH];
    for (int k = 0; k < 2 * KH; k++) {
      int e = 0;
      if (max_a[(size_t)gi * 2 * KH + k] > 0) e = (int)std::ceil(std::log2(max_a[(size_t)gi * 2 * KH + k] / 128.0));
      // the marker's column carries the null rows' -60000 as well: its scale must leave 2^(-60000 * 2^s) = 0 in f32
      // (a model whose live constants are all tiny would otherwise get s = -14 and a null row worth 2^-3.7)
      e = std::max(k == KB ? -8 : -14, std::min(14, e));
      skg[(size_t)k] = e;
      tabg[(size_t)k] = (float)std::ldexp(1.0, e);
    }
    for (int d = 0; d < D; d++) {
      // one clamp per dimension keeps x' 2^s and x'^2 2^s inside the fp16 range
      const double x_lin = 60000.0 * std::ldexp(1.0, -skg[(size_t)lin_slot(d)]);
      const double x_quad = std::sqrt(60000.0 * std::ldexp(1.0, -skg[(size_t)(lin_slot(d) + 1)]));
      tabg[(size_t)2 * KH + d] = (float)(0.99 * std::min((double)kF16Clamp, std::min(x_lin, x_quad)));
    }
  }
  std::vector<double> rem((size_t)n_cslab);
  for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
    const double *c = &coef64[(size_t)r * stride];
    const RowSpec &rs = rows[(size_t)r];
    const int *skg = &sk[(size_t)rs.pg * 2 * KH];
    const float *tabg = &tab[(size_t)rs.pg * 3 * KH];
    if (rs.g >= 0) {
      // clamp guarantee: peak - 1/2 p (clamp - |mu'|)^2 far below the floor in every dimension
      const double peak = diag_log_sqrt_det(&m.var[(size_t)rs.g * D], D) + rs.logw;
      for (int d = 0; d < D; d++) {
        const double v = m.var[(size_t)rs.g * D + d];
        const double p = v > 0 ? 1 / v : 0;
        const double reach = (double)tabg[(size_t)2 * KH + d] -
                             std::fabs(m.mean[(size_t)rs.g * D + d] - (double)g->pivot[(size_t)rs.pg * D + d]);
        if (!(reach > 0) || !(peak - 0.5 * p * reach * reach < -160.0)) {
          *bad_state = row_state[(size_t)r];
          return false;
        }
      }
    }
    bool null_row = false;
    slab_constants(c, &null_row);
    std::fill(rem.begin(), rem.end(), 0.0);
    for (int k = 0; k < 2 * KH; k++) {
      int j = 0, d = 0;
      const int kind = slot_kind(k, &j, &d);
      double coef = 0;
      if (kind == 0) coef = cs[(size_t)j];
      else if (kind == 1) coef = rem[(size_t)j];
      else if (kind == 2) coef = null_row ? 0.0 : c[2 * d];
      else if (kind == 3) coef = null_row ? 0.0 : c[2 * d + 1];
      double v = std::ldexp(coef, kind == 1 ? 0 : -skg[(size_t)k]);
      // null / zero-weight rows carry kNullConst: any constant whose 2^x is zero in f32 does
      if (k == KB && null_row) v = -60000.0;
      if (!(std::fabs(v) <= 60000.0)) {
        *bad_state = rs.g >= 0 ? row_state[(size_t)r] : -1;
        return false;
      }
      const _Float16 h1 = (_Float16)v;
      const _Float16 h2 = (_Float16)(v - (double)h1);
      // what the two terms left of a constant goes to the remainder's slot (the next one) in that slot's own scale
      if (kind == 0) rem[(size_t)j] = null_row ? 0.0 : std::ldexp((v - (double)h1) - (double)h2, skg[(size_t)k] - skg[(size_t)k + 1]);
      const uint16_t hs[2] = {bits(h1), bits(h2)};
      for (int sp = 0; sp < 2; sp++) a[split_tile_index(nk16, 2, r, k, sp)] = hs[sp];
    }
  }
  if (m.n_pg() > 0) L.pg_tab.upload(tab.data(), tab.size());
  L.a16h.upload(a.data(), a.size());
  L.f16tab.upload(tab.data(), (size_t)3 * KH);   // (the first group's: what single-pivot launches read)
  return true;
}

// Which states the two-term fp16 form may score (gmm.h, KAPPA_LIMIT_F16): every Gaussian of the state that stays on
// the matrix path is below the conditioning limits.  Range and clamp conditions are checked when the rows are packed.
void f16x2_state_eligibility(const aasr_gmm *g, std::vector<uint8_t> &ok) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const double lim2 = m.dim < 8 ? KAPPA2_LIMIT_F16_LOWDIM : KAPPA2_LIMIT_F16;
  std::vector<uint8_t> g_ok((size_t)m.G, 1);
  for (int64_t i = 0; i < m.G; i++) {
    if (!g->outlier.empty() && g->outlier[(size_t)i]) continue;   // a null row in every matrix layout
    double k2 = 0;
    const double k = kappa_terms(&m.mean[(size_t)i * D], &m.var[(size_t)i * D], g->pivot.data(), D, &k2);
    g_ok[(size_t)i] = k <= KAPPA_LIMIT_F16 && std::sqrt(k2) <= lim2;
  }
  ok.assign((size_t)m.S, 1);
  for (int64_t s = 0; s < m.S; s++)
    for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++)
      if (!g_ok[(size_t)m.mix_idx[k]]) ok[(size_t)s] = 0;
}

// Builds the grouped (paired) or the independent track layout (the header of this section).
static void build_track_layout(aasr_gmm *g, TrackLayout &L, bool grouped) {
  const HostModel &m = g->host;
  L.ok = false;
  L.grouped = grouped;
  L.states_f16 = 0;
  L.n_pg = 0;
  L.split_cap = TRACK_MAX_SPLITS;
  const int P = m.n_pg();   // pivot groups (engine-internal multi-pivot models): grouped layouts only
  if (P > 0 && !grouped) return;
  double ref = 0;
  if (!choose_reference(m, g->outlier, &ref)) return;
  L.ref_ln = (float)(ref * 0.69314718055994530942);
  const int64_t rows_real = std::max<int64_t>(1, (int64_t)m.mix_idx.size());

  // ---- the states, ascending (one "section": the index is kept for the cut candidates)
  std::vector<int64_t> order[1];
  std::vector<int> st_pg;   // pivot group of every state
  if (P > 0) st_pg.resize((size_t)m.S);
  for (int64_t s = 0; s < m.S; s++) {
    if (P > 0) {
      const int pgi = m.pg_of_state(s);
      st_pg[(size_t)s] = pgi;
      if (s >= m.pg_real_end[(size_t)pgi]) continue;   // a padding column: no rows, never closed
    }
    order[0].push_back(s);
  }
  const int n_sec = 1;

  // ---- placement: (track, first quad) per state; close events; cut candidates per section
  std::vector<int8_t> st_track((size_t)m.S);
  std::vector<int64_t> st_pos((size_t)m.S);
  int64_t len[2] = {0, 0};
  int64_t closed[2] = {0, 0};
  struct Cand { std::vector<int64_t> tile, k0, k1; std::vector<int> pg; };   // pg: the pivot group that starts there, -1: none
  Cand cand[1];
  struct PairEv { int64_t s0, s1, last; bool f16, f32; };   // grouped: the pair's states, its last quad, its flush flags
  std::vector<PairEv> pairs;
  int64_t sec_tile[3] = {0, 0, 0};
  int64_t quads_used = 0;   // quad positions before the sections were rounded up to whole tiles
  auto quads_of = [&](int64_t s) {
    return std::max<int64_t>(1, ((int64_t)(m.mix_off[s + 1] - m.mix_off[s]) + 3) / 4);
  };
  auto sec_grouped = [&](int) { return grouped; };
  for (int sc = 0; sc < n_sec; sc++) {
    const std::vector<int64_t> &st = order[sc];
    cand[sc].tile.push_back(std::max(len[0], len[1]) / 8);
    cand[sc].k0.push_back(closed[0]);
    cand[sc].k1.push_back(closed[1]);
    cand[sc].pg.push_back(P > 0 ? 0 : -1);
    int cur_pg = 0;
    if (sec_grouped(sc)) {
      // Pairs are formed inside groups of 16 output columns: (16 g, 16 g + 1), ... (a lone last state takes a pair with an
      // empty partner track).  A group is staged and flushed as whole lines.
      size_t i = 0;
      while (i < st.size()) {
        const int64_t a = st[i];
        if (P > 0 && st_pg[(size_t)a] != cur_pg) {
          // a pivot group starts: on a whole tile (the groups are runs of whole tiles), on a whole line of output
          // columns (the close counters jump to the group's first column), at a cut point of its own
          cur_pg = st_pg[(size_t)a];
          const int64_t top = (len[0] + 7) / 8 * 8;
          len[0] = len[1] = top;
          closed[0] = closed[1] = m.pg_begin[(size_t)cur_pg] / 2;
          if (cand[sc].tile.back() == top / 8 && cand[sc].tile.size() > 1) {
            cand[sc].k0.back() = closed[0];
            cand[sc].k1.back() = closed[1];
            cand[sc].pg.back() = cur_pg;
          } else {
            cand[sc].tile.push_back(top / 8);
            cand[sc].k0.push_back(closed[0]);
            cand[sc].k1.push_back(closed[1]);
            cand[sc].pg.push_back(cur_pg);
          }
        }
        int64_t b = -1;
        if (i + 1 < st.size() && (st[i + 1] >> 4) == (a >> 4)) b = st[i + 1];
        const size_t nxt = i + (b >= 0 ? 2 : 1);
        int64_t q = quads_of(a);
        if (b >= 0) q = std::max(q, quads_of(b));
        st_track[(size_t)a] = 0;
        st_pos[(size_t)a] = len[0];
        if (b >= 0) {
          st_track[(size_t)b] = 1;
          st_pos[(size_t)b] = len[0];
        }
        len[0] += q;
        len[1] = len[0];
        closed[0]++;
        closed[1]++;
        const bool end = nxt >= st.size();
        const bool f16 = end || (st[nxt] >> 4) != (a >> 4);
        const bool f32 = end || (st[nxt] >> 5) != (a >> 5);
        pairs.push_back({a, b, len[0] - 1, f16, f32});
        if (len[0] % 8 == 0 && f32 && !end) {
          cand[sc].tile.push_back(len[0] / 8);
          cand[sc].k0.push_back(closed[0]);
          cand[sc].k1.push_back(closed[1]);
          cand[sc].pg.push_back(-1);
        }
        i = nxt;
      }
    } else {
      // cut candidates are created by padding both tracks to a tile boundary
      // roughly every 1/32 of the expected length
      int64_t total_quads = 0;
      for (int64_t s : st) total_quads += quads_of(s);
      const int64_t sync_every = std::max<int64_t>(64, total_quads / 2 / 32);
      int64_t next_sync = std::max(len[0], len[1]) + sync_every;
      for (size_t i = 0; i < st.size(); i++) {
        const int64_t s = st[i];
        int h = len[1] < len[0] ? 1 : 0;
        st_track[(size_t)s] = (int8_t)h;
        st_pos[(size_t)s] = len[h];
        len[h] += quads_of(s);
        closed[h]++;
        if (std::min(len[0], len[1]) >= next_sync && i + 1 < st.size()) {
          int64_t top = (std::max(len[0], len[1]) + 7) / 8 * 8;
          len[0] = len[1] = top;
          cand[sc].tile.push_back(top / 8);
          cand[sc].k0.push_back(closed[0]);
          cand[sc].k1.push_back(closed[1]);
          cand[sc].pg.push_back(-1);
          next_sync = top + sync_every;
        }
      }
    }
    // a section ends on a tile boundary
    quads_used += std::max(len[0], len[1]) - sec_tile[sc] * 8;
    const int64_t top = (std::max(len[0], len[1]) + 7) / 8 * 8;
    len[0] = len[1] = top;
    int64_t end_tile = top / 8;
    if (sc == n_sec - 1) end_tile = std::max<int64_t>(1, end_tile);
    if (cand[sc].tile.back() == end_tile && cand[sc].tile.size() > 1 && cand[sc].pg.back() < 0) {  // the end is always the last boundary
      cand[sc].tile.pop_back();
      cand[sc].k0.pop_back();
      cand[sc].k1.pop_back();
      cand[sc].pg.pop_back();
    }
    cand[sc].tile.push_back(end_tile);
    cand[sc].k0.push_back(closed[0]);
    cand[sc].k1.push_back(closed[1]);
    cand[sc].pg.push_back(-1);
    sec_tile[sc + 1] = end_tile;
  }
  const int64_t tiles = std::max<int64_t>(1, sec_tile[n_sec]);
  if (grouped && (double)(quads_used * 8) > 1.25 * (double)rows_real + 64 * (n_sec + P)) return;  // too much padding

  // ---- rows, close bits, per-track state lists / pair table
  std::vector<RowSpec> rows((size_t)tiles * TILE_ROWS, RowSpec{-1, 0.0, 0.0});
  std::vector<int32_t> row_state((size_t)tiles * TILE_ROWS, -1);
  std::vector<uint16_t> close_mask((size_t)tiles, 0);
  std::vector<int32_t> sid[2];
  for (int sc = 0; sc < n_sec; sc++)
    for (int64_t s : order[sc]) {
      const int h = st_track[(size_t)s];
      const int64_t p0 = st_pos[(size_t)s];
      const int32_t a = m.mix_off[s], b = m.mix_off[s + 1];
      for (int32_t k = a; k < b; k++) {
        if (!g->outlier.empty() && g->outlier[(size_t)m.mix_idx[k]]) continue;  // stays a null row
        const int64_t r = track_row(p0 + (k - a) / 4, h, (k - a) % 4);
        rows[(size_t)r] = RowSpec{m.mix_idx[k], m.logw((size_t)k), ref, P > 0 ? st_pg[(size_t)s] : 0};
        row_state[(size_t)r] = (int32_t)s;
      }
      if (!sec_grouped(sc)) {
        const int64_t last = p0 + quads_of(s) - 1;
        close_mask[(size_t)(last / 8)] |= (uint16_t)(1u << (last % 8 + 8 * h));
        sid[h].push_back((int32_t)s);
      }
    }
  if (grouped) {
    // a pair closes where its longer member ends; both tracks carry the bit (the kernels read track 0's)
    for (const PairEv &pe : pairs) {
      close_mask[(size_t)(pe.last / 8)] |= (uint16_t)((1u << (pe.last % 8)) | (1u << (pe.last % 8 + 8)));
      sid[0].push_back((int32_t)pe.s0);
      if (pe.s1 >= 0) sid[1].push_back((int32_t)pe.s1);
    }
  }
  const size_t ns = std::max(sid[0].size(), sid[1].size()) + 1;
  std::vector<int32_t> sid_flat(2 * ns, 0);
  for (int h = 0; h < 2; h++)
    for (size_t k = 0; k < sid[h].size(); k++) sid_flat[h * ns + k] = sid[h][k];
  L.sid_stride = (int32_t)ns;
  L.sid.upload(sid_flat.data(), sid_flat.size());
  // row-cut table
  if (P > 0) {
    build_split_table_pg(L, cand[0].tile, cand[0].k0, cand[0].k1, cand[0].pg, P);
    if (L.max_splits < P) return;
    L.n_pg = P;
    L.pg_pivot.upload(m.pg_pivot.data(), m.pg_pivot.size());
    L.pg_colend.upload(m.pg_real_end.data(), m.pg_real_end.size());
  } else {
    build_split_table(L.splits, &L.max_splits, tiles, cand[0].tile, cand[0].k0, cand[0].k1);
  }
  std::vector<double> coef64;
  pack_rows(g, rows, L.rows, &coef64);
  L.sc = P > 0 && m.pg_sc();
  if (L.sc) {
    // slab-constant layout: seven dimensions per slab, two fp16 terms only
    L.a16 = DevBuf<uint16_t>();
    L.nk16 = 0;
    for (int c : {1, 2, 3, 4, 5, 6, 8})
      if (7 * c >= m.dim) { L.nk16 = c; break; }
  } else {
    pack_bf16x3(m.dim, coef64, tiles, L);
  }
  static const int f16_env = AASR_EXPERIMENT_ENV("AASR_F16X2") ? atoi(AASR_EXPERIMENT_ENV("AASR_F16X2")) : 1;   // 0: never pack the f16x2 form
  L.a16h = DevBuf<uint16_t>();
  int64_t bad_state = -1;
  if (P > 0 && m.pg_arith == 3) {
    // a three-term multi-pivot model: no fp16 rows
  } else if (P == 0 && g->f16_whole_rejected) {
    // the load-time probe rejected states of this model: the whole-model two-term rows stay away
  } else if (f16_env && (P > 0 ||   // (a multi-pivot model: the planner put only states that qualify here)
                         (g->kappa_matrix <= KAPPA_LIMIT_F16 &&
                          g->kappa2_matrix <= (m.dim < 8 ? KAPPA2_LIMIT_F16_LOWDIM : KAPPA2_LIMIT_F16)))) {
    if (pack_f16x2(g, rows, row_state, coef64, tiles, L, &bad_state)) L.states_f16 = m.S;
    else g->f16_bad_state = bad_state;
  }
  L.rows.rows = (int64_t)m.mix_idx.size();  // real rows (algorithmic work)
  close_mask.push_back(0);  // the kernels read the bits as aligned 32-bit words (scalar loads)
  L.close.upload(close_mask.data(), close_mask.size());
  L.rows_padded = tiles * TILE_ROWS;
  L.ref_log2 = ref;
  L.row_gauss.resize(rows.size());
  for (size_t r = 0; r < rows.size(); r++) L.row_gauss[r] = (int32_t)rows[r].g;
  L.ok = true;
}

void gmm_build_tracks(aasr_gmm *g, bool grouped) { build_track_layout(g, grouped ? g->paired : g->tracks, grouped); }

}  // namespace aasr

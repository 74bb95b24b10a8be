// gmm_model.cc -- host-side build of the device-resident model: the f32 tile packers, gmm_build (validate, reset,
// dispatch to the layout builders of gmm_tracks.cc / gmm_parts.cc / gmm_centred.cc / gmm_fullcov.cc), the model as
// dimension parts, class routing, gmm_set_transforms and the f64 / per-Gaussian operands.
//
// Constants: DiagonalGaussian::set_constant (aku/Distributions.cc:1273-1288) -- no (2*pi)^(-d/2) term.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gmm_build.h"

namespace aasr {

// ---------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------

// Writes explicit coefficient rows (coef[r][k], k = 2*kk + h) into the tile
// layout; rows beyond n_rows are zero.
void pack_coef_rows(int nkk, const std::vector<double> &coef, int64_t n_rows, PackedRows &out) {
  out.nkk = nkk;
  out.rows = n_rows;
  out.tiles = std::max<int64_t>(1, (n_rows + TILE_ROWS - 1) / TILE_ROWS);
  const size_t tile_floats = (size_t)(nkk / 2) * 64 * 4;
  const size_t K = 2 * (size_t)nkk;
  std::vector<float> a((size_t)out.tiles * tile_floats, 0.0f);
  for (int64_t r = 0; r < n_rows; r++)
    for (int kk = 0; kk < nkk; kk++)
      for (int h = 0; h < 2; h++) a[coef_tile_index(nkk, r, kk, h)] = (float)coef[(size_t)r * K + 2 * kk + h];
  out.a.upload(a.data(), a.size());
}

// Write rows into the [tiles][nkk/2][64][4] layout the kernel streams (coef_tile_index)
// with K index k = 2*kk + h:  kk<dim: h=0 -> p*mu'*log2e, h=1 -> -p/2*log2e;
// kk==dim: h=0 -> constant*log2e; everything else 0.
void pack_rows(const aasr_gmm *g, const std::vector<RowSpec> &rows, PackedRows &out, std::vector<double> *a64_host,
               bool upload_f32) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const int nkk = pick_nkk(D);
  if (nkk < 0)
    raise(AASR_ERR_UNSUPPORTED, "feature dimension %d > 63 is not built in this engine yet", D);
  out.nkk = nkk;
  out.rows = (int64_t)rows.size();
  out.tiles = std::max<int64_t>(1, (out.rows + TILE_ROWS - 1) / TILE_ROWS);
  const size_t tile_floats = (size_t)(nkk / 2) * 64 * 4;
  std::vector<float> a((size_t)out.tiles * tile_floats, 0.0f);
  if (a64_host) a64_host->assign((size_t)out.tiles * TILE_ROWS * (2 * D + 1), 0.0);
  std::vector<double> coef(2 * (size_t)nkk);
  for (int64_t r = 0; r < out.tiles * TILE_ROWS; r++) {
    std::fill(coef.begin(), coef.end(), 0.0);
    if (r < out.rows && rows[(size_t)r].g >= 0) {
      const RowSpec &rs = rows[(size_t)r];
      const double *mu = &m.mean[(size_t)rs.g * D];
      const double *var = &m.var[(size_t)rs.g * D];
      const double cst = diag_log_sqrt_det(var, D);
      double quad = 0;
      for (int d = 0; d < D; d++) {
        double p = (var[d] > 0) ? 1 / var[d] : 0;
        double muc = mu[d] - (double)g->pivot[(size_t)rs.pg * D + d];
        coef[2 * d] = p * muc * kLog2e;
        coef[2 * d + 1] = -0.5 * p * kLog2e;
        quad += p * muc * muc;
      }
      double c = cst + rs.logw - 0.5 * quad;
      if (!std::isfinite(c)) {
        if (c > 0 || std::isnan(c))
          raise(AASR_ERR_INVALID,
                "Gaussian %ld has a non-finite constant (precision product overflow)", (long)rs.g);
        coef[2 * D] = kNullConst;
      } else {
        coef[2 * D] = c * kLog2e + rs.bias;
      }
    } else {
      coef[2 * D] = kNullConst;  // padding row: contributes exp2(-1e30 - max) = 0
    }
    for (int kk = 0; kk < nkk; kk++)
      for (int h = 0; h < 2; h++) a[coef_tile_index(nkk, r, kk, h)] = (float)coef[2 * kk + h];
    if (a64_host)
      for (int k = 0; k < 2 * D + 1; k++)
        (*a64_host)[(size_t)r * (2 * D + 1) + k] = coef[k];
  }
  out.a.upload(a.data(), a.size());
}

// dim > 63: parts of <= 63 dimensions as pools of one-component states (see aasr_gmm::dim_parts)
static void build_dim_split(aasr_gmm *g) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const int n_parts = (D + 62) / 63;
  const int per = (D + n_parts - 1) / n_parts;
  g->dim_part_off.clear();
  for (int p = 0; p < n_parts; p++) g->dim_part_off.push_back(std::min(D, p * per));
  g->dim_part_off.push_back(D);
  for (int p = 0; p < n_parts; p++) {
    const int d0 = g->dim_part_off[(size_t)p], d1 = g->dim_part_off[(size_t)p + 1];
    HostModel pm;
    pm.dim = d1 - d0;
    pm.G = m.G;
    pm.S = m.G;
    pm.mean.resize((size_t)m.G * pm.dim);
    pm.var.resize((size_t)m.G * pm.dim);
    for (int64_t i = 0; i < m.G; i++)
      for (int d = d0; d < d1; d++) {
        pm.mean[(size_t)i * pm.dim + (d - d0)] = m.mean[(size_t)i * D + d];
        pm.var[(size_t)i * pm.dim + (d - d0)] = m.var[(size_t)i * D + d];
      }
    pm.mix_off.resize((size_t)m.G + 1);
    pm.mix_idx.resize((size_t)m.G);
    pm.mix_w.assign((size_t)m.G, 1.0);
    for (int64_t i = 0; i <= m.G; i++) pm.mix_off[(size_t)i] = (int32_t)i;
    for (int64_t i = 0; i < m.G; i++) pm.mix_idx[(size_t)i] = (int32_t)i;
    pm.weights_normalized = true;
    auto sub = std::make_unique<aasr_gmm>();
    sub->device = g->device;
    gmm_build(sub.get(), pm);
    g->dim_parts.push_back(std::move(sub));
  }
  std::vector<float> logw(m.mix_idx.size());
  for (size_t k = 0; k < m.mix_idx.size(); k++) logw[k] = (float)m.logw(k);
  g->dim_mix_off.upload(m.mix_off.data(), m.mix_off.size());
  g->dim_mix_idx.upload(m.mix_idx.data(), std::max<size_t>(1, m.mix_idx.size()));
  g->dim_mix_logw.upload(logw.data(), std::max<size_t>(1, logw.size()));
}

// Per-class constrained MLLR on a diagonal pool (ConstrainedMllr, aku/ModelModules.cc:164-232;
// AdaptedGaussian::compute_likelihood = g(A f + b) * |det|, aku/ModelModules.hh:172-173, det = the
// product of A's diagonal, aku/LinearAlgebra.cc:73-86): see class_routing in gmm.h.
static void build_class_routing(aasr_gmm *g) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const int nc = m.n_transforms + 1;
  g->mix.rows = (int64_t)m.mix_idx.size();
  g->paired.ok = g->tracks.ok = g->centred_ok = false;
  g->full.ok = false;
  g->ill_conditioned = false;
  if (g->class_g2t != m.g2t || (int)g->class_models.size() != nc) {
    // sub-models: the components of every state that belong to the class, over the class's own pool
    g->class_models.clear();
    g->class_models.resize((size_t)nc);
    for (int c = 0; c < nc; c++) {
      const int tid = c - 1;
      std::vector<int32_t> remap((size_t)m.G, -1);
      HostModel sm;
      sm.dim = D;
      sm.S = m.S;
      sm.weights_normalized = true;  // the parent's weights are final: no second normalisation
      sm.mix_off.assign(1, 0);
      for (int64_t s = 0; s < m.S; s++) {
        for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) {
          const int32_t gi = m.mix_idx[k];
          if (m.g2t[(size_t)gi] != tid) continue;
          if (remap[(size_t)gi] < 0) {
            remap[(size_t)gi] = (int32_t)sm.G++;
            sm.mean.insert(sm.mean.end(), &m.mean[(size_t)gi * D], &m.mean[(size_t)gi * D] + D);
            sm.var.insert(sm.var.end(), &m.var[(size_t)gi * D], &m.var[(size_t)gi * D] + D);
          }
          sm.mix_idx.push_back(remap[(size_t)gi]);
          sm.mix_w.push_back(m.mix_w[k]);
        }
        sm.mix_off.push_back((int32_t)sm.mix_idx.size());
      }
      if (sm.mix_idx.empty()) continue;
      auto sub = std::make_unique<aasr_gmm>();
      sub->device = g->device;
      sub->parent_gauss.assign((size_t)sm.G, -1);
      for (int64_t gi = 0; gi < m.G; gi++)
        if (remap[(size_t)gi] >= 0) sub->parent_gauss[(size_t)remap[(size_t)gi]] = (int32_t)gi;
      gmm_build(sub.get(), sm);
      g->class_models[(size_t)c] = std::move(sub);
    }
    g->class_g2t = m.g2t;
  }
  // this speaker's transforms
  g->class_a.resize((size_t)nc);
  g->class_b.resize((size_t)nc);
  g->class_logdet.assign((size_t)nc, 0.0);
  for (int c = 1; c < nc; c++) {
    const double *W = &m.xform[(size_t)(c - 1) * D * (D + 1)];
    std::vector<double> A((size_t)D * D), b((size_t)D);
    const double det = split_transform(W, D, A.data(), b.data());
    g->class_a[(size_t)c].upload(A.data(), A.size());
    g->class_b[(size_t)c].upload(b.data(), b.size());
    g->class_logdet[(size_t)c] = det != 0 ? std::log(std::fabs(det)) : -INFINITY;
  }
  g->class_routing = true;
}

// Sets (W = [b | A], one matrix) or clears (W = nullptr) the pool's one frame transform: the frames are transformed
// once before scoring (gmm_adapted_frames).  Returns log|det| for the caller to put where its rows want it: into
// aasr_gmm::out_bias_ln (rows packed without a bias) or HostModel::logw_bias (folded into every weight); -inf for a
// zero on the diagonal: every state at the floor.
static double set_frame_transform(aasr_gmm *g, const double *W) {
  g->xf_a.release();
  g->xf_b.release();
  if (!W) return 0;
  const int D = g->host.dim;
  std::vector<double> A((size_t)D * D), b((size_t)D);
  const double det = split_transform(W, D, A.data(), b.data());
  g->xf_a.upload(A.data(), A.size());
  g->xf_b.upload(b.data(), b.size());
  return std::log(std::fabs(det));
}

// What gmm_build refuses, before it touches the handle
static void validate_model(const HostModel &m) {
  if (m.dim <= 0 || m.G <= 0 || m.S <= 0)
    raise(AASR_ERR_INVALID, "empty model (dim %d, %ld Gaussians, %ld states)", m.dim, (long)m.G, (long)m.S);
  if ((int64_t)m.mix_off.size() != m.S + 1)
    raise(AASR_ERR_INVALID, "mix_off must hold num_states+1 entries");
  if (m.dim + 1 > 64 && m.any_full())
    raise(AASR_ERR_UNSUPPORTED, "feature dimension %d > 63 is built for diagonal pools only", m.dim);
  for (size_t k = 0; k < m.mix_idx.size(); k++)
    if (m.mix_idx[k] < 0 || m.mix_idx[k] >= m.G)
      raise(AASR_ERR_INVALID, "mixture component %zu points at Gaussian %d outside the pool of %ld",
            k, m.mix_idx[k], (long)m.G);
  if (m.n_transforms > 0) {
    if ((int64_t)m.g2t.size() != m.G ||
        (int64_t)m.xform.size() != (int64_t)m.n_transforms * m.dim * (m.dim + 1))
      raise(AASR_ERR_INVALID, "transform arrays do not match the model");
    for (int32_t t : m.g2t)
      if (t < -1 || t >= m.n_transforms) raise(AASR_ERR_INVALID, "transform index %d out of range", t);
  }
  if (m.n_pg() == 0 && m.any_full() &&
      ((int64_t)m.cov.size() != m.G * m.dim * m.dim || (int64_t)m.is_full.size() != m.G))
    raise(AASR_ERR_INVALID, "covariance array does not match the pool size");
}

// The general layout (aasr_gmm::mix): component-expanded rows in state order + the segment descriptors of the
// chunked epilogue
static void build_mix_rows(aasr_gmm *g) {
  const HostModel &m = g->host;
  std::vector<RowSpec> rows;
  rows.reserve(m.mix_idx.size());
  std::vector<int32_t> chunk_seg_begin;
  std::vector<uint32_t> seg_desc;
  std::vector<int32_t> seg_out;
  int64_t total_rows = (int64_t)m.mix_idx.size();
  int64_t n_chunks = std::max<int64_t>(1, (total_rows + TILE_ROWS - 1) / TILE_ROWS) * (TILE_ROWS / CHUNK_ROWS);
  std::vector<std::vector<std::pair<uint32_t, int32_t>>> per_chunk((size_t)n_chunks);
  int64_t row = 0;
  for (int64_t s = 0; s < m.S; s++) {
    int32_t a = m.mix_off[s], b = m.mix_off[s + 1];
    if (b <= a) {
      // a state without components scores the floor; emit a zero-length
      // closing segment so the column is still written
      int64_t c = std::min<int64_t>(row / CHUNK_ROWS, n_chunks - 1);
      uint32_t rb = (uint32_t)(row - c * CHUNK_ROWS);
      if (rb > CHUNK_ROWS) rb = CHUNK_ROWS;
      per_chunk[(size_t)c].push_back({rb | (rb << 8), (int32_t)s});
      continue;
    }
    for (int32_t k = a; k < b; k++) {
      const bool out_k = !g->outlier.empty() && g->outlier[(size_t)m.mix_idx[k]];
      rows.push_back({out_k ? (int64_t)-1 : (int64_t)m.mix_idx[k], m.logw((size_t)k)});
    }
    int64_t r0 = row, r1 = row + (b - a);
    for (int64_t c = r0 / CHUNK_ROWS; c * CHUNK_ROWS < r1; c++) {
      int64_t lo = std::max(r0, c * CHUNK_ROWS), hi = std::min(r1, (c + 1) * CHUNK_ROWS);
      uint32_t desc = (uint32_t)(lo - c * CHUNK_ROWS) | ((uint32_t)(hi - c * CHUNK_ROWS) << 8);
      if (lo > r0) desc |= 1u << 16;  // continues a segment opened in an earlier chunk
      if (hi < r1) desc |= 1u << 17;  // stays open into the next chunk
      per_chunk[(size_t)c].push_back({desc, (int32_t)s});
    }
    row = r1;
  }
  chunk_seg_begin.push_back(0);
  for (auto &v : per_chunk) {
    for (auto &p : v) {
      seg_desc.push_back(p.first);
      seg_out.push_back(p.second);
    }
    chunk_seg_begin.push_back((int32_t)seg_desc.size());
  }
  pack_rows(g, rows, g->mix, nullptr);
  g->mix.chunk_seg_begin.upload(chunk_seg_begin.data(), chunk_seg_begin.size());
  g->mix.seg_desc.upload(seg_desc.data(), seg_desc.size());
  g->mix.seg_out.upload(seg_out.data(), seg_out.size());
}

void gmm_build(aasr_gmm *g, const HostModel &model) {
  require_device();
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      g->num_cus = cus;
  }
  // ---- validate
  validate_model(model);
  g->host = model;
  HostModel &m = g->host;
  // Mixture::normalize_weights (Distributions.cc:2067-2075) -- once: a rebuild (CMLLR,
  // model cache) must not divide by a sum that is already 1 +- 1 ulp
  if (!m.weights_normalized) {
    for (int64_t s = 0; s < m.S; s++) {
      double sum = 0;
      for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) sum += m.mix_w[k];
      for (int32_t k = m.mix_off[s]; k < m.mix_off[s + 1]; k++) m.mix_w[k] /= sum;
    }
    m.weights_normalized = true;
  }
  // ---- reset: what every kind of model starts from (class_models stay: build_class_routing keeps them where the
  // classes' membership has not changed)
  g->dim = m.dim;
  g->G = m.G;
  g->S = m.S;
  g->outlier.clear();
  g->hyb_enabled = false;
  g->hyb_states = g->hyb_rows = 0;
  g->f16_probe_moved = 0;
  g->f16_whole_rejected = false;
  g->rows_unbiased = false;
  g->dim_parts.clear();
  g->engine_parts.clear();
  g->engine_colmap = DevBuf<int32_t>();
  g->engine_colmap_h.clear();
  g->engine_cols = 0;
  g->class_routing = false;
  m.logw_bias = 0;
  g->out_bias_ln = set_frame_transform(g, nullptr);
  // ---- dispatch
  if (m.n_pg() > 0) {
    build_pg_model(g);
    return;
  }
  const bool wide = m.dim + 1 > 64;   // scored as dimension parts (gmm_dim_split_score)
  if (!wide) {
    // centring pivot: per-dimension mean of the pool means, rounded to float so
    // the device subtracts exactly the value the constants were built with
    g->pivot.assign(m.dim, 0.0f);
    for (int d = 0; d < m.dim; d++) {
      double acc = 0;
      for (int64_t i = 0; i < m.G; i++) acc += m.mean[(size_t)i * m.dim + d];
      g->pivot[d] = (float)(acc / (double)m.G);
    }
    g->d_pivot.upload(g->pivot.data(), g->pivot.size());
  }
  if (m.n_transforms > 0 && !m.global_xform() && !m.any_full()) {
    // regression classes on a diagonal pool: every class is a model over its own Gaussians and adapted frames
    build_class_routing(g);
    return;
  }
  g->class_models.clear();
  g->class_g2t.clear();
  if (wide) {
    // the model as dimension parts; one transform for the whole pool: the frames transformed once, log|det| at the output
    build_dim_split(g);
    if (m.global_xform()) g->out_bias_ln = set_frame_transform(g, m.xform.data());
    return;
  }
  if (m.factor_path()) {
    // full-covariance Gaussians and per-class CMLLR are scored through factor
    // rows by k_gmm_full_score only
    g->mix.rows = (int64_t)m.mix_idx.size();
    g->paired.ok = g->tracks.ok = g->centred_ok = false;
    gmm_build_fullcov(g);
    return;
  }
  g->full.ok = false;
  // one transform for every Gaussian == transform the frames once, add log|det| (folded into the weights)
  if (m.global_xform()) m.logw_bias = set_frame_transform(g, m.xform.data());

  find_outliers(g);
  build_mix_rows(g);
  g->f16_bad_state = -1;
  gmm_build_tracks(g, true);
  if (!g->paired.ok) gmm_build_tracks(g, false);
  // which states could take the plain two-term rows around the pool's one pivot (the probe and the planner of the engine
  // parts start from it)
  f16x2_state_eligibility(g, g->f16_state_ok);
  if (g->f16_bad_state >= 0) g->f16_state_ok[(size_t)g->f16_bad_state] = 0;   // range / clamp failure of one state's rows
  gmm_build_centred(g);
  g->rows_unbiased = m.logw_bias == 0;
  // profiling hook: AASR_LAYOUTS=<mask> restricts the kernels like
  // aasr_debug_set_layouts (1 grouped, 2 independent tracks, 4 centred, 0 general)
  if (const char *e = getenv("AASR_PREC")) {
    g->use_bf16x3 = atoi(e) == AASR_PREC_BF16X3 || atoi(e) == AASR_PREC_F16X2;
    g->precision = g->use_bf16x3 ? atoi(e) : AASR_PREC_F32;
    if (atoi(e) == AASR_PREC_F64 && !m.any_full()) g->precision = AASR_PREC_F64;  // the tools' switch to the reference's arithmetic
  }
  if (const char *e = AASR_EXPERIMENT_ENV("AASR_LAYOUTS")) {
    g->layout_mask = atoi(e);
    if ((g->layout_mask & 2) && !g->tracks.ok) gmm_build_tracks(g, false);
  }
  gmm_probe_f16x2(g);   // load-time guard of the two-term fp16 rows
  gmm_plan_engine_parts(g);
}

void gmm_set_transforms(aasr_gmm *g, int32_t n_transforms, const int32_t *gauss_to_transform, const double *W) {
  HostModel &cur = g->host;
  const int D = cur.dim;
  bool global = n_transforms == 1;
  if (global)
    for (int64_t i = 0; i < cur.G && global; i++) global = gauss_to_transform[i] == 0;
  // In place: none / one transform for the whole pool, over rows packed without a bias, on the
  // kernels that take the bias at their output (the track layouts; the centred form through an extra pass; outlier
  // routing adds it to the centred share when it merges).  A
  // speaker change then costs two small uploads instead of re-packing every row (70 ms at 50 k
  // Gaussians).  A model of more than 63 dimensions (the model as parts, gmm_dim_split_score) always takes it: the frames
  // transformed once and |det| on every component; it keeps its pool_built / pool_centred_built flags as they are.
  const bool dim_split = !g->dim_parts.empty();
  if ((n_transforms == 0 || global) &&
      (dim_split || (g->rows_unbiased && !cur.any_full() && !g->class_routing &&
                     (g->paired.ok || g->tracks.ok || (g->ill_conditioned && g->centred_ok))))) {
    cur.n_transforms = n_transforms;
    cur.g2t.clear();
    cur.xform.clear();
    if (!dim_split) g->pool_built = g->pool_centred_built = false;
    g->f64_built = false;
    if (n_transforms > 0) {
      cur.g2t.assign(gauss_to_transform, gauss_to_transform + cur.G);
      cur.xform.assign(W, W + (size_t)D * (D + 1));
    }
    g->out_bias_ln = set_frame_transform(g, n_transforms > 0 ? W : nullptr);
    return;
  }
  // everything else is a rebuild (regression classes: as class sub-models, gmm_build)
  HostModel m = cur;
  m.n_transforms = 0;
  m.g2t.clear();
  m.xform.clear();
  g->pool_built = false;
  g->pool_centred_built = false;
  g->f64_built = false;
  if (global && !m.any_full() && !g->rows_unbiased) {
    // coming from per-class transforms or from rows with a folded bias: build the unadapted rows
    // once, then take the in-place path if this model can (the usual case)
    gmm_build(g, m);
    if (g->rows_unbiased && (g->paired.ok || g->tracks.ok || (g->ill_conditioned && g->centred_ok))) {
      gmm_set_transforms(g, n_transforms, gauss_to_transform, W);
      return;
    }
  }
  m.n_transforms = n_transforms;
  if (n_transforms > 0) {
    m.g2t.assign(gauss_to_transform, gauss_to_transform + m.G);
    m.xform.assign(W, W + (size_t)n_transforms * D * (D + 1));
  }
  gmm_build(g, m);
}

// AASR_PREC_F64 operands: per mixture component the reference's own quantities in double --
// mean, precision (1 / variance, 0 for a non-positive variance), the constant log sqrt(prod
// precision) (0 when the product is not positive: the "invalid" Gaussian,
// aku/Distributions.cc:1117-1135) and the normalised mixture weight.
void gmm_build_f64(aasr_gmm *g, bool any_dim) {
  const HostModel &m = g->host;
  const int D = m.dim;
  // (asked again on records that a caller with any_dim built: the kernels with dimension instances still refuse)
  if (D > 192 && !any_dim) raise(AASR_ERR_UNSUPPORTED, "no f64 kernel instance for dimension %d", D);
  if (g->f64_built) return;
  // the frame vector is a per-lane array of doubles, instances up to 192 dimensions.  What the compiler makes of it in
  // k_stats_items (code object notes, tests/test_kernel_notes.py): in registers without scratch up to <128> (255 VGPRs
  // at <96>, 256 + 82 AGPRs at <128>); <192> would need 384 for the frame alone, takes all 512 (256 + 256 AGPRs) and
  // still spills 97 VGPRs, 248 bytes of scratch per lane
  // beyond them (any_dim: a kernel whose loops run over the dimension from memory) the records are padded to whole 8s
  const int dimp = D <= 64 ? centred_dimp_for(D) : D <= 96 ? 96 : D <= 128 ? 128 : D <= 192 ? 192 : (D + 7) / 8 * 8;
  const int rec = 2 * dimp + 2;
  const size_t K = m.mix_idx.size();
  std::vector<double> recs(std::max<size_t>(K, 1) * rec, 0.0);
  for (size_t k = 0; k < K; k++) {
    const int64_t gi = m.mix_idx[k];
    for (int d = 0; d < D; d++) {
      const double v = m.var[(size_t)gi * D + d];
      recs[k * rec + d] = m.mean[(size_t)gi * D + d];
      recs[k * rec + dimp + d] = v > 0 ? 1 / v : 0;
    }
    recs[k * rec + 2 * dimp] = diag_log_sqrt_det(&m.var[(size_t)gi * D], D);
    recs[k * rec + 2 * dimp + 1] = m.mix_w[k];
  }
  g->f64_recs.upload(recs.data(), recs.size());
  g->f64_state_off.upload(m.mix_off.data(), m.mix_off.size());
  g->f64_det = 1.0;
  if (m.n_transforms > 0 && m.global_xform()) {
    std::vector<double> A((size_t)D * D), b((size_t)D);
    const double det = split_transform(m.xform.data(), D, A.data(), b.data());
    g->f64_A.upload(A.data(), A.size());
    g->f64_b.upload(b.data(), b.size());
    g->f64_det = std::fabs(det);
  }
  g->f64_classes = 0;
  if (m.n_transforms > 0 && !m.global_xform()) {
    // regression classes: class c = transform c - 1 (class 0: Gaussians without one); per class
    // A, b and |prod diag A| as above, per record the class of its Gaussian
    const int nc = m.n_transforms + 1;
    std::vector<double> A((size_t)nc * D * D, 0.0), b((size_t)nc * D, 0.0), det((size_t)nc, 1.0);
    for (int i = 0; i < D; i++) A[(size_t)i * D + i] = 1.0;  // class 0: identity
    for (int t = 0; t < m.n_transforms; t++)
      det[(size_t)t + 1] = std::fabs(split_transform(&m.xform[(size_t)t * D * (D + 1)], D, &A[(size_t)(t + 1) * D * D],
                                                     &b[(size_t)(t + 1) * D]));
    std::vector<int32_t> rc(std::max<size_t>(K, 1), 0);
    for (size_t k = 0; k < K; k++) rc[k] = m.g2t[(size_t)m.mix_idx[k]] + 1;
    g->f64_class_A.upload(A.data(), A.size());
    g->f64_class_b.upload(b.data(), b.size());
    g->f64_class_det.upload(det.data(), det.size());
    g->f64_rec_class.upload(rc.data(), rc.size());
    g->f64_classes = nc;
  }
  g->f64_dimp = dimp;
  g->f64_built = true;
}

void gmm_build_pool(aasr_gmm *g) {
  if (g->pool_built) return;
  std::vector<RowSpec> rows((size_t)g->G);
  for (int64_t i = 0; i < g->G; i++) rows[(size_t)i] = {i, 0.0};
  pack_rows(g, rows, g->pool, nullptr);
  g->pool_built = true;
}

}  // namespace aasr

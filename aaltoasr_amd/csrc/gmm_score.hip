// gmm_score.hip -- frame x Gaussian scoring kernels for gfx950 (MI355X).
//
// Replaces the per-frame loop
//   HmmSet::precompute_likelihoods        aku/HmmSet.cc:484-501
//     PDFPool::precompute_likelihoods     aku/Distributions.cc:2663-2682
//       DiagonalGaussian::compute_log_likelihood   :1040-1062  (+ exp :1033)
//     Mixture::compute_likelihood         aku/Distributions.cc:2078-2086
// with one launch over a block of frames.
//
// Formulation.  ll_g(x) = c_g - 1/2 sum_d p_gd (x_d - mu_gd)^2 is expanded
// around a per-dimension pivot v (x' = x - v, mu' = mu - v) into a dense
// contraction over K = 2*dim + 1 (+ the constant's remainder in the split forms):
//     log2e * ll = sum_d [p mu' log2e] x'_d + [-p/2 log2e] x'_d^2 + C_g * 1
// so the frame x Gaussian quadratic forms are a GEMM on the matrix cores with the
// mixture log-sum-exp fused behind it, frame-stationary: a wave keeps the K x 64
// operand of its 64 frames in registers, the Gaussian rows stream past through LDS.
//
// The files of the scoring unit, and which kernel serves what.  Every kernel instance is instantiated in
// exactly one of them (tools/kernel_notes.py --digest lists them all; tests/test_kernel_notes.py checks it):
//   gmm_score_common.h     what more than one of them uses, and the launchers called across the files
//   gmm_score_f32.hip      k_gmm_diag_score           f32 MFMA, LDS-staged epilogue: any layout (diagnostic) and the per-Gaussian view
//                          k_gmm_diag_score_tracks    AASR_PREC_F32: f32 MFMA, track layouts, in-register epilogue
//   gmm_score_pl.h         k_gmm_diag_score_pl        AASR_PREC_F16X2 (the default; what bench.py times) and BF16X3 up to five slabs: the
//                                                     software-pipelined kernel; + k_frame_operand, the row cuts, launch_split
//   gmm_score_f16x2.hip    ... its two-term instances (launch_split<2>); the phase trace of experiment builds
//   gmm_score_bf16x3.hip   ... its three-term instances (launch_split<3>), and
//                          k_gmm_diag_score_bf16x3    AASR_PREC_BF16X3 beyond five K slabs (39 dimensions): phase-shifted wave groups
//   gmm_score_full.hip     k_gmm_full_score[_bf16x3]  full-covariance pools (f32 / two fp16 / three bf16 terms)
//   gmm_score_exact.hip    k_gmm_diag_score_centred, k_outlier_merge   beyond every expanded form's limits: no MFMA; outlier routing
//                          k_gmm_diag_score_f64[_classes]              AASR_PREC_F64: the reference's arithmetic in double
//   gmm_score.hip (here)   launch_bf16 (the precision chooser), gmm_probe_f16x2 (load-time guard of the two-term form), then the
//                          dispatch: transforms, classes, engine parts, dimension parts, gmm_score_launch*, gmm_gauss_launch
#include <hip/hip_runtime.h>
#include <mutex>
#include <unordered_map>

#include <cmath>
#include <cstdlib>

#include "gmm_score_common.h"

namespace aasr {

// the split-operand kernel the handle's precision asks for (f16x2 only where the layout is eligible)
static bool launch_bf16(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                        float *d_out, hipStream_t stream, const ClusterArgs *cl = nullptr, int64_t pitch = 0) {
  if (g->precision == AASR_PREC_F16X2 && L.a16h.p && launch_split<2>(g, L, d_frames, F, d_out, stream, cl, pitch))
    return true;
  return launch_split<3>(g, L, d_frames, F, d_out, stream, cl, pitch);
}

// Verdicts of the probe, keyed by what it depends on (the model's arrays, pivots, the rows' eligibility, the round and the
// tolerance): a rebuild of the same content -- a second handle on the same files, a transform that is taken off again, a
// sub-model rebuilt for a speaker whose classes did not change -- takes the verdict instead of scoring the probe frames
// again.  Process-wide, bounded (256 entries), under a mutex.
namespace {
struct ProbeCache {
  std::mutex mu;
  std::unordered_map<uint64_t, std::vector<int32_t>> verdicts;   // key -> states rejected in that round
  int64_t runs = 0, hits = 0;
};
ProbeCache &probe_cache() {
  static ProbeCache c;
  return c;
}
inline uint64_t fnv1a(const void *p, size_t n, uint64_t h) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n; i++) {
    h ^= b[i];
    h *= 0x100000001b3ull;
  }
  return h;
}
template <typename T>
inline uint64_t fnv_vec(const std::vector<T> &v, uint64_t h) {
  const uint64_t n = v.size();
  h = fnv1a(&n, sizeof n, h);
  return v.empty() ? h : fnv1a(v.data(), v.size() * sizeof(T), h);
}
}  // namespace
// Diagnostic (tests): device runs of the probe and verdicts taken from the cache since the library was loaded
extern "C" void aasr_debug_probe_counts(int64_t *runs, int64_t *hits) {
  ProbeCache &c = probe_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  if (runs) *runs = c.runs;
  if (hits) *hits = c.hits;
}

// ---------------------------------------------------------------------------
// Load-time guard of the two-term fp16 form.  Which states get it is decided by conditioning limits that were set
// from sweeps (gmm.h, KAPPA_LIMIT_F16): a bound in the statistical sense, not a proof.  So every model that got fp16
// rows is probed once when it is built: frames placed on its own Gaussians -- 0.5 to 2.5 sigma out in every dimension,
// and one dimension at a time pushed to +-6 sigma -- are scored by the f16x2 path on the device and in double on the
// host (the formula of aku/Distributions.cc:1040-1062, 2078-2086 over the same components), and a state whose visible
// values differ by more than 5e-5 (half the 1e-4 contract) loses the fp16 rows: it moves to the three-term section of
// the mixed layout (per-state precision routing), the rest of the model keeps the fast form.  The number of probe
// frames is sized so that the host side stays at a few million frame x component pairs (24 ... 192 frames).
// AASR_F16_PROBE=0 switches the guard off.
// ---------------------------------------------------------------------------
void gmm_probe_f16x2(aasr_gmm *g) {
  static const int probe_env = AASR_EXPERIMENT_ENV("AASR_F16_PROBE") ? atoi(AASR_EXPERIMENT_ENV("AASR_F16_PROBE")) : 1;
  static const float probe_tol = getenv("AASR_F16_PROBE_TOL") ? (float)atof(getenv("AASR_F16_PROBE_TOL")) : 5.0e-5f;  // test hook
  g->f16_probe_moved = 0;
  if (!probe_env || !g->dim_parts.empty() || g->class_routing || g->host.factor_path() || g->ill_conditioned) return;
  const HostModel &m = g->host;
  const int D = m.dim;
  const int64_t S = m.S, K = (int64_t)m.mix_idx.size();
  if (K == 0) return;
  const int P = (int)std::max<int64_t>(24, std::min<int64_t>(192, 4000000 / K));
  // per mixture component: constant + log weight (natural log), as pack_rows forms them; components routed to the
  // centred kernel (outliers) are not part of the matrix path's sum
  std::vector<double> cst((size_t)K);
  std::vector<uint8_t> live((size_t)K, 1);
  for (int64_t k = 0; k < K; k++) {
    const int64_t gi = m.mix_idx[(size_t)k];
    if (!g->outlier.empty() && g->outlier[(size_t)gi]) live[(size_t)k] = 0;
    double prod = 1;
    for (int d = 0; d < D; d++) {
      const double v = m.var[(size_t)gi * D + d];
      prod *= v > 0 ? 1 / v : 0;
    }
    cst[(size_t)k] = ((prod > 0) ? std::log(std::sqrt(prod)) : prod) + m.logw((size_t)k);
    if (!std::isfinite(cst[(size_t)k])) live[(size_t)k] = 0;
  }
  for (int round = 0; round < 2; round++) {
    TrackLayout &L0 = g->paired.ok ? g->paired : g->tracks;
    if (!L0.ok) return;
    // (a three-term engine part -- gmm_plan_engine_parts admits states to it beyond the one-pivot forms' limits -- is
    // probed the same way on its own rows)
    const bool pg3 = m.n_pg() > 0 && m.pg_arith == 3;
    const TrackLayout *LF = pg3 ? (L0.a16.p ? &L0 : nullptr) : (L0.a16h.p ? &L0 : nullptr);
    if (!LF) return;
    // probe frames (deterministic): frame i sits on mixture component (i * step) % K
    std::vector<float> fr((size_t)P * D);
    uint64_t st = 0x9e3779b97f4a7c15ull + (uint64_t)round * 77;
    auto uni = [&]() {   // xorshift64*, uniform in (0, 1)
      st ^= st >> 12; st ^= st << 25; st ^= st >> 27;
      return ((st * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
    };
    const int64_t step = std::max<int64_t>(1, K / P) | 1;
    for (int i = 0; i < P; i++) {
      const int64_t k = ((int64_t)i * step + round) % K;
      const int64_t gi = m.mix_idx[(size_t)k];
      static const double amps[4] = {0.5, 1.0, 1.5, 2.5};
      const double amp = i < P * 2 / 3 ? amps[i & 3] : 1.0;
      const int far_d = i < P * 2 / 3 ? -1 : (int)(uni() * D) % D;
      // every other far frame is far along SEVERAL dimensions at once (round 6: where tools/fuzz_fitted.py found the
      // round-5 limits wanting): ~ a sixth of the dimensions at +-3.5 .. 5 sigma, 8-12 sigma in all at 39 dimensions
      const bool multi = far_d >= 0 && ((i >> 1) & 1);
      for (int d = 0; d < D; d++) {
        const double v = m.var[(size_t)gi * D + d];
        const double sd = v > 0 ? std::sqrt(v) : 0.0;
        // a normal deviate from twelve uniforms is plenty here
        double z = -6.0;
        for (int u = 0; u < 12; u++) z += uni();
        double x = m.mean[(size_t)gi * D + d] + amp * sd * z;
        if (d == far_d) x = m.mean[(size_t)gi * D + d] + ((i & 1) ? 6.0 : -6.0) * sd;
        else if (multi && uni() < 1.0 / 6.0) x = m.mean[(size_t)gi * D + d] + (uni() < 0.5 ? -1.0 : 1.0) * (3.5 + 1.5 * uni()) * sd;
        fr[(size_t)i * D + d] = (float)x;
      }
    }
    // the verdict of this round, if the same content has been probed before
    uint64_t key = 0xcbf29ce484222325ull;
    {
      const int64_t hdr[8] = {D, S, K, P, round, pg3 ? 1 : 0, 0, m.pg_arith};
      key = fnv1a(hdr, sizeof hdr, key);
      const double tol_d = (double)probe_tol, bias_d = g->out_bias_ln, lwb = m.logw_bias;
      key = fnv1a(&tol_d, sizeof tol_d, key);
      key = fnv1a(&bias_d, sizeof bias_d, key);
      key = fnv1a(&lwb, sizeof lwb, key);
      key = fnv_vec(m.mean, key);
      key = fnv_vec(m.var, key);
      key = fnv_vec(m.mix_off, key);
      key = fnv_vec(m.mix_idx, key);
      key = fnv_vec(m.mix_w, key);
      key = fnv_vec(m.pg_pivot, key);
      key = fnv_vec(m.pg_begin, key);
      key = fnv_vec(m.pg_real_end, key);
      key = fnv_vec(g->pivot, key);
      key = fnv_vec(g->f16_state_ok, key);
      key = fnv_vec(g->outlier, key);
    }
    std::vector<uint8_t> bad((size_t)S, 0);
    int64_t n_bad = 0;
    bool cached = false;
    {
      ProbeCache &pc = probe_cache();
      std::lock_guard<std::mutex> lk(pc.mu);
      auto it = pc.verdicts.find(key);
      if (it != pc.verdicts.end()) {
        cached = true;
        pc.hits++;
        for (int32_t s2 : it->second)
          if (s2 >= 0 && s2 < S && !bad[(size_t)s2]) { bad[(size_t)s2] = 1; n_bad++; }
      }
    }
    if (!cached) {
    DevBuf<float> d_fr, d_a;
    d_fr.upload(fr.data(), fr.size());
    d_a.alloc((size_t)P * S);
    const int prec = g->precision;
    const bool use = g->use_bf16x3;
    g->precision = AASR_PREC_F16X2;
    g->use_bf16x3 = true;
    const bool ok_a = pg3 ? launch_split<3>(g, *LF, d_fr.p, P, d_a.p, nullptr) : launch_bf16(g, *LF, d_fr.p, P, d_a.p, nullptr);
    g->precision = prec;
    g->use_bf16x3 = use;
    if (!ok_a) return;
    std::vector<float> a((size_t)P * S);
    AASR_HIP(hipMemcpy(a.data(), d_a.p, a.size() * 4, hipMemcpyDeviceToHost));
    std::vector<double> ph((size_t)D);
    for (int i = 0; i < P; i++) {
      const float *x = &fr[(size_t)i * D];
      for (int64_t s2 = 0; s2 < S; s2++) {
        if (!g->f16_state_ok[(size_t)s2] || bad[(size_t)s2]) continue;
        double sum = 0;
        for (int32_t k = m.mix_off[s2]; k < m.mix_off[s2 + 1]; k++) {
          if (!live[(size_t)k]) continue;
          const int64_t gi = m.mix_idx[(size_t)k];
          const double *mu = &m.mean[(size_t)gi * D], *var = &m.var[(size_t)gi * D];
          double q = 0;
          for (int d = 0; d < D; d++) {
            const double t = (double)x[d] - mu[d];
            q += var[d] > 0 ? t * t / var[d] : 0.0;
          }
          sum += std::exp(cst[(size_t)k] - 0.5 * q);
        }
        const double ref = std::log(std::max(sum, 1e-50)) + g->out_bias_ln;
        // (three-term part: 3/4 of the contract -- its operands carry 24 bits, what the probe sees there is the f32
        // accumulators' granularity at |log2 value| ~ 100, 5-7e-5 on the probe's 6-sigma frames, not conditioning)
        // (slab-constant part: admitted by limits calibrated off the data up to 7.5e-5, tools/exp_calib.py)
        if (ref > -103.0 && !(std::fabs((double)a[(size_t)i * S + s2] - ref) <= (double)probe_tol * ((pg3 || m.pg_sc()) ? 1.5 : 1.0))) {
          bad[(size_t)s2] = 1;
          n_bad++;
        }
      }
    }
    {
      ProbeCache &pc = probe_cache();
      std::lock_guard<std::mutex> lk(pc.mu);
      pc.runs++;
      if (pc.verdicts.size() >= 256) pc.verdicts.clear();
      std::vector<int32_t> &v = pc.verdicts[key];
      v.clear();
      for (int64_t s2 = 0; s2 < S; s2++)
        if (bad[(size_t)s2]) v.push_back((int32_t)s2);
    }
    }   // !cached
    if (n_bad == 0) return;
    g->f16_probe_moved += n_bad;
    for (int64_t s2 = 0; s2 < S; s2++)
      if (bad[(size_t)s2]) g->f16_state_ok[(size_t)s2] = 0;
    if (m.n_pg() > 0) return;   // a multi-pivot engine part: the planner takes the marked states out and builds it again
    // the whole-model fp16 rows are gone: the model keeps its three-term rows, and the planner of the engine parts (which
    // runs next and starts from f16_state_ok) gives the states that still qualify their two-term rows back
    g->f16_whole_rejected = true;   // (a layout built later -- aasr_debug_set_layouts -- must not pack them again)
    g->paired.a16h = DevBuf<uint16_t>();
    g->paired.states_f16 = 0;
    g->tracks.a16h = DevBuf<uint16_t>();
    g->tracks.states_f16 = 0;
    return;
  }
}

__global__ void k_affine_frames(const float *__restrict__ x, int64_t F, int dim,
                                const double *__restrict__ A, const double *__restrict__ b,
                                float *__restrict__ y) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= F * dim) return;
  int64_t f = idx / dim;
  int i = (int)(idx - f * dim);
  double acc = b[i];
  for (int j = 0; j < dim; j++) acc += A[(size_t)i * dim + j] * (double)x[f * dim + j];
  y[idx] = (float)acc;
}

// Diagnostic (not part of the public ABI): restrict the kernels the scoring
// launcher may use (bit 0 grouped tracks, bit 1 independent tracks, bit 2 the
// centred-form kernel; with bits 0-1 clear and bit 2 set the centred kernel is
// forced, with all clear the general LDS-staged MFMA kernel).  Lets the tests
// cover every kernel.
extern "C" void aasr_debug_set_layouts(aasr_gmm *g, int mask) {
  if (!g) return;
  g->layout_mask = mask;
  if ((mask & 2) && !g->tracks.ok) gmm_build_tracks(g, false);
}
// which kernel a launch would use now: 4 centred, 1 grouped tracks,
// 2 independent tracks, 0 general LDS-staged MFMA kernel
extern "C" int aasr_debug_active_layout(const aasr_gmm *g) {
  if (!g) return -1;
  if ((g->layout_mask & 4) && (g->ill_conditioned || g->precision == AASR_PREC_F32_CENTRED ||
                               !(g->layout_mask & 3)) && g->centred_ok)
    return 4;
  if ((g->layout_mask & 1) && g->paired.ok) return 1;
  if ((g->layout_mask & 2) && g->tracks.ok) return 2;
  return 0;
}
extern "C" double aasr_debug_kappa(const aasr_gmm *g) { return g ? g->kappa : -1.0; }
// Diagnostic: the model's OWN one-pivot layout -- out[0] whole-model two-term rows packed, [1] outlier routing on, [2] outlier
// components, [3] states that hold them, [4] scored in the centred form as a whole, [5] states the probe moved
extern "C" void aasr_debug_own_layout(const aasr_gmm *g, int64_t *out) {
  if (!g || !out) return;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  out[0] = (L.ok && L.a16h.p) ? 1 : 0;
  out[1] = g->hyb_enabled ? 1 : 0;
  out[2] = g->hyb_rows;
  out[3] = g->hyb_states;
  out[4] = g->ill_conditioned ? 1 : 0;
  out[5] = g->f16_probe_moved;
}

// Diagnostic: what the scoring calls on this handle did with the outlier components since it was built -- out[0] launches
// of the scoring kernel's HYB instance (the merge in its close logic), out[1] runs of the merge pass (score_outliers)
extern "C" void aasr_debug_outlier_path(const aasr_gmm *g, int64_t *out) {
  if (!g || !out) return;
  out[0] = g->hyb_fused_launches;
  out[1] = g->hyb_merge_passes;
}
// Diagnostic switch: 0 leaves the outlier components of every call to the merge pass, 1 (the default) lets the launcher
// fuse the merge into the scoring kernel where its rules admit it
extern "C" void aasr_debug_set_outlier_fuse(aasr_gmm *g, int on) {
  if (g) g->hyb_fuse_off = !on;
}

// Diagnostic (tests, bench.py): the engine parts of a model (gmm_plan_engine_parts) -- out[0] parts, out[1] columns of an
// engine score row, then per part (up to three) {arithmetic (2 / 3 / 0: ordinary model), states, pivot groups, rows
// with the padding}; returns 0 when the model has none.
// Diagnostic: the column of every state in an engine score row ([S]) and, for engine part `part`, its pivot groups --
// first column / one past the last real column of every group (relative to the part's first column, which is returned in
// *col0) and the groups' pivots [groups][dim].  Returns the number of groups (0: an ordinary model), -1: no such part.
extern "C" int aasr_debug_engine_layout(const aasr_gmm *g, int part, int32_t *colmap, int32_t *begin, int32_t *real_end,
                                       float *pivots, int64_t *col0) {
  if (!g || part < 0 || (size_t)part >= g->engine_parts.size()) return -1;
  if (colmap) std::copy(g->engine_colmap_h.begin(), g->engine_colmap_h.end(), colmap);
  const auto &ep = g->engine_parts[(size_t)part];
  if (col0) *col0 = ep.col0;
  const aasr::HostModel &m = ep.model->host;
  const int P = m.n_pg();
  for (int p = 0; p < P; p++) {
    if (begin) begin[p] = m.pg_begin[(size_t)p];
    if (real_end) real_end[p] = m.pg_real_end[(size_t)p];
  }
  if (pivots) std::copy(m.pg_pivot.begin(), m.pg_pivot.end(), pivots);
  return P;
}
extern "C" const char *aasr_debug_engine_plan_note(const aasr_gmm *g) { return g ? g->engine_plan_note.c_str() : ""; }
extern "C" int aasr_debug_engine_parts(const aasr_gmm *g, int64_t *out, int n) {
  if (!g || !out || n < 14) return -1;
  for (int i = 0; i < n; i++) out[i] = 0;
  out[0] = (int64_t)g->engine_parts.size();
  out[1] = g->engine_cols;
  for (size_t i = 0; i < g->engine_parts.size() && i < 3; i++) {
    const auto &part = g->engine_parts[i];
    out[2 + 4 * i] = part.arith;
    out[3 + 4 * i] = part.states;
    out[4 + 4 * i] = part.arith ? part.model->paired.n_pg : 0;
    out[5 + 4 * i] = part.arith ? part.model->paired.rows_padded : (int64_t)part.model->host.mix_idx.size();
  }
  return (int)g->engine_parts.size();
}

// The exact part of a clustered scoring pass: a track layout with the selection
// masks applied and no 1e-50 floor (k_cluster_merge adds the centre terms and
// floors).
// which == 0: grouped layout, 1: independent tracks (gmm_cluster_layout()).
// A f + b for every frame under the model's global transform (into the handle's scratch)
const float *gmm_adapted_frames(aasr_gmm *g, const float *d_frames, int64_t F, hipStream_t stream) {
  if (!g->xf_a.p) return d_frames;
  g->d_xframes.ensure((size_t)F * g->dim);
  const int64_t n = F * g->dim;
  hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_frames, F, g->dim,
                     g->xf_a.p, g->xf_b.p, g->d_xframes.p);
  AASR_HIP(hipGetLastError());
  return g->d_xframes.p;
}

void gmm_tracks_masked_launch(aasr_gmm *g, int which, const float *d_frames, int64_t F,
                              float *d_out, const unsigned long long *maskrow,
                              hipStream_t stream, int64_t pitch) {
  const TrackLayout &L = which == 0 ? g->paired : g->tracks;
  if (!L.ok) raise(AASR_ERR_UNSUPPORTED, "Gaussian clustering needs a track layout for this model");
  ClusterArgs cl;
  cl.maskrow = maskrow;
  cl.rows_padded = L.rows_padded;
  cl.floor_val = NEG_BIG_F;
  if (g->use_bf16x3 && launch_bf16(g, L, d_frames, F, d_out, stream, &cl, pitch)) return;
  if (!launch_tracks(g, L, d_frames, F, d_out, stream, &cl, pitch))
    raise(AASR_ERR_UNSUPPORTED, "no track kernel instance for this model");
}

// Clustered pass over a model with outlier-routed Gaussians: the outlier components in the centred
// form, masked by their clusters' selection bits, added to what the masked track kernel wrote.
void gmm_outliers_masked_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, const int32_t *crow,
                                const unsigned long long *maskw, int c1, int64_t n_words, hipStream_t stream) {
  score_outliers(g, d_frames, F, d_out, stream, crow, maskw, c1, n_words);
}

// Clustered pass over a model that is scored in the centred form as a whole.
void gmm_centred_masked_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, const int32_t *crow,
                               const unsigned long long *maskw, int c1, int64_t n_words, hipStream_t stream) {
  if (!g->centred_ok) raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", g->dim);
  CentredOps ops{g->centred_recs.p, g->centred_state_off.p, g->centred_splits.p, g->centred_max_splits, g->S, 1};
  ops.n_recs = (int64_t)g->host.mix_idx.size();
  ops.crow = crow;
  ops.maskw = maskw;
  ops.c1 = c1;
  ops.n_words = n_words;
  if (!launch_centred_ops(g, ops, g->centred_dimp, d_frames, F, d_out, stream))
    raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", g->dim);
}

// Class routing (gmm.h): out[i] = log(exp(out[i]) + exp(part[i] + logdet)); a value AT the floor
// holds nothing (a sub-model writes the floor for states it has no component of).
__global__ void k_class_merge(float *__restrict__ out, const float *__restrict__ part, float logdet,
                              int first, int64_t n, int floors) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!floors) {  // clustered pass: exact parts without floors, k_cluster_merge applies it
    const float b = part[i] + logdet;
    if (first) {
      out[i] = b;
    } else {
      const float a = out[i];
      const float hi = fmaxf(a, b), lo = fminf(a, b);
      out[i] = hi + log1pf(expf(lo - hi));
    }
    return;
  }
  const float a = first ? LOG_TINY_F : out[i];
  float b = part[i];
  float r = a;
  if (b > LOG_TINY_F) {
    b += logdet;
    if (a > LOG_TINY_F) {
      const float hi = fmaxf(a, b), lo = fminf(a, b);
      r = hi + log1pf(expf(lo - hi));
    } else {
      r = b;
    }
  }
  out[i] = fmaxf(r, LOG_TINY_F);
}

__global__ void k_fill_value(float *__restrict__ out, float v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

__global__ void k_fill_floor(float *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = LOG_TINY_F;
}

static void score_classes(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, hipStream_t stream) {
  const int64_t S = g->S;
  int64_t pass = std::max<int64_t>(64, (int64_t)(g_score_pass_bytes / (double)(S * 4)));
  if (pass > F) pass = F;
  g->class_scratch.ensure((size_t)pass * (size_t)S);
  g->class_xframes.ensure((size_t)pass * (size_t)g->dim);
  for (int64_t f0 = 0; f0 < F; f0 += pass) {
    const int64_t n = std::min(pass, F - f0);
    const float *fr = d_frames + f0 * g->dim;
    float *out = d_out + f0 * S;
    const int64_t total = n * S;
    bool first = true;
    for (size_t c = 0; c < g->class_models.size(); c++) {
      aasr_gmm *sub = g->class_models[c].get();
      if (!sub) continue;
      const double logdet = c == 0 ? 0.0 : g->class_logdet[c];
      if (!(logdet > -INFINITY)) continue;  // det == 0: the adapted Gaussians contribute nothing
      const float *xf = fr;
      if (c > 0) {
        // f' = A f + b (AdaptedFeatureVector::calculate_new_ada_vector, aku/ModelModules.hh:208-212)
        const int64_t nv = n * g->dim;
        hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream, fr, n,
                           g->dim, g->class_a[c].p, g->class_b[c].p, g->class_xframes.p);
        AASR_HIP(hipGetLastError());
        xf = g->class_xframes.p;
      }
      sub->precision = g->precision;
      sub->use_bf16x3 = g->use_bf16x3;
      sub->layout_mask = g->layout_mask;
      gmm_score_launch(sub, xf, n, g->class_scratch.p, stream);
      hipLaunchKernelGGL(k_class_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out,
                         g->class_scratch.p, (float)logdet, first ? 1 : 0, total, 1);
      AASR_HIP(hipGetLastError());
      first = false;
    }
    if (first) {  // no class has anything: every state at the floor
      hipLaunchKernelGGL(k_fill_floor, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, total);
      AASR_HIP(hipGetLastError());
    }
  }
}

void gmm_classes_exact_launch(aasr_gmm *g, const float *d_frames, int64_t n, float *d_out,
                              const std::function<void(aasr_gmm *, size_t, const float *, float *)> &exact,
                              hipStream_t stream) {
  const int64_t S = g->S, total = n * S;
  g->class_scratch.ensure((size_t)total);
  g->class_xframes.ensure((size_t)n * (size_t)g->dim);
  bool first = true;
  for (size_t c = 0; c < g->class_models.size(); c++) {
    aasr_gmm *sub = g->class_models[c].get();
    if (!sub) continue;
    const double logdet = c == 0 ? 0.0 : g->class_logdet[c];
    if (!(logdet > -INFINITY)) continue;  // det == 0: the adapted Gaussians' exact values are 0
    const float *xf = d_frames;
    if (c > 0) {
      const int64_t nv = n * g->dim;
      hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream, d_frames, n,
                         g->dim, g->class_a[c].p, g->class_b[c].p, g->class_xframes.p);
      AASR_HIP(hipGetLastError());
      xf = g->class_xframes.p;
    }
    exact(sub, c, xf, g->class_scratch.p);
    hipLaunchKernelGGL(k_class_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_out,
                       g->class_scratch.p, (float)logdet, first ? 1 : 0, total, 0);
    AASR_HIP(hipGetLastError());
    first = false;
  }
  if (first) {  // no class has an exact part: nothing but the centres' share
    hipLaunchKernelGGL(k_fill_value, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_out, NEG_BIG_F, total);
    AASR_HIP(hipGetLastError());
  }
}

// log|det| of an in-place global transform for the kernels that do not take it at their output: the general kernel (a
// diagnostic layout) and the centred form of ill-conditioned models, whose launch floors at 1e-50 / |det|
// (outlier_part_floor) so that this floor is the only one that acts; the track kernels fold log|det| into their reference
// exponent
__global__ void k_add_bias(float *__restrict__ out, float bias, int64_t n, int64_t S, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t f = i / S;
  float *o = out + f * pitch + (i - f * S);
  *o = fmaxf(*o + bias, LOG_TINY_F);
}
__global__ void k_add_bias_nofloor(float *__restrict__ out, float bias, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += bias;
}
// (clustered passes: exact parts carry no floor before the merge)
void gmm_add_bias_nofloor(float *d_out, int64_t n, float bias, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_add_bias_nofloor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_out, bias, n);
  AASR_HIP(hipGetLastError());
}
static void add_output_bias(const aasr_gmm *g, float *d_out, int64_t F, hipStream_t stream, int64_t pitch = 0) {
  const int64_t n = F * g->S;
  hipLaunchKernelGGL(k_add_bias, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_out,
                     (float)g->out_bias_ln, n, g->S, pitch > 0 ? pitch : g->S);
  AASR_HIP(hipGetLastError());
}

// Whether scores can be written with a row pitch other than S: the bf16x3 track kernels can
// (rows padded to a multiple of 16 floats make every 64-byte output group a whole cache line).
static bool engine_parts_public(const aasr_gmm *g);
bool gmm_score_pitch_ok(const aasr_gmm *g) {
  if (!g->dim_parts.empty()) return false;
  if (engine_parts_public(g)) return true;
  if (g->cl.enabled && gmm_engine_parts_clustered(g)) return true;
  if (g->host.factor_path() || g->class_routing || g->precision == AASR_PREC_F64) return false;
  if (g->hyb_enabled && g->cl.enabled) return false;   // (the clustered pass over outlier routing writes dense rows)
  // a model scored in the centred form as a whole: the kernel writes runs of 32 states per frame row at any pitch
  if (g->ill_conditioned) return g->centred_ok && !g->cl.enabled && (g->layout_mask & 4);
  if (g->cl.enabled && !gmm_cluster_pitch_ok(g)) return false;
  if ((g->layout_mask & 3) != 3) return false;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  // both track kernels (f32 and bf16x3) take a row pitch; the centred kernel does not
  return (g->precision == AASR_PREC_F32 || g->precision == AASR_PREC_BF16X3 || g->precision == AASR_PREC_F16X2) && L.ok;
}

// The cases in which gmm_score_launch_pitched() is one launch of a track kernel (plus its frame operand) that writes state s
// into column s: a one-pivot two-term, three-term or f32 layout with nothing beside it -- no engine parts, clustering, class
// routing, outlier or centred pass, frame transform or dimension parts.
bool gmm_score_single_track_launch(const aasr_gmm *g, int64_t pitch) {
  if (pitch < g->S || !g->dim_parts.empty() || g->cl.enabled || g->class_routing || g->host.factor_path()) return false;
  if (g->precision != AASR_PREC_F32 && g->precision != AASR_PREC_BF16X3 && g->precision != AASR_PREC_F16X2) return false;
  if (gmm_engine_parts_active(g) || g->ill_conditioned || g->hyb_enabled || g->xf_a.p) return false;
  if ((g->layout_mask & 3) != 3) return false;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  if (!L.ok || L.n_pg > 1) return false;
  return pitch == g->S || gmm_score_pitch_ok(g);
}

// Mirrors launch_bf16 / launch_split / launch_split_instance for the layout gmm_score_launch_pitched scores a one-pivot
// model with: two terms where the precision asks for them and the layout has the rows, else three -- on the pipelined
// kernel up to five K slabs, on the wave-group kernel (no operand launch) beyond; no split rows: the f32 track kernel.
int gmm_score_frame_operand_terms(const aasr_gmm *g) {
  if (!g->use_bf16x3) return 0;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  if (!L.ok || L.n_pg > 1) return 0;
  if (L.nk16 < 1 || L.nk16 == 7 || L.nk16 > 8) return 0;   // (no split instance: launch_split returns false)
  if (g->precision == AASR_PREC_F16X2 && L.a16h.p) return 2;
  return L.a16.p && L.nk16 <= 5 ? 3 : 0;
}

void gmm_form_frame_operand(aasr_gmm *g, const float *d_frames, int64_t F, hipStream_t stream) {
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  const int ns = gmm_score_frame_operand_terms(g);
  if (ns == 2) form_frame_operand<2>(g, L, d_frames, F, stream);
  else if (ns == 3) form_frame_operand<3>(g, L, d_frames, F, stream);
  else g->fop_ahead = aasr_gmm::FopAhead();
}

void gmm_drop_frame_operand(const aasr_gmm *g) { g->fop_ahead = aasr_gmm::FopAhead(); }

// ---------------------------------------------------------------------------
// The engine's own score layout (recipe driver, aasr_run_utterance, aasr_gmm_score_lna_dev: scores that only the LNA pass
// reads): rows padded to whole lines; a model with engine parts: every part in its own column range, read through a
// column map.
// ---------------------------------------------------------------------------
// Engine parts (gmm_plan_engine_parts): the model as internal multi-pivot models over disjoint sets of its states.  They
// carry the default arithmetic only -- the other precisions are verification modes on the model's own layouts -- and
// nothing that merges by state column (clustering, class routing).
bool gmm_engine_parts_active(const aasr_gmm *g) {
  return !g->engine_parts.empty() && g->precision == AASR_PREC_F16X2 && g->use_bf16x3 && !g->cl.enabled &&
         !g->class_routing && g->dim_parts.empty() && (g->layout_mask & 3) == 3;
}

bool gmm_engine_parts_clustered(const aasr_gmm *g) {
  return !g->engine_parts.empty() && g->cl.enabled && g->precision == AASR_PREC_F16X2 && g->use_bf16x3 && !g->class_routing &&
         g->dim_parts.empty() && (g->layout_mask & 3) == 3;
}

// ... and public-layout calls (column = state) go through them too, with the columns gathered back: the parts are planned
// only for models whose own one-pivot layouts cannot put every state on two fp16 terms, and what those layouts do with the
// rest -- three bf16 terms up to their limits, the centred form beyond -- is slower than the parts + a gather of the columns.
// The exception: a model whose own layout HAS every state on plain two-term rows and only a few Gaussians off the matrix
// path (outlier routing) -- the public layout then costs those few rows in the centred form and their states' merge, less
// than the gather of the whole matrix (measured per 449 280 frames: 1.6 us per centred row, ~20 us per merged state -- its
// column's read-modify-write touches a line per frame -- as a pass of its own, nothing where the scoring kernel merges in
// its close logic (k_gmm_diag_score_pl<..., HYB>), 2.4 ms for the gather): one far-out Gaussian in 1 % / 10 % / 40 % of the
// states of configs[2]: see DESIGN 4.2.
static bool engine_parts_public(const aasr_gmm *g) {
  if (!gmm_engine_parts_active(g)) return false;
  static const int force_sc = AASR_EXPERIMENT_ENV("AASR_EXP_FORCE_SC") ? atoi(AASR_EXPERIMENT_ENV("AASR_EXP_FORCE_SC")) : 0;   // EXPERIMENT
  if (force_sc) return true;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  if (L.ok && L.a16h.p && g->hyb_enabled && !g->ill_conditioned && !g->cl.enabled) {
    // (the scoring kernel merges the outliers' sums in its close logic where it can: hyb_fuse_begin)
    // (... while such states are sparse: where they follow each other within a tile's time the close logic waits for its
    // values -- 40 % of the states of configs[2]: 15 ms against 11 through the parts)
    const bool fusable = g->hyb_tab.p && L.grouped && (g->layout_mask & 1) && 8 * g->hyb_states <= g->S;
    if (fusable ? 1.7 * (double)g->hyb_rows < 2400.0
                : 1.7 * (double)g->hyb_rows + 20.0 * (double)g->hyb_states < 1500.0)
      return false;
  }
  return true;
}

int64_t gmm_engine_pitch(const aasr_gmm *g) {
  // the parts' pitch only while the parts are what a scoring call runs: under another precision (verification modes on
  // the model's own layouts) the model's own rule holds (the parts' pitch there sent outlier-routed and
  // centred models into a pitched launch they do not have).  Scratch is sized with gmm_engine_pitch_max.
  if (gmm_engine_parts_active(g) || gmm_engine_parts_clustered(g)) return std::max(g->engine_cols, (g->S + 31) / 32 * 32);
  if (!gmm_score_pitch_ok(g)) return g->S;
  return (g->S + 31) / 32 * 32;
}

// the largest row pitch gmm_engine_pitch() can return for this model whatever the precision, clustering or transform
// state: what a caller sizes its scratch with (aasr_gmm_score_scratch_floats)
int64_t gmm_engine_pitch_max(const aasr_gmm *g) {
  return std::max((g->S + 31) / 32 * 32, g->engine_cols);
}

const int32_t *gmm_engine_colmap(const aasr_gmm *g) {
  return gmm_engine_parts_active(g) ? g->engine_colmap.p : nullptr;
}

__global__ void k_scatter_columns(const float *__restrict__ in, int64_t F, int64_t n, float *__restrict__ out, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F * n) return;
  const int64_t f = i / n;
  out[f * pitch + (i - f * n)] = in[i];
}

// out[f][s] = rows[f][colmap[s]]: the engine's score rows back in the public layout.  A workgroup walks frames; a thread
// keeps the columns of its states (s = tid, tid + 256, ...) in registers, so a frame costs one gather of its row (L2: the
// row was written a moment ago) and coalesced stores.
template <int VPT>
__global__ __launch_bounds__(256) void k_gather_columns(const float *__restrict__ rows, int64_t F, int64_t in_pitch,
                                                        const int32_t *__restrict__ colmap, int64_t S,
                                                        float *__restrict__ out, int64_t out_pitch) {
  int col[VPT];
#pragma unroll
  for (int j = 0; j < VPT; j++) {
    const int64_t s = threadIdx.x + 256 * j;
    col[j] = s < S ? colmap[s] : -1;
  }
  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    const float *r = rows + f * in_pitch;
    float *o = out + f * out_pitch;
    float v[VPT];
#pragma unroll
    for (int j = 0; j < VPT; j++) v[j] = col[j] >= 0 ? r[col[j]] : 0.0f;
#pragma unroll
    for (int j = 0; j < VPT; j++)
      if (col[j] >= 0) o[threadIdx.x + 256 * j] = v[j];
  }
}

__global__ __launch_bounds__(256) void k_gather_columns_any(const float *__restrict__ rows, int64_t F, int64_t in_pitch,
                                                            const int32_t *__restrict__ colmap, int64_t S,
                                                            float *__restrict__ out, int64_t out_pitch) {
  for (int64_t f = blockIdx.x; f < F; f += gridDim.x)
    for (int64_t s = threadIdx.x; s < S; s += 256) out[f * out_pitch + s] = rows[f * in_pitch + colmap[s]];
}

static void launch_gather_columns(const aasr_gmm *g, const float *rows, int64_t F, int64_t in_pitch, float *out,
                                  int64_t out_pitch, hipStream_t stream) {
  const unsigned blocks = (unsigned)std::min<int64_t>(F, (int64_t)(g->num_cus > 0 ? g->num_cus : 256) * 16);
  if (g->S <= 256 * 4)
    hipLaunchKernelGGL(k_gather_columns<4>, dim3(blocks), dim3(256), 0, stream, rows, F, in_pitch, g->engine_colmap.p, g->S, out, out_pitch);
  else if (g->S <= 256 * 16)
    hipLaunchKernelGGL(k_gather_columns<16>, dim3(blocks), dim3(256), 0, stream, rows, F, in_pitch, g->engine_colmap.p, g->S, out, out_pitch);
  else
    hipLaunchKernelGGL(k_gather_columns_any, dim3(blocks), dim3(256), 0, stream, rows, F, in_pitch, g->engine_colmap.p, g->S, out, out_pitch);
  AASR_HIP(hipGetLastError());
}

void gmm_scatter_columns(const float *dense, int64_t F, int64_t n, float *out, int64_t pitch, hipStream_t stream) {
  const int64_t tot = F * n;
  if (tot <= 0) return;
  hipLaunchKernelGGL(k_scatter_columns, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, dense, F, n, out, pitch);
  AASR_HIP(hipGetLastError());
}
void gmm_gather_engine_columns(const aasr_gmm *g, const float *rows, int64_t F, int64_t in_pitch, float *out, int64_t out_pitch,
                               hipStream_t stream) {
  launch_gather_columns(g, rows, F, in_pitch, out, out_pitch, stream);
}

static void launch_engine_parts(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, int64_t pitch,
                                hipStream_t stream) {
  if (g->xf_a.p) {   // one constrained-MLLR transform for the pool: the frames transformed once, log|det| at the output
    if ((size_t)F * g->dim > g->d_xframes.n) AASR_HIP(hipDeviceSynchronize());
    g->d_xframes.ensure((size_t)F * g->dim);
    const int64_t n = F * g->dim;
    hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_frames, F, g->dim,
                       g->xf_a.p, g->xf_b.p, g->d_xframes.p);
    AASR_HIP(hipGetLastError());
    d_frames = g->d_xframes.p;
  }
  for (auto &part : g->engine_parts) {
    aasr_gmm *sub = part.model.get();
    sub->out_bias_ln = g->out_bias_ln;
    float *o = d_out + part.col0;
    bool done = false;
    if (part.arith == 2 || part.arith == 4) done = launch_split<2>(sub, sub->paired, d_frames, F, o, stream, nullptr, pitch);
    else if (part.arith == 3) done = launch_split<3>(sub, sub->paired, d_frames, F, o, stream, nullptr, pitch);
    else {
      sub->precision = g->precision;
      sub->use_bf16x3 = g->use_bf16x3;
      if (gmm_score_pitch_ok(sub)) {
        gmm_score_launch_pitched(sub, d_frames, F, o, pitch, stream);
      } else {   // (an ill-conditioned remainder: its kernels write dense rows)
        if ((size_t)F * sub->S > g->engine_part_scratch.n) AASR_HIP(hipDeviceSynchronize());
        g->engine_part_scratch.ensure((size_t)F * sub->S);
        gmm_score_launch(sub, d_frames, F, g->engine_part_scratch.p, stream);
        const int64_t n = F * sub->S;
        hipLaunchKernelGGL(k_scatter_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           g->engine_part_scratch.p, F, sub->S, o, pitch);
        AASR_HIP(hipGetLastError());
      }
      done = true;
    }
    if (!done) raise(AASR_ERR_UNSUPPORTED, "no kernel instance for an engine part of the model");
  }
}

// public layout through the engine parts: chunks of frames into the handle's scratch, columns gathered back
static void launch_engine_parts_public(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, int64_t pitch,
                                       hipStream_t stream) {
  const int64_t ep = gmm_engine_pitch(g);
  const int64_t chunk = std::max<int64_t>(512, std::min<int64_t>(F, (int64_t)(1.0e9 / (4.0 * (double)ep))) / 512 * 512);
  if ((size_t)std::min(chunk, F) * ep > g->engine_scratch.n) {
    AASR_HIP(hipDeviceSynchronize());
    g->engine_scratch.ensure((size_t)std::min(chunk, F) * ep);
  }
  for (int64_t f0 = 0; f0 < F; f0 += chunk) {
    const int64_t fc = std::min(chunk, F - f0);
    launch_engine_parts(g, d_frames + f0 * g->dim, fc, g->engine_scratch.p, ep, stream);
    launch_gather_columns(g, g->engine_scratch.p, fc, ep, d_out + f0 * pitch, pitch, stream);
  }
}

void gmm_score_launch_engine(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, int64_t pitch,
                             hipStream_t stream) {
  if (F <= 0) return;
  if (gmm_engine_parts_active(g) && pitch >= g->engine_cols) {
    launch_engine_parts(g, d_frames, F, d_out, pitch, stream);
    return;
  }
  gmm_score_launch_pitched(g, d_frames, F, d_out, pitch, stream);
}

void gmm_score_launch_pitched(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, int64_t pitch,
                              hipStream_t stream) {
  if (F <= 0) return;
  if (pitch == g->S) {
    gmm_score_launch(g, d_frames, F, d_out, stream);
    return;
  }
  if (pitch > g->S && engine_parts_public(g)) {
    launch_engine_parts_public(g, d_frames, F, d_out, pitch, stream);
    return;
  }
  if (pitch < g->S || !gmm_score_pitch_ok(g))
    raise(AASR_ERR_UNSUPPORTED, "a row pitch other than the state count needs the track kernels");
  if (g->cl.enabled) {
    gmm_cluster_score_launch(g, d_frames, F, d_out, stream, pitch);
    return;
  }
  if (g->xf_a.p) {
    g->d_xframes.ensure((size_t)F * g->dim);
    const int64_t n = F * g->dim;
    hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       d_frames, F, g->dim, g->xf_a.p, g->xf_b.p, g->d_xframes.p);
    AASR_HIP(hipGetLastError());
    d_frames = g->d_xframes.p;
  }
  if (g->ill_conditioned) {
    if (!launch_centred(g, d_frames, F, d_out, stream, pitch))
      raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", g->dim);
    if (g->out_bias_ln != 0) add_output_bias(g, d_out, F, stream, pitch);
    return;
  }
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  hyb_fuse_begin(g, L, d_frames, F, stream);
  const bool done = (g->use_bf16x3 && launch_bf16(g, L, d_frames, F, d_out, stream, nullptr, pitch)) ||
                    launch_tracks(g, L, d_frames, F, d_out, stream, nullptr, pitch);
  const bool fused = g->hyb_fuse.used;   // (not what hyb_fuse_begin offered: what the launch took)
  g->hyb_fuse = aasr_gmm::HybFuse();
  if (!done) raise(AASR_ERR_UNSUPPORTED, "no track kernel instance for this model");
  // the Gaussians the matrix layouts left out (null rows): centred form, merged per state into the padded rows (where
  // the scoring kernel has not merged them itself)
  if (g->hyb_enabled && !fused) score_outliers(g, d_frames, F, d_out, stream, nullptr, nullptr, 0, 1, pitch);
}

// ---------------------------------------------------------------------------
// Feature dimension > 63: the model as parts of <= 63 dimensions (aasr_gmm::dim_parts).  ll_g(x) = sum over the
// parts of the part's own diagonal Gaussian (constants included: log sqrt prod p factorises too), so every part
// scores its column range per Gaussian -- no floor, natural log -- and k_dim_split_combine adds them per mixture
// component and forms log max(sum_k w_k e^ll, 1e-50) with a running maximum.  Frames are taken in chunks so that the
// per-Gaussian scores of all parts stay below ~1.5 GB.
// ---------------------------------------------------------------------------
__global__ void k_slice_columns(const float *__restrict__ x, int64_t F, int dim, int d0, int dp, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F * dp) return;
  const int64_t f = i / dp;
  const int d = (int)(i - f * dp);
  out[i] = x[f * dim + d0 + d];
}

__global__ __launch_bounds__(256) void k_dim_split_combine(const float *__restrict__ part_ll, int parts, int64_t Fc,
                                                           int64_t G, const int32_t *__restrict__ mix_off,
                                                           const int32_t *__restrict__ mix_idx,
                                                           const float *__restrict__ mix_logw, int64_t S,
                                                           float *__restrict__ out, int per_gaussian, float bias_ln,
                                                           const unsigned long long *__restrict__ maskw, int c1,
                                                           const int32_t *__restrict__ gclus, int64_t f_first) {
  const int64_t n = per_gaussian ? G : S;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Fc * n) return;
  const int64_t f = i / n, s = i - f * n;
  if (per_gaussian) {
    float v = 0.0f;
    for (int p = 0; p < parts; p++) v += part_ll[((int64_t)p * Fc + f) * G + s];
    out[i] = v;
    return;
  }
  // the parts' log-likelihoods are added in double: at several hundred dimensions |ll| ~ 10^3, where a float sum's
  // rounding alone (6e-5 per addition) reaches the 1e-4 bar; only differences to the running maximum go through expf
  double m = -3.0e38, sum = 0.0;
  for (int32_t k = mix_off[s]; k < mix_off[s + 1]; k++) {
    const float lw = mix_logw[k];
    if (!(lw > NEG_BIG_F)) continue;   // zero weight
    double v = (double)lw + (double)bias_ln;   // log |det| of the pool's one constrained-MLLR transform (AdaptedGaussian), else 0
    const int64_t gi = mix_idx[k];
    if (maskw) {   // Gaussian clustering: only the members of clusters selected for this frame are evaluated exactly
      const int64_t fa = f_first + f;
      if (!((maskw[(fa >> 6) * c1 + gclus[gi]] >> (fa & 63)) & 1ull)) continue;
    }
    for (int p = 0; p < parts; p++) v += (double)part_ll[((int64_t)p * Fc + f) * G + gi];
    const double mn = fmax(m, v);
    sum = sum * (double)__expf((float)(m - mn)) + (double)__expf((float)(v - mn));
    m = mn;
  }
  if (maskw) {   // the exact part alone, no floor: the merge adds the centres' share
    out[i] = sum > 0.0 ? (float)(m + (double)__logf((float)sum)) : NEG_BIG_F;
    return;
  }
  const float ll = sum > 0.0 ? (float)(m + (double)__logf((float)sum)) : LOG_TINY_F;
  out[i] = fmaxf(ll, LOG_TINY_F);
}

void gmm_dim_split_score(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, bool per_gaussian,
                         hipStream_t stream, const unsigned long long *maskw, int c1, const int32_t *gclus,
                         bool frames_adapted) {
  const int parts = (int)g->dim_parts.size();
  const int64_t chunk = std::max<int64_t>(64, std::min<int64_t>(F, (int64_t)(1.5e9 / (4.0 * (double)g->G * parts))));
  int max_dp = 0;
  for (int p = 0; p < parts; p++) max_dp = std::max(max_dp, g->dim_part_off[(size_t)p + 1] - g->dim_part_off[(size_t)p]);
  if ((size_t)chunk * max_dp > g->dim_part_x.n || (size_t)parts * chunk * g->G > g->dim_part_ll.n)
    AASR_HIP(hipDeviceSynchronize());   // growing frees the old buffers
  g->dim_part_x.ensure((size_t)chunk * max_dp);
  g->dim_part_ll.ensure((size_t)parts * chunk * g->G);
  const int64_t n_out = per_gaussian ? g->G : g->S;
  if (g->xf_a.p && !frames_adapted) {
    // one transform for the whole pool: the Gaussians are evaluated on A f + b (k_affine_frames handles any dimension)
    if (per_gaussian) raise(AASR_ERR_UNSUPPORTED, "per-Gaussian log-likelihoods are not built for adapted pools");
    g->d_xframes.ensure((size_t)F * g->dim);
    const int64_t n = F * g->dim;
    hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_frames, F, g->dim,
                       g->xf_a.p, g->xf_b.p, g->d_xframes.p);
    AASR_HIP(hipGetLastError());
    d_frames = g->d_xframes.p;
  }
  for (int64_t f0 = 0; f0 < F; f0 += chunk) {
    const int64_t fc = std::min(chunk, F - f0);
    for (int p = 0; p < parts; p++) {
      const int d0 = g->dim_part_off[(size_t)p], dp = g->dim_part_off[(size_t)p + 1] - d0;
      const int64_t n = fc * dp;
      hipLaunchKernelGGL(k_slice_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_frames + f0 * g->dim,
                         fc, g->dim, d0, dp, g->dim_part_x.p);
      AASR_HIP(hipGetLastError());
      g->dim_parts[(size_t)p]->precision = g->precision == AASR_PREC_F64 ? AASR_PREC_F32 : g->precision;
      gmm_gauss_launch(g->dim_parts[(size_t)p].get(), g->dim_part_x.p, fc, g->dim_part_ll.p + (size_t)p * fc * g->G, stream);
    }
    const int64_t n = fc * n_out;
    hipLaunchKernelGGL(k_dim_split_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g->dim_part_ll.p, parts,
                       fc, g->G, g->dim_mix_off.p, g->dim_mix_idx.p, g->dim_mix_logw.p, g->S, d_out + f0 * n_out,
                       per_gaussian ? 1 : 0, g->xf_a.p ? (float)g->out_bias_ln : 0.0f, maskw, c1, gclus, f0);
    AASR_HIP(hipGetLastError());
  }
}

void gmm_score_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                      hipStream_t stream) {
  if (F <= 0) return;
  if (!g->dim_parts.empty()) {
    if (g->cl.enabled) {
      if (g->precision == AASR_PREC_F64)
        raise(AASR_ERR_UNSUPPORTED, "Gaussian clustering on a model of more than 63 dimensions: float arithmetic only");
      gmm_cluster_score_launch(g, d_frames, F, d_out, stream);
      return;
    }
    if (g->precision == AASR_PREC_F64) {   // the reference's arithmetic in double: instances up to 192 dimensions
      score_f64_for_f32_callers(g, d_frames, F, d_out, stream);
      return;
    }
    gmm_dim_split_score(g, d_frames, F, d_out, false, stream);
    return;
  }
  if (g->precision == AASR_PREC_F64) {
    score_f64_for_f32_callers(g, d_frames, F, d_out, stream);
    return;
  }
  if (g->cl.enabled) {
    gmm_cluster_score_launch(g, d_frames, F, d_out, stream);
    return;
  }
  if (g->class_routing) {
    score_classes(g, d_frames, F, d_out, stream);
    return;
  }
  if (g->host.factor_path()) {
    gmm_full_launch(g, d_frames, F, d_out, stream);
    return;
  }
  if (engine_parts_public(g)) {
    launch_engine_parts_public(g, d_frames, F, d_out, g->S, stream);
    return;
  }
  if (g->xf_a.p) {
    // global constrained-MLLR transform: f' = A f + b once per frame
    // (AdaptedFeatureVector::calculate_new_ada_vector, aku/ModelModules.hh:208-212)
    g->d_xframes.ensure((size_t)F * g->dim);
    const int64_t n = F * g->dim;
    hipLaunchKernelGGL(k_affine_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       d_frames, F, g->dim, g->xf_a.p, g->xf_b.p, g->d_xframes.p);
    AASR_HIP(hipGetLastError());
    d_frames = g->d_xframes.p;
  }
  // numerically safe path first when the model needs it (or it is forced)
  if ((g->layout_mask & 4) && (g->ill_conditioned || g->precision == AASR_PREC_F32_CENTRED ||
                               !(g->layout_mask & 3) ) && g->centred_ok)
    if (launch_centred(g, d_frames, F, d_out, stream)) {
      if (g->out_bias_ln != 0) add_output_bias(g, d_out, F, stream);
      return;
    }
  // layout choice: grouped tracks > independent tracks > general (LDS-staged)
  bool done = false;
  bool fused = false;
  if (!done && (g->layout_mask & 1) && g->paired.ok) {
    hyb_fuse_begin(g, g->paired, d_frames, F, stream);
    done = (g->use_bf16x3 && launch_bf16(g, g->paired, d_frames, F, d_out, stream)) ||
           launch_tracks(g, g->paired, d_frames, F, d_out, stream);
    fused = g->hyb_fuse.used;   // (not what hyb_fuse_begin offered: what the launch took)
    g->hyb_fuse = aasr_gmm::HybFuse();
  }
  if (!done && (g->layout_mask & 2) && g->tracks.ok)
    done = (g->use_bf16x3 && launch_bf16(g, g->tracks, d_frames, F, d_out, stream)) ||
           launch_tracks(g, g->tracks, d_frames, F, d_out, stream);
  if (!done) {
    launch_diag<0>(g, g->mix, d_frames, F, d_out, g->S, stream);
    if (g->out_bias_ln != 0) add_output_bias(g, d_out, F, stream);  // this kernel has no output bias
  }
  // the Gaussians the matrix layouts left out (null rows): centred form, merged per state
  if (g->hyb_enabled && !fused) score_outliers(g, d_frames, F, d_out, stream);
}

void gmm_gauss_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                      hipStream_t stream) {
  if (!g->dim_parts.empty()) {
    gmm_dim_split_score(g, d_frames, F, d_out, true, stream);
    return;
  }
  if (g->xf_a.p || g->class_routing || g->host.n_transforms > 0)
    raise(AASR_ERR_UNSUPPORTED, "per-Gaussian log-likelihoods are not built for adapted pools");
  if (g->host.any_full()) {
    // full-covariance pools: every Gaussian as a one-component state of an internal model, scored
    // by the factor-row kernel (values below the 1e-50 floor come out at the floor)
    if (!g->pool_view) {
      HostModel pm = g->host;
      pm.S = pm.G;
      pm.mix_off.resize((size_t)pm.G + 1);
      pm.mix_idx.resize((size_t)pm.G);
      pm.mix_w.assign((size_t)pm.G, 1.0);
      for (int64_t i = 0; i <= pm.G; i++) pm.mix_off[(size_t)i] = (int32_t)i;
      for (int64_t i = 0; i < pm.G; i++) pm.mix_idx[(size_t)i] = (int32_t)i;
      pm.weights_normalized = true;
      pm.hmm_label.clear();
      pm.hmm_states.clear();
      auto sub = std::make_unique<aasr_gmm>();
      sub->device = g->device;
      gmm_build(sub.get(), pm);
      g->pool_view = std::move(sub);
    }
    g->pool_view->precision = g->precision;
    g->pool_view->use_bf16x3 = g->use_bf16x3;
    gmm_score_launch(g->pool_view.get(), d_frames, F, d_out, stream);
    return;
  }
  if (g->ill_conditioned || g->hyb_enabled) {
    // variance-floored Gaussians: the expanded form loses eps * kappa, so the whole pool is
    // evaluated in the centred form (one-record states, no floor)
    gmm_build_pool_centred(g);
    CentredOps ops{g->poolc_recs.p, g->poolc_state_off.p, g->poolc_splits.p, g->poolc_max_splits, g->G, 1};
    ops.n_recs = g->G;
    ops.floor_val = NEG_BIG_F;
    if (!launch_centred_ops(g, ops, g->centred_dimp, d_frames, F, d_out, stream))
      raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", g->dim);
    return;
  }
  gmm_build_pool(g);
  launch_diag<1>(g, g->pool, d_frames, F, d_out, g->G, stream);
}

}  // namespace aasr

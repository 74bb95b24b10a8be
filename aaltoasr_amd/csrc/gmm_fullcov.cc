// gmm_fullcov.cc -- factor rows of full-covariance pools and of per-class CMLLR (k_gmm_full_score).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gmm_build.h"

namespace aasr {

// ---------------------------------------------------------------------------
// Full-covariance Gaussians (G2; FullCovarianceGaussian, Distributions.cc
// :1412-1446, 1466-1488, 1559-1586).  The reference inverts Sigma (LU), takes
// log sqrt det P by its own Cholesky and scores with the 819-term exponential
// form theta.phi(f).  Here Sigma = R R^T (Cholesky, double, host) and
//     -1/2 (x-mu)^T P (x-mu) = -1/2 || R^-1 (x-mu) ||^2
// so each component contributes the dim rows of sqrt(log2e/2)*R^-1 (and the
// bias -R^-1 mu' in the constant column) to the streamed operand: the MFMA
// accumulators hold y directly, the epilogue squares and sums -- no
// cancellation, K = dim+1 instead of dim(dim+3)/2.  A diagonal Gaussian in a
// mixed pool is the special case R = diag(sigma).  Non-SPD covariance: the
// reference zeroes the precision and the constant (an "invalid" Gaussian with
// log-likelihood 0); mirrored.
// ---------------------------------------------------------------------------
void gmm_build_fullcov(aasr_gmm *g) {
  const HostModel &m = g->host;
  FullLayout &L = g->full;
  L.ok = false;
  const int D = m.dim;
  // K = D + 1 coefficient slots (k = 0..D) -> K/2 = D/2 + 1 MFMA steps;
  // pick_nkk(x) returns the smallest kernel instance >= x + 1
  const int nkk = pick_nkk(D / 2);
  if (nkk < 0) raise(AASR_ERR_UNSUPPORTED, "feature dimension %d is not built for full covariances", D);
  const int K2 = 2 * nkk;
  if (D + 1 > K2) raise(AASR_ERR_UNSUPPORTED, "feature dimension %d is not built for full covariances", D);
  const int gq = (D + 3) / 4;  // quads per component
  const double sc = std::sqrt(0.5 * kLog2e);

  // per-Gaussian factor rows, constants
  // y = W x + beta per Gaussian (original feature space)
  std::vector<double> Wall((size_t)m.G * D * D, 0.0), Beta((size_t)m.G * D, 0.0), cst((size_t)m.G, 0.0);
  std::vector<double> r, w, a((size_t)D * D), wt((size_t)D * D), bt((size_t)D);
  double max_c = -INFINITY;
  for (int64_t gi = 0; gi < m.G; gi++) {
    if (m.any_full() && m.is_full[(size_t)gi]) {
      for (int i = 0; i < D * D; i++) a[(size_t)i] = m.cov[(size_t)gi * D * D + i];
    } else {
      std::fill(a.begin(), a.end(), 0.0);
      for (int i = 0; i < D; i++) a[(size_t)i * D + i] = m.var[(size_t)gi * D + i];
    }
    if (cholesky_lower(D, a.data(), r)) {
      invert_lower(D, r, w);
      double ld = 0;
      for (int i = 0; i < D; i++) ld += std::log(r[(size_t)i * D + i]);
      cst[(size_t)gi] = -ld;  // log sqrt det P
      if (!m.gauss_bias.empty()) cst[(size_t)gi] += m.gauss_bias[(size_t)gi];
      for (int i = 0; i < D; i++) {
        double bi = 0;
        for (int d = 0; d < D; d++) {
          Wall[(size_t)gi * D * D + (size_t)i * D + d] = w[(size_t)i * D + d];
          bi -= w[(size_t)i * D + d] * m.mean[(size_t)gi * D + d];
        }
        Beta[(size_t)gi * D + i] = bi;
      }
    } else {
      cst[(size_t)gi] = 0.0;  // invalid: precision 0, constant 0
    }
    // model-side CMLLR: the Gaussian sees A f + b  ->  W' = W A, beta' = W b + beta,
    // likelihood times |prod diag A|
    if (m.n_transforms > 0 && m.g2t[(size_t)gi] >= 0) {
      const double *X = &m.xform[(size_t)m.g2t[(size_t)gi] * D * (D + 1)];
      double *Wg = &Wall[(size_t)gi * D * D];
      double *Bg = &Beta[(size_t)gi * D];
      const double det = transform_diag_product(X, D);
      for (int i = 0; i < D; i++) {
        double bi = Bg[i];
        for (int j = 0; j < D; j++) {
          double acc = 0;
          for (int d = 0; d < D; d++) acc += Wg[(size_t)i * D + d] * X[(size_t)d * (D + 1) + 1 + j];
          wt[(size_t)i * D + j] = acc;
          bi += Wg[(size_t)i * D + j] * X[(size_t)j * (D + 1)];
        }
        bt[(size_t)i] = bi;
      }
      for (int i = 0; i < D * D; i++) Wg[i] = wt[(size_t)i];
      for (int i = 0; i < D; i++) Bg[i] = bt[(size_t)i];
      cst[(size_t)gi] += std::log(std::fabs(det));  // -inf when a diagonal entry is 0
    }
    if (std::isfinite(cst[(size_t)gi])) max_c = std::max(max_c, cst[(size_t)gi]);
  }
  double ref = std::floor(std::min(kRefMax, kPeakMax - max_c * kLog2e));
  if (!(ref >= kRefMin))
    raise(AASR_ERR_UNSUPPORTED,
          "full-covariance model leaves no f32 exponent headroom (peak log-likelihood %.1f)", max_c);
  L.ref_ln = (float)(ref * 0.69314718055994530942);

  // placement: states on the shorter track, components back to back
  std::vector<int8_t> st_track((size_t)m.S);
  std::vector<int64_t> st_pos((size_t)m.S);
  int64_t len[2] = {0, 0};
  int64_t ks[2] = {0, 0}, kg[2] = {0, 0};
  std::vector<int64_t> cand[5];
  for (auto &c : cand) c.push_back(0);
  auto quads_of = [&](int64_t s) {
    return std::max<int64_t>(1, (int64_t)(m.mix_off[s + 1] - m.mix_off[s]) * gq);
  };
  int64_t total_quads = 0;
  for (int64_t s = 0; s < m.S; s++) total_quads += quads_of(s);
  const int64_t sync_every = std::max<int64_t>(64, total_quads / 2 / 32);
  int64_t next_sync = sync_every;
  for (int64_t s = 0; s < m.S; s++) {
    int h = len[1] < len[0] ? 1 : 0;
    st_track[(size_t)s] = (int8_t)h;
    st_pos[(size_t)s] = len[h];
    len[h] += quads_of(s);
    ks[h]++;
    kg[h] += std::max<int64_t>(1, m.mix_off[s + 1] - m.mix_off[s]);
    if (std::min(len[0], len[1]) >= next_sync && s + 1 < m.S) {
      int64_t top = (std::max(len[0], len[1]) + 7) / 8 * 8;
      len[0] = len[1] = top;
      cand[0].push_back(top / 8);
      cand[1].push_back(ks[0]);
      cand[2].push_back(ks[1]);
      cand[3].push_back(kg[0]);
      cand[4].push_back(kg[1]);
      next_sync = top + sync_every;
    }
  }
  const int64_t tiles = std::max<int64_t>(1, (std::max(len[0], len[1]) + 7) / 8);
  if (cand[0].back() == tiles)
    for (auto &c : cand) c.pop_back();
  cand[0].push_back(tiles);
  cand[1].push_back(ks[0]);
  cand[2].push_back(ks[1]);
  cand[3].push_back(kg[0]);
  cand[4].push_back(kg[1]);

  std::vector<double> coef((size_t)tiles * TILE_ROWS * K2, 0.0);
  L.row_gauss.assign((size_t)tiles * TILE_ROWS, -1);
  L.rows_padded = tiles * TILE_ROWS;
  std::vector<uint32_t> close((size_t)tiles, 0);
  std::vector<float> gc[2];
  std::vector<int32_t> sid[2];
  std::vector<float> gc_tile((size_t)(tiles + 1) * 16, kNullConst);
  std::vector<int32_t> sid_tile((size_t)(tiles + 1) * 16, 0);
  for (int64_t s = 0; s < m.S; s++) {
    const int h = st_track[(size_t)s];
    int64_t p = st_pos[(size_t)s];
    const int32_t a0 = m.mix_off[s], b0 = m.mix_off[s + 1];
    if (b0 <= a0) {
      // empty state: one null component whose constant underflows to nothing
      gc[h].push_back(kNullConst);
      close[(size_t)(p / 8)] |= 1u << (p % 8 + 8 * h);
      close[(size_t)(p / 8)] |= 1u << (16 + p % 8 + 8 * h);
      sid[h].push_back((int32_t)s);
      gc_tile[(size_t)(p / 8) * 16 + h * 8 + p % 8] = kNullConst;
      sid_tile[(size_t)(p / 8) * 16 + h * 8 + p % 8] = (int32_t)s;
      continue;
    }
    for (int32_t k = a0; k < b0; k++) {
      const int64_t gi = m.mix_idx[k];
      const double *W = &Wall[(size_t)gi * D * D];
      for (int i = 0; i < D; i++) {
        const int64_t row = track_row(p + i / 4, h, i % 4);
        L.row_gauss[(size_t)row] = (int32_t)gi;
        double *cr = &coef[(size_t)row * K2];
        double bias = Beta[(size_t)gi * D + i];  // + W v: frames arrive pivot-centred
        for (int d = 0; d < D; d++) {
          cr[d] = sc * W[(size_t)i * D + d];
          bias += W[(size_t)i * D + d] * (double)g->pivot[d];
        }
        cr[D] = sc * bias;
      }
      const double wgt = m.mix_w[k];
      const double c = cst[(size_t)gi] + (wgt > 0 ? std::log(wgt) : -INFINITY);
      gc[h].push_back(std::isfinite(c) ? (float)(c * kLog2e + ref) : kNullConst);
      const int64_t last = p + gq - 1;
      close[(size_t)(last / 8)] |= 1u << (last % 8 + 8 * h);
      gc_tile[(size_t)(last / 8) * 16 + h * 8 + last % 8] = gc[h].back();
      if (k + 1 == b0) {
        close[(size_t)(last / 8)] |= 1u << (16 + last % 8 + 8 * h);
        sid[h].push_back((int32_t)s);
        sid_tile[(size_t)(last / 8) * 16 + h * 8 + last % 8] = (int32_t)s;
      }
      p += gq;
    }
  }
  const size_t gs = std::max(gc[0].size(), gc[1].size()) + 1;
  const size_t ss = std::max(sid[0].size(), sid[1].size()) + 1;
  std::vector<float> gflat(2 * gs, kNullConst);
  std::vector<int32_t> sflat(2 * ss, 0);
  for (int h = 0; h < 2; h++) {
    for (size_t k = 0; k < gc[h].size(); k++) gflat[h * gs + k] = gc[h][k];
    for (size_t k = 0; k < sid[h].size(); k++) sflat[h * ss + k] = sid[h][k];
  }
  L.g_stride = (int32_t)gs;
  L.s_stride = (int32_t)ss;
  L.gconst.upload(gflat.data(), gflat.size());
  L.sid.upload(sflat.data(), sflat.size());
  L.gc_tile.upload(gc_tile.data(), gc_tile.size());
  L.sid_tile.upload(sid_tile.data(), sid_tile.size());
  close.push_back(0);  // the bf16x3 kernel requests the next tile's word one tile ahead
  L.close.upload(close.data(), close.size());
  // split table, entries of 8 ints
  {
    std::vector<int32_t> table((size_t)TRACK_MAX_SPLITS * (TRACK_MAX_SPLITS + 1) * 8, 0);
    L.max_splits = 1;
    const size_t nc = cand[0].size();
    for (int R = 1; R <= TRACK_MAX_SPLITS; R++) {
      std::vector<size_t> pick{0};
      bool ok = true;
      for (int i = 1; i < R && ok; i++) {
        double want = (double)tiles * i / R;
        size_t best = pick.back();
        double bd = 1e300;
        for (size_t c = pick.back() + 1; c + 1 < nc; c++) {
          double dd = std::fabs((double)cand[0][c] - want);
          if (dd < bd) { bd = dd; best = c; }
        }
        if (best == pick.back()) ok = false;
        pick.push_back(best);
      }
      if (!ok) break;
      pick.push_back(nc - 1);
      int64_t worst = 0;
      for (int i = 0; i < R; i++) worst = std::max(worst, cand[0][pick[i + 1]] - cand[0][pick[i]]);
      if ((double)worst > 1.25 * (double)tiles / R + 1) break;
      int32_t *row = &table[(size_t)(R - 1) * (TRACK_MAX_SPLITS + 1) * 8];
      for (int i = 0; i <= R; i++)
        for (int c = 0; c < 5; c++) row[8 * i + c] = (int32_t)cand[c][pick[i]];
      L.max_splits = R;
    }
    L.splits.upload(table.data(), table.size());
  }
  pack_coef_rows(nkk, coef, tiles * TILE_ROWS, L.rows);
  // three-term bf16 split of the same rows (AASR_PREC_BF16X3): K index = column, padded to 16
  {
    const int nk16 = (D + 1 + 15) / 16;
    L.nk16 = 0;
    L.a16 = DevBuf<uint16_t>();
    if (nk16 <= 4) {
      const size_t tile_elems = (size_t)nk16 * 3 * 2 * 64 * 8;
      std::vector<uint16_t> a((size_t)tiles * tile_elems, 0);
      for (int64_t r = 0; r < tiles * TILE_ROWS; r++)
        for (int k = 0; k <= D; k++) {
          const float x = (float)coef[(size_t)r * K2 + k];
          float b1, b2, b3;
          const uint16_t hs[3] = {bf16_rne(x, &b1), bf16_rne(x - b1, &b2), bf16_rne((x - b1) - b2, &b3)};
          for (int sp = 0; sp < 3; sp++) a[split_tile_index(nk16, 3, r, k, sp)] = hs[sp];
        }
      L.a16.upload(a.data(), a.size());
      L.nk16 = nk16;
      // two-term fp16 split (AASR_PREC_F16X2), where the pool qualifies: conditioning estimate below the limit, every
      // coefficient inside the fp16 range, and every coordinate weighs enough in some row of every Gaussian that a
      // frame clamped to +-kFullF16Clamp there is far below the floor (|y| >= 64: q >= 4096 in log2 units).
      // Per-column power-of-two scales: an fp16 `lo` term below 2^-14 is a subnormal with an ABSOLUTE error of 3e-8, which
      // the other operand multiplies.  With unnormalised features (variance 10^3: coefficients ~ 1/sigma = 0.03, frame
      // components ~ 100) every coefficient's `lo` term is subnormal and y = R^-1 (x - mu) is off by 3e-6 per column --
      // 2e-4 in the state once |y| ~ 10 multiplies it.  Column k of the rows is therefore multiplied by 2^s_k, s_k chosen
      // so that the pool's largest coefficient of the column sits at ~1, and the kernel multiplies the frame operand by
      // 2^-s_k (exact): coefficients and frame components then both sit around 2^0 whatever the features' scale, as they
      // do for normalised features, where the two-term rows were measured.  (Scaling the coefficients up to 128, the
      // diagonal form's choice, pushes the FRAME operand into the subnormals instead: measured fivefold worse.)
      L.a16h = DevBuf<uint16_t>();
      L.f16scale = DevBuf<float>();
      static const bool f16_env = !(AASR_EXPERIMENT_ENV("AASR_F16X2") && atoi(AASR_EXPERIMENT_ENV("AASR_F16X2")) == 0);
      std::vector<double> kap((size_t)m.G, 0.0), colmax((size_t)m.G * D, 0.0), poolmax((size_t)D, 0.0);
      for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
        const int32_t gi = r < (int64_t)L.row_gauss.size() ? L.row_gauss[(size_t)r] : -1;
        if (gi < 0) continue;
        const double b = coef[(size_t)r * K2 + D];
        kap[(size_t)gi] += b * b;
        for (int k = 0; k < D; k++) {
          const double w = std::fabs(coef[(size_t)r * K2 + k]);
          colmax[(size_t)gi * D + k] = std::max(colmax[(size_t)gi * D + k], w);
          poolmax[(size_t)k] = std::max(poolmax[(size_t)k], w);
        }
      }
      std::vector<int> sk((size_t)D, 0);
      std::vector<float> scale((size_t)(16 * nk16), 1.0f);
      for (int k = 0; k < D; k++) {
        int e = 0;
        if (poolmax[(size_t)k] > 0) e = (int)std::lround(-std::log2(poolmax[(size_t)k]));
        e = std::max(-14, std::min(14, e));
        sk[(size_t)k] = e;
        scale[(size_t)k] = (float)std::ldexp(1.0, -e);   // the frame operand's factor
      }
      double amax = 0;
      for (int64_t r = 0; r < tiles * TILE_ROWS; r++)
        for (int k = 0; k <= D; k++)
          amax = std::max(amax, std::fabs(std::ldexp(coef[(size_t)r * K2 + k], k < D ? sk[(size_t)k] : 0)));
      L.kappa = 0;
      bool heavy = true;
      std::vector<char> seen((size_t)m.G, 0);
      for (int32_t gi : L.row_gauss)
        if (gi >= 0) seen[(size_t)gi] = 1;
      for (int64_t gi = 0; gi < m.G; gi++) {
        if (!seen[(size_t)gi]) continue;
        L.kappa = std::max(L.kappa, kap[(size_t)gi]);
        bool all_zero = true;   // the reference's "invalid" Gaussian: zero rows, constant 0
        for (int k = 0; k < D; k++) all_zero = all_zero && colmax[(size_t)gi * D + k] == 0.0;
        if (all_zero) continue;
        for (int k = 0; k < D; k++)
          heavy = heavy && std::ldexp(colmax[(size_t)gi * D + k], sk[(size_t)k]) * (double)kFullF16Clamp >= 64.0;
      }
      if (f16_env && L.kappa <= (D < 8 ? FULL_KAPPA_LIMIT_F16_LOWDIM : FULL_KAPPA_LIMIT_F16) && amax < 60000.0 && heavy) {
        const size_t tile_h = (size_t)nk16 * 2 * 2 * 64 * 8;
        std::vector<uint16_t> ah((size_t)tiles * tile_h, 0);
        for (int64_t r = 0; r < tiles * TILE_ROWS; r++)
          for (int k = 0; k <= D; k++) {
            const double x = std::ldexp(coef[(size_t)r * K2 + k], k < D ? sk[(size_t)k] : 0);   // split on the host in double
            const _Float16 hi = (_Float16)x;
            const _Float16 lo = (_Float16)(x - (double)hi);
            uint16_t hs[2];
            memcpy(&hs[0], &hi, 2);
            memcpy(&hs[1], &lo, 2);
            for (int sp = 0; sp < 2; sp++) ah[split_tile_index(nk16, 2, r, k, sp)] = hs[sp];
          }
        L.a16h.upload(ah.data(), ah.size());
        L.f16scale.upload(scale.data(), scale.size());
      }
    }
  }
  L.ok = true;
}

}  // namespace aasr

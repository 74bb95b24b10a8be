// gmm_model.cc -- model file readers and host-side packing of the streamed
// Gaussian operand.
//
// File formats: PDFPool::read_gk (aku/Distributions.cc:2811-2910),
// DiagonalGaussian::read (:1131-1150), HmmSet::read_mc (aku/HmmSet.cc:156-180),
// Mixture::read (aku/Distributions.cc:2418-2434), HmmSet::read_legacy_ph
// (aku/HmmSet.cc:194-329).  Constants: DiagonalGaussian::set_constant
// (aku/Distributions.cc:1273-1288) -- no (2*pi)^(-d/2) term.
#include <map>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstring>
#include <fstream>
#include <sstream>

#include "gmm.h"

namespace aasr {

static const double kLog2e = 1.4426950408889634073599246810019;
// log2-domain value standing in for log(0): exp2(x - max) underflows to 0 for
// any live component, and an all-null segment still reduces to a finite value
// that the 1e-50 floor then clamps.
static const float kNullConst = -1.0e30f;

// ---------------------------------------------------------------------------
// Subspace-constrained Gaussians: PCGMM / SCGMM entries of a
// 'variable' .gk file (aku/Distributions.cc:2843-2868).  The reference evaluates
// them per frame through K quadratic features shared by the pool
// (PrecisionSubspace::precompute / ExponentialSubspace::precompute,
// aku/Subspaces.cc:458-469, 745-768) and a K-term dot product per Gaussian
// (aku/Distributions.cc:1638-1648, 1851-1859).  For scoring, such a Gaussian IS a
// full-precision Gaussian with P = sum_b lambda_b S_b: it is expanded here, once,
// into covariance P^-1 and mean P^-1 m~ (P^-1 psi) and takes the dense
// factor-row kernels (k_gmm_full_score) like any 'full' entry.
//   pcgmm: const = log sqrt det P - 1/2 m~^T P^-1 m~ (recompute_constant, :1785-1802) is
//          exactly the full Gaussian's.  AS WRITTEN the reference's expression ends at a stray
//          ';' (:1643-1645) and drops the lambda.q term, i.e. evaluates const + m~.f -- not a
//          density.  This engine scores the intended form; AASR_PCGMM_AS_WRITTEN=1 refuses
//          PCGMM models instead of scoring them (the oracle restates both forms).
//   scgmm: the scoring quadratic uses Pvec with the exact sqrt 2 of map_m2v, the constant
//          (:1905-1914) uses P_b = map_v2m(Pvec_b) with a FLOAT 1/sqrt 2 and is
//          log det P - psi^T P^-1 psi - d log(2*3.1416) as written (no halves); the difference
//          to the normalised constant is carried in HostModel::gauss_bias.
// PARITY UNPINNED (not compiled in the reference: USE_SUBSPACE_COV is never defined).
// ---------------------------------------------------------------------------
struct SubspaceTables {
  std::map<int, std::vector<std::vector<double>>> precision;    // ssid -> [K][d*d]
  std::map<int, std::vector<std::vector<double>>> exponential;  // ssid -> [K][d + d(d+1)/2]
};

static bool chol_spd(int d, const std::vector<double> &a, std::vector<double> &l) {
  l.assign((size_t)d * d, 0.0);
  for (int j = 0; j < d; j++) {
    double s = a[(size_t)j * d + j];
    for (int k = 0; k < j; k++) s -= l[(size_t)j * d + k] * l[(size_t)j * d + k];
    if (!(s > 0)) return false;
    const double ljj = std::sqrt(s);
    l[(size_t)j * d + j] = ljj;
    for (int i = j + 1; i < d; i++) {
      double t = 0.5 * (a[(size_t)i * d + j] + a[(size_t)j * d + i]);
      for (int k = 0; k < j; k++) t -= l[(size_t)i * d + k] * l[(size_t)j * d + k];
      l[(size_t)i * d + j] = t / ljj;
    }
  }
  return true;
}

// inverse and log-determinant of an SPD matrix through its Cholesky factor
static bool spd_inverse(int d, const std::vector<double> &a, std::vector<double> &inv, double *logdet) {
  std::vector<double> l, w((size_t)d * d, 0.0);
  if (!chol_spd(d, a, l)) return false;
  double ld = 0;
  for (int c = 0; c < d; c++) {  // w = l^-1
    ld += 2.0 * std::log(l[(size_t)c * d + c]);
    w[(size_t)c * d + c] = 1.0 / l[(size_t)c * d + c];
    for (int i = c + 1; i < d; i++) {
      double s = 0;
      for (int k = c; k < i; k++) s += l[(size_t)i * d + k] * w[(size_t)k * d + c];
      w[(size_t)i * d + c] = -s / l[(size_t)i * d + i];
    }
  }
  inv.assign((size_t)d * d, 0.0);
  for (int i = 0; i < d; i++)
    for (int j = 0; j <= i; j++) {
      double s = 0;
      for (int k = i; k < d; k++) s += w[(size_t)k * d + i] * w[(size_t)k * d + j];
      inv[(size_t)i * d + j] = inv[(size_t)j * d + i] = s;
    }
  *logdet = ld;
  return true;
}

// PrecisionSubspace::read_subspace (aku/Subspaces.cc:185-208) / ExponentialSubspace::read_subspace
// (:1175-1198): "<ssid> <feature dim> <basis dim>" then one basis element per row
static void read_subspace(std::istream &in, bool precision, int dim, SubspaceTables &t) {
  int ssid = 0, fea_dim = 0, basis_dim = 0;
  in >> ssid >> fea_dim >> basis_dim;
  if (in.fail() || basis_dim <= 0 || basis_dim > 4096)
    raise(AASR_ERR_INVALID, "%s: error reading stream", precision ? "PrecisionSubspace::read_subspace()"
                                                                  : "ExponentialSubspace::read_subspace()");
  if (fea_dim != dim)
    raise(AASR_ERR_INVALID, "subspace %d has feature dimension %d, the pool %d", ssid, fea_dim, dim);
  const size_t n = precision ? (size_t)dim * dim : (size_t)dim + (size_t)dim * (dim + 1) / 2;
  std::vector<std::vector<double>> basis((size_t)basis_dim, std::vector<double>(n));
  for (auto &b : basis)
    for (double &v : b) in >> v;
  if (in.fail()) raise(AASR_ERR_INVALID, "error reading the basis of subspace %d", ssid);
  (precision ? t.precision : t.exponential)[ssid] = std::move(basis);
}

// PrecisionConstrainedGaussian::read (aku/Distributions.cc:1683-1704) /
// SubspaceConstrainedGaussian::read (:1886-1916), expanded into mean + covariance of pool entry g
static void read_subspace_gaussian(std::istream &in, bool pcgmm, const SubspaceTables &t, HostModel &m,
                                   long g) {
  static const bool as_written = getenv("AASR_PCGMM_AS_WRITTEN") && atoi(getenv("AASR_PCGMM_AS_WRITTEN")) != 0;
  const int D = m.dim;
  int ssid = 0, ss_dim = 0;
  in >> ssid >> ss_dim;
  const auto &tab = pcgmm ? t.precision : t.exponential;
  const auto it = tab.find(ssid);
  if (in.fail() || it == tab.end())
    raise(AASR_ERR_INVALID, "%s Gaussian %ld names subspace %d, which has not been defined", pcgmm ? "pcgmm" : "scgmm",
          g, ssid);
  if (ss_dim <= 0 || ss_dim > (int)it->second.size())
    raise(AASR_ERR_INVALID, "Gaussian %ld uses %d coefficients, subspace %d has %zu basis elements", g, ss_dim, ssid,
          it->second.size());
  std::vector<double> lin((size_t)D, 0.0), lambda((size_t)ss_dim);
  if (pcgmm)
    for (double &v : lin) in >> v;  // the transformed mean m~ = P mu
  for (double &v : lambda) in >> v;
  if (in.fail()) raise(AASR_ERR_INVALID, "Error in reading Gaussian specifications");
  if (pcgmm && as_written)
    raise(AASR_ERR_UNSUPPORTED,
          "AASR_PCGMM_AS_WRITTEN: the reference's PrecisionConstrainedGaussian::compute_log_likelihood "
          "(aku/Distributions.cc:1643-1645) ends at a stray ';' and evaluates const + m~.f, a linear function of "
          "the frame; this engine only scores the intended density (oracle.SubspaceModel restates both)");
  // precision used by the scoring expression, and the one the constant is computed from
  std::vector<double> P((size_t)D * D, 0.0), Pc;
  if (pcgmm) {
    for (int b = 0; b < ss_dim; b++)
      for (size_t i = 0; i < (size_t)D * D; i++) P[i] += lambda[(size_t)b] * it->second[(size_t)b][i];
    Pc = P;
  } else {
    Pc.assign((size_t)D * D, 0.0);
    const float a_f = (float)(1.0 / std::sqrt(2.0));  // map_v2m's float factor (aku/LinearAlgebra.cc:248)
    const double a_d = 1.0 / std::sqrt(2.0);           // what map_m2v's sqrt(2) in the feature amounts to
    for (int b = 0; b < ss_dim; b++) {
      const std::vector<double> &th = it->second[(size_t)b];
      for (int d = 0; d < D; d++) lin[(size_t)d] += lambda[(size_t)b] * th[(size_t)d];
      size_t pos = (size_t)D;
      for (int i = 0; i < D; i++)
        for (int j = 0; j <= i; j++, pos++) {
          if (i == j) {
            P[(size_t)i * D + i] += lambda[(size_t)b] * th[pos];
            Pc[(size_t)i * D + i] += lambda[(size_t)b] * th[pos];
          } else {
            P[(size_t)i * D + j] += lambda[(size_t)b] * (a_d * th[pos]);
            P[(size_t)j * D + i] += lambda[(size_t)b] * (a_d * th[pos]);
            Pc[(size_t)i * D + j] += lambda[(size_t)b] * ((double)a_f * th[pos]);
            Pc[(size_t)j * D + i] += lambda[(size_t)b] * ((double)a_f * th[pos]);
          }
        }
    }
  }
  std::vector<double> cov, covc;
  double logdet = 0, logdetc = 0;
  if (!spd_inverse(D, P, cov, &logdet) || !spd_inverse(D, Pc, covc, &logdetc))
    raise(AASR_ERR_INVALID, "%s Gaussian %ld: its precision matrix is not positive definite", pcgmm ? "pcgmm" : "scgmm",
          g);
  const size_t Dz = (size_t)D;
  if (m.is_full.empty()) {
    m.is_full.assign((size_t)m.G, 0);
    m.cov.assign((size_t)m.G * Dz * Dz, 0.0);
  }
  m.is_full[(size_t)g] = 1;
  double quad = 0, quadc = 0;  // lin^T P^-1 lin with either precision
  for (size_t i = 0; i < Dz; i++) {
    double mu = 0, muc = 0;
    for (size_t j = 0; j < Dz; j++) {
      mu += cov[i * Dz + j] * lin[j];
      muc += covc[i * Dz + j] * lin[j];
      m.cov[(size_t)g * Dz * Dz + i * Dz + j] = cov[i * Dz + j];
    }
    m.mean[(size_t)g * Dz + i] = mu;
    m.var[(size_t)g * Dz + i] = cov[i * Dz + i];
    quad += lin[i] * mu;
    quadc += lin[i] * muc;
  }
  if (!pcgmm) {
    // as written: log det(P) - psi^T P^-1 psi - d log(2 * 3.1416); the expanded Gaussian supplies
    // log sqrt det(P) - 1/2 psi^T P^-1 psi
    const double written = logdetc - quadc - (double)D * std::log(2 * 3.1416);
    if (m.gauss_bias.empty()) m.gauss_bias.assign((size_t)m.G, 0.0);
    m.gauss_bias[(size_t)g] = written - (0.5 * logdet - 0.5 * quad);
  }
}

void read_gk_pool(const char *gk, HostModel &m) {
  {
    std::ifstream in(gk);
    if (!in) raise(AASR_ERR_IO, "PDFPool::read_gk(): could not open %s", gk);
    long pdfs = 0;
    std::string type;
    in >> pdfs >> m.dim >> type;
    if (!in || pdfs < 0 || m.dim <= 0)
      raise(AASR_ERR_INVALID, "PDFPool::read_gk(): error reading file: %s", gk);
    bool variable = (type == "variable");
    bool all_full = (type == "full_cov");
    if (!variable && !all_full && type != "diagonal_cov") {
      if (type == "pcgmm" || type == "scgmm")
        // the legacy header forms construct the Gaussians without a subspace
        // (aku/Distributions.cc:2886-2897: a null m_ps / m_es): nothing to score with
        raise(AASR_ERR_UNSUPPORTED,
              "gk header type '%s' names no subspace; use the 'variable' form with "
              "precision_subspace / exponential_subspace entries", type.c_str());
      raise(AASR_ERR_INVALID, "Unknown model type");
    }
    SubspaceTables subspaces;
    m.G = pdfs;
    const size_t D = (size_t)m.dim;
    m.mean.resize((size_t)pdfs * D);
    m.var.assign((size_t)pdfs * D, 0.0);
    for (long g = 0; g < pdfs; g++) {
      bool full = all_full;
      if (variable) {
        in >> type;
        if (type == "precision_subspace" || type == "exponential_subspace") {
          read_subspace(in, type == "precision_subspace", m.dim, subspaces);
          g--;  // a definition, not a pool entry (aku/Distributions.cc:2843-2856)
          continue;
        }
        if (type == "pcgmm" || type == "scgmm") {
          read_subspace_gaussian(in, type == "pcgmm", subspaces, m, g);
          continue;
        }
        if (type == "full") {
          full = true;
        } else if (type != "diag") {
          raise(AASR_ERR_INVALID, "Unknown model type\n%s", type.c_str());
        }
      }
      for (size_t i = 0; i < D; i++) in >> m.mean[(size_t)g * D + i];
      if (full) {
        if (m.is_full.empty()) {
          m.is_full.assign((size_t)pdfs, 0);
          m.cov.assign((size_t)pdfs * D * D, 0.0);
        }
        m.is_full[(size_t)g] = 1;
        // FullCovarianceGaussian::read (aku/Distributions.cc:1466-1488): row-major d x d
        for (size_t i = 0; i < D * D; i++) in >> m.cov[(size_t)g * D * D + i];
        for (size_t i = 0; i < D; i++) m.var[(size_t)g * D + i] = m.cov[(size_t)g * D * D + i * D + i];
      } else {
        for (size_t i = 0; i < D; i++) in >> m.var[(size_t)g * D + i];
      }
      if (in.fail())
        raise(AASR_ERR_INVALID, "Error in reading Gaussian specifications");
    }
  }
}

HostModel read_model_files(const char *gk, const char *mc, const char *ph) {
  HostModel m;
  read_gk_pool(gk, m);
  {
    std::ifstream in(mc);
    if (!in) raise(AASR_ERR_IO, "HmmSet::read_mc(): could not open %s", mc);
    long pdfs = 0;
    in >> pdfs;
    if (!in || pdfs < 0) raise(AASR_ERR_INVALID, "HmmSet::read_mc(): bad header in %s", mc);
    m.S = pdfs;
    m.mix_off.assign(1, 0);
    for (long s = 0; s < pdfs; s++) {
      int n = 0;
      in >> n;
      for (int k = 0; k < n; k++) {
        int idx;
        double w;
        in >> idx >> w;
        if (in.fail())
          raise(AASR_ERR_INVALID, "Error in reading mixture specifications");
        m.mix_idx.push_back(idx);
        m.mix_w.push_back(w);
      }
      m.mix_off.push_back((int32_t)m.mix_idx.size());
    }
  }
  if (ph) {
    // Legacy PHONE file: only the state inventory matters for scoring.  State
    // index == emission pdf index (aku/HmmSet.cc:245,319-322); the number of
    // states is 1 + the largest pdf index referenced.
    std::ifstream in(ph);
    if (!in) raise(AASR_ERR_IO, "HmmSet::read_ph(): could not open %s", ph);
    std::string buf;
    in >> buf;
    if (buf != "PHONE") raise(AASR_ERR_INVALID, "HmmSet::read_ph(): not a PHONE file: %s", ph);
    int phonemes = 0;
    in >> phonemes;
    long max_pdf = -1;
    for (int h = 0; h < phonemes; h++) {
      int index = 0, states = 0;
      std::string label;
      in >> index >> states >> label;
      if (!in) raise(AASR_ERR_INVALID, "HmmSet::read_ph(): read error in %s", ph);
      states -= 2;
      int dummy;
      in >> dummy >> dummy;
      m.hmm_label.push_back(label);
      m.hmm_states.emplace_back();
      for (int s = 0; s < states; s++) {
        int pdf;
        in >> pdf;
        if (pdf > max_pdf) max_pdf = pdf;
        m.hmm_states.back().push_back(pdf);
      }
      for (int s = -2; s < states; s++) {
        int source = 0, transitions = 0;
        in >> source >> transitions;
        for (int t = 0; t < transitions; t++) {
          int target;
          double prob;
          in >> target >> prob;
        }
      }
      if (!in) raise(AASR_ERR_INVALID, "HmmSet::read_ph(): read error in %s", ph);
    }
    long nstates = max_pdf + 1;
    if (nstates > m.S)
      raise(AASR_ERR_INVALID, "ph file references pdf %ld but mc file has %ld mixtures", max_pdf, (long)m.S);
    // states beyond the ph inventory are not emitted (num_states() = ph count)
    if (nstates < m.S) {
      m.S = nstates;
      m.mix_off.resize((size_t)nstates + 1);
      m.mix_idx.resize((size_t)m.mix_off.back());
      m.mix_w.resize((size_t)m.mix_off.back());
    }
  }
  return m;
}

// ---------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------

// Writes explicit coefficient rows (coef[r][k], k = 2*kk + h) into the tile
// layout; rows beyond n_rows are zero.
static void pack_coef_rows(int nkk, const std::vector<double> &coef, int64_t n_rows,
                           PackedRows &out) {
  out.nkk = nkk;
  out.rows = n_rows;
  out.tiles = std::max<int64_t>(1, (n_rows + TILE_ROWS - 1) / TILE_ROWS);
  const size_t tile_floats = (size_t)(nkk / 2) * 64 * 4;
  const size_t K = 2 * (size_t)nkk;
  std::vector<float> a((size_t)out.tiles * tile_floats, 0.0f);
  for (int64_t r = 0; r < n_rows; r++) {
    int64_t t = r / TILE_ROWS;
    int j = (int)(r % TILE_ROWS);
    int mb = j / 32, r32 = j % 32;
    for (int kk = 0; kk < nkk; kk++) {
      int q = kk / 2, e = kk % 2;
      for (int h = 0; h < 2; h++) {
        size_t idx = (size_t)t * tile_floats + ((size_t)q * 64 + (size_t)(h * 32 + r32)) * 4 + (size_t)(mb * 2 + e);
        a[idx] = (float)coef[(size_t)r * K + 2 * kk + h];
      }
    }
  }
  out.a.upload(a.data(), a.size());
}

struct RowSpec {
  int64_t g;        // pool Gaussian, < 0 for a null (padding) row
  double logw;      // log mixture weight (natural), -inf for zero weight
  double bias = 0;  // added to the constant in log2 units (paired layout reference)
  int pg = 0;       // pivot group of the row's state (multi-pivot layouts; the model's one pivot otherwise)
};

// Write rows into the [tiles][nkk/2][64][4] layout the kernel streams:
// lane l = h*32 + r32 of kk-pair q holds
//   { A[r32][2(2q)+h], A[r32][2(2q+1)+h], A[32+r32][2(2q)+h], A[32+r32][2(2q+1)+h] }
// with K index k = 2*kk + h:  kk<dim: h=0 -> p*mu'*log2e, h=1 -> -p/2*log2e;
// kk==dim: h=0 -> constant*log2e; everything else 0.
static void pack_rows(const aasr_gmm *g, const std::vector<RowSpec> &rows,
                      PackedRows &out, std::vector<double> *a64_host, bool upload_f32 = true) {
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
      // DiagonalGaussian::read + set_constant (Distributions.cc:1144-1147, 1273-1288)
      double prod = 1, quad = 0;
      for (int d = 0; d < D; d++) {
        double p = (var[d] > 0) ? 1 / var[d] : 0;
        prod *= p;
      }
      double cst = (prod > 0) ? std::log(std::sqrt(prod)) : prod;
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
    int64_t t = r / TILE_ROWS;
    int j = (int)(r % TILE_ROWS);
    int mb = j / 32, r32 = j % 32;
    for (int kk = 0; kk < nkk; kk++) {
      int q = kk / 2, e = kk % 2;
      for (int h = 0; h < 2; h++) {
        size_t idx = (size_t)t * tile_floats + ((size_t)q * 64 + (size_t)(h * 32 + r32)) * 4 + (size_t)(mb * 2 + e);
        a[idx] = (float)coef[2 * kk + h];
      }
    }
    if (a64_host)
      for (int k = 0; k < 2 * D + 1; k++)
        (*a64_host)[(size_t)r * (2 * D + 1) + k] = coef[k];
  }
  out.a.upload(a.data(), a.size());
}

void gmm_build_tracks(aasr_gmm *g, bool grouped);
static void f16x2_state_eligibility(const aasr_gmm *g, std::vector<uint8_t> &ok);
static void find_outliers(aasr_gmm *g);
static void build_class_routing(aasr_gmm *g);
static void build_pg_model(aasr_gmm *g);

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

void gmm_build(aasr_gmm *g, const HostModel &model) {
  require_device();
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      g->num_cus = cus;
  }
  g->host = model;
  HostModel &m = g->host;
  g->outlier.clear();
  g->hyb_enabled = false;
  g->hyb_states = g->hyb_rows = 0;
  g->f16_probe_moved = 0;
  g->f16_whole_rejected = false;
  g->rows_unbiased = false;
  g->out_bias_ln = 0;
  g->dim = m.dim;
  g->G = m.G;
  g->S = m.S;
  if (m.dim <= 0 || m.G <= 0 || m.S <= 0)
    raise(AASR_ERR_INVALID, "empty model (dim %d, %ld Gaussians, %ld states)", m.dim, (long)m.G, (long)m.S);
  if ((int64_t)m.mix_off.size() != m.S + 1)
    raise(AASR_ERR_INVALID, "mix_off must hold num_states+1 entries");
  g->dim_parts.clear();
  if (m.dim + 1 > 64 && m.any_full())
    raise(AASR_ERR_UNSUPPORTED, "feature dimension %d > 63 is built for diagonal pools only", m.dim);
  for (size_t k = 0; k < m.mix_idx.size(); k++)
    if (m.mix_idx[k] < 0 || m.mix_idx[k] >= m.G)
      raise(AASR_ERR_INVALID, "mixture component %zu points at Gaussian %d outside the pool of %ld",
            k, m.mix_idx[k], (long)m.G);
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
  if (m.n_transforms > 0) {
    if ((int64_t)m.g2t.size() != m.G ||
        (int64_t)m.xform.size() != (int64_t)m.n_transforms * m.dim * (m.dim + 1))
      raise(AASR_ERR_INVALID, "transform arrays do not match the model");
    for (int32_t t : m.g2t)
      if (t < -1 || t >= m.n_transforms) raise(AASR_ERR_INVALID, "transform index %d out of range", t);
  }
  g->engine_parts.clear();
  g->engine_colmap = DevBuf<int32_t>();
  g->engine_colmap_h.clear();
  g->engine_cols = 0;
  if (m.n_pg() > 0) {
    build_pg_model(g);
    return;
  }
  if (m.dim + 1 > 64) {
    // the model as dimension parts (gmm_dim_split_score).  Regression classes: every class is such a model over its
    // own Gaussians and adapted frames (class routing); one transform for the whole pool: the frames transformed once
    m.logw_bias = 0;
    g->xf_a.release();
    g->xf_b.release();
    g->class_routing = false;
    if (m.n_transforms > 0 && !m.global_xform()) {
      build_class_routing(g);
      return;
    }
    g->class_models.clear();
    g->class_g2t.clear();
    build_dim_split(g);
    if (m.n_transforms > 0) {
      const int D = m.dim;
      std::vector<double> A((size_t)D * D), b((size_t)D);
      double det = 1;
      for (int i = 0; i < D; i++) {
        b[(size_t)i] = m.xform[(size_t)i * (D + 1)];
        for (int j = 0; j < D; j++) A[(size_t)i * D + j] = m.xform[(size_t)i * (D + 1) + 1 + j];
        det *= A[(size_t)i * D + i];
      }
      g->xf_a.upload(A.data(), A.size());
      g->xf_b.upload(b.data(), b.size());
      g->out_bias_ln = std::log(std::fabs(det));
    }
    return;
  }
  // centring pivot: per-dimension mean of the pool means, rounded to float so
  // the device subtracts exactly the value the constants were built with
  g->pivot.assign(m.dim, 0.0f);
  for (int d = 0; d < m.dim; d++) {
    double acc = 0;
    for (int64_t i = 0; i < m.G; i++) acc += m.mean[(size_t)i * m.dim + d];
    g->pivot[d] = (float)(acc / (double)m.G);
  }
  g->d_pivot.upload(g->pivot.data(), g->pivot.size());
  if (m.any_full() &&
      ((int64_t)m.cov.size() != m.G * m.dim * m.dim || (int64_t)m.is_full.size() != m.G))
    raise(AASR_ERR_INVALID, "covariance array does not match the pool size");
  m.logw_bias = 0;
  g->xf_a.release();
  g->xf_b.release();
  g->class_routing = false;
  if (m.n_transforms > 0 && !m.global_xform() && !m.any_full()) {
    build_class_routing(g);
    return;
  }
  g->class_models.clear();
  g->class_g2t.clear();
  if (m.factor_path()) {
    // full-covariance Gaussians and per-class CMLLR are scored through factor
    // rows by k_gmm_full_score only
    g->mix.rows = (int64_t)m.mix_idx.size();
    g->paired.ok = g->tracks.ok = g->centred_ok = false;
    gmm_build_fullcov(g);
    return;
  }
  g->full.ok = false;
  if (m.global_xform()) {
    // one transform for every Gaussian == transform the frames once, add log|det|
    const int D = m.dim;
    std::vector<double> A((size_t)D * D), b((size_t)D);
    double det = 1;
    for (int i = 0; i < D; i++) {
      b[(size_t)i] = m.xform[(size_t)i * (D + 1)];
      for (int j = 0; j < D; j++) A[(size_t)i * D + j] = m.xform[(size_t)i * (D + 1) + 1 + j];
      det *= A[(size_t)i * D + i];
    }
    m.logw_bias = std::log(std::fabs(det));
    g->xf_a.upload(A.data(), A.size());
    g->xf_b.upload(b.data(), b.size());
  }

  find_outliers(g);

  // component-expanded rows in state order + segment metadata
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
static void build_pg_model(aasr_gmm *g) {
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
  m.logw_bias = 0;
  g->xf_a.release();
  g->xf_b.release();
  g->class_routing = false;
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
      double kk = 0, k2 = 0;
      for (int d = 0; d < D; d++) {
        const double v = m.var[(size_t)gi * D + d];
        const double pr = v > 0 ? 1 / v : 0;
        const double mc = m.mean[(size_t)gi * D + d] - (double)pv[d];
        kk += pr * mc * mc;
        k2 += (pr * mc * mc) * (pr * mc * mc);
      }
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
    const double *mu = &m.mean[(size_t)gi * D], *var = &m.var[(size_t)gi * D];
    double kk = 0, k2 = 0;
    for (int d = 0; d < D; d++) {
      const double pr = var[d] > 0 ? 1 / var[d] : 0;
      const double mc = mu[d] - (double)pv[d];
      const double t = pr * mc * mc;
      kk += t;
      k2 += t * t;
    }
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
static const double kRefMin = 56.0, kRefMax = 72.0;
static const double kPeakMax = 120.0;  // max (peak*log2e + ref) accepted

static bool choose_reference(const HostModel &m, const std::vector<uint8_t> &outlier, double *ref_out) {
  const int D = m.dim;
  double max_peak_log2 = -INFINITY;
  for (size_t k = 0; k < m.mix_idx.size(); k++) {
    if (!outlier.empty() && outlier[(size_t)m.mix_idx[k]]) continue;  // scored in the centred form
    const double *var = &m.var[(size_t)m.mix_idx[k] * D];
    double prod = 1;
    for (int d = 0; d < D; d++) prod *= (var[d] > 0) ? 1 / var[d] : 0;
    double cst = (prod > 0) ? std::log(std::sqrt(prod)) : prod;
    double peak = cst + m.logw(k);
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
static inline uint16_t bf16_rne(float x, float *back) {
  uint32_t u;
  memcpy(&u, &x, 4);
  uint32_t r = u + 0x7fffu + ((u >> 16) & 1u);
  uint16_t h = (uint16_t)(r >> 16);
  uint32_t b = (uint32_t)h << 16;
  memcpy(back, &b, 4);
  return h;
}

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
    const int64_t t = r / TILE_ROWS;
    const int jrow = (int)(r % TILE_ROWS);
    const int mb = jrow / 32, m32 = jrow % 32;
    for (int k = 0; k < 2 * KH; k++) {
      // K order of the split-term kernels: the constant, (f16x2: its remainder,) then coef64's own interleaved order
      const double v = k == 0 ? c[2 * D] : (k >= 2 && k - 2 < 2 * D ? c[k - 2] : 0.0);
      float x = (float)v, b1, b2, b3;
      uint16_t h1 = bf16_rne(x, &b1);
      uint16_t h2 = bf16_rne(x - b1, &b2);
      uint16_t h3 = bf16_rne((x - b1) - b2, &b3);
      const uint16_t hs[3] = {h1, h2, h3};
      const int slab = k / 16, hk = (k % 16) / 8, i = k % 8;
      const int lane = hk * 32 + m32;
      for (int sp = 0; sp < 3; sp++) {
        size_t idx = (size_t)t * tile_elems + ((((size_t)slab * 3 + sp) * 2 + mb) * 64 + lane) * 8 + i;
        a[idx] = hs[sp];
      }
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
      double prod = 1;
      for (int d = 0; d < D; d++) {
        const double v = m.var[(size_t)rs.g * D + d];
        prod *= v > 0 ? 1 / v : 0;
      }
      const double peak = (prod > 0 ? std::log(std::sqrt(prod)) : prod) + rs.logw;
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
    const int64_t t = r / TILE_ROWS;
    const int jrow = (int)(r % TILE_ROWS);
    const int mb = jrow / 32, m32 = jrow % 32;
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
      const int slab = k / 16, hk = (k % 16) / 8, i = k % 8;
      const int lane = hk * 32 + m32;
      for (int sp = 0; sp < 2; sp++) {
        size_t idx = (size_t)t * tile_elems + ((((size_t)slab * 2 + sp) * 2 + mb) * 64 + lane) * 8 + i;
        a[idx] = hs[sp];
      }
    }
  }
  if (m.n_pg() > 0) L.pg_tab.upload(tab.data(), tab.size());
  L.a16h.upload(a.data(), a.size());
  L.f16tab.upload(tab.data(), (size_t)3 * KH);   // (the first group's: what single-pivot launches read)
  return true;
}

static inline int64_t track_row(int64_t pos, int h, int e) {
  // quad position `pos` of track h, element e -> row in the tile-major layout
  int64_t t = pos / 8;
  int mb = (int)((pos / 4) % 2), q = (int)(pos % 4);
  return t * TILE_ROWS + mb * 32 + 8 * q + 4 * h + e;
}

// Which states the two-term fp16 form may score (gmm.h, KAPPA_LIMIT_F16): every Gaussian of the state that stays on
// the matrix path is below the conditioning limits.  Range and clamp conditions are checked when the rows are packed.
static void f16x2_state_eligibility(const aasr_gmm *g, std::vector<uint8_t> &ok) {
  const HostModel &m = g->host;
  const int D = m.dim;
  const double lim2 = m.dim < 8 ? KAPPA2_LIMIT_F16_LOWDIM : KAPPA2_LIMIT_F16;
  std::vector<uint8_t> g_ok((size_t)m.G, 1);
  for (int64_t i = 0; i < m.G; i++) {
    if (!g->outlier.empty() && g->outlier[(size_t)i]) continue;   // a null row in every matrix layout
    double k = 0, k2 = 0;
    for (int d = 0; d < D; d++) {
      const double v = m.var[(size_t)i * D + d];
      const double p = v > 0 ? 1 / v : 0;
      const double mc = m.mean[(size_t)i * D + d] - (double)g->pivot[d];
      k += p * mc * mc;
      k2 += (p * mc * mc) * (p * mc * mc);
    }
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
    double prod = 1;
    for (int d = 0; d < D; d++) {
      double v = m.var[(size_t)gi * D + d];
      double p = v > 0 ? 1 / v : 0;
      prod *= p;
      const double mu = m.mean[(size_t)gi * D + d];
      float *gq = &recs[r * rec + (size_t)(d / 4) * 16];
      gq[d % 4] = (float)mu;
      gq[4 + d % 4] = (float)(mu - (double)(float)mu);
      gq[8 + d % 4] = (float)(-0.5 * p * kLog2e);
    }
    double cst = (prod > 0) ? std::log(std::sqrt(prod)) : prod;
    double c = cst + (pool ? 0.0 : m.logw(k));
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

static int centred_dimp_for(int D) {
  for (int c : {8, 16, 24, 32, 40, 48, 64})
    if (D <= c) return c;
  return 0;
}

// Conditioning of the expanded form, kappa_g = sum_d p (mu - pivot)^2 per Gaussian (and its 2-norm
// over d, KAPPA2_LIMIT).  A model whose worst Gaussian exceeds a limit is scored entirely in the centred form -- unless the
// offenders are a minority (at most a quarter of the mixture components): then only they are,
// over the states that hold them (outlier routing), and the rest keeps the matrix path.
static void find_outliers(aasr_gmm *g) {
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
    double k = 0, k2 = 0;
    for (int d = 0; d < D; d++) {
      double v = m.var[(size_t)i * D + d];
      double p = v > 0 ? 1 / v : 0;
      double mc = m.mean[(size_t)i * D + d] - (double)g->pivot[d];
      k += p * mc * mc;
      k2 += (p * mc * mc) * (p * mc * mc);
    }
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
static bool cholesky_lower(int d, const double *a, std::vector<double> &r) {
  r.assign((size_t)d * d, 0.0);
  for (int j = 0; j < d; j++) {
    double s = a[(size_t)j * d + j];
    for (int k = 0; k < j; k++) s -= r[(size_t)j * d + k] * r[(size_t)j * d + k];
    if (!(s > 0)) return false;
    double rjj = std::sqrt(s);
    r[(size_t)j * d + j] = rjj;
    for (int i = j + 1; i < d; i++) {
      double t = 0.5 * (a[(size_t)i * d + j] + a[(size_t)j * d + i]);
      for (int k = 0; k < j; k++) t -= r[(size_t)i * d + k] * r[(size_t)j * d + k];
      r[(size_t)i * d + j] = t / rjj;
    }
  }
  return true;
}

static void invert_lower(int d, const std::vector<double> &r, std::vector<double> &w) {
  w.assign((size_t)d * d, 0.0);
  for (int c = 0; c < d; c++) {
    w[(size_t)c * d + c] = 1.0 / r[(size_t)c * d + c];
    for (int i = c + 1; i < d; i++) {
      double s = 0;
      for (int k = c; k < i; k++) s += r[(size_t)i * d + k] * w[(size_t)k * d + c];
      w[(size_t)i * d + c] = -s / r[(size_t)i * d + i];
    }
  }
}

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
      double det = 1;
      for (int i = 0; i < D; i++) det *= X[(size_t)i * (D + 1) + 1 + i];
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
      for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
        const int64_t t = r / TILE_ROWS;
        const int jrow = (int)(r % TILE_ROWS);
        const int mb = jrow / 32, m32 = jrow % 32;
        for (int k = 0; k <= D; k++) {
          const float x = (float)coef[(size_t)r * K2 + k];
          float b1, b2, b3;
          const uint16_t hs[3] = {bf16_rne(x, &b1), bf16_rne(x - b1, &b2), bf16_rne((x - b1) - b2, &b3)};
          const int slab = k / 16, hk = (k % 16) / 8, i = k % 8;
          const int lane = hk * 32 + m32;
          for (int sp = 0; sp < 3; sp++)
            a[(size_t)t * tile_elems + ((((size_t)slab * 3 + sp) * 2 + mb) * 64 + lane) * 8 + i] = hs[sp];
        }
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
        for (int64_t r = 0; r < tiles * TILE_ROWS; r++) {
          const int64_t t = r / TILE_ROWS;
          const int jrow = (int)(r % TILE_ROWS);
          const int mb = jrow / 32, m32 = jrow % 32;
          for (int k = 0; k <= D; k++) {
            const double x = std::ldexp(coef[(size_t)r * K2 + k], k < D ? sk[(size_t)k] : 0);   // split on the host in double
            const _Float16 hi = (_Float16)x;
            const _Float16 lo = (_Float16)(x - (double)hi);
            uint16_t hs[2];
            memcpy(&hs[0], &hi, 2);
            memcpy(&hs[1], &lo, 2);
            const int slab = k / 16, hk = (k % 16) / 8, i = k % 8;
            const int lane = hk * 32 + m32;
            for (int sp = 0; sp < 2; sp++)
              ah[(size_t)t * tile_h + ((((size_t)slab * 2 + sp) * 2 + mb) * 64 + lane) * 8 + i] = hs[sp];
          }
        }
        L.a16h.upload(ah.data(), ah.size());
        L.f16scale.upload(scale.data(), scale.size());
      }
    }
  }
  L.ok = true;
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
    double det = 1;
    for (int i = 0; i < D; i++) {
      b[(size_t)i] = W[(size_t)i * (D + 1)];
      for (int j = 0; j < D; j++) A[(size_t)i * D + j] = W[(size_t)i * (D + 1) + 1 + j];
      det *= A[(size_t)i * D + i];
    }
    g->class_a[(size_t)c].upload(A.data(), A.size());
    g->class_b[(size_t)c].upload(b.data(), b.size());
    g->class_logdet[(size_t)c] = det != 0 ? std::log(std::fabs(det)) : -INFINITY;
  }
  g->class_routing = true;
}

void gmm_set_transforms(aasr_gmm *g, int32_t n_transforms, const int32_t *gauss_to_transform, const double *W) {
  HostModel &cur = g->host;
  const int D = cur.dim;
  bool global = n_transforms == 1;
  if (global)
    for (int64_t i = 0; i < cur.G && global; i++) global = gauss_to_transform[i] == 0;
  if (!g->dim_parts.empty()) {
    // feature dimension > 63 (the model as parts, gmm_dim_split_score): one transform for the whole pool is the frames
    // transformed once and |det| on every component; regression classes are not built there
    if (n_transforms > 0 && !global) {   // regression classes: rebuild as class sub-models (gmm_build)
      HostModel m = cur;
      m.n_transforms = n_transforms;
      m.g2t.assign(gauss_to_transform, gauss_to_transform + m.G);
      m.xform.assign(W, W + (size_t)n_transforms * D * (D + 1));
      g->pool_built = g->pool_centred_built = g->f64_built = false;
      gmm_build(g, m);
      return;
    }
    cur.n_transforms = n_transforms;
    cur.g2t.clear();
    cur.xform.clear();
    g->f64_built = false;
    if (n_transforms == 0) {
      g->xf_a.release();
      g->xf_b.release();
      g->out_bias_ln = 0;
      return;
    }
    cur.g2t.assign(gauss_to_transform, gauss_to_transform + cur.G);
    cur.xform.assign(W, W + (size_t)D * (D + 1));
    std::vector<double> A((size_t)D * D), b((size_t)D);
    double det = 1;
    for (int i = 0; i < D; i++) {
      b[(size_t)i] = W[(size_t)i * (D + 1)];
      for (int j = 0; j < D; j++) A[(size_t)i * D + j] = W[(size_t)i * (D + 1) + 1 + j];
      det *= A[(size_t)i * D + i];   // the reference's "determinant": the product of the diagonal (LinearAlgebra.cc:73-86)
    }
    g->xf_a.upload(A.data(), A.size());
    g->xf_b.upload(b.data(), b.size());
    g->out_bias_ln = std::log(std::fabs(det));
    return;
  }
  // In place: none / one transform for the whole pool, over rows packed without a bias, on the
  // kernels that take the bias at their output (the track layouts; the centred form through an extra pass; outlier
  // routing adds it to the centred share when it merges).  A
  // speaker change then costs two small uploads instead of re-packing every row (70 ms at 50 k
  // Gaussians).
  if ((n_transforms == 0 || global) && g->rows_unbiased && !cur.any_full() && !g->class_routing &&
      (g->paired.ok || g->tracks.ok || (g->ill_conditioned && g->centred_ok))) {
    cur.n_transforms = n_transforms;
    cur.g2t.clear();
    cur.xform.clear();
    g->pool_built = false;
    g->pool_centred_built = false;
    g->f64_built = false;
    if (n_transforms == 0) {
      g->xf_a.release();
      g->xf_b.release();
      g->out_bias_ln = 0;
      return;
    }
    cur.g2t.assign(gauss_to_transform, gauss_to_transform + cur.G);
    cur.xform.assign(W, W + (size_t)D * (D + 1));
    std::vector<double> A((size_t)D * D), b((size_t)D);
    double det = 1;
    for (int i = 0; i < D; i++) {
      b[(size_t)i] = W[(size_t)i * (D + 1)];
      for (int j = 0; j < D; j++) A[(size_t)i * D + j] = W[(size_t)i * (D + 1) + 1 + j];
      det *= A[(size_t)i * D + i];
    }
    g->xf_a.upload(A.data(), A.size());
    g->xf_b.upload(b.data(), b.size());
    g->out_bias_ln = std::log(std::fabs(det));  // -inf for a zero diagonal: every state at the floor
    return;
  }
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

// AASR_PREC_F64 operands: per mixture component the reference's own quantities in double --
// mean, precision (1 / variance, 0 for a non-positive variance), the constant log sqrt(prod
// precision) (0 when the product is not positive: the "invalid" Gaussian,
// aku/Distributions.cc:1117-1135) and the normalised mixture weight.
void gmm_build_f64(aasr_gmm *g) {
  if (g->f64_built) return;
  const HostModel &m = g->host;
  const int D = m.dim;
  // the frame vector is a per-lane array of doubles, instances up to 192 dimensions.  What the compiler makes of it in
  // k_stats_items (code object notes, tests/test_kernel_notes.py): in registers without scratch up to <128> (255 VGPRs
  // at <96>, 256 + 82 AGPRs at <128>); <192> would need 384 for the frame alone, takes all 512 (256 + 256 AGPRs) and
  // still spills 97 VGPRs, 248 bytes of scratch per lane
  const int dimp = D <= 64 ? centred_dimp_for(D) : D <= 96 ? 96 : D <= 128 ? 128 : D <= 192 ? 192 : 0;
  if (!dimp) raise(AASR_ERR_UNSUPPORTED, "no f64 kernel instance for dimension %d", D);
  const int rec = 2 * dimp + 2;
  const size_t K = m.mix_idx.size();
  std::vector<double> recs(std::max<size_t>(K, 1) * rec, 0.0);
  for (size_t k = 0; k < K; k++) {
    const int64_t gi = m.mix_idx[k];
    double prod = 1;
    for (int d = 0; d < D; d++) {
      const double v = m.var[(size_t)gi * D + d];
      const double p = v > 0 ? 1 / v : 0;
      prod *= p;
      recs[k * rec + d] = m.mean[(size_t)gi * D + d];
      recs[k * rec + dimp + d] = p;
    }
    recs[k * rec + 2 * dimp] = prod > 0 ? std::log(std::sqrt(prod)) : prod;
    recs[k * rec + 2 * dimp + 1] = m.mix_w[k];
  }
  g->f64_recs.upload(recs.data(), recs.size());
  g->f64_state_off.upload(m.mix_off.data(), m.mix_off.size());
  g->f64_det = 1.0;
  if (m.n_transforms > 0 && m.global_xform()) {
    // W = [b | A] (ConstrainedMllr::load_transform); determinant = the product of A's diagonal
    // (full_matrix_determinant, aku/LinearAlgebra.cc:73-86)
    std::vector<double> A((size_t)D * D), b((size_t)D);
    double det = 1;
    for (int i = 0; i < D; i++) {
      b[(size_t)i] = m.xform[(size_t)i * (D + 1)];
      for (int j = 0; j < D; j++) A[(size_t)i * D + j] = m.xform[(size_t)i * (D + 1) + 1 + j];
      det *= A[(size_t)i * D + i];
    }
    g->f64_A.upload(A.data(), A.size());
    g->f64_b.upload(b.data(), b.size());
    g->f64_det = std::fabs(det);
  }
  g->f64_classes = 0;
  if (m.n_transforms > 0 && !m.global_xform()) {
    // regression classes: class c = transform c - 1 (class 0: Gaussians without one); per class
    // W = [b | A] and |prod diag A| as above, per record the class of its Gaussian
    const int nc = m.n_transforms + 1;
    std::vector<double> A((size_t)nc * D * D, 0.0), b((size_t)nc * D, 0.0), det((size_t)nc, 1.0);
    for (int i = 0; i < D; i++) A[(size_t)i * D + i] = 1.0;  // class 0: identity
    for (int t = 0; t < m.n_transforms; t++) {
      const double *W = &m.xform[(size_t)t * D * (D + 1)];
      double dt = 1;
      for (int i = 0; i < D; i++) {
        b[(size_t)(t + 1) * D + i] = W[(size_t)i * (D + 1)];
        for (int j = 0; j < D; j++) A[((size_t)(t + 1) * D + i) * D + j] = W[(size_t)i * (D + 1) + 1 + j];
        dt *= W[(size_t)i * (D + 1) + 1 + i];
      }
      det[(size_t)t + 1] = std::fabs(dt);
    }
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

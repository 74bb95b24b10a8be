// gmm_files.cc -- readers of the model's text files into a HostModel.  Needs no device.
//
// File formats: PDFPool::read_gk (aku/Distributions.cc:2811-2910),
// DiagonalGaussian::read (:1131-1150), HmmSet::read_mc (aku/HmmSet.cc:156-180),
// Mixture::read (aku/Distributions.cc:2418-2434), HmmSet::read_legacy_ph
// (aku/HmmSet.cc:194-329).
#include <map>
#include <cmath>
#include <cstdlib>
#include <fstream>

#include "gmm_build.h"

namespace aasr {

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

// inverse and log-determinant of an SPD matrix through its Cholesky factor
static bool spd_inverse(int d, const std::vector<double> &a, std::vector<double> &inv, double *logdet) {
  std::vector<double> l, w;
  if (!cholesky_lower(d, a.data(), l)) return false;
  invert_lower(d, l, w);
  double ld = 0;
  for (int c = 0; c < d; c++) ld += 2.0 * std::log(l[(size_t)c * d + c]);
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

}  // namespace aasr

// mllr.cc -- constrained MLLR estimation (aku/mllr.cc, aku/MllrTrainer.cc): the statistics handle that drives the
// device accumulation (mllr_accum.hip), the host solver of MllTrainerComponent::calculate_transform /
// calculate_alpha (MllrTrainer.cc:165-253) in double with its own LU, and the mllr main loop over a recipe
// (aasr_run_mllr_recipe, mllr.cc:54-71, 126-145, 213-332), over .phn files or, with aasr_run_mllr_networks_recipe, over
// the recipe's HMM networks (mllr.cc:73-104: network_pass.h, fb_frame_entries.hip, mllr_entries.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "common.h"
#include "feat.h"
#include "gmm.h"
#include "mllr.h"
#include "mllt.h"
#include "network_pass.h"
#include "recipe_pass.h"

using namespace aasr;

// ---- the statistics handle ---------------------------------------------------------------------

struct aasr_mllr {
  aasr_gmm *gmm = nullptr;
  int D = 0, S = 0, max_comps = 0;
  int64_t SL = 0;  // doubles of the accumulator and of one slab
  DevBuf<double> inv_var, mean_var, w, u, slab, acc;
  DevBuf<int32_t> d_pdf, ok;
  std::vector<int32_t> h_pdf;  // host staging of the last call's pdfs, kept until their upload is done
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  bool fetched = false;
  std::vector<double> h_acc;
  ~aasr_mllr() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace aasr {

static void check_mllr_model(const aasr_gmm *g) {
  if (g->host.any_full() || !g->host.gauss_bias.empty())
    raise(AASR_ERR_UNSUPPORTED, "mllr: full-covariance and subspace Gaussians are not supported (diagonal pools only)");
  if (g->host.n_transforms > 0)
    raise(AASR_ERR_UNSUPPORTED, "mllr: the statistics are collected on the unadapted model (a model transform is loaded)");
}

// The launches of a call, each of at most MLLR_CHUNK MLLR_MAX_CHUNKS frames: they follow each other on the stream and
// share w, u, ok and the slab.  Per launch pass1(p, f0), which launches pass 1 for the frames from f0 on (p.x and p.n are
// set; it adds what its kernel reads of the frames), then the rank pass.
template <class Pass1>
static void mllr_launches(aasr_mllr *h, const double *d_frames, int64_t n_frames, hipStream_t st, Pass1 pass1) {
  const int64_t launch = (int64_t)MLLR_CHUNK * MLLR_MAX_CHUNKS;
  const int64_t cap = std::min(launch, n_frames);
  h->w.ensure((size_t)cap * h->D);
  h->u.ensure((size_t)cap * (h->D + 1));
  h->ok.ensure((size_t)cap);
  h->slab.ensure((size_t)((cap + MLLR_CHUNK - 1) / MLLR_CHUNK) * h->SL);
  MllrParams p{};
  p.dim = h->D;
  p.recs = h->gmm->f64_recs.p;
  p.dimp = h->gmm->f64_dimp;
  p.rec = 2 * p.dimp + 2;
  p.state_off = h->gmm->f64_state_off.p;
  p.inv_var = h->inv_var.p;
  p.mean_var = h->mean_var.p;
  p.max_comps = h->max_comps;
  p.w = h->w.p;
  p.u = h->u.p;
  p.ok = h->ok.p;
  for (int64_t f0 = 0; f0 < n_frames; f0 += launch) {
    p.x = d_frames + (size_t)f0 * h->D;
    p.n = (int32_t)std::min(launch, n_frames - f0);
    pass1(p, f0);
    mllr_rank_launch(p, h->slab.p, h->acc.p, st);
  }
  h->fetched = false;
}

}  // namespace aasr

extern "C" {

aasr_status aasr_mllr_create(aasr_gmm *gmm, aasr_mllr **out) {
  return guarded([&] {
    if (!gmm || !out) raise(AASR_ERR_INVALID, "aasr_mllr_create: null argument");
    *out = nullptr;
    check_mllr_model(gmm);
    const HostModel &m = gmm->host;
    if (m.dim < 1 || m.dim > MLLR_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "mllr: no accumulation kernel for dimension %d (1 ... %d)", m.dim, MLLR_MAX_DIM);
    int max_comps = 0;
    for (int64_t s = 0; s < m.S; s++) max_comps = std::max(max_comps, m.mix_off[(size_t)s + 1] - m.mix_off[(size_t)s]);
    if (mllr_weights_lds_bytes(m.dim, max_comps) > 60 * 1024)
      raise(AASR_ERR_UNSUPPORTED, "mllr: mixtures of %d components exceed the weight kernel's LDS", max_comps);
    require_device();
    std::unique_ptr<aasr_mllr> h(new aasr_mllr());
    h->gmm = gmm;
    h->D = m.dim;
    h->S = (int)m.S;
    h->max_comps = max_comps;
    h->SL = mllr_slab_doubles(h->D);
    gmm_build_f64(gmm);
    // per record 1 / covar and mean / covar as MllTrainerComponent::collect_data forms them (MllrTrainer.cc:155-159);
    // a non-positive variance has precision 0 in the records (gmm_build_f64's rule) and weighs nothing here
    const size_t K = m.mix_idx.size();
    std::vector<double> iv(std::max<size_t>(1, K) * h->D, 0.0), mv(std::max<size_t>(1, K) * h->D, 0.0);
    for (size_t k = 0; k < K; k++) {
      const int64_t gi = m.mix_idx[k];
      for (int d = 0; d < h->D; d++) {
        const double v = m.var[(size_t)gi * h->D + d];
        iv[k * h->D + d] = v > 0 ? 1 / v : 0;
        mv[k * h->D + d] = v > 0 ? m.mean[(size_t)gi * h->D + d] / v : 0;
      }
    }
    h->inv_var.upload(iv.data(), iv.size());
    h->mean_var.upload(mv.data(), mv.size());
    h->acc.alloc((size_t)h->SL);
    AASR_HIP(hipMemset(h->acc.p, 0, h->acc.n * sizeof(double)));
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

void aasr_mllr_destroy(aasr_mllr *h) { delete h; }

aasr_status aasr_mllr_reset(aasr_mllr *h, void *stream) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_mllr_reset: null argument");
    AASR_HIP(hipMemsetAsync(h->acc.p, 0, h->acc.n * sizeof(double), (hipStream_t)stream));
    h->fetched = false;
  });
}

aasr_status aasr_mllr_accumulate_dev(aasr_mllr *h, const double *d_frames, int64_t n_frames, const int32_t *pdf,
                                     void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || (n_frames > 0 && (!d_frames || !pdf)))
      raise(AASR_ERR_INVALID, "aasr_mllr_accumulate_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_mllr_accumulate_dev: more than 2^31 frames in one call");
    if (n_frames == 0) return;
    check_mllr_model(h->gmm);
    for (int64_t f = 0; f < n_frames; f++)
      if (pdf[f] >= h->S)
        raise(AASR_ERR_INVALID, "aasr_mllr_accumulate_dev: pdf %d of frame %ld out of range", pdf[f], (long)f);
    const hipStream_t st = (hipStream_t)stream;
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    h->h_pdf.assign(pdf, pdf + n_frames);
    h->d_pdf.ensure((size_t)n_frames);
    AASR_HIP(hipMemcpyAsync(h->d_pdf.p, h->h_pdf.data(), (size_t)n_frames * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AASR_HIP(hipEventRecord(h->staged, st));
    h->staged_pending = true;
    mllr_launches(h, d_frames, n_frames, st, [&](MllrParams &p, int64_t f0) {
      p.pdf = h->d_pdf.p + f0;
      mllr_weights_launch(p, st);
    });
  });
}

aasr_status aasr_mllr_accumulate_weighted_dev(aasr_mllr *h, const double *d_frames, int64_t n_frames, const int64_t *d_off,
                                              const int32_t *d_pdf, const double *d_weight, int64_t n_entries, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || n_entries < 0 || (n_frames > 0 && (!d_frames || !d_off)) || (n_entries > 0 && (!d_pdf || !d_weight)))
      raise(AASR_ERR_INVALID, "aasr_mllr_accumulate_weighted_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_mllr_accumulate_weighted_dev: more than 2^31 frames in one call");
    if (n_frames == 0) return;
    check_mllr_model(h->gmm);
    const hipStream_t st = (hipStream_t)stream;
    MllrEntryParams q{};
    q.pdf = d_pdf;
    q.weight = d_weight;
    q.n_entries = n_entries;
    q.n_states = h->S;
    mllr_launches(h, d_frames, n_frames, st, [&](MllrParams &p, int64_t f0) {
      q.p = p;
      q.off = d_off + f0;
      mllr_entry_weights_launch(q, st);
    });
  });
}

aasr_status aasr_mllr_fetch(aasr_mllr *h, void *stream) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_mllr_fetch: null argument");
    const hipStream_t st = (hipStream_t)stream;
    h->h_acc.resize((size_t)h->SL);
    AASR_HIP(hipMemcpyAsync(h->h_acc.data(), h->acc.p, (size_t)h->SL * sizeof(double), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
    h->staged_pending = false;
    h->fetched = true;
  });
}

aasr_status aasr_mllr_get(const aasr_mllr *h, double *G, double *k, double *beta) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_mllr_get: null argument");
    if (!h->fetched) raise(AASR_ERR_INVALID, "aasr_mllr_get: call aasr_mllr_fetch after the last accumulation");
    const int D = h->D, E = D + 1, PB = mllr_pb(D), NT = mllr_g_tiles(PB);
    const double *a = h->h_acc.data();
    // the tiles on and below the diagonal, mirrored
    if (G)
      for (int i = 0; i < D; i++)
        for (int r = 0; r < E; r++)
          for (int c = 0; c <= r; c++) {
            const int R = r / 16, C = c / 16;
            const double v = a[((size_t)i * NT + (size_t)R * (R + 1) / 2 + C) * 256 + (r % 16) * 16 + c % 16];
            G[((size_t)i * E + r) * E + c] = v;
            G[((size_t)i * E + c) * E + r] = v;
          }
    const double *kt = a + (size_t)D * NT * 256;
    auto kat = [&](int r, int c) { return kt[((size_t)(r / 16) * PB + c / 16) * 256 + (r % 16) * 16 + c % 16]; };
    if (k)
      for (int i = 0; i < D; i++)
        for (int c = 0; c < E; c++) k[(size_t)i * E + c] = kat(i, c);
    if (beta) *beta = kat(D, 0);
  });
}

}  // extern "C"

// ---- the host solver ---------------------------------------------------------------------------

namespace aasr {

// LU with partial pivoting of the n x n row-major matrix a in place (dgetrf's algorithm: the pivot of a column is its
// entry of largest magnitude at or below the diagonal, the first such), the inverse from the factors (dgetri's
// result); *det: the product of U's diagonal WITHOUT the permutation's sign, which is what the reference multiplies
// up after LUFactorizeIP (MllrTrainer.cc:207-211).  false: a zero pivot.
bool lu_inverse(std::vector<double> &a, int n, double *det) {  // shared with estimate.cc (mllt.h)
  std::vector<int> piv((size_t)n);
  for (int c = 0; c < n; c++) {
    int p = c;
    double best = std::fabs(a[(size_t)c * n + c]);
    for (int r = c + 1; r < n; r++)
      if (std::fabs(a[(size_t)r * n + c]) > best) {
        best = std::fabs(a[(size_t)r * n + c]);
        p = r;
      }
    piv[(size_t)c] = p;
    if (!(best > 0)) return false;  // (a NaN column as well)
    if (p != c)
      for (int j = 0; j < n; j++) std::swap(a[(size_t)c * n + j], a[(size_t)p * n + j]);
    const double d = a[(size_t)c * n + c];
    for (int r = c + 1; r < n; r++) {
      const double l = a[(size_t)r * n + c] / d;
      a[(size_t)r * n + c] = l;
      if (l != 0)
        for (int j = c + 1; j < n; j++) a[(size_t)r * n + j] -= l * a[(size_t)c * n + j];
    }
  }
  if (det) {
    double d = 1;
    for (int i = 0; i < n; i++) d *= a[(size_t)i * n + i];
    *det = d;
  }
  // P A = L U: A^-1 = U^-1 L^-1 P, column by column
  std::vector<double> inv((size_t)n * n), y((size_t)n);
  for (int c = 0; c < n; c++) {
    for (int i = 0; i < n; i++) y[(size_t)i] = 0;
    y[(size_t)c] = 1;
    for (int i = 0; i < n; i++) {  // L z = e_c
      double s = y[(size_t)i];
      for (int j = 0; j < i; j++) s -= a[(size_t)i * n + j] * y[(size_t)j];
      y[(size_t)i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {  // U v = z
      double s = y[(size_t)i];
      for (int j = i + 1; j < n; j++) s -= a[(size_t)i * n + j] * y[(size_t)j];
      y[(size_t)i] = s / a[(size_t)i * n + i];
    }
    for (int i = 0; i < n; i++) inv[(size_t)i * n + c] = y[(size_t)i];
  }
  // ... times P: undo the row exchanges as column exchanges, last first
  for (int c = n - 1; c >= 0; c--)
    if (piv[(size_t)c] != c)
      for (int i = 0; i < n; i++) std::swap(inv[(size_t)i * n + c], inv[(size_t)i * n + piv[(size_t)c]]);
  a.swap(inv);
  return true;
}

// x^T (A y) (MllTrainerComponent::get_product)
static double xAy(const std::vector<double> &x, const double *A, const double *y, int n, std::vector<double> &work) {
  for (int i = 0; i < n; i++) {
    double s = 0;
    for (int j = 0; j < n; j++) s += A[(size_t)i * n + j] * y[j];
    work[(size_t)i] = s;
  }
  double s = 0;
  for (int i = 0; i < n; i++) s += x[(size_t)i] * work[(size_t)i];
  return s;
}

// MllTrainerComponent::calculate_transform (MllrTrainer.cc:165-231)
static void mllr_solve(int dim, const double *G, const double *k, double beta, double *W) {
  const int E = dim + 1;
  std::vector<std::vector<double>> inv_G((size_t)dim);
  for (int i = 0; i < dim; i++) {
    inv_G[(size_t)i].assign(G + (size_t)i * E * E, G + (size_t)(i + 1) * E * E);
    if (!lu_inverse(inv_G[(size_t)i], E, nullptr)) raise(AASR_ERR_INVALID, "mllr: zero pivot in G_%d (singular statistics)", i);
  }
  std::vector<double> trans((size_t)dim * E, 0.0), A((size_t)dim * dim), p((size_t)E), w((size_t)E), work((size_t)E);
  for (int i = 0; i < dim; i++) trans[(size_t)i * E + i + 1] = 1;
  for (int round = 0; round < 20 * dim; round++) {
    const int row = round % dim;
    for (int i = 0; i < dim; i++)
      for (int j = 0; j < dim; j++) A[(size_t)j * dim + i] = trans[(size_t)i * E + j + 1];
    double detA = 1;
    if (!lu_inverse(A, dim, &detA)) raise(AASR_ERR_INVALID, "mllr: zero pivot in A (round %d)", round);
    p[0] = 0;
    for (int i = 0; i < dim; i++) p[(size_t)i + 1] = detA * A[(size_t)row * dim + i];  // the cofactor row: detA A^-1
    const double *Gi = inv_G[(size_t)row].data(), *kr = k + (size_t)row * E;
    // calculate_alpha (MllrTrainer.cc:233-253)
    const double c2 = xAy(p, Gi, p.data(), E, work);
    const double c1 = xAy(p, Gi, kr, E, work);
    const double a1 = (-c1 + std::sqrt(c1 * c1 + 4 * c2 * beta)) / (2 * c2);
    const double a2 = (-c1 - std::sqrt(c1 * c1 + 4 * c2 * beta)) / (2 * c2);
    const double m1 = beta * std::log(std::fabs(a1 * c2 + c1)) - (c2 / 2) * a1 * a1;
    const double m2 = beta * std::log(std::fabs(a2 * c2 + c1)) - (c2 / 2) * a2 * a2;
    const double alpha = m1 > m2 ? a1 : a2;
    for (int i = 0; i < E; i++) p[(size_t)i] = alpha * p[(size_t)i] + kr[i];
    for (int i = 0; i < E; i++) {  // w = inv_G^T p
      double s = 0;
      for (int j = 0; j < E; j++) s += Gi[(size_t)j * E + i] * p[(size_t)j];
      w[(size_t)i] = s;
    }
    for (int i = 0; i < E; i++) trans[(size_t)row * E + i] = w[(size_t)i];
  }
  std::copy(trans.begin(), trans.end(), W);
}

// MllrTrainer::calculate_transform(LinTransformModule *) (MllrTrainer.cc:98-145): W = [b | A], composed with the
// module's transform when it has one, narrowed to float
static void mllr_compose(int dim, const double *W, const float *old_A, const float *old_b, float *A_out, float *b_out) {
  const int E = dim + 1;
  std::vector<double> A((size_t)dim * dim), b((size_t)dim);
  for (int i = 0; i < dim; i++) {
    b[(size_t)i] = W[(size_t)i * E];
    for (int j = 0; j < dim; j++) A[(size_t)i * dim + j] = W[(size_t)i * E + 1 + j];
  }
  if (old_A && old_b) {
    // line 127 is Blas_Mat_Vec_Mult(old_A, b, b): b is overwritten in place while it is read.  dgemv with beta = 0
    // clears y first, so with x and y the same vector the result is old_A * 0 = 0, and line 128 leaves b = old_b.
    // The new bias does not survive the composition in the reference; neither does it here.
    std::vector<double> nb((size_t)dim);
    for (int i = 0; i < dim; i++) nb[(size_t)i] = 0.0 + 1.0 * (double)old_b[i];
    std::vector<double> nA((size_t)dim * dim);
    for (int i = 0; i < dim; i++)
      for (int j = 0; j < dim; j++) {
        double s = 0;
        for (int l = 0; l < dim; l++) s += A[(size_t)i * dim + l] * (double)old_A[(size_t)l * dim + j];
        nA[(size_t)i * dim + j] = s;
      }
    A.swap(nA);
    b.swap(nb);
  }
  for (int i = 0; i < dim; i++) {
    b_out[i] = (float)b[(size_t)i];
    for (int j = 0; j < dim; j++) A_out[(size_t)i * dim + j] = (float)A[(size_t)i * dim + j];
  }
}

}  // namespace aasr

extern "C" {

aasr_status aasr_mllr_solve(int32_t dim, const double *G, const double *k, double beta, double *W) {
  return guarded([&] {
    if (dim < 1 || !G || !k || !W) raise(AASR_ERR_INVALID, "aasr_mllr_solve: bad argument");
    mllr_solve(dim, G, k, beta, W);
  });
}

aasr_status aasr_mllr_compose(int32_t dim, const double *W, const float *old_A, const float *old_b, float *A, float *b) {
  return guarded([&] {
    if (dim < 1 || !W || !A || !b || (!old_A != !old_b)) raise(AASR_ERR_INVALID, "aasr_mllr_compose: bad argument");
    mllr_compose(dim, W, old_A, old_b, A, b);
  });
}

void aasr_mllr_default_options(aasr_mllr_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->minframes = 1000;
}

}  // extern "C"

// ---- the mllr main loop over a recipe ----------------------------------------------------------

namespace {

constexpr int64_t PHN_GROUP_FRAMES = (int64_t)1 << 18;

// What the loop carries from group to group and from speaker to speaker
struct MllrRun {
  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  const aasr_topo *topo = nullptr;
  const aasr_mllr_options *opt = nullptr;
  aasr_mllr *h = nullptr;
  GroupStager *stager = nullptr;
  std::vector<RecipeInfo> infos;
  FeatModule *ltm = nullptr;  // -M: the lin_transform module that takes the transform; null: the model's cmllr block
  std::string module;
  std::vector<double> G, k, W;
  std::string cur_speaker;  // empty: no trainer yet
  int64_t num_frames = 0;
  // the network mode (aasr_run_mllr_networks_recipe)
  aasr_fb_options fo;
  NetworkCache net_cache;
  GroupScores scores;
  double total_ll = 0, max_dev = 0;  // the forward totals; max |1 - s_t| over the run
  int64_t entries = 0;
  MllrRun(const aasr_topo *topo_, int32_t num_states) : topo(topo_), net_cache(topo_, num_states) {}
};

// calculate_transform (aku/mllr.cc:39-52) for cur_speaker
void finish_speaker(MllrRun &r) {
  const int D = aasr_gmm_dim(r.gmm);
  const hipStream_t stream = r.stager->stream;
  aasr_spkc *spk = r.opt->speakers;
  if (r.opt->info > 0) {
    printf("%s: ", r.cur_speaker.c_str());
    fflush(stdout);
    fprintf(stderr, "Calculating transform for %s\n", r.cur_speaker.c_str());
  }
  double beta = 0;
  if (aasr_mllr_fetch(r.h, stream) != AASR_OK || aasr_mllr_get(r.h, r.G.data(), r.k.data(), &beta) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  try {
    mllr_solve(D, r.G.data(), r.k.data(), beta, r.W.data());
  } catch (Error &e) {
    raise(e.code, "speaker %s: %s", r.cur_speaker.c_str(), e.msg.c_str());
  }
  if (r.ltm) {
    FeatModule *ltm = r.ltm;
    std::vector<float> Af((size_t)D * D), bf((size_t)D);
    const bool defined = ltm->matrix_defined && ltm->bias_defined;  // LinTransformModule::is_defined
    mllr_compose(D, r.W.data(), defined ? ltm->matrix.data() : nullptr, defined ? ltm->bias.data() : nullptr, Af.data(),
                 bf.data());
    spkc_feature_rewritten(spk, r.module);  // (the stream is idle: the fetch waited)
    ltm->matrix = Af;
    ltm->bias = bf;
    ltm->matrix_defined = ltm->bias_defined = true;
    ltm->d_matrix.upload(ltm->matrix.data(), ltm->matrix.size());
    ltm->d_bias.upload(ltm->bias.data(), ltm->bias.size());
  } else {
    spkc_cmllr_add_global_transform(spk, r.W);
    if (r.opt->info > 0) {  // MllrTrainer.cc:78-80: an ostream's default formatting of a double
      std::ostringstream os;
      os << beta << " frames, " << 1 << " transform matrices";
      printf("%s\n", os.str().c_str());
      fflush(stdout);
    }
  }
  if (aasr_mllr_reset(r.h, stream) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  r.cur_speaker.clear();
}

// more lines of cur_speaker for a group that holds `lines` of them and rows_total frames
bool group_takes_more(const MllrRun &r, size_t next, size_t lines, int64_t rows_total, int64_t max_frames) {
  return next < r.infos.size() && r.infos[next].speaker_id == r.cur_speaker && lines < 1024 && rows_total < max_frames;
}

// the frames carry the speaker's CURRENT transform, as the reference's feature generator does
void stage_group(MllrRun &r, size_t group_first, const std::vector<std::vector<int16_t>> &audio,
                 const std::vector<int32_t> &start, const std::vector<int32_t> &rows) {
  r.stager->stage(audio, start, rows, [&](size_t i) {
    // set_utterance per line (aku/mllr.cc:289-290); a parameter change waits for the queued features
    const RecipeInfo &u = r.infos[group_first + i];
    if (!u.utterance_id.empty() && aasr_spkc_set_utterance(r.opt->speakers, u.utterance_id.c_str()) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  });
}

// A group over .phn files: utterances of cur_speaker from *next on, their frames in one device buffer, one accumulation.
// -> the group's frames
int64_t phn_group(MllrRun &r, const TopoTables &tt, size_t *next) {
  const float fr = aasr_feat_frame_rate(r.feat);
  const hipStream_t stream = r.stager->stream;
  const size_t group_first = *next;
  std::vector<std::vector<int16_t>> audio;
  std::vector<int32_t> start, rows, pdfs;
  int64_t rows_total = 0;
  while (group_takes_more(r, *next, audio.size(), rows_total, PHN_GROUP_FRAMES)) {
    const RecipeInfo &u = r.infos[(*next)++];
    announce(u, r.opt->info, (int)(*next - 1), (int)r.infos.size());
    audio.push_back(load_utterance_input(r.feat, u));
    // train_mllr hands the segmentator's PDF index to model.state() and takes that state's emission_pdf
    // (aku/mllr.cc:136-140): a double lookup.  In the .ph files this engine reads a state's emission pdf is the
    // state's own index (HmmSet::read_ph, legacy format) and the engine takes state == pdf throughout, so
    // both lookups are the identity here and the segmentation's index is used as it is.
    const Segmentation seg = read_state_sequence(r.topo, tt, u, r.opt->ophn != 0, fr,
                                                 aasr_feat_eof_frame(r.feat, (int64_t)audio.back().size()));
    if (!seg.initialized) audio.back().clear();
    start.push_back(seg.start_frame);
    rows.push_back((int32_t)seg.pdf.size());
    pdfs.insert(pdfs.end(), seg.pdf.begin(), seg.pdf.end());
    rows_total += (int64_t)seg.pdf.size();
  }
  stage_group(r, group_first, audio, start, rows);
  if (rows_total > 0) {
    if (aasr_mllr_accumulate_dev(r.h, r.stager->d_x.p, rows_total, pdfs.data(), stream) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    AASR_HIP(hipStreamSynchronize(stream));  // the group's host audio and pdfs go out of scope
  }
  return rows_total;
}

// A group over HMM networks (get_segmentator and train_mllr, aku/mllr.cc:73-104, 126-145): utterances of cur_speaker
// from *next on, the network step (network_pass.h), the frame-major entries, the weighted accumulation.
// -> the frames of the utterances that ran
int64_t network_group(MllrRun &r, size_t *next) {
  const float fr = aasr_feat_frame_rate(r.feat);
  const hipStream_t stream = r.stager->stream;
  const int S = aasr_gmm_num_states(r.gmm);
  const size_t group_first = *next;
  NetworkGroup g;
  while (group_takes_more(r, *next, g.size(), g.rows_total, NETWORK_GROUP_FRAMES)) {
    const RecipeInfo &u = r.infos[(*next)++];
    announce(u, r.opt->info, (int)(*next - 1), (int)r.infos.size());
    g.add(r.feat, r.net_cache, u, u.hmmnet_path, fr);
  }
  stage_group(r, group_first, g.audio, g.start, g.rows);
  // in model mode the model is the unadapted one the statistics are collected on (loading is disabled)
  const bool f64 = aasr_gmm_get_precision(r.gmm) == AASR_PREC_F64;
  const void *d_scores = nullptr;
  const FbBatchPtr batch = run_network_group(r.fo, r.gmm, *r.stager, g, r.scores, f64, &d_scores);
  aasr_fb_batch *b = batch.get();
  int64_t n_entries = 0;
  const int64_t *d_off = nullptr;
  const int32_t *d_pdf = nullptr;
  const double *d_weight = nullptr;
  if (aasr_fb_batch_frame_entries_dev(b, S, g.row0.data(), g.rows_total, stream, &n_entries, &d_off, &d_pdf, &d_weight) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  r.entries += n_entries;
  // the messages in recipe order, and the frame sums
  int64_t frames = 0;
  for (size_t i = 0; i < g.size(); i++) {
    const RecipeInfo &u = r.infos[group_first + i];
    double fw = 0;
    if (!report_network_outcome(b, i, r.fo, RetryMessages::BAUM_WELCH, u, &fw)) continue;
    check_frame_sums(b, i, g, u, &r.max_dev);
    r.total_ll += fw;  // train_mllr: get_total_log_likelihood (aku/mllr.cc:143-144)
    frames += g.rows[i];
  }
  if (n_entries > 0 &&
      aasr_mllr_accumulate_weighted_dev(r.h, r.stager->d_x.p, g.rows_total, d_off, d_pdf, d_weight, n_entries, stream) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  // the batch owns the entries that the accumulation reads: it goes when the stream is done with them
  AASR_HIP(hipStreamSynchronize(stream));
  return frames;
}

}  // namespace

// nopt: the network mode (aasr_run_mllr_networks_recipe), or NULL for the .phn files
static aasr_status run_mllr_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                   const aasr_mllr_options *opt, const aasr_mllr_network_options *nopt,
                                   aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat || !gmm || !topo || !recipe_path || !opt || !opt->speakers)
      raise(AASR_ERR_INVALID, "%s: null argument", nopt ? "aasr_run_mllr_networks_recipe" : "aasr_run_mllr_recipe");
    if (nopt && opt->ophn)
      raise(AASR_ERR_UNSUPPORTED, "mllr: -O is not supported with --networks (a network line has no segmentation to choose)");
    const auto t0 = std::chrono::steady_clock::now();
    aasr_spkc *spk = opt->speakers;
    MllrRun r(topo, aasr_gmm_num_states(gmm));
    r.feat = feat;
    r.gmm = gmm;
    r.opt = opt;
    // Recipe::read with cluster_speakers = true, then sort_infos (aku/mllr.cc:213-216)
    r.infos = read_recipe_file(recipe_path, opt->num_batches, opt->batch_index, true);
    std::stable_sort(r.infos.begin(), r.infos.end(),
                     [](const RecipeInfo &a, const RecipeInfo &b) { return a.speaker_id < b.speaker_id; });
    const std::vector<RecipeInfo> &infos = r.infos;
    refuse_line_limits(infos, "mllr");
    const int D = aasr_gmm_dim(gmm);
    check_feature_dim(gmm, feat);
    if (opt->module && opt->module[0]) {
      r.module = opt->module;
      auto it = feat->by_name.find(r.module);
      if (it == feat->by_name.end()) raise(AASR_ERR_INVALID, "unknown module requested: %s", r.module.c_str());
      r.ltm = &feat->mods[(size_t)it->second];
      if (r.ltm->type != MOD_LIN_TRANSFORM || r.ltm->dim != D || r.ltm->src_dim != D)
        raise(AASR_ERR_INVALID, "mllr: -M %s is not a lin_transform module of %d x %d", r.module.c_str(), D, D);
    } else {
      if (aasr_spkc_set_model(spk, gmm) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      spkc_cmllr_disable_loading(spk);  // the statistics are collected on the unadapted model (aku/mllr.cc:263-266)
    }
    {
      const aasr_status cs = aasr_mllr_create(gmm, &r.h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_mllr, void (*)(aasr_mllr *)> hguard(r.h, aasr_mllr_destroy);
    const TopoTables tt(topo);
    GroupStager stager(feat, spk);
    r.stager = &stager;
    const int E = D + 1;
    r.G.resize((size_t)D * E * E);
    r.k.resize((size_t)D * E);
    r.W.resize((size_t)D * E);
    network_fb_options(&r.fo, nopt ? nopt->fw_beam : 0, nopt ? nopt->bw_beam : 0, false, 1, nopt && nopt->viterbi);
    r.fo.want_pdf_occ = 1;
    r.fo.device_occ = 1;
    r.fo.max_attempts = 5;  // (counter >= 5, aku/mllr.cc:90)
    std::set<std::string> updated;

    size_t next = 0;
    while (next < infos.size()) {
      if (infos[next].speaker_id.empty()) raise(AASR_ERR_INVALID, "Speaker ID is missing");
      // set_speaker (aku/mllr.cc:54-71): the previous speaker's transform first
      if (infos[next].speaker_id != r.cur_speaker) {
        if (!r.cur_speaker.empty()) finish_speaker(r);
        r.cur_speaker = infos[next].speaker_id;
        updated.insert(r.cur_speaker);
        if (aasr_spkc_set_speaker(spk, r.cur_speaker.c_str()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      }
      r.num_frames += nopt ? network_group(r, &next) : phn_group(r, tt, &next);
    }
    if (!r.cur_speaker.empty()) finish_speaker(r);
    if (nopt && opt->info > 0) {
      fprintf(stderr, "Largest |1 - sum of PDF probabilities| of a frame: %g\n", r.max_dev);
      fprintf(stderr, "Weighted entries: %lld over %lld frames\n", (long long)r.entries, (long long)r.num_frames);
    }

    // the new speaker configuration (aku/mllr.cc:318-332)
    if (opt->out) write_speaker_file_for_batch(spk, updated, opt->num_batches, opt->batch_index, opt->out);
    if (opt->info > 0 && r.total_ll != 0) fprintf(stderr, "Total log likelihood: %f\n", r.total_ll);  // aku/mllr.cc:334-336
    fill_run_stats(stats, (int64_t)infos.size(), r.num_frames, t0, 0);
  });
}


extern "C" {

aasr_status aasr_run_mllr_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                 const aasr_mllr_options *opt, aasr_run_stats *stats) {
  return run_mllr_recipe(feat, gmm, topo, recipe_path, opt, nullptr, stats);
}

void aasr_mllr_network_default_options(aasr_mllr_network_options *o) {
  if (o) memset(o, 0, sizeof *o);
}

aasr_status aasr_run_mllr_networks_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                          const aasr_mllr_options *opt, const aasr_mllr_network_options *net,
                                          aasr_run_stats *stats) {
  return run_mllr_recipe(feat, gmm, topo, recipe_path, opt, net && net->networks ? net : nullptr, stats);
}

}  // extern "C"

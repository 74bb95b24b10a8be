// lda.cc -- LDA estimation (aku/lda.cc): the class-scatter handle that drives the device accumulation
// (scatter_accum.hip), the host solver of lda.cc:380-446 in double without LAPACK (Cholesky reduction, cyclic
// Jacobi), the state selection (lda.cc:113-115, 247-263) and the lda main loop over a recipe (aasr_run_lda_recipe,
// lda.cc:143-372, 448-462), over .phn segmentations or (aasr_run_lda_networks_recipe) with the posteriors of the
// recipe's HMM networks as weighted entries (network_pass.h, scatter_entries.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"
#include "feat.h"
#include "gmm.h"
#include "hmmnet.h"
#include "jacobi.h"
#include "network_pass.h"
#include "recipe_pass.h"
#include "scatter.h"

using namespace aasr;

// ---- the scatter handle ------------------------------------------------------------------------

struct aasr_scatter {
  int C = 0, D = 0, PB = 0;
  int64_t TS = 0;  // doubles of a class's accumulator and of an item's slab
  int64_t slab_bytes = SCATTER_SLAB_BYTES;
  DevBuf<double> acc, slab;
  DevBuf<int32_t> d_rows;
  DevBuf<ScatterItem> d_items;
  DevBuf<ScatterGroup> d_groups;
  // host staging of the last call's lists, kept until their upload is done
  std::vector<int32_t> h_rows, count;
  std::vector<ScatterItem> h_items;
  std::vector<ScatterGroup> h_groups;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  bool fetched = false;
  std::vector<double> h_acc;
  int32_t shape[3] = {0, 0, 0};
  ~aasr_scatter() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

// The launches of h->h_items, at most max_items items each (scatter.h); within a launch the items of a class are one
// group.  Uploads the items and the groups and queues the launches: by_entry, rows / weight are an entry list and its
// weights (k_scatter_entries), otherwise the compressed row list and the frames' weights or null (k_scatter_items).
static void scatter_queue_items(aasr_scatter *h, const double *d_frames, const int32_t *d_rows, const double *d_weight,
                                bool by_entry, hipStream_t st) {
  const int64_t NI = (int64_t)h->h_items.size();
  const int64_t max_items =
      std::max<int64_t>(1, std::min<int64_t>(SCATTER_MAX_ITEMS, h->slab_bytes / (h->TS * (int64_t)sizeof(double))));
  struct Launch {
    int item0, n_items, group0, n_groups;
  };
  std::vector<Launch> launches;
  h->h_groups.clear();
  for (int64_t i0 = 0; i0 < NI; i0 += max_items) {
    const int n = (int)std::min(max_items, NI - i0);
    Launch L{(int)i0, n, (int)h->h_groups.size(), 0};
    for (int i = 0; i < n; i++) {
      const int32_t c = h->h_items[(size_t)(i0 + i)].cls;
      if (L.n_groups > 0 && h->h_groups.back().cls == c) h->h_groups.back().count++;
      else {
        h->h_groups.push_back(ScatterGroup{c, i, 1, 0});
        L.n_groups++;
      }
    }
    launches.push_back(L);
  }
  h->d_items.ensure(h->h_items.size());
  h->d_groups.ensure(h->h_groups.size());
  h->slab.ensure((size_t)std::min(NI, max_items) * h->TS);
  AASR_HIP(hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(ScatterItem), hipMemcpyHostToDevice, st));
  AASR_HIP(hipMemcpyAsync(h->d_groups.p, h->h_groups.data(), h->h_groups.size() * sizeof(ScatterGroup), hipMemcpyHostToDevice, st));
  AASR_HIP(hipEventRecord(h->staged, st));
  h->staged_pending = true;
  ScatterParams p{};
  p.x = d_frames;
  p.weight = d_weight;
  p.rows = d_rows;
  p.items = h->d_items.p;
  p.dim = h->D;
  for (const Launch &L : launches) {  // (the launches of a call follow each other on the stream and share the slab)
    if (by_entry) scatter_entries_launch(p, L.item0, L.n_items, h->d_groups.p + L.group0, L.n_groups, h->slab.p, h->acc.p, st);
    else scatter_launch(p, L.item0, L.n_items, h->d_groups.p + L.group0, L.n_groups, h->slab.p, h->acc.p, st);
  }
  h->shape[0] = h->PB;
  h->shape[1] = (int32_t)NI;
  h->shape[2] = (int32_t)launches.size();
  h->fetched = false;
}

extern "C" {

aasr_status aasr_scatter_create(int32_t n_classes, int32_t dim, aasr_scatter **out) {
  return guarded([&] {
    if (!out || n_classes < 1 || dim < 1) raise(AASR_ERR_INVALID, "aasr_scatter_create: bad argument");
    *out = nullptr;
    if (dim > SCATTER_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "scatter: no accumulation kernel for dimension %d (1 ... %d)", dim, SCATTER_MAX_DIM);
    require_device();
    std::unique_ptr<aasr_scatter> h(new aasr_scatter());
    h->C = n_classes;
    h->D = dim;
    h->PB = scatter_pb(dim);
    h->TS = scatter_class_doubles(dim);
    h->acc.alloc((size_t)h->C * h->TS);
    AASR_HIP(hipMemset(h->acc.p, 0, h->acc.n * sizeof(double)));
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

void aasr_scatter_destroy(aasr_scatter *h) { delete h; }

aasr_status aasr_scatter_accumulate_dev(aasr_scatter *h, const double *d_frames, int64_t n_frames, const int32_t *cls,
                                        const double *d_weight, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || (n_frames > 0 && (!d_frames || !cls)))
      raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_dev: more than 2^31 frames in one call");
    for (int64_t f = 0; f < n_frames; f++)
      if (cls[f] < -1 || cls[f] >= h->C)
        raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_dev: class %d of frame %ld out of range", cls[f], (long)f);
    const hipStream_t st = (hipStream_t)stream;
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    // the compressed row list: the rows of class 0 in frame order, then those of class 1, ... (a counting sort)
    h->count.assign((size_t)h->C + 1, 0);
    int64_t kept = 0;
    for (int64_t f = 0; f < n_frames; f++)
      if (cls[f] >= 0) {
        h->count[(size_t)cls[f] + 1]++;
        kept++;
      }
    if (kept == 0) return;
    for (int c = 0; c < h->C; c++) h->count[(size_t)c + 1] += h->count[(size_t)c];  // now: first entry of every class
    h->h_rows.resize((size_t)kept);
    h->h_items.clear();
    for (int c = 0; c < h->C; c++)
      for (int32_t s = h->count[(size_t)c]; s < h->count[(size_t)c + 1]; s += SCATTER_ITEM)
        h->h_items.push_back(ScatterItem{s, std::min<int32_t>(SCATTER_ITEM, h->count[(size_t)c + 1] - s), c, 0});
    {
      std::vector<int32_t> &at = h->count;  // (the fill moves every class's first entry to its end)
      for (int64_t f = 0; f < n_frames; f++)
        if (cls[f] >= 0) h->h_rows[(size_t)at[(size_t)cls[f]]++] = (int32_t)f;
    }
    h->d_rows.ensure(h->h_rows.size());
    AASR_HIP(hipMemcpyAsync(h->d_rows.p, h->h_rows.data(), h->h_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    scatter_queue_items(h, d_frames, h->d_rows.p, d_weight, false, st);
  });
}

aasr_status aasr_scatter_accumulate_weighted_dev(aasr_scatter *h, const double *d_frames, int64_t n_frames, const int64_t *cnt,
                                                 const int32_t *d_rows, const double *d_weights, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || !cnt) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: more than 2^31 frames in one call");
    if (cnt[0] != 0) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: cnt[0] is %lld, not 0", (long long)cnt[0]);
    for (int c = 0; c < h->C; c++)
      if (cnt[c + 1] < cnt[c]) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: cnt decreases at class %d", c);
    const int64_t entries = cnt[h->C];
    if (entries > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: more than 2^31 entries in one call");
    if (entries == 0) return;
    if (!d_frames || !d_rows || !d_weights || n_frames == 0)
      raise(AASR_ERR_INVALID, "aasr_scatter_accumulate_weighted_dev: %lld entries without frames, rows or weights", (long long)entries);
    const hipStream_t st = (hipStream_t)stream;
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    // every class's run of the entry list cut into items; the list itself stays where it is
    h->h_items.clear();
    for (int c = 0; c < h->C; c++)
      for (int64_t s = cnt[c]; s < cnt[c + 1]; s += SCATTER_ITEM)
        h->h_items.push_back(ScatterItem{(int32_t)s, (int32_t)std::min<int64_t>(SCATTER_ITEM, cnt[c + 1] - s), c, 0});
    scatter_queue_items(h, d_frames, d_rows, d_weights, true, st);
  });
}

aasr_status aasr_scatter_fetch(aasr_scatter *h, void *stream) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_scatter_fetch: null argument");
    const hipStream_t st = (hipStream_t)stream;
    h->h_acc.resize((size_t)h->C * h->TS);
    AASR_HIP(hipMemcpyAsync(h->h_acc.data(), h->acc.p, h->h_acc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipStreamSynchronize(st));
    h->staged_pending = false;
    h->fetched = true;
  });
}

aasr_status aasr_scatter_get(const aasr_scatter *h, double *gamma, double *sum_x, double *sum_xx) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_scatter_get: null argument");
    if (!h->fetched) raise(AASR_ERR_INVALID, "aasr_scatter_get: call aasr_scatter_fetch after the last accumulation");
    const int D = h->D;
    const size_t tri = (size_t)D * (D + 1) / 2;
    for (int c = 0; c < h->C; c++) {
      const double *a = h->h_acc.data() + (size_t)c * h->TS;
      // entry (r, q), r >= q, of G_c = sum gamma xi xi^T
      auto at = [&](int r, int q) { return a[((size_t)(r / 16) * (r / 16 + 1) / 2 + q / 16) * 256 + (r % 16) * 16 + q % 16]; };
      if (gamma) gamma[c] = at(0, 0);
      if (sum_x)
        for (int i = 0; i < D; i++) sum_x[(size_t)c * D + i] = at(i + 1, 0);
      if (sum_xx) {
        double *o = sum_xx + (size_t)c * tri;
        for (int i = 0; i < D; i++)
          for (int j = 0; j <= i; j++) *o++ = at(i + 1, j + 1);
      }
    }
  });
}

void aasr_debug_scatter_shape(const aasr_scatter *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 3; i++) out[i] = h ? h->shape[i] : 0;
}

aasr_status aasr_debug_scatter_set_slab_bytes(aasr_scatter *h, int64_t bytes) {
  return guarded([&] {
    if (!h || bytes < 1) raise(AASR_ERR_INVALID, "aasr_debug_scatter_set_slab_bytes: bad argument");
    h->slab_bytes = bytes;
  });
}

}  // extern "C"

// ---- the host solver ---------------------------------------------------------------------------

namespace aasr {

const double *scatter_device_accumulator(const aasr_scatter *h) { return h->acc.p; }

// Cyclic Jacobi on the symmetric n x n row-major matrix a: on return a's diagonal holds the eigenvalues and the
// COLUMNS of v the eigenvectors.  Every rotation annihilates one off-diagonal pair (Rutishauser's formulas); sweeps
// until the off-diagonal sum of squares is below eps^2 of the matrix's.
void jacobi_eigen(std::vector<double> &a, int n, std::vector<double> &v) {
  v.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) v[(size_t)i * n + i] = 1;
  double total = 0;
  for (double x : a) total += x * x;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) off += 2 * a[(size_t)p * n + q] * a[(size_t)p * n + q];
    if (!(off > 1e-32 * total)) break;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0) continue;
        const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < n; k++) {  // columns p and q
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {  // rows p and q
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0;
        for (int k = 0; k < n; k++) {
          const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
          v[(size_t)k * n + p] = c * vkp - s * vkq;
          v[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
}

// indices of the eigenvalues on a's diagonal by falling value (a tie: the lower index)
static std::vector<int> falling_order(const std::vector<double> &a, int n) {
  std::vector<int> idx((size_t)n);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return a[(size_t)x * n + x] > a[(size_t)y * n + y]; });
  return idx;
}

// mean = sum_x / gamma; cov = sum_xx / gamma - mean mean^T (FullStatisticsAccumulator::get_mean_estimate,
// get_covariance_estimate, Distributions.cc:123-130), full symmetric [d x d] from the packed lower triangle
static void mean_cov(int d, double gamma, const double *sx, const double *sxx, std::vector<double> &mean, std::vector<double> &cov) {
  mean.resize((size_t)d);
  cov.resize((size_t)d * d);
  for (int i = 0; i < d; i++) mean[(size_t)i] = sx[i] / gamma;
  const double inv = 1 / gamma;
  const double *s = sxx;
  for (int i = 0; i < d; i++)
    for (int j = 0; j <= i; j++) {
      const double v = *s++ * inv + -1.0 * mean[(size_t)i] * mean[(size_t)j];
      cov[(size_t)i * d + j] = cov[(size_t)j * d + i] = v;
    }
}

static void lda_solve(int n_classes, int d, const double *gamma, const double *sum_x, const double *sum_xx, const int32_t *selected,
                      double max_gamma, int td, double *lda) {
  const size_t tri = (size_t)d * (d + 1) / 2;
  int n_sel = 0;
  for (int c = 0; c < n_classes; c++)
    if (selected[c]) {
      n_sel++;
      if (!(gamma[c] > 0)) raise(AASR_ERR_INVALID, "lda: selected class %d has no frames", c);
    }
  if (n_sel < td + 1)
    raise(AASR_ERR_INVALID, "lda: %d selected classes cannot carry %d dimensions (at least %d are needed)", n_sel, td, td + 1);
  // the whole data: the selected classes' sums, added in class order (lda.cc:363 adds frame by frame)
  double g_all = 0;
  std::vector<double> sx_all((size_t)d, 0.0), sxx_all(tri, 0.0);
  for (int c = 0; c < n_classes; c++) {
    if (!selected[c]) continue;
    g_all += gamma[c];
    for (int i = 0; i < d; i++) sx_all[(size_t)i] += sum_x[(size_t)c * d + i];
    for (size_t k = 0; k < tri; k++) sxx_all[k] += sum_xx[(size_t)c * tri + k];
  }
  std::vector<double> data_mean, data_cov, tmean, tcov;
  mean_cov(d, g_all, sx_all.data(), sxx_all.data(), data_mean, data_cov);
  std::vector<double> B((size_t)d * d, 0.0), W((size_t)d * d, 0.0);
  for (int c = 0; c < n_classes; c++) {
    if (!selected[c]) continue;
    mean_cov(d, gamma[c], sum_x + (size_t)c * d, sum_xx + (size_t)c * tri, tmean, tcov);
    for (int i = 0; i < d; i++) tmean[(size_t)i] += -1 * data_mean[(size_t)i];
    const double g = std::min(gamma[c], max_gamma);
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) {
        B[(size_t)i * d + j] += g * tmean[(size_t)i] * tmean[(size_t)j];
        W[(size_t)i * d + j] += g * tcov[(size_t)i * d + j];
      }
  }
  // W = L L^T
  std::vector<double> L((size_t)d * d, 0.0);
  for (int j = 0; j < d; j++) {
    double s = W[(size_t)j * d + j];
    for (int k = 0; k < j; k++) s -= L[(size_t)j * d + k] * L[(size_t)j * d + k];
    if (!(s > 0)) raise(AASR_ERR_INVALID, "lda: W is not positive definite (pivot %d)", j);
    const double ljj = std::sqrt(s);
    L[(size_t)j * d + j] = ljj;
    for (int i = j + 1; i < d; i++) {
      double t = W[(size_t)i * d + j];
      for (int k = 0; k < j; k++) t -= L[(size_t)i * d + k] * L[(size_t)j * d + k];
      L[(size_t)i * d + j] = t / ljj;
    }
  }
  // M = L^-1 B L^-T: X = L^-1 B by forward substitution on the columns, then M^T = L^-1 X^T
  std::vector<double> X((size_t)d * d), M((size_t)d * d);
  for (int c = 0; c < d; c++)
    for (int i = 0; i < d; i++) {
      double s = B[(size_t)i * d + c];
      for (int k = 0; k < i; k++) s -= L[(size_t)i * d + k] * X[(size_t)k * d + c];
      X[(size_t)i * d + c] = s / L[(size_t)i * d + i];
    }
  for (int r = 0; r < d; r++)  // row r of X is column r of X^T
    for (int i = 0; i < d; i++) {
      double s = X[(size_t)r * d + i];
      for (int k = 0; k < i; k++) s -= L[(size_t)i * d + k] * M[(size_t)r * d + k];
      M[(size_t)r * d + i] = s / L[(size_t)i * d + i];
    }
  for (int i = 0; i < d; i++)  // (symmetric up to rounding: make it so)
    for (int j = 0; j < i; j++) M[(size_t)i * d + j] = M[(size_t)j * d + i] = 0.5 * (M[(size_t)i * d + j] + M[(size_t)j * d + i]);
  std::vector<double> Y;
  jacobi_eigen(M, d, Y);
  const std::vector<int> lead = falling_order(M, d);
  // P [d x td]: column j = L^-T y_j, normalised to unit length (dgeev's normalisation)
  std::vector<double> P((size_t)d * td), col((size_t)d);
  for (int j = 0; j < td; j++) {
    const int e = lead[(size_t)j];
    for (int i = d - 1; i >= 0; i--) {  // L^T z = y
      double s = Y[(size_t)i * d + e];
      for (int k = i + 1; k < d; k++) s -= L[(size_t)k * d + i] * col[(size_t)k];
      col[(size_t)i] = s / L[(size_t)i * d + i];
    }
    double nrm = 0;
    for (int i = 0; i < d; i++) nrm += col[(size_t)i] * col[(size_t)i];
    nrm = std::sqrt(nrm);
    for (int i = 0; i < d; i++) P[(size_t)i * td + j] = col[(size_t)i] / nrm;
  }
  // fea_cov = P^T data_cov P
  std::vector<double> T((size_t)td * d, 0.0), F((size_t)td * td, 0.0);
  for (int a = 0; a < td; a++)
    for (int j = 0; j < d; j++) {
      double s = 0;
      for (int i = 0; i < d; i++) s += P[(size_t)i * td + a] * data_cov[(size_t)i * d + j];
      T[(size_t)a * d + j] = s;
    }
  for (int a = 0; a < td; a++)
    for (int b = 0; b <= a; b++) {
      double s = 0;
      for (int j = 0; j < d; j++) s += T[(size_t)a * d + j] * P[(size_t)j * td + b];
      F[(size_t)a * td + b] = F[(size_t)b * td + a] = s;
    }
  std::vector<double> V;
  jacobi_eigen(F, td, V);
  const std::vector<int> order = falling_order(F, td);
  for (int r = 0; r < td; r++) {
    const int e = order[(size_t)r];
    const double ev = F[(size_t)e * td + e];
    if (!(ev > 0)) raise(AASR_ERR_INVALID, "lda: the projected covariance has a non-positive eigenvalue (%g)", ev);
    const double sc = 1 / std::sqrt(ev);
    double *row = lda + (size_t)r * d;
    int big = 0;
    for (int j = 0; j < d; j++) {
      double s = 0;
      for (int a = 0; a < td; a++) s += sc * V[(size_t)a * td + e] * P[(size_t)j * td + a];
      row[j] = s;
      if (std::fabs(s) > std::fabs(row[big])) big = j;
    }
    if (row[big] < 0)
      for (int j = 0; j < d; j++) row[j] = -row[j];
  }
}

static void lda_select(int n_states, const double *count, double mingamma, int maxmem, int dim, const int32_t *silence,
                       int n_silence, int32_t *selected) {
  int maxpos = (int)std::min<double>(((double)maxmem * 1000 * 1000) / ((double)dim * dim * sizeof(double)), (double)n_states);
  maxpos = std::max(0, maxpos);
  std::vector<int> idx((size_t)n_states);
  std::iota(idx.begin(), idx.end(), 0);
  // falling count; std::sort in the reference leaves equal counts in any order, here the lower state index goes first
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return count[a] > count[b]; });
  for (int i = 0; i < n_states; i++) selected[i] = 0;
  for (int i = 0; i < maxpos; i++)
    if (count[idx[(size_t)i]] >= mingamma) selected[idx[(size_t)i]] = 1;
  for (int i = 0; i < n_silence; i++) {
    if (silence[i] < 0 || silence[i] >= n_states) raise(AASR_ERR_INVALID, "aasr_lda_select: silence state %d out of range", silence[i]);
    selected[silence[i]] = 0;
  }
}

// the lin_transform module `name` of a configuration text, host only: its configured dim (0: none given); *matrix_len:
// the length of its configured matrix (0: none given)
static int configured_transform_dim(const std::string &text, const std::string &name, size_t *matrix_len = nullptr) {
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
    int dim = 0;
    cfg.get("dim", dim);
    if (matrix_len) {
      std::vector<float> m;
      cfg.get("matrix", m);
      *matrix_len = m.size();
    }
    return dim;
  }
  raise(AASR_ERR_INVALID, "unknown module requested: %s", name.c_str());
}

// the states of the silence HMMs _ and __ (lda.cc:84-90); model.hmm() throws for an unknown label
static std::vector<int32_t> silence_states(const aasr_topo *topo) {
  std::vector<int32_t> silence;
  for (const char *label : {"_", "__"}) {
    const int32_t hi = aasr_topo_hmm_index(topo, label);
    if (hi < 0) raise(AASR_ERR_INVALID, "lda: no HMM %s in the model", label);
    std::vector<int32_t> st((size_t)aasr_topo_hmm_num_states(topo, hi));
    if (aasr_topo_hmm_states(topo, hi, st.data()) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    silence.insert(silence.end(), st.begin(), st.end());
  }
  return silence;
}

// The LDA of the handle's sums (lda.cc:375-462): fetch, the matrix from the selected classes, the module's new
// transformation, the configuration file.  gamma: the fetched class weights, for a caller that selected by them
static void solve_and_write(aasr_feat *feat, FeatModule *ltm, aasr_scatter *h, hipStream_t stream, int S, int D, int td,
                            const aasr_lda_options *opt, std::vector<int32_t> &selected,
                            const std::function<void(const std::vector<double> &)> &select) {
  const size_t tri = (size_t)D * (D + 1) / 2;
  std::vector<double> gamma((size_t)S), sx((size_t)S * D), sxx((size_t)S * tri), lda((size_t)td * D);
  if (aasr_scatter_fetch(h, stream) != AASR_OK || aasr_scatter_get(h, gamma.data(), sx.data(), sxx.data()) != AASR_OK)
    raise(AASR_ERR_INVALID, "%s", aasr_last_error());
  if (opt->state_gamma) std::copy(gamma.begin(), gamma.end(), opt->state_gamma);
  if (select) select(gamma);
  if (opt->info > 0) {
    printf("Compute the LDA\n");
    fflush(stdout);
  }
  // a selected state whose frames all lay past the feature end has no accumulator worth the name: it adds
  // nothing to B and W in the reference (gamma 0); leave it out
  for (int s = 0; s < S; s++)
    if (selected[(size_t)s] && !(gamma[(size_t)s] > 0)) selected[(size_t)s] = 0;
  lda_solve(S, D, gamma.data(), sx.data(), sxx.data(), selected.data(), opt->maxgamma, td, lda.data());
  // LinTransformModule::set_transformation_matrix (FeatureModules.cc:1273-1296): the working and the
  // configured matrix both, in float
  std::vector<float> tr(lda.begin(), lda.end());
  ltm->matrix = tr;
  ltm->orig_matrix = tr;
  ltm->matrix_defined = true;
  ltm->d_matrix.upload(ltm->matrix.data(), ltm->matrix.size());
  if (opt->out) {
    const std::string text = feat_write_configuration(feat);
    write_text_file(opt->out, text.data(), text.size());
  }
}

}  // namespace aasr

extern "C" {

aasr_status aasr_lda_solve(int32_t n_classes, int32_t dim, const double *gamma, const double *sum_x, const double *sum_xx,
                           const int32_t *selected, double max_gamma, int32_t target_dim, double *lda) {
  return guarded([&] {
    if (n_classes < 1 || dim < 1 || target_dim < 1 || target_dim > dim || !gamma || !sum_x || !sum_xx || !selected || !lda)
      raise(AASR_ERR_INVALID, "aasr_lda_solve: bad argument");
    std::vector<double> out((size_t)target_dim * dim);
    lda_solve(n_classes, dim, gamma, sum_x, sum_xx, selected, max_gamma, target_dim, out.data());
    std::copy(out.begin(), out.end(), lda);
  });
}

aasr_status aasr_lda_select(int32_t n_states, const double *count, double mingamma, int32_t maxmem, int32_t dim,
                            const int32_t *silence, int32_t n_silence, int32_t *selected) {
  return guarded([&] {
    if (n_states < 1 || dim < 1 || !count || !selected || n_silence < 0 || (n_silence > 0 && !silence))
      raise(AASR_ERR_INVALID, "aasr_lda_select: bad argument");
    lda_select(n_states, count, mingamma, maxmem, dim, silence, n_silence, selected);
  });
}

void aasr_lda_default_options(aasr_lda_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->target_dim = 39;
  o->maxmem = 3000;
  o->mingamma = 50;
  o->maxgamma = 1000000;
}

}  // extern "C"

// ---- the lda main loop over a recipe -----------------------------------------------------------

extern "C" aasr_status aasr_run_lda_recipe(const char *feat_cfg_text, const aasr_topo *topo, const char *recipe_path,
                                           aasr_lda_options *opt, aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat_cfg_text || !topo || !recipe_path || !opt || !opt->module)
      raise(AASR_ERR_INVALID, "aasr_run_lda_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    opt->seconds_scatter = opt->seconds_features = 0;
    // ---- host only, before the device is opened
    const std::string module = opt->module;
    const int td = opt->target_dim;
    {
      const int cd = configured_transform_dim(feat_cfg_text, module);
      if (cd > 0 && cd != td)
        raise(AASR_ERR_INVALID, "lda: -d %d but module %s has dimension %d", td, module.c_str(), cd);
    }
    const std::vector<int32_t> silence = silence_states(topo);
    const int S = aasr_topo_num_states(topo);
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, 1, 1, true);  // lda.cc:144
    refuse_line_limits(infos, "lda");

    // ---- the device
    std::unique_ptr<aasr_feat> feat(feat_create(feat_cfg_text));
    FeatModule *ltm = &feat->mods[(size_t)feat->by_name.at(module)];
    if (ltm->dim != td) raise(AASR_ERR_INVALID, "lda: -d %d but module %s has dimension %d", td, module.c_str(), ltm->dim);
    // lda.cc:105-109: the statistics are those of the module's source, not of the chain's output.  The batch
    // evaluator takes any module as its target, so the one handle serves: the speaker configuration's parameters
    // reach the source's ancestors as they reach every other module.
    const int source = ltm->sources[0];
    const int D = feat->mods[(size_t)source].dim;
    if (td > D) raise(AASR_ERR_INVALID, "lda: -d %d exceeds the source dimension %d", td, D);
    if (D > SCATTER_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "lda: source dimension %d (module %s): 1 ... %d are built", D,
            feat->mods[(size_t)source].name.c_str(), SCATTER_MAX_DIM);
    aasr_spkc *spk = nullptr;
    if (opt->speakers) {
      if (aasr_spkc_create(feat.get(), nullptr, &spk) != AASR_OK || aasr_spkc_read_file(spk, opt->speakers) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    std::unique_ptr<aasr_spkc, void (*)(aasr_spkc *)> spguard(spk, aasr_spkc_destroy);
    const float fr = aasr_feat_frame_rate(feat.get());

    // ---- pass 1: the states' frame counts, from the segmentations and the audio lengths
    const TopoTables tt(topo);
    std::vector<Segmentation> utts(infos.size());
    std::vector<double> count((size_t)S, 0.0);
    for (size_t f = 0; f < infos.size(); f++) {
      const RecipeInfo &u = infos[f];
      announce(u, opt->info);
      const int eof = aasr_feat_eof_frame(feat.get(), (int64_t)load_utterance_input(feat.get(), u).size());
      utts[f] = read_state_sequence(topo, tt, u, opt->ophn != 0, fr, eof);
      for (int32_t s : utts[f].pdf) {
        if (s >= S) raise(AASR_ERR_INVALID, "%s: state %d outside the model", u.transcript_path.c_str(), s);
        if (s >= 0) count[(size_t)s] += 1;
      }
    }
    std::vector<int32_t> selected((size_t)S);
    {
      const int maxpos = (int)std::min<double>(((double)opt->maxmem * 1000 * 1000) / ((double)D * D * sizeof(double)), (double)S);
      if (opt->info) printf("Collecting statistics at maximum for %d states\n", maxpos);
      if (opt->info > 0) printf("Reserving memory\n");
      lda_select(S, count.data(), opt->mingamma, opt->maxmem, D, silence.data(), opt->no_silence ? (int)silence.size() : 0,
                 selected.data());
      if (opt->no_silence && opt->info > 0) printf("Discarding %d silence states\n", (int)silence.size());
      if (opt->info) printf("Collecting statistics for %d states\n", (int)std::count(selected.begin(), selected.end(), 1));
      fflush(stdout);
    }

    // ---- pass 2: the source module's frames of a group of utterances in one device buffer, one accumulation
    aasr_scatter *h = nullptr;
    {
      const aasr_status cs = aasr_scatter_create(S, D, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_scatter, void (*)(aasr_scatter *)> hguard(h, aasr_scatter_destroy);
    GroupStager stager(feat.get(), spk, source);
    const hipStream_t stream = stager.stream;
    hipEvent_t ev[3];
    for (hipEvent_t &e : ev) AASR_HIP(hipEventCreate(&e));
    struct EvGuard {
      hipEvent_t *e;
      ~EvGuard() {
        for (int i = 0; i < 3; i++) (void)hipEventDestroy(e[i]);
      }
    } evguard{ev};
    const int64_t max_group_frames = (int64_t)1 << 18;
    int64_t num_frames = 0;
    size_t next = 0;
    while (next < infos.size()) {
      const size_t group_first = next;
      std::vector<std::vector<int16_t>> audio;
      std::vector<int32_t> start, rows, cls;
      int64_t rows_total = 0;
      while (next < infos.size() && audio.size() < 1024 && rows_total < max_group_frames) {
        const Segmentation &ut = utts[next];
        announce(infos[next], opt->info);
        audio.emplace_back();
        if (!ut.pdf.empty()) audio.back() = load_utterance_input(feat.get(), infos[next]);
        start.push_back(ut.start_frame);
        rows.push_back((int32_t)ut.pdf.size());
        for (int32_t s : ut.pdf) cls.push_back(s >= 0 && selected[(size_t)s] ? s : -1);
        rows_total += (int64_t)ut.pdf.size();
        next++;
      }
      stager.stage(audio, start, rows, [&](size_t i) {
        if (i == 0) AASR_HIP(hipEventRecord(ev[0], stream));  // the features' interval opens once the buffers stand
        apply_speaker(spk, infos[group_first + i]);  // lda.cc:284-289; a parameter change waits for the queued features
      });
      AASR_HIP(hipEventRecord(ev[1], stream));
      if (rows_total > 0 && aasr_scatter_accumulate_dev(h, stager.d_x.p, rows_total, cls.data(), nullptr, stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      AASR_HIP(hipEventRecord(ev[2], stream));
      AASR_HIP(hipStreamSynchronize(stream));  // the group's host audio goes out of scope
      float ms = 0;
      AASR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      opt->seconds_features += ms * 1e-3;
      AASR_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
      opt->seconds_scatter += ms * 1e-3;
      num_frames += rows_total;
    }

    solve_and_write(feat.get(), ltm, h, stream, S, D, td, opt, selected, nullptr);
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, opt->seconds_scatter + opt->seconds_features);
  });
}

// ---- the same over the recipe's HMM networks ---------------------------------------------------

namespace {

// what aasr_run_lda_networks_recipe refuses on the host; -> the recipe's lines and the silence states
void lda_networks_host_checks(const char *feat_cfg_text, const aasr_topo *topo, const char *recipe_path,
                              const aasr_lda_options *opt, std::vector<RecipeInfo> *infos, std::vector<int32_t> *silence) {
  if (!feat_cfg_text || !topo || !recipe_path || !opt || !opt->module)
    raise(AASR_ERR_INVALID, "aasr_run_lda_networks_recipe: null argument");
  if (opt->ophn)
    raise(AASR_ERR_UNSUPPORTED, "lda: -O is not supported with --networks (a network line has no segmentation to choose)");
  const std::string module = opt->module;
  size_t matrix_len = 0;
  const int cd = configured_transform_dim(feat_cfg_text, module, &matrix_len);
  if (cd > 0 && cd != opt->target_dim)
    raise(AASR_ERR_INVALID, "lda: -d %d but module %s has dimension %d", opt->target_dim, module.c_str(), cd);
  if (matrix_len == 0)
    raise(AASR_ERR_INVALID,
          "lda: --networks scores the output of the whole feature chain, but module %s has no matrix in the configuration",
          module.c_str());
  *silence = silence_states(topo);
  *infos = read_recipe_file(recipe_path, 1, 1, true);  // lda.cc:144
  refuse_line_limits(*infos, "lda");
  for (const RecipeInfo &u : *infos)
    if (u.hmmnet_path.empty()) raise(AASR_ERR_INVALID, "Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe.");
}

}  // namespace

extern "C" {

void aasr_lda_network_default_options(aasr_lda_network_options *o) {
  if (o) memset(o, 0, sizeof *o);
  if (o) o->ac_scale = 1;
}

aasr_status aasr_lda_networks_check(const char *feat_cfg_text, const aasr_topo *topo, const char *recipe_path,
                                    const aasr_lda_options *opt) {
  return guarded([&] {
    std::vector<RecipeInfo> infos;
    std::vector<int32_t> silence;
    lda_networks_host_checks(feat_cfg_text, topo, recipe_path, opt, &infos, &silence);
  });
}

aasr_status aasr_run_lda_networks_recipe(const char *feat_cfg_text, aasr_gmm *gmm, const aasr_topo *topo,
                                         const char *recipe_path, aasr_lda_options *opt,
                                         const aasr_lda_network_options *nopt, aasr_run_stats *stats) {
  if (!nopt || !nopt->networks) return aasr_run_lda_recipe(feat_cfg_text, topo, recipe_path, opt, stats);
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    // ---- host only, before the device is opened
    std::vector<RecipeInfo> infos;
    std::vector<int32_t> silence;
    lda_networks_host_checks(feat_cfg_text, topo, recipe_path, opt, &infos, &silence);
    if (!gmm) raise(AASR_ERR_INVALID, "aasr_run_lda_networks_recipe: null argument");
    opt->seconds_scatter = opt->seconds_features = 0;
    const std::string module = opt->module;
    const int td = opt->target_dim;
    const int S = aasr_topo_num_states(topo);

    // ---- the device
    std::unique_ptr<aasr_feat> feat(feat_create(feat_cfg_text));
    FeatModule *ltm = &feat->mods[(size_t)feat->by_name.at(module)];
    if (ltm->dim != td) raise(AASR_ERR_INVALID, "lda: -d %d but module %s has dimension %d", td, module.c_str(), ltm->dim);
    const int source = ltm->sources[0];  // lda.cc:105-109: the statistics are those of the module's source
    const int D = feat->mods[(size_t)source].dim;
    if (td > D) raise(AASR_ERR_INVALID, "lda: -d %d exceeds the source dimension %d", td, D);
    if (D > SCATTER_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "lda: source dimension %d (module %s): 1 ... %d are built", D,
            feat->mods[(size_t)source].name.c_str(), SCATTER_MAX_DIM);
    aasr_spkc *spk = nullptr;
    if (opt->speakers) {
      if (aasr_spkc_create(feat.get(), nullptr, &spk) != AASR_OK || aasr_spkc_read_file(spk, opt->speakers) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    std::unique_ptr<aasr_spkc, void (*)(aasr_spkc *)> spguard(spk, aasr_spkc_destroy);
    check_feature_dim(gmm, feat.get());
    if (aasr_gmm_num_states(gmm) != S)
      raise(AASR_ERR_INVALID, "lda: the model has %d states but the HMM definitions have %d", aasr_gmm_num_states(gmm), S);
    const float fr = aasr_feat_frame_rate(feat.get());
    const bool f64 = aasr_gmm_get_precision(gmm) == AASR_PREC_F64;

    {
      const int maxpos = (int)std::min<double>(((double)opt->maxmem * 1000 * 1000) / ((double)D * D * sizeof(double)), (double)S);
      if (opt->info) printf("Collecting statistics at maximum for %d states\n", maxpos);
      if (opt->info > 0) printf("Reserving memory\n");
      fflush(stdout);
    }
    aasr_scatter *h = nullptr;
    {
      const aasr_status cs = aasr_scatter_create(S, D, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_scatter, void (*)(aasr_scatter *)> hguard(h, aasr_scatter_destroy);
    // two stagings per group: the chain's output, which the model scores, and the module's source, which is summed.
    // Each has a stream of its own; a speaker change that rewrites feature parameters waits for both.
    GroupStager scored(feat.get(), spk, -1), summed(feat.get(), spk, source);
    const hipStream_t stream = scored.stream, sum_stream = summed.stream;
    struct Unhook {
      aasr_spkc *s;
      ~Unhook() {
        if (s) spkc_set_before_change(s, nullptr);
      }
    } unhook{spk};
    if (spk)
      spkc_set_before_change(spk, [stream, sum_stream]() {
        AASR_HIP(hipStreamSynchronize(stream));
        AASR_HIP(hipStreamSynchronize(sum_stream));
      });
    hipEvent_t ev[6];
    for (hipEvent_t &e : ev) AASR_HIP(hipEventCreate(&e));
    struct EvGuard {
      hipEvent_t *e;
      ~EvGuard() {
        for (int i = 0; i < 6; i++) (void)hipEventDestroy(e[i]);
      }
    } evguard{ev};
    aasr_fb_options fo;
    network_fb_options(&fo, nopt->fw_beam, nopt->bw_beam, nopt->ac_scale_given != 0, nopt->ac_scale, nopt->viterbi != 0);
    fo.want_pdf_occ = 1;
    fo.device_occ = 1;
    fo.max_attempts = 5;  // (counter >= 5, lda.cc:190)
    NetworkCache net_cache(topo, S);
    GroupScores scores;
    std::vector<int64_t> cnt((size_t)S + 1);
    double max_dev = 0;
    int64_t entries = 0, num_frames = 0;
    StageTimers tm;
    tm.on = getenv("AASR_RECIPE_TIMING") != nullptr;
    size_t next = 0;
    while (next < infos.size()) {
      double t = now_s();
      const size_t group_first = next;
      NetworkGroup g;
      while (next < infos.size() && g.size() < 1024 &&
             (g.size() == 0 || (g.rows_total < NETWORK_GROUP_FRAMES && g.rows_total * S < NETWORK_GROUP_SCORES))) {
        const RecipeInfo &u = infos[next++];
        announce(u, opt->info);
        g.add(feat.get(), net_cache, u, u.hmmnet_path, fr);
      }
      tm.host += now_s() - t;
      t = now_s();
      const auto speaker_of = [&](size_t i) { apply_speaker(spk, infos[group_first + i]); };  // lda.cc:163-168
      AASR_HIP(hipEventRecord(ev[0], stream));
      scored.stage(g.audio, g.start, g.rows, speaker_of);
      AASR_HIP(hipEventRecord(ev[1], stream));
      if (tm.on) AASR_HIP(hipStreamSynchronize(stream));
      tm.feat += now_s() - t;
      const void *d_scores = nullptr;
      const FbBatchPtr batch = run_network_group(fo, gmm, scored, g, scores, f64, &d_scores, &tm);
      aasr_fb_batch *b = batch.get();
      t = now_s();
      const int32_t *d_rows = nullptr;
      const double *d_weights = nullptr;
      if (aasr_fb_batch_entries_dev(b, S, g.row0.data(), stream, cnt.data(), &d_rows, &d_weights) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      AASR_HIP(hipEventRecord(ev[2], stream));  // the entries stand
      entries += cnt[(size_t)S];
      tm.fb += now_s() - t;
      for (size_t i = 0; i < g.size(); i++) {
        const RecipeInfo &u = infos[group_first + i];
        if (!report_network_outcome(b, i, fo, RetryMessages::BAUM_WELCH, u)) continue;
        check_frame_sums(b, i, g, u, &max_dev);
        num_frames += g.rows[i];
      }
      // the same utterances and frame ranges at the module's source: an entry's row number addresses both buffers
      t = now_s();
      AASR_HIP(hipEventRecord(ev[3], sum_stream));
      summed.stage(g.audio, g.start, g.rows, speaker_of);
      AASR_HIP(hipEventRecord(ev[4], sum_stream));
      if (tm.on) AASR_HIP(hipStreamSynchronize(sum_stream));
      tm.feat += now_s() - t;
      t = now_s();
      AASR_HIP(hipStreamWaitEvent(sum_stream, ev[2], 0));
      if (cnt[(size_t)S] > 0 && aasr_scatter_accumulate_weighted_dev(h, summed.d_x.p, g.rows_total, cnt.data(), d_rows,
                                                                     d_weights, sum_stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      AASR_HIP(hipEventRecord(ev[5], sum_stream));
      // the batch owns the entries that the accumulation reads, the group its audio: they go when the streams are done
      AASR_HIP(hipStreamSynchronize(stream));
      AASR_HIP(hipStreamSynchronize(sum_stream));
      tm.acc += now_s() - t;
      float ms = 0;
      AASR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      opt->seconds_features += ms * 1e-3;
      AASR_HIP(hipEventElapsedTime(&ms, ev[3], ev[4]));
      opt->seconds_features += ms * 1e-3;
      AASR_HIP(hipEventElapsedTime(&ms, ev[4], ev[5]));
      opt->seconds_scatter += ms * 1e-3;
    }
    if (opt->info > 0) {
      fprintf(stderr, "Largest |1 - sum of PDF probabilities| of a frame: %g\n", max_dev);
      fprintf(stderr, "Weighted entries: %lld over %lld frames\n", (long long)entries, (long long)num_frames);
    }
    if (tm.on)
      fprintf(stderr,
              "lda timing: input and networks %.3f s, features (both stagings) %.3f s, scoring %.3f s, forward-backward and "
              "entries %.3f s, accumulation %.3f s\n",
              tm.host, tm.feat, tm.score, tm.fb, tm.acc);

    // ---- the selection on the fetched gamma (lda.cc:247-263), then the LDA
    std::vector<int32_t> selected((size_t)S, 0);
    solve_and_write(feat.get(), ltm, h, sum_stream, S, D, td, opt, selected, [&](const std::vector<double> &gamma) {
      lda_select(S, gamma.data(), opt->mingamma, opt->maxmem, D, silence.data(), opt->no_silence ? (int)silence.size() : 0,
                 selected.data());
      if (opt->no_silence && opt->info > 0) printf("Discarding %d silence states\n", (int)silence.size());
      if (opt->info) printf("Collecting statistics for %d states\n", (int)std::count(selected.begin(), selected.end(), 1));
      fflush(stdout);
    });
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, opt->seconds_scatter + opt->seconds_features);
  });
}

}  // extern "C"

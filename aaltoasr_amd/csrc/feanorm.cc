// feanorm.cc -- feature normalization and PCA estimation (aku/feanorm.cc): the moments handle that drives the device
// reduction (moments_accum.hip), the blocked sums of feanorm.cc:181-242 on the host, the PCA of feanorm.cc:281-325 in
// double without LAPACK (the cyclic Jacobi solver of lda.cc) and the feanorm main loop over a recipe
// (aasr_run_feanorm_recipe).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"
#include "feat.h"
#include "jacobi.h"
#include "moments.h"
#include "recipe_pass.h"

using namespace aasr;

// ---- the moments handle ------------------------------------------------------------------------

struct aasr_moments {
  int D = 0, PB = 0;
  bool full = false;
  int64_t TS = 0;  // doubles of a segment's sums and of an item's slab
  int32_t launch_segments = MOMENTS_MAX_SEGMENTS;
  DevBuf<double> slab, d_out;
  DevBuf<MomentsItem> d_items;
  DevBuf<MomentsGroup> d_groups;
  // host staging of the last call's lists, kept until their upload is done
  std::vector<MomentsItem> h_items;
  std::vector<MomentsGroup> h_groups;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  // per call the segments' sums as they come back (a chunk is never resized: a copy may be on its way into it)
  std::deque<std::vector<double>> chunks;
  struct Seg {
    int32_t len, utt;
    const double *sums;
  };
  std::vector<Seg> segs;
  bool fetched = true;
  int32_t shape[3] = {0, 0, 0};
  ~aasr_moments() {
    if (staged) (void)hipEventDestroy(staged);
  }
  // entry (r, q), r >= q, of a full-mode segment's G = sum xi xi^T
  static double at(const double *a, int r, int q) {
    return a[((size_t)(r / 16) * (r / 16 + 1) / 2 + q / 16) * 256 + (r % 16) * 16 + q % 16];
  }
  size_t xx_doubles() const { return full ? (size_t)D * (D + 1) / 2 : (size_t)D; }
  // one segment's sums in the layout of aasr_moments_get
  void unpack(const Seg &s, double *count, double *sx, double *sxx) const {
    const double *a = s.sums;
    if (!full) {
      *count = a[0];
      for (int i = 0; i < D; i++) sx[i] = a[1 + i];
      for (int i = 0; i < D; i++) sxx[i] = a[1 + D + i];
      return;
    }
    *count = at(a, 0, 0);
    for (int i = 0; i < D; i++) sx[i] = at(a, i + 1, 0);
    for (int i = 0; i < D; i++)
      for (int j = 0; j <= i; j++) *sxx++ = at(a, i + 1, j + 1);
  }
};

extern "C" {

aasr_status aasr_moments_create(int32_t dim, int32_t mode, aasr_moments **out) {
  return guarded([&] {
    if (!out || dim < 1 || (mode != AASR_MOMENTS_DIAG && mode != AASR_MOMENTS_FULL))
      raise(AASR_ERR_INVALID, "aasr_moments_create: bad argument");
    *out = nullptr;
    if (mode == AASR_MOMENTS_FULL && dim > MOMENTS_MAX_DIM)
      raise(AASR_ERR_UNSUPPORTED, "moments: no full-mode kernel for dimension %d (1 ... %d)", dim, MOMENTS_MAX_DIM);
    require_device();
    std::unique_ptr<aasr_moments> h(new aasr_moments());
    h->D = dim;
    h->full = mode == AASR_MOMENTS_FULL;
    h->PB = h->full ? scatter_pb(dim) : 0;
    h->TS = moments_doubles(dim, h->full);
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

void aasr_moments_destroy(aasr_moments *h) { delete h; }

aasr_status aasr_moments_accumulate_dev(aasr_moments *h, const double *d_frames, int64_t n_frames, const int32_t *segments,
                                        int32_t n_segments, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || n_segments < 0 || (n_segments > 0 && (!d_frames || !segments)))
      raise(AASR_ERR_INVALID, "aasr_moments_accumulate_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_moments_accumulate_dev: more than 2^31 frames in one call");
    for (int32_t s = 0; s < n_segments; s++) {
      const int64_t first = segments[3 * s], len = segments[3 * s + 1];
      if (first < 0 || len < 1 || first + len > n_frames)
        raise(AASR_ERR_INVALID, "aasr_moments_accumulate_dev: segment %d (rows %ld ... %ld) outside the %ld frames", s,
              (long)first, (long)(first + len), (long)n_frames);
    }
    if (n_segments == 0) return;
    const hipStream_t st = (hipStream_t)stream;
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    // items: every segment in runs of MOMENTS_RUN rows from its first row.  Launches: whole segments, as many as the
    // slab bound and the segment bound allow, one at the least.
    const int64_t max_items = std::max<int64_t>(1, MOMENTS_SLAB_BYTES / (h->TS * (int64_t)sizeof(double)));
    const int max_segs = std::max(1, std::min<int>(h->launch_segments, MOMENTS_MAX_SEGMENTS));
    struct Launch {
      int item0, n_items, group0, n_groups;
    };
    std::vector<Launch> launches;
    h->h_items.clear();
    h->h_groups.clear();
    int64_t slab_items = 0;
    for (int32_t s = 0; s < n_segments; s++) {
      const int32_t first = segments[3 * s], len = segments[3 * s + 1];
      const int n = (len + MOMENTS_RUN - 1) / MOMENTS_RUN;
      if (launches.empty() || launches.back().n_groups >= max_segs || launches.back().n_items + (int64_t)n > max_items)
        launches.push_back(Launch{(int)h->h_items.size(), 0, (int)h->h_groups.size(), 0});
      Launch &L = launches.back();
      h->h_groups.push_back(MomentsGroup{L.n_items, n, s, 0});
      for (int32_t r = 0; r < len; r += MOMENTS_RUN)
        h->h_items.push_back(MomentsItem{first + r, std::min<int32_t>(MOMENTS_RUN, len - r)});
      L.n_items += n;
      L.n_groups++;
      slab_items = std::max<int64_t>(slab_items, L.n_items);
    }
    h->d_items.ensure(h->h_items.size());
    h->d_groups.ensure(h->h_groups.size());
    h->slab.ensure((size_t)slab_items * h->TS);
    h->d_out.ensure((size_t)n_segments * h->TS);
    AASR_HIP(hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(MomentsItem), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_groups.p, h->h_groups.data(), h->h_groups.size() * sizeof(MomentsGroup), hipMemcpyHostToDevice, st));
    AASR_HIP(hipEventRecord(h->staged, st));
    h->staged_pending = true;
    for (const Launch &L : launches)  // (the launches of a call follow each other on the stream and share the slab)
      moments_launch(d_frames, h->D, h->full, h->d_items.p, L.item0, L.n_items, h->d_groups.p + L.group0, L.n_groups,
                     h->slab.p, h->d_out.p, st);
    h->chunks.emplace_back((size_t)n_segments * h->TS);
    std::vector<double> &chunk = h->chunks.back();
    AASR_HIP(hipMemcpyAsync(chunk.data(), h->d_out.p, chunk.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int32_t s = 0; s < n_segments; s++)
      h->segs.push_back(aasr_moments::Seg{segments[3 * s + 1], segments[3 * s + 2], chunk.data() + (size_t)s * h->TS});
    h->shape[0] = h->PB;
    h->shape[1] = (int32_t)h->h_items.size();
    h->shape[2] = (int32_t)launches.size();
    h->fetched = false;
  });
}

aasr_status aasr_moments_fetch(aasr_moments *h, void *stream) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_moments_fetch: null argument");
    AASR_HIP(hipStreamSynchronize((hipStream_t)stream));
    h->staged_pending = false;
    h->fetched = true;
  });
}

int64_t aasr_moments_num_segments(const aasr_moments *h) { return h ? (int64_t)h->segs.size() : 0; }

aasr_status aasr_moments_get(const aasr_moments *h, double *count, int32_t *utterance, double *sum_x, double *sum_xx) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_moments_get: null argument");
    if (!h->fetched) raise(AASR_ERR_INVALID, "aasr_moments_get: call aasr_moments_fetch after the last accumulation");
    const size_t nx = h->xx_doubles();
    std::vector<double> sx((size_t)h->D), sxx(nx);
    for (size_t s = 0; s < h->segs.size(); s++) {
      double c = 0;
      h->unpack(h->segs[s], &c, sx.data(), sxx.data());
      if (count) count[s] = c;
      if (utterance) utterance[s] = h->segs[s].utt;
      if (sum_x) std::copy(sx.begin(), sx.end(), sum_x + s * (size_t)h->D);
      if (sum_xx) std::copy(sxx.begin(), sxx.end(), sum_xx + s * nx);
    }
  });
}

aasr_status aasr_moments_blocked(const aasr_moments *h, int32_t block_size, const int32_t *keep, double *count, double *sum_x,
                                 double *sum_xx) {
  return guarded([&] {
    if (!h || block_size < 1) raise(AASR_ERR_INVALID, "aasr_moments_blocked: bad argument");
    if (!h->fetched) raise(AASR_ERR_INVALID, "aasr_moments_blocked: call aasr_moments_fetch after the last accumulation");
    const size_t nx = h->xx_doubles();
    std::vector<double> sx((size_t)h->D), sxx(nx), gx((size_t)h->D, 0.0), gxx(nx, 0.0);
    double g = 0;
    const double bs = (double)block_size;
    for (size_t s = 0; s < h->segs.size(); s++) {
      if (keep && !keep[s]) continue;
      double c = 0;
      h->unpack(h->segs[s], &c, sx.data(), sxx.data());
      for (int i = 0; i < h->D; i++) gx[(size_t)i] += sx[(size_t)i] / bs;
      for (size_t k = 0; k < nx; k++) gxx[k] += sxx[k] / bs;
      g += c / bs;
    }
    if (count) *count = g;
    if (sum_x) std::copy(gx.begin(), gx.end(), sum_x);
    if (sum_xx) std::copy(gxx.begin(), gxx.end(), sum_xx);
  });
}

void aasr_debug_moments_shape(const aasr_moments *h, int32_t *out) {
  if (!out) return;
  for (int i = 0; i < 3; i++) out[i] = h ? h->shape[i] : 0;
}

aasr_status aasr_debug_moments_set_launch_segments(aasr_moments *h, int32_t n) {
  return guarded([&] {
    if (!h || n < 1) raise(AASR_ERR_INVALID, "aasr_debug_moments_set_launch_segments: bad argument");
    h->launch_segments = n;
  });
}

}  // extern "C"

// ---- the PCA -----------------------------------------------------------------------------------

namespace aasr {

// |det m| of the n x n row-major matrix from its LU factors with partial pivoting (feanorm.cc:304-309)
static double abs_determinant(std::vector<double> m, int n) {
  double det = 1;
  for (int k = 0; k < n; k++) {
    int piv = k;
    for (int i = k + 1; i < n; i++)
      if (std::fabs(m[(size_t)i * n + k]) > std::fabs(m[(size_t)piv * n + k])) piv = i;
    if (piv != k)
      for (int j = 0; j < n; j++) std::swap(m[(size_t)k * n + j], m[(size_t)piv * n + j]);
    const double p = m[(size_t)k * n + k];
    det *= p;
    if (p == 0) return 0;
    for (int i = k + 1; i < n; i++) {
      const double f = m[(size_t)i * n + k] / p;
      for (int j = k + 1; j < n; j++) m[(size_t)i * n + j] -= f * m[(size_t)k * n + j];
    }
  }
  return std::fabs(det);
}

static void feanorm_pca(int d, const double *cov, const double *scale, bool unit_determinant, double *pca, double *eigenvalues) {
  std::vector<double> a(cov, cov + (size_t)d * d), v;
  for (int i = 0; i < d; i++)  // (symmetric up to rounding: make it so)
    for (int j = 0; j < i; j++) a[(size_t)i * d + j] = a[(size_t)j * d + i] = 0.5 * (a[(size_t)i * d + j] + a[(size_t)j * d + i]);
  jacobi_eigen(a, d, v);
  std::vector<int> order((size_t)d);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * d + x] < a[(size_t)y * d + y]; });
  std::vector<double> tr((size_t)d * d);
  for (int i = 0; i < d; i++) {
    const int e = order[(size_t)i];
    const double ev = a[(size_t)e * d + e];
    if (!(ev > 0)) raise(AASR_ERR_INVALID, "feanorm: the covariance has a non-positive eigenvalue (%g)", ev);
    if (eigenvalues) eigenvalues[i] = ev;
    for (int j = 0; j < d; j++) tr[(size_t)i * d + j] = v[(size_t)j * d + e];  // the inverse of the eigenvector matrix
  }
  auto by_scale = [&]() {
    if (!scale) return;
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) tr[(size_t)i * d + j] /= scale[j];
  };
  if (unit_determinant) {  // feanorm.cc:296-312
    by_scale();
    const double sc = std::pow(abs_determinant(tr, d), 1 / (double)d);
    for (double &x : tr) x *= 1 / sc;
  } else {  // feanorm.cc:315-324
    for (int i = 0; i < d; i++) {
      const int e = order[(size_t)i];
      for (int j = 0; j < d; j++) tr[(size_t)i * d + j] /= std::sqrt(a[(size_t)e * d + e]);
    }
    by_scale();
  }
  for (int i = 0; i < d; i++) {
    double *row = tr.data() + (size_t)i * d;
    int big = 0;
    for (int j = 1; j < d; j++)
      if (std::fabs(row[j]) > std::fabs(row[big])) big = j;
    if (row[big] < 0)
      for (int j = 0; j < d; j++) row[j] = -row[j];
  }
  std::copy(tr.begin(), tr.end(), pca);
}

// What the refusals need of a configuration text, on the host: every module's name, type, sources and -- where the
// module types' rules give it without the device -- dimension (-1: not known here).
struct ScannedModule {
  std::string name, type;
  std::vector<int> sources;
  int dim = -1;
};

static std::vector<ScannedModule> scan_configuration(const std::string &text) {
  std::vector<ScannedModule> mods;
  size_t pos = 0;
  float sample_rate = 0;
  while (pos < text.size()) {
    size_t e = text.find('\n', pos);
    if (e == std::string::npos) e = text.size();
    const std::string line = str_clean(text.substr(pos, e - pos), " \t");
    pos = e + 1;
    if (line.empty()) continue;
    if (line != "module") raise(AASR_ERR_INVALID, "expected keyword 'module' in the feature configuration: %s", line.c_str());
    ModuleConfig cfg;
    cfg.read(text, &pos);
    ScannedModule m;
    cfg.get("name", m.name);
    cfg.get("type", m.type);
    std::vector<std::string> srcs;
    cfg.get("sources", srcs);
    bool known = true;
    for (const std::string &s : srcs) {
      int found = -1;
      for (size_t k = 0; k < mods.size(); k++)
        if (mods[k].name == s) found = (int)k;
      if (found < 0) raise(AASR_ERR_INVALID, "unknown source module: %s", s.c_str());
      m.sources.push_back(found);
      known = known && mods[(size_t)found].dim > 0;
    }
    const int sdim = known && !m.sources.empty() ? mods[(size_t)m.sources[0]].dim : -1;
    const std::string &t = m.type;
    if (t == "audiofile") {
      float frame_rate = 125;
      cfg.get("sample_rate", sample_rate);
      cfg.get("frame_rate", frame_rate);
      m.dim = (int)(2 * (int)sample_rate / frame_rate);
      cfg.get("window_width", m.dim);
    } else if (t == "fft") {
      if (sdim > 0) m.dim = sdim / 2 + 1;
    } else if (t == "mel") {
      if (sample_rate > 0) m.dim = (int)((21 + 2) * log10f(1 + (int)sample_rate / 1400.0) / log10f(1 + 16000 / 1400.0) - 2);
    } else if (t == "power" || t == "mel_power") {
      m.dim = 1;
    } else if (t == "dct") {
      m.dim = 12;
      cfg.get("dim", m.dim);
    } else if (t == "delta" || t == "normalization" || t == "mean_subtractor" || t == "vtln" || t == "quanteq") {
      m.dim = sdim;
    } else if (t == "lin_transform") {
      m.dim = sdim;
      cfg.get("dim", m.dim);
    } else if (t == "merge") {
      m.dim = known ? 0 : -1;
      if (known)
        for (int s : m.sources) m.dim += mods[(size_t)s].dim;
    } else if (t == "concat") {
      int left = 0, right = 0;
      cfg.get("left", left);
      cfg.get("right", right);
      if (sdim > 0) m.dim = sdim * (1 + left + right);
    }  // pre, sr_norm, user types: the device-side graph decides
    if (m.dim < 1) m.dim = -1;
    mods.push_back(m);
  }
  if (mods.empty()) raise(AASR_ERR_INVALID, "no feature modules defined");
  return mods;
}

static int scanned_module(const std::vector<ScannedModule> &mods, const std::string &name) {
  for (size_t k = 0; k < mods.size(); k++)
    if (mods[k].name == name) return (int)k;
  raise(AASR_ERR_INVALID, "unknown module requested: %s", name.c_str());
}

static void refuse_pca_source(const std::string &pca, int source_dim, int dim) {
  if (source_dim != dim)
    raise(AASR_ERR_INVALID, "feanorm: the source of module %s has dimension %d but the statistics have dimension %d", pca.c_str(),
          source_dim, dim);
}

static void refuse_full_dim(int dim) {
  if (dim > MOMENTS_MAX_DIM)
    raise(AASR_ERR_UNSUPPORTED, "feanorm: --cov and -P need the full second moments; dimension %d: 1 ... %d are built", dim,
          MOMENTS_MAX_DIM);
}

}  // namespace aasr

extern "C" {

aasr_status aasr_feanorm_pca(int32_t dim, const double *cov, const double *scale, int32_t unit_determinant, double *pca,
                             double *eigenvalues) {
  return guarded([&] {
    if (dim < 1 || !cov || !pca) raise(AASR_ERR_INVALID, "aasr_feanorm_pca: bad argument");
    std::vector<double> out((size_t)dim * dim), ev((size_t)dim);
    feanorm_pca(dim, cov, scale, unit_determinant != 0, out.data(), ev.data());
    std::copy(out.begin(), out.end(), pca);
    if (eigenvalues) std::copy(ev.begin(), ev.end(), eigenvalues);
  });
}

void aasr_feanorm_default_options(aasr_feanorm_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->block_size = 1000;
}

}  // extern "C"

// ---- the feanorm main loop over a recipe -------------------------------------------------------

extern "C" aasr_status aasr_run_feanorm_recipe(const char *feat_cfg_text, const char *recipe_path, aasr_feanorm_options *opt,
                                               aasr_run_stats *stats) {
  return guarded([&] {
    if (!feat_cfg_text || !recipe_path || !opt) raise(AASR_ERR_INVALID, "aasr_run_feanorm_recipe: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    opt->seconds_moments = opt->seconds_features = opt->blocks = 0;
    // ---- host only, before the device is opened (feanorm.cc:70-113, in its order)
    const bool full = opt->cov != 0 || opt->pca != nullptr;
    const bool utt_mode = opt->utt != nullptr;
    {
      const std::vector<ScannedModule> mods = scan_configuration(feat_cfg_text);
      int dim = mods.back().dim;
      if (opt->module) {
        const ScannedModule &nm = mods[(size_t)scanned_module(mods, opt->module)];
        if (nm.type != "normalization") raise(AASR_ERR_INVALID, "Module %s is not a normalization module", opt->module);
        dim = nm.dim;
      } else {
        if (utt_mode) raise(AASR_ERR_INVALID, "--utt requires the normalization module (--module)");
        if (opt->out) fprintf(stderr, "Warning: No --module given, configuration will be written unaltered\n");
      }
      if (opt->pca) {
        const ScannedModule &pm = mods[(size_t)scanned_module(mods, opt->pca)];
        if (pm.type != "lin_transform") raise(AASR_ERR_INVALID, "Module %s is not a linear transformation module", opt->pca);
        const int sd = pm.sources.empty() ? -1 : mods[(size_t)pm.sources[0]].dim;
        if (sd > 0 && dim > 0) refuse_pca_source(opt->pca, sd, dim);
      }
      if (opt->block_size < 1) raise(AASR_ERR_INVALID, "feanorm: the block size must be at least 1 (-b %d)", opt->block_size);
      if (!opt->speakers && utt_mode) raise(AASR_ERR_INVALID, "--utt requires --speakers");
      if (full && dim > 0) refuse_full_dim(dim);
    }
    const std::vector<RecipeInfo> infos = read_recipe_file(recipe_path, 0, 0, false);  // feanorm.cc:131-133

    // ---- the device
    std::unique_ptr<aasr_feat> feat(feat_create(feat_cfg_text));
    FeatModule *nm = opt->module ? &feat->mods[(size_t)feat->by_name.at(opt->module)] : nullptr;
    FeatModule *pm = opt->pca ? &feat->mods[(size_t)feat->by_name.at(opt->pca)] : nullptr;
    // feanorm.cc:77-80, 198: the statistics are those of the normalization module's first source; the batch evaluator
    // takes any module as its target, so the one handle serves (as in the lda driver)
    const int target = nm ? nm->sources[0] : -1;
    const int D = nm ? nm->dim : aasr_feat_dim(feat.get());
    if (pm) refuse_pca_source(opt->pca, feat->mods[(size_t)pm->sources[0]].dim, D);
    if (full) refuse_full_dim(D);
    aasr_spkc *spk = nullptr;
    if (opt->speakers) {
      if (aasr_spkc_create(feat.get(), nullptr, &spk) != AASR_OK || aasr_spkc_read_file(spk, opt->speakers) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    }
    std::unique_ptr<aasr_spkc, void (*)(aasr_spkc *)> spguard(spk, aasr_spkc_destroy);
    const float fr = aasr_feat_frame_rate(feat.get());
    const int bs = opt->block_size;

    aasr_moments *h = nullptr;
    {
      const aasr_status cs = aasr_moments_create(D, full ? AASR_MOMENTS_FULL : AASR_MOMENTS_DIAG, &h);
      if (cs != AASR_OK) raise(cs, "%s", last_error().c_str());
    }
    std::unique_ptr<aasr_moments, void (*)(aasr_moments *)> hguard(h, aasr_moments_destroy);
    GroupStager stager(feat.get(), spk, target);
    const hipStream_t stream = stager.stream;
    hipEvent_t ev[3];
    for (hipEvent_t &e : ev) AASR_HIP(hipEventCreate(&e));
    struct EvGuard {
      hipEvent_t *e;
      ~EvGuard() {
        for (int i = 0; i < 3; i++) (void)hipEventDestroy(e[i]);
      }
    } evguard{ev};

    // ---- the pass: a group of utterances' frames in one device buffer, one accumulation; with --utt a group is one
    // utterance, whose normalization must stand on the module before the next line's set_speaker reads it back
    const int64_t max_group_frames = (int64_t)1 << 18;
    const size_t nx = full ? (size_t)D * (D + 1) / 2 : (size_t)D;
    std::vector<int32_t> keep;  // per segment: it enters the global sums
    std::vector<double> ux((size_t)D), uxx(nx), sx((size_t)D), sxx(nx);
    int64_t num_frames = 0;
    size_t next = 0;
    while (next < infos.size()) {
      const size_t group_first = next;
      std::vector<std::vector<int16_t>> audio;
      std::vector<int32_t> start, rows, segs;
      int64_t rows_total = 0;
      const size_t seg0 = keep.size();
      while (next < infos.size() && audio.size() < (utt_mode ? 1 : 1024) && rows_total < max_group_frames) {
        const RecipeInfo &u = infos[next];
        announce(u, opt->info);
        audio.push_back(load_utterance_input(feat.get(), u));  // gen.open: a missing file stops the run
        const int eof = aasr_feat_eof_frame(feat.get(), (int64_t)audio.back().size());
        // feanorm.cc:169-175
        const int first = (int)(u.start_time * fr);
        int last = (int)(u.end_time * fr);
        if (last == 0) last = INT_MAX;
        const int n = std::max(0, std::min(last, eof) - first);
        const bool ended_at_eof = first < last && eof < last;  // generate(eof) ran and left the loop
        start.push_back(first);
        rows.push_back(n);
        for (int k = 0; k < n; k += bs) {
          const int len = std::min(bs, n - k);
          segs.insert(segs.end(), {(int32_t)(rows_total + k), len, (int32_t)next});
          keep.push_back(len == bs || ended_at_eof ? 1 : 0);  // feanorm.cc:178-195, 216-229
        }
        rows_total += n;
        next++;
      }
      stager.stage(audio, start, rows, [&](size_t i) {
        if (i == 0) AASR_HIP(hipEventRecord(ev[0], stream));  // the features' interval opens once the buffers stand
        apply_speaker(spk, infos[group_first + i]);  // feanorm.cc:146-152; a parameter change waits for the queued features
      });
      AASR_HIP(hipEventRecord(ev[1], stream));
      if (aasr_moments_accumulate_dev(h, stager.d_x.p, rows_total, segs.data(), (int32_t)(segs.size() / 3), stream) != AASR_OK)
        raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      AASR_HIP(hipEventRecord(ev[2], stream));
      AASR_HIP(hipStreamSynchronize(stream));  // the group's host audio goes out of scope; its sums are on the host
      float ms = 0;
      AASR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      opt->seconds_features += ms * 1e-3;
      AASR_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
      opt->seconds_moments += ms * 1e-3;
      num_frames += rows_total;
      if (utt_mode && !infos[group_first].utterance_id.empty()) {
        // feanorm.cc:247-266: the utterance's sums are its blocks' sums added in order, undivided
        std::fill(ux.begin(), ux.end(), 0.0);
        std::fill(uxx.begin(), uxx.end(), 0.0);
        for (size_t s = seg0; s < keep.size(); s++) {
          double c = 0;
          h->unpack(h->segs[s], &c, sx.data(), sxx.data());
          for (int d = 0; d < D; d++) ux[(size_t)d] += sx[(size_t)d];
          for (size_t k = 0; k < nx; k++) uxx[k] += sxx[k];
        }
        const int utt_frames = rows[0];
        std::vector<float> mean((size_t)D), scale((size_t)D);
        for (int d = 0; d < D; d++) {
          const double m = ux[(size_t)d] / (double)utt_frames;
          const double second = full ? uxx[(size_t)d * (d + 1) / 2 + d] : uxx[(size_t)d];
          mean[(size_t)d] = m;
          double var = sqrtf(second / (double)utt_frames - m * m);
          if (var <= 0) var = 1;
          scale[(size_t)d] = 1 / var;
        }
        // NormalizationModule::set_normalization, behind the speaker configuration's back
        spkc_feature_rewritten(spk, opt->module);
        nm->mean = mean;
        nm->scale = scale;
        nm->d_mean.upload(nm->mean.data(), nm->mean.size());
        nm->d_scale.upload(nm->scale.data(), nm->scale.size());
      }
    }

    // ---- feanorm.cc:268-279: the blocked sums on the host in recipe order, mean and scale
    if (aasr_moments_fetch(h, stream) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    double count = 0;
    std::vector<double> gm((size_t)D), gxx(nx);
    if (aasr_moments_blocked(h, bs, keep.data(), &count, gm.data(), gxx.data()) != AASR_OK)
      raise(AASR_ERR_INVALID, "%s", aasr_last_error());
    opt->blocks = count;
    auto second = [&](int d1, int d2) {  // d1 >= d2
      return full ? gxx[(size_t)d1 * (d1 + 1) / 2 + d2] : gxx[(size_t)d1];
    };
    std::vector<float> mean((size_t)D), scale((size_t)D);
    for (int d = 0; d < D; d++) {
      gm[(size_t)d] /= count;
      mean[(size_t)d] = gm[(size_t)d];
    }
    for (int d = 0; d < D; d++) scale[(size_t)d] = 1 / sqrtf(second(d, d) / count - gm[(size_t)d] * gm[(size_t)d]);
    std::vector<double> cov;
    if (full) {
      cov.resize((size_t)D * D);
      for (int d1 = 0; d1 < D; d1++)
        for (int d2 = 0; d2 < D; d2++)
          cov[(size_t)d1 * D + d2] = second(std::max(d1, d2), std::min(d1, d2)) / count - gm[(size_t)d1] * gm[(size_t)d2];
    }
    std::vector<double> tr;
    if (pm) {
      tr.resize((size_t)D * D);
      const std::vector<double> sc(scale.begin(), scale.end());
      feanorm_pca(D, cov.data(), sc.data(), opt->unit_determinant != 0, tr.data(), nullptr);
    }
    if (opt->print) {  // feanorm.cc:327-337
      printf("mean:\n");
      for (int d = 0; d < D; d++) printf("%f ", mean[(size_t)d]);
      printf("\n");
      printf("variance:\n");
      for (int d = 0; d < D; d++) printf("%f ", 1 / (scale[(size_t)d] * scale[(size_t)d]));
      printf("\n");
    }
    if (opt->cov) {  // feanorm.cc:339-351
      for (int d1 = 0; d1 < D; d1++) {
        for (int d2 = 0; d2 < D; d2++) printf("%f ", cov[(size_t)d1 * D + d2]);
        printf("\n");
      }
    }
    fflush(stdout);
    if (utt_mode) {  // feanorm.cc:353-369: every speaker and utterance
      char *text = nullptr;
      int64_t len = 0;
      if (aasr_spkc_write_text(spk, nullptr, -1, nullptr, -1, &text, &len) != AASR_OK) raise(AASR_ERR_INVALID, "%s", aasr_last_error());
      std::unique_ptr<char, void (*)(void *)> tguard(text, free);
      write_text_file(opt->utt, text, (size_t)len);
    }
    if (nm && !utt_mode) {  // feanorm.cc:371-372
      nm->mean = mean;
      nm->scale = scale;
      nm->d_mean.upload(nm->mean.data(), nm->mean.size());
      nm->d_scale.upload(nm->scale.data(), nm->scale.size());
    }
    if (pm) {  // LinTransformModule::set_transformation_matrix: the working and the configured matrix both, in float
      const std::vector<float> trf(tr.begin(), tr.end());
      pm->matrix = trf;
      pm->orig_matrix = trf;
      pm->matrix_defined = true;
      pm->d_matrix.upload(pm->matrix.data(), pm->matrix.size());
    }
    if (opt->out) {
      const std::string text = feat_write_configuration(feat.get());
      write_text_file(opt->out, text.data(), text.size());
    }
    fill_run_stats(stats, (int64_t)infos.size(), num_frames, t0, opt->seconds_moments + opt->seconds_features);
  });
}

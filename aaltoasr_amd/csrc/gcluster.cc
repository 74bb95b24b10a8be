// gcluster.cc -- clustering of the Gaussian pool (aku/gcluster.cc, diagonal mode, one group): the operands of the
// device kernels (kl_cluster.h), the two step entries on plain arrays, the run (make_initial_clusters,
// refine_clustering(4), save_clustering) and its entries on a .gk file, on arrays and on a loaded model.
//
// Host and device share the work as the arithmetic demands.  Distances and centre sums: the device.  The
// log-determinants, sum_k log(cov[k]) in dimension order: the host, with the C library's log -- the reference's value
// is that function's, and the device's log need not round as it does.  So every step ends with the centres'
// covariances on the host and their log-determinants and validity back on the device: one synchronisation per step,
// which also brings the map and the minima when -i asks for them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "kl_cluster.h"

using namespace aasr;

namespace {

// sum_k log(cov[k]), gcluster.cc:121-124 / 215-218
double log_det(const double *cov, int D) {
  double t = 0;
  for (int k = 0; k < D; k++) t += log(cov[k]);
  return t;
}

// [G][D] mean and cov -> [D][G][2]
std::vector<double> pack_gaussians(int D, int G, const double *mean, const double *cov) {
  std::vector<double> out((size_t)D * G * 2);
  for (int64_t g = 0; g < G; g++)
    for (int k = 0; k < D; k++) {
      out[((size_t)k * G + g) * 2] = mean[(size_t)g * D + k];
      out[((size_t)k * G + g) * 2 + 1] = cov ? cov[(size_t)g * D + k] : 1.0;
    }
  return out;
}

// [C][D] centres -> the chunked operand; centre c = row row_of[c] of mean (nullptr: row c); no covariance: 1
std::vector<double> pack_centres(int D, int C, const double *mean, const double *cov, const int32_t *row_of) {
  std::vector<double> out((size_t)klc_centre_doubles(D, C));
  for (size_t i = 0; i < out.size(); i += 2) out[i] = 0.0, out[i + 1] = 1.0;
  for (int c = 0; c < C; c++) {
    const size_t r = row_of ? (size_t)row_of[c] : (size_t)c;
    for (int k = 0; k < D; k++) {
      const size_t at = (size_t)klc_centre_at(D, c, k);
      out[at] = mean[r * D + k];
      out[at + 1] = cov ? cov[r * D + k] : 1.0;
    }
  }
  return out;
}

// fill_random_permutation (gcluster.cc:167-179): rand() once per position, also for the last
std::vector<int32_t> random_permutation(int num) {
  std::vector<int32_t> p((size_t)num);
  for (int i = 0; i < num; i++) p[(size_t)i] = i;
  for (int i = 0; i < num; i++) std::swap(p[(size_t)i], p[(size_t)(i + rand() % (num - i))]);
  return p;
}

void check_shape(const char *who, int D, int G, int C) {
  if (D < 1 || G < 1 || C < 1) raise(AASR_ERR_INVALID, "%s: dim, n_gauss and n_clusters must be positive", who);
  if ((int64_t)D * G > ((int64_t)1 << 40) || (int64_t)D * C > ((int64_t)1 << 40))
    raise(AASR_ERR_INVALID, "%s: arrays too large", who);
}

// the pool and the centres on the device, and one step of the run
struct Run {
  int D, G, C;
  DevBuf<double> gauss, g_ldet, mean, cov, centres, c_mean, c_cov, c_ldet, dist;
  DevBuf<int32_t> c_valid, c_count, map;
  std::vector<double> h_c_cov, h_c_ldet, h_dist;
  std::vector<int32_t> h_count, h_valid, h_map;
  hipStream_t st = nullptr;

  Run(int D_, int G_, int C_, const double *mean_, const double *cov_, const double *ldet_) : D(D_), G(G_), C(C_) {
    const std::vector<double> packed = pack_gaussians(D, G, mean_, cov_);
    gauss.upload(packed.data(), packed.size());
    g_ldet.upload(ldet_, (size_t)G);
    mean.upload(mean_, (size_t)G * D);
    cov.upload(cov_, (size_t)G * D);
    centres.alloc((size_t)klc_centre_doubles(D, C));
    c_mean.alloc((size_t)C * D);
    c_cov.alloc((size_t)C * D);
    c_ldet.alloc((size_t)C);
    c_valid.alloc((size_t)C);
    c_count.alloc((size_t)C);
    map.alloc((size_t)G);
    dist.alloc((size_t)G);
    h_c_cov.resize((size_t)C * D);
    h_c_ldet.assign((size_t)C, 0.0);
    h_count.resize((size_t)C);
    h_valid.assign((size_t)C, 0);
    h_map.resize((size_t)G);
    h_dist.resize((size_t)G);
  }

  void set_centres(const std::vector<double> &packed) {
    AASR_HIP(hipMemcpyAsync(centres.p, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, st));
    AASR_HIP(hipStreamSynchronize(st));  // (the host vector goes out of scope)
  }

  // assignment, centre sums, the step's one synchronisation, the centres' log-determinants and validity
  void step(bool euclid, bool want_map) {
    KlcAssignParams a{gauss.p, g_ldet.p, centres.p, c_ldet.p, c_valid.p, D, G, C, map.p, dist.p};
    klc_assign_launch(a, euclid, st);
    KlcCentreParams c{mean.p, cov.p, map.p, D, G, C, c_mean.p, c_cov.p, centres.p, c_count.p};
    klc_centres_launch(c, st);
    AASR_HIP(hipMemcpyAsync(h_c_cov.data(), c_cov.p, h_c_cov.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    AASR_HIP(hipMemcpyAsync(h_count.data(), c_count.p, h_count.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (want_map) {
      AASR_HIP(hipMemcpyAsync(h_map.data(), map.p, h_map.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AASR_HIP(hipMemcpyAsync(h_dist.data(), dist.p, h_dist.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    AASR_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < C; j++) {
      h_valid[(size_t)j] = h_count[(size_t)j] > 0;
      h_c_ldet[(size_t)j] = h_valid[(size_t)j] ? log_det(h_c_cov.data() + (size_t)j * D, D) : 0.0;
    }
    AASR_HIP(hipMemcpyAsync(c_ldet.p, h_c_ldet.data(), (size_t)C * sizeof(double), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(c_valid.p, h_valid.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
};

// the reference's checks on the options, in its order (gcluster.cc:379-436); host only
void check_options(const aasr_gcluster_options &o, int64_t G) {
  if (o.clusters < 2) raise(AASR_ERR_INVALID, "Invalid number of clusters");
  if (o.iterations < 1) raise(AASR_ERR_INVALID, "Invalid number of iterations");
  if (o.regtree && o.base)
    raise(AASR_ERR_UNSUPPORTED,
          "gcluster: -R/--regtree with -b/--base (one group of clusters per regression class, merged down to -C) is not "
          "supported; only the single group over the whole pool is");
  if (o.regtree || o.base) raise(AASR_ERR_INVALID, "Both tree and model must be given");
  if (G < o.clusters) raise(AASR_ERR_INVALID, "Not enough Gaussians to cluster!");
  if (o.full)
    raise(AASR_ERR_UNSUPPORTED,
          "gcluster: -F/--full (full-covariance cluster centres) is not supported; only the diagonal mode is");
}

// make_initial_clusters + refine_clustering(4) + the renumbering of save_clustering: cluster_of [G], opt->written
void cluster_pool(int D, int G, const double *mean, const double *cov, aasr_gcluster_options *opt, int32_t *cluster_of) {
  check_options(*opt, G);
  check_shape("gcluster", D, G, opt->clusters);
  require_device();
  const int C = opt->clusters;
  if (opt->progress) fprintf(stderr, "make initial clusters\n");
  std::vector<double> ldet((size_t)G);
  for (int g = 0; g < G; g++) ldet[(size_t)g] = log_det(cov + (size_t)g * D, D);
  srand(1);  // what a fresh process has: the tool's permutation, also from a long-lived caller
  const std::vector<int32_t> perm = random_permutation(G);

  Run run(D, G, C, mean, cov, ldet.data());
  opt->seconds_steps = 0;
  auto timed_step = [&](bool euclid, bool want_map) {
    const auto t0 = std::chrono::steady_clock::now();
    run.step(euclid, want_map);  // (ends behind its synchronisation; the uploads that follow are a few kilobytes)
    opt->seconds_steps += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  run.set_centres(pack_centres(D, C, mean, nullptr, perm.data()));
  timed_step(true, false);
  if (opt->progress) fprintf(stderr, "start clustering\n");
  const int passes = 4;  // gcluster.cc:455: refine_clustering(4), whatever -t says
  for (int iter = 0; iter < passes; iter++) {
    const bool last = iter + 1 == passes;
    timed_step(false, last || opt->info > 0);
    if (opt->info > 0) {
      double total_kl = 0;
      for (int g = 0; g < G; g++) {
        if (opt->info > 1) printf("Gaussian %i in cluster %i, distance %g\n", g, run.h_map[(size_t)g], run.h_dist[(size_t)g]);
        total_kl += run.h_dist[(size_t)g];
      }
      printf("Iteration %i: Average Kullback-Leibler divergence = %g\n", iter + 1, total_kl / (double)G);
      fflush(stdout);
    }
  }
  // save_clustering: the valid clusters renumbered in order; a Gaussian's cluster has it as a member, so it is valid
  std::vector<int32_t> real_id((size_t)C);
  int32_t next = 0;
  for (int j = 0; j < C; j++) real_id[(size_t)j] = run.h_valid[(size_t)j] ? next++ : -1;
  if (next == 0) raise(AASR_ERR_INVALID, "No valid clusters!");
  for (int g = 0; g < G; g++) cluster_of[g] = real_id[(size_t)run.h_map[(size_t)g]];
  opt->written = next;
}

// covariance diagonals of a parsed pool (Gaussian::get_covariance(Vector&))
std::vector<double> pool_diagonal(const HostModel &m) {
  const size_t D = (size_t)m.dim;
  std::vector<double> d((size_t)m.G * D);
  for (size_t g = 0; g < (size_t)m.G; g++) {
    const bool full = m.any_full() && m.is_full[g];
    for (size_t k = 0; k < D; k++) d[g * D + k] = full ? m.cov[(g * D + k) * D + k] : m.var[g * D + k];
  }
  return d;
}

void check_pool_size(const HostModel &m) {
  if (m.G > INT32_MAX || m.dim < 1) raise(AASR_ERR_INVALID, "gcluster: pool of %ld Gaussians, %d dimensions", (long)m.G, m.dim);
}

}  // namespace

extern "C" {

aasr_status aasr_gcluster_assign(int32_t dim, int32_t n_gauss, const double *mean, const double *cov, const double *ldet,
                                 int32_t n_clusters, const double *c_mean, const double *c_cov, const double *c_ldet,
                                 const int32_t *c_valid, int32_t euclid, int32_t *out_index, double *out_dist) {
  return guarded([&] {
    if (!mean || !c_mean || !out_index || !out_dist || (!euclid && (!cov || !ldet || !c_cov || !c_ldet || !c_valid)))
      raise(AASR_ERR_INVALID, "aasr_gcluster_assign: null argument");
    check_shape("aasr_gcluster_assign", dim, n_gauss, n_clusters);
    require_device();
    const int D = dim, G = n_gauss, C = n_clusters;
    const std::vector<double> pg = pack_gaussians(D, G, mean, euclid ? nullptr : cov);
    const std::vector<double> pc = pack_centres(D, C, c_mean, euclid ? nullptr : c_cov, nullptr);
    DevBuf<double> d_g, d_gl, d_c, d_cl, d_dist;
    DevBuf<int32_t> d_cv, d_idx;
    d_g.upload(pg.data(), pg.size());
    d_c.upload(pc.data(), pc.size());
    if (!euclid) {
      d_gl.upload(ldet, (size_t)G);
      d_cl.upload(c_ldet, (size_t)C);
      d_cv.upload(c_valid, (size_t)C);
    }
    d_idx.alloc((size_t)G);
    d_dist.alloc((size_t)G);
    KlcAssignParams p{d_g.p, d_gl.p, d_c.p, d_cl.p, d_cv.p, D, G, C, d_idx.p, d_dist.p};
    klc_assign_launch(p, euclid != 0, nullptr);
    AASR_HIP(hipMemcpy(out_index, d_idx.p, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost));
    AASR_HIP(hipMemcpy(out_dist, d_dist.p, (size_t)G * sizeof(double), hipMemcpyDeviceToHost));
  });
}

aasr_status aasr_gcluster_centres(int32_t dim, int32_t n_gauss, const double *mean, const double *cov, int32_t n_clusters,
                                  const int32_t *map, double *c_mean, double *c_cov, double *c_ldet, int32_t *c_valid) {
  return guarded([&] {
    if (!mean || !cov || !map || !c_mean || !c_cov || !c_ldet || !c_valid)
      raise(AASR_ERR_INVALID, "aasr_gcluster_centres: null argument");
    check_shape("aasr_gcluster_centres", dim, n_gauss, n_clusters);
    for (int g = 0; g < n_gauss; g++)
      if (map[g] < 0 || map[g] >= n_clusters)
        raise(AASR_ERR_INVALID, "aasr_gcluster_centres: cluster %d of Gaussian %d out of range", map[g], g);
    require_device();
    const int D = dim, G = n_gauss, C = n_clusters;
    DevBuf<double> d_m, d_v, d_cm, d_cc, d_pk;
    DevBuf<int32_t> d_map, d_cnt;
    d_m.upload(mean, (size_t)G * D);
    d_v.upload(cov, (size_t)G * D);
    d_map.upload(map, (size_t)G);
    d_cm.alloc((size_t)C * D);
    d_cc.alloc((size_t)C * D);
    d_pk.alloc((size_t)klc_centre_doubles(D, C));
    d_cnt.alloc((size_t)C);
    KlcCentreParams p{d_m.p, d_v.p, d_map.p, D, G, C, d_cm.p, d_cc.p, d_pk.p, d_cnt.p};
    klc_centres_launch(p, nullptr);
    std::vector<int32_t> count((size_t)C);
    AASR_HIP(hipMemcpy(c_mean, d_cm.p, (size_t)C * D * sizeof(double), hipMemcpyDeviceToHost));
    AASR_HIP(hipMemcpy(c_cov, d_cc.p, (size_t)C * D * sizeof(double), hipMemcpyDeviceToHost));
    AASR_HIP(hipMemcpy(count.data(), d_cnt.p, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int j = 0; j < C; j++) {
      c_valid[j] = count[(size_t)j] > 0;
      c_ldet[j] = c_valid[j] ? log_det(c_cov + (size_t)j * D, D) : 0.0;
    }
  });
}

int32_t aasr_debug_gcluster_chunk(void) { return KLC_CHUNK; }

void aasr_gcluster_default_options(aasr_gcluster_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->clusters = 1000;
  o->iterations = 4;
}

aasr_status aasr_gcluster_arrays(int32_t dim, int32_t n_gauss, const double *mean, const double *cov,
                                 aasr_gcluster_options *opt, int32_t *cluster_of) {
  return guarded([&] {
    if (!mean || !cov || !opt || !cluster_of || dim < 1 || n_gauss < 0)
      raise(AASR_ERR_INVALID, "aasr_gcluster_arrays: bad argument");
    cluster_pool(dim, n_gauss, mean, cov, opt, cluster_of);
  });
}

aasr_status aasr_run_gcluster(const char *gk_path, const char *out_path, aasr_gcluster_options *opt) {
  return guarded([&] {
    if (!gk_path || !out_path || !opt) raise(AASR_ERR_INVALID, "aasr_run_gcluster: null argument");
    HostModel m;
    read_gk_pool(gk_path, m);
    check_pool_size(m);
    const std::vector<double> diag = pool_diagonal(m);
    std::vector<int32_t> cluster_of((size_t)m.G);
    cluster_pool(m.dim, (int)m.G, m.mean.data(), diag.data(), opt, cluster_of.data());
    // save_clustering (gcluster.cc:337-350)
    std::ofstream out(out_path);
    if (!out) raise(AASR_ERR_IO, "save_clustering: Could not open file `%s'.", out_path);
    out << opt->written << "\n";
    for (int64_t g = 0; g < m.G; g++) out << g << " " << cluster_of[(size_t)g] << "\n";
    if (opt->info > 0) {
      printf("Wrote %i clusters\n", opt->written);
      fflush(stdout);
    }
    out.flush();
    if (!out) raise(AASR_ERR_IO, "Error writing file: %s", out_path);
  });
}

aasr_status aasr_gmm_cluster(aasr_gmm *h, int32_t n_clusters, int32_t info) {
  return guarded([&] {
    if (!h) raise(AASR_ERR_INVALID, "aasr_gmm_cluster: null handle");
    const HostModel &m = h->host;
    check_pool_size(m);
    aasr_gcluster_options opt;
    aasr_gcluster_default_options(&opt);
    opt.clusters = n_clusters;
    opt.info = info;
    const std::vector<double> diag = pool_diagonal(m);
    std::vector<int32_t> gi((size_t)m.G + 1), ci((size_t)m.G + 1);
    cluster_pool(m.dim, (int)m.G, m.mean.data(), diag.data(), &opt, ci.data());
    for (int64_t g = 0; g < m.G; g++) gi[(size_t)g] = (int32_t)g;
    // PDFPool::read_clustering runs its loop body once more at the end of the file: the last pair counts twice
    gi[(size_t)m.G] = gi[(size_t)m.G - 1];
    ci[(size_t)m.G] = ci[(size_t)m.G - 1];
    gmm_set_clustering(h, opt.written, (int64_t)gi.size(), gi.data(), ci.data());
  });
}

}  // extern "C"

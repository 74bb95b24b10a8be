// stats_files.cc -- the files of the statistics handle (stats.cc): the dump writers of HmmSet::dump_statistics
// (.gks, .mcs, .phs), the .lls writer, aasr_stats_write over a fetched handle, and the host-only entries that read a
// .phn segmentation (the reader is recipe_pass.cc's).
#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "common.h"
#include "recipe_pass.h"
#include "stats.h"

using namespace aasr;

extern "C" {

// ---- dump writers (HmmSet::dump_statistics, HmmSet.cc:546-625) --------------------------------

aasr_status aasr_stats_write_gks(const char *path, int32_t pool_size, int32_t dim, int32_t mode, const int64_t *feacount,
                                 const double *gamma, const double *aux_gamma, const double *sum_x, const double *sum_xx) {
  return guarded([&] {
    if (!path || pool_size < 0 || dim < 0 || (pool_size > 0 && (!feacount || !gamma || !aux_gamma || !sum_x || !sum_xx)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_gks: bad argument");
    std::ofstream gks(path, std::ofstream::binary);
    if (!gks) raise(AASR_ERR_IO, "HmmSet::dump_gk_statistics(): could not open %s", path);
    gks.write((const char *)&pool_size, sizeof(int));
    gks.write((const char *)&dim, sizeof(int));
    gks.write((const char *)&mode, sizeof(int));
    const int zero = 0, end = -1;
    for (int g = 0; gks && g < pool_size; g++) {
      gks.write((const char *)&g, sizeof(int));
      if (feacount[g] > 0) {  // Gaussian::dump_statistics: the ML buffer, when it was accumulated
        gks.write((const char *)&zero, sizeof(int));
        const int fc = (int)feacount[g];
        gks.write((const char *)&fc, sizeof(int));
        gks.write((const char *)&gamma[g], sizeof(double));
        gks.write((const char *)&aux_gamma[g], sizeof(double));
        for (int d = 0; d < dim; d++) {
          const float t = (float)sum_x[(size_t)g * dim + d];
          gks.write((const char *)&t, sizeof(float));
        }
        for (int d = 0; d < dim; d++) {
          const float t = (float)sum_xx[(size_t)g * dim + d];
          gks.write((const char *)&t, sizeof(float));
        }
      }
      gks.write((const char *)&end, sizeof(int));
    }
    if (!gks) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

// FullStatisticsAccumulator::dump_statistics (Distributions.cc:42-60) under HmmSet::dump_gk_statistics
aasr_status aasr_stats_write_gks_full(const char *path, int32_t pool_size, int32_t dim, const int64_t *feacount,
                                      const double *gamma, const double *aux_gamma, const double *sum_x,
                                      const double *sum_xx_packed) {
  return guarded([&] {
    if (!path || pool_size < 0 || dim < 0 || (pool_size > 0 && (!feacount || !gamma || !aux_gamma || !sum_x || !sum_xx_packed)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_gks_full: bad argument");
    std::ofstream gks(path, std::ofstream::binary);
    if (!gks) raise(AASR_ERR_IO, "HmmSet::dump_gk_statistics(): could not open %s", path);
    const int mode = 3;  // PDF_ML_STATS | PDF_ML_FULL_STATS
    gks.write((const char *)&pool_size, sizeof(int));
    gks.write((const char *)&dim, sizeof(int));
    gks.write((const char *)&mode, sizeof(int));
    const int zero = 0, end = -1;
    const size_t tri = (size_t)dim * (dim + 1) / 2;
    std::vector<float> t((size_t)dim + tri);
    for (int g = 0; gks && g < pool_size; g++) {
      gks.write((const char *)&g, sizeof(int));
      if (feacount[g] > 0) {
        gks.write((const char *)&zero, sizeof(int));
        const int fc = (int)feacount[g];
        gks.write((const char *)&fc, sizeof(int));
        gks.write((const char *)&gamma[g], sizeof(double));
        gks.write((const char *)&aux_gamma[g], sizeof(double));
        for (int d = 0; d < dim; d++) t[(size_t)d] = (float)sum_x[(size_t)g * dim + d];
        for (size_t e = 0; e < tri; e++) t[(size_t)dim + e] = (float)sum_xx_packed[(size_t)g * tri + e];  // row by row, j <= i
        gks.write((const char *)t.data(), (std::streamsize)(t.size() * sizeof(float)));
      }
      gks.write((const char *)&end, sizeof(int));
    }
    if (!gks) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_mcs(const char *path, int32_t num_pdfs, int32_t mode, const int32_t *mix_off,
                                 const int32_t *mix_idx, const int64_t *count, const double *gamma,
                                 const double *aux_gamma, const double *mixture_ll) {
  return guarded([&] {
    if (!path || num_pdfs < 0 || (num_pdfs > 0 && (!mix_off || !mix_idx || !count || !gamma || !mixture_ll)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_mcs: bad argument");
    std::ofstream mcs(path);
    if (!mcs) raise(AASR_ERR_IO, "HmmSet::dump_mc_statistics(): could not open %s", path);
    mcs << num_pdfs << std::endl;
    mcs << mode << std::endl;
    for (int i = 0; i < num_pdfs; i++) {
      mcs << i << std::endl;
      // Mixture::dump_statistics (Distributions.cc:2192-2208)
      mcs.precision(10);
      if (count[i] > 0) {
        const int n = mix_off[i + 1] - mix_off[i];
        mcs << 0 << " " << n;
        for (int k = 0; k < n; k++) mcs << " " << mix_idx[mix_off[i] + k] << " " << gamma[mix_off[i] + k];
        mcs << " " << (aux_gamma ? aux_gamma[i] : 0.0) << " " << mixture_ll[i];
        mcs << std::endl;
      }
      mcs << "-1" << std::endl;
    }
    if (!mcs) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_phs(const char *path, int32_t num_transitions, const int32_t *source,
                                 const int32_t *target_offset, const double *count) {
  return guarded([&] {
    if (!path || num_transitions < 0 || (num_transitions > 0 && (!source || !target_offset || !count)))
      raise(AASR_ERR_INVALID, "aasr_stats_write_phs: bad argument");
    if (num_transitions == 0) return;  // dump_ph_statistics writes nothing without transitions
    std::ofstream phs(path);
    if (!phs) raise(AASR_ERR_IO, "HmmSet::dump_ph_statistics(): could not open %s", path);
    phs << num_transitions << std::endl;
    for (int t = 0; t < num_transitions; t++)
      if (count[t] > 0) {
        phs << source[t] << " ";
        phs << target_offset[t] << " ";
        phs << count[t] << std::endl;
      }
    if (!phs) raise(AASR_ERR_IO, "write error on %s", path);
  });
}

aasr_status aasr_stats_write_lls(const char *path, double loglik, int64_t frames) {
  return guarded([&] {
    if (!path) raise(AASR_ERR_INVALID, "aasr_stats_write_lls: null argument");
    std::ofstream lls(path);
    if (!lls) return;  // stats.cc:779: no file, no message
    lls.precision(12);
    lls << "Numerator loglikelihood: " << loglik << std::endl;
    lls << "Number of frames: " << frames << std::endl;
  });
}

aasr_status aasr_stats_write(const aasr_stats *h, const char *base) {
  return guarded([&] {
    require_fetched(h, "aasr_stats_write");
    if (!base) raise(AASR_ERR_INVALID, "aasr_stats_write: null argument");
    const std::string b(base);
    auto ok = [](aasr_status s) {
      if (s != AASR_OK) raise(s, "%s", last_error().c_str());
    };
    ok(aasr_stats_write_phs((b + ".phs").c_str(), (int32_t)h->tr_source.size(), h->tr_source.data(), h->tr_offset.data(),
                            h->tr_count.data()));
    std::vector<int64_t> count((size_t)std::max(1, h->S));
    std::vector<double> gamma((size_t)std::max(1, h->K)), mll((size_t)std::max(1, h->S)), aux((size_t)std::max(1, h->S), 0.0);
    ok(aasr_stats_mixtures(h, count.data(), gamma.data(), mll.data()));
    ok(aasr_stats_write_mcs((b + ".mcs").c_str(), h->S, h->full ? 3 : 1, h->mix_off.data(), h->mix_idx.data(), count.data(),
                            gamma.data(), aux.data(), mll.data()));
    const size_t G1 = (size_t)std::max(1, h->G);
    std::vector<int64_t> fc(G1);
    std::vector<double> gg(G1), ga(G1), sx(G1 * h->D + 1), sxx(G1 * h->D + 1);
    ok(aasr_stats_gaussians(h, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
    if (h->full)
      ok(aasr_stats_write_gks_full((b + ".gks").c_str(), h->G, h->D, fc.data(), gg.data(), ga.data(), sx.data(), h->h_full.data()));
    else
      ok(aasr_stats_write_gks((b + ".gks").c_str(), h->G, h->D, 1, fc.data(), gg.data(), ga.data(), sx.data(), sxx.data()));
  });
}

// ---- host-only segmentation reader ---------------------------------------------------------------

static aasr_status read_segmentation_call(const char *what, const aasr_topo *topo, const char *path, float frame_rate,
                                          int32_t first_frame, int32_t last_frame, int32_t eof_frame, int32_t flags,
                                          int32_t transitions, int32_t *start_frame, int32_t **pdf, int32_t **transition,
                                          int32_t *n_frames) {
  return guarded([&] {
    if (!topo || !path || !start_frame || !pdf || !transition || !n_frames) raise(AASR_ERR_INVALID, "%s: null argument", what);
    *pdf = nullptr;
    *transition = nullptr;
    if (flags & ~(AASR_PHN_STATE_NUM_LABELS | AASR_PHN_RELATIVE_SAMPLES)) raise(AASR_ERR_INVALID, "%s: unknown flags %d", what, flags);
    TopoTables tt(topo);
    Segmentation seg = read_segmentation(topo, tt, path, frame_rate, first_frame, last_frame, eof_frame, transitions != 0, flags);
    const size_t n = seg.pdf.size();
    *pdf = (int32_t *)malloc(std::max<size_t>(1, n) * sizeof(int32_t));
    *transition = (int32_t *)malloc(std::max<size_t>(1, n) * sizeof(int32_t));
    if (!*pdf || !*transition) {
      free(*pdf);
      free(*transition);
      *pdf = *transition = nullptr;
      raise(AASR_ERR_INVALID, "out of memory");
    }
    std::copy(seg.pdf.begin(), seg.pdf.end(), *pdf);
    std::fill(*transition, *transition + n, -1);  // (what the reader leaves out when no transitions are asked for)
    std::copy(seg.tr.begin(), seg.tr.end(), *transition);
    *start_frame = seg.start_frame;
    *n_frames = seg.initialized ? (int32_t)n : -1;
  });
}

aasr_status aasr_stats_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate, int32_t first_frame,
                                         int32_t last_frame, int32_t eof_frame, int32_t transitions,
                                         int32_t *start_frame, int32_t **pdf, int32_t **transition, int32_t *n_frames) {
  return read_segmentation_call("aasr_stats_read_segmentation", topo, path, frame_rate, first_frame, last_frame, eof_frame, 0,
                                transitions, start_frame, pdf, transition, n_frames);
}

aasr_status aasr_phn_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate, int32_t first_frame,
                                       int32_t last_frame, int32_t eof_frame, int32_t flags, int32_t transitions,
                                       int32_t *start_frame, int32_t **pdf, int32_t **transition, int32_t *n_frames) {
  return read_segmentation_call("aasr_phn_read_segmentation", topo, path, frame_rate, first_frame, last_frame, eof_frame,
                                flags, transitions, start_frame, pdf, transition, n_frames);
}
}  // extern "C"

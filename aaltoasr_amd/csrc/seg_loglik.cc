// seg_loglik.cc -- the handle of the per-frame log-likelihood of a state segmentation (seg_loglik.h): what
// aku/vtln.cc:99-114 asks of the model, safe_log(Mixture::compute_likelihood(frame)) of one pdf per frame, for many
// frames in one launch.  The row list is the statistics handle's (rows_by_pdf, stats.h), and so are the models it
// refuses and what it does with frames whose pdf is out of range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "common.h"
#include "gmm.h"
#include "seg_loglik.h"
#include "stats.h"

using namespace aasr;

struct aasr_segll {
  aasr_gmm *gmm = nullptr;
  int D = 0, S = 0, dimp = 0;
  int32_t stride = 0, sub = 0;
  DevBuf<int32_t> d_rows;
  DevBuf<SegllItem> d_items;
  // host staging of the last call, kept until its uploads are done
  std::vector<int32_t> h_rows;
  std::vector<SegllItem> h_items;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  // the last launch (aasr_debug_segll_shape): items, rows per sub-block, LDS bytes, LDS row stride, rows of its largest item
  int32_t last_shape[5] = {0, 0, 0, 0, 0};
  ~aasr_segll() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

extern "C" {

aasr_status aasr_segll_create(aasr_gmm *gmm, aasr_segll **out) {
  return guarded([&] {
    if (!gmm || !out) raise(AASR_ERR_INVALID, "aasr_segll_create: null argument");
    *out = nullptr;
    check_stats_model(gmm, "segll");  // (before the device is asked for anything)
    int32_t stride, sub;
    segll_shape(gmm->host.dim, &stride, &sub);
    if (gmm->host.dim < 1 || sub < 1)
      raise(AASR_ERR_UNSUPPORTED, "segll: a row of %d dimensions does not fit the kernel's LDS", gmm->host.dim);
    require_device();
    std::unique_ptr<aasr_segll> h(new aasr_segll());
    h->gmm = gmm;
    h->D = gmm->host.dim;
    h->S = (int)gmm->host.S;
    h->stride = stride;
    h->sub = sub;
    gmm_build_f64(gmm, true);
    h->dimp = gmm->f64_dimp;
    AASR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
  });
}

void aasr_segll_destroy(aasr_segll *h) { delete h; }

void aasr_debug_segll_shape(const aasr_segll *h, int32_t *out) {
  if (!h || !out) return;
  std::copy(h->last_shape, h->last_shape + 5, out);
}

aasr_status aasr_segll_score_dev(aasr_segll *h, const double *d_frames, int64_t n_frames, const int32_t *pdf,
                                 double *d_frame_ll, void *stream) {
  return guarded([&] {
    if (!h || n_frames < 0 || (n_frames > 0 && (!d_frames || !pdf || !d_frame_ll)))
      raise(AASR_ERR_INVALID, "aasr_segll_score_dev: bad argument");
    if (n_frames > INT32_MAX) raise(AASR_ERR_INVALID, "aasr_segll_score_dev: more than 2^31 frames in one call");
    if (n_frames == 0) return;
    // the model may have changed under the handle (a speaker's transform): refused as at create, records rebuilt
    check_stats_model(h->gmm, "segll");
    gmm_build_f64(h->gmm, true);
    const hipStream_t st = (hipStream_t)stream;
    // the host tables of the previous call may still be on their way to the device
    if (h->staged_pending) AASR_HIP(hipEventSynchronize(h->staged));
    h->staged_pending = false;
    std::vector<int64_t> cnt;
    rows_by_pdf("aasr_segll_score_dev", h->S, pdf, n_frames, &cnt, &h->h_rows);
    h->h_items.clear();
    int32_t largest = 0;
    for (int s = 0; s < h->S; s++)  // (a mixture without components gets its items too: total 0, safe_log(0) per frame)
      for (int64_t b = cnt[(size_t)s]; b < cnt[(size_t)s + 1]; b += SEGLL_ITEM) {
        SegllItem it;
        it.row_begin = b;
        it.pdf = s;
        it.n = (int32_t)std::min<int64_t>(SEGLL_ITEM, cnt[(size_t)s + 1] - b);
        largest = std::max(largest, it.n);
        h->h_items.push_back(it);
      }
    if (h->h_items.empty()) return;
    h->d_rows.ensure(h->h_rows.size());
    h->d_items.ensure(h->h_items.size());
    AASR_HIP(hipMemcpyAsync(h->d_rows.p, h->h_rows.data(), h->h_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AASR_HIP(hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(SegllItem), hipMemcpyHostToDevice, st));
    AASR_HIP(hipEventRecord(h->staged, st));
    h->staged_pending = true;
    SegllParams p{};
    p.x = d_frames;
    p.rows = h->d_rows.p;
    p.items = h->d_items.p;
    p.recs = h->gmm->f64_recs.p;
    p.state_off = h->gmm->f64_state_off.p;
    p.frame_ll = d_frame_ll;
    p.dim = h->D;
    p.dimp = h->gmm->f64_dimp;
    p.stride = h->stride;
    p.sub = std::min(h->sub, largest);  // (no more LDS than the call's largest item fills: more workgroups a CU)
    const int32_t shape[5] = {(int32_t)h->h_items.size(), p.sub, (int32_t)((size_t)p.sub * p.stride * sizeof(double)),
                              p.stride, largest};
    std::copy(shape, shape + 5, h->last_shape);
    segll_items_launch(p, (int)h->h_items.size(), st);
  });
}

}  // extern "C"

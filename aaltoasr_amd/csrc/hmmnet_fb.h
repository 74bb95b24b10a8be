// hmmnet_fb.h -- device layout of the forward-backward pass over HMM networks, shared by the kernel
// (hmmnet_fb.hip) and its handle (hmmnet_fb.cc).
//
// One workgroup of FB_THREADS lanes runs one utterance: serial in frames, parallel over arcs and nodes.
// Per utterance the device keeps the node scores of every frame after the epsilon closure (beta, (T + 1) x
// nodes doubles) and the per-frame best backward score (T doubles) -- not T x arcs arc scores: the forward
// pass recomputes an arc's backward value and its pruning decision from those with the code the backward pass
// ran (fb_raw / fb_value).
//
// The two working node vectors (the row under construction; alpha and the next alpha) live in LDS when the
// network has at most FB_LDS_NODES nodes (2 x 2048 doubles = 32 KB, plus the 2 KB reduction pad: 34 KB of the
// CU's 160 KB, so four utterances fit a CU) and in global memory beyond that or when the handle was created
// with force_global.  aasr_debug_fb_shape reports which form the last launch ran.  The arc-sized scratch
// (two doubles per emitting arc) is in global memory in both forms.
//
// With want_path the Viterbi walk also keeps which emitting arc it took at each frame: T int32 per utterance in a
// path buffer, stored by the lane that walks, next to the occupancy it sets.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aasr {

enum { FB_OK = 1, FB_FAILED_BACKWARD = 2, FB_FAILED_FORWARD = 3 };
enum { FB_THREADS = 256, FB_LDS_NODES = 2048 };
enum { FB_MODE_BAUM_WELCH = 0, FB_MODE_VITERBI = 1 };

constexpr double FB_ZERO = -1e15;                    // HmmNetBaumWelch::LLType::zero()
constexpr double FB_LOG_TINY = -115.12925464970229;  // log(util::tiny_for_log = 1e-50)

// One network in the batch's blobs: counts and, per array of hmmnet.h, its first element.
struct FbNetDev {
  int32_t n_nodes, n_em, n_ep, n_bl, n_fl, n_pdf, n_tr, initial, final_node;
  // into the int32 blob (the handle refuses blobs of 2^31 elements)
  int32_t em_begin, em_src, em_tgt, em_pdf, em_slot, em_trslot, in_begin, in_arcs, pdf_begin, pdf_arcs, tr_begin,
      tr_arcs, eo_begin, ep_src, ep_tgt, ei_begin, ei_arcs, bl_begin, bl_nodes, fl_begin, fl_nodes;
  // into the double blob
  int32_t em_logp, em_static, ep_score;
};

struct FbUttDev {
  FbNetDev net;
  int64_t row0;      // score row of the utterance's first frame
  int32_t T;         // frames
  int64_t beta;      // (T + 1) x n_nodes doubles in the work buffer
  int64_t best;      // T doubles
  int64_t arcs;      // 2 x n_em doubles
  int64_t nodes;     // 2 x n_nodes doubles (the global form's node vectors)
  int64_t occ;       // T x n_pdf doubles in the occupancy buffer (want_pdf_occ)
  int64_t trocc;     // n_tr doubles in the transition occupancy buffer (want_tr_occ)
  int64_t path;      // T int32 in the path buffer (want_path)
};

struct FbResult {
  double backward_total, forward_total;
  int32_t status;
  int32_t attempts;  // launches that ran this utterance
};

struct FbParams {
  const int32_t *ints;
  const double *doubles;
  const FbUttDev *utt;
  const int32_t *list;   // the utterances of this launch
  const void *scores;    // state log-likelihood rows (float, or double when f64)
  int64_t pitch;
  int32_t f64, mode, want_pdf_occ, want_tr_occ;
  double fw_beam, bw_beam, ac_scale;
  double *work, *occ, *trocc;
  FbResult *result;
  int32_t *path;         // nullptr, or Viterbi mode's emitting arc of every frame (want_path)
};

void hmmnet_fb_launch(const FbParams &p, int32_t n_list, bool lds_form, hipStream_t stream);

}  // namespace aasr

// gmm_score_lna.cc -- scoring and the LNA pass of a batch as one call: frame chunks scored one after another on the caller's
// stream, the LNA pass of chunk c on a side stream beside the scoring of chunk c + 1.
//
// The two stages want complementary resources: the scoring kernel is bound by the matrix pipe and leaves HBM at an eighth
// of its rate, the LNA pass is bound by vector issue and HBM and leaves the matrix pipe idle.  They fit on a CU together:
// a scoring workgroup puts two waves of 208 allocated VGPRs on every SIMD, the unmapped LNA instance
// (k_state_norm_lna_reg<VPT, false>) needs at most 96, and 64 B of LDS beside the scoring kernel's 131 264
// (tests/test_lna_unmapped_notes.py holds the three figures).
//
// Order on the device:   stream:  [operand of all frames] score(0) E0 score(1) E1 ... score(n-1) E(n-1) wait(D)
//                        side:    wait(E0) lna(0) wait(E1) lna(1) ... lna(n-1) D
// so a caller that knows only `stream` sees scores and bytes in stream order, as after the two separate calls.  Scores do
// not depend on where the frames are cut (every plan and both wave forms of the scoring kernel give identical bits), and a
// chunk's LNA pass writes the bytes of its own frames only: the result is that of the plain sequence, bit for bit.
//
// Whether the two kernels really share the CUs is decided by which of them arrives first, and nothing here can order
// that (measured).  When E(c) fires, score(c + 1) is the next packet of the caller's queue and lna(c) the next
// of the side queue.  An LNA grid that gets ahead -- 20 us are enough -- takes every wave slot; a scoring workgroup needs
// 416 of a SIMD's 512 VGPRs free at once, and the dispatcher refills each slot an LNA workgroup leaves with the next
// one, so the scoring kernel starts when the LNA grid is exhausted: the kernels run one after the other, which costs
// nothing against the plain sequence and gains nothing.  With the scoring kernel ahead, one LNA workgroup per CU runs
// beside it.  On the runtime this was measured on, the wait across queues resolves about 8 us later than the one inside a
// queue, so the scoring kernel is ahead PROVIDED no other kernel lies between score(c) and score(c + 1).  That is why the
// frame operand of all chunks is formed by one launch in front (gmm_form_frame_operand) where the scoring kernel reads
// one: a per-chunk k_frame_operand launch between two scoring kernels is exactly the 20 us the LNA grid needs.  It is an
// observed latency difference, not a guarantee: another runtime may resolve the race the other way and get the serial
// form.
#include <algorithm>
#include <memory>

#include "gmm.h"

namespace aasr {

namespace {

constexpr int kEvents = 8;   // scored-events, used round robin (a re-recorded event leaves earlier waits on it untouched)

struct SideStream {
  hipStream_t side = nullptr;
  hipEvent_t scored[kEvents] = {};
  hipEvent_t lna_done = nullptr;
  ~SideStream() {
    if (side) (void)hipStreamSynchronize(side);
    for (hipEvent_t e : scored)
      if (e) (void)hipEventDestroy(e);
    if (lna_done) (void)hipEventDestroy(lna_done);
    if (side) (void)hipStreamDestroy(side);
  }
};

SideStream *side_of(aasr_gmm *g) {
  if (!g->score_lna_side) {
    auto s = std::make_shared<SideStream>();
    AASR_HIP(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
    for (hipEvent_t &e : s->scored) AASR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    AASR_HIP(hipEventCreateWithFlags(&s->lna_done, hipEventDisableTiming));
    g->score_lna_side = s;
  }
  return static_cast<SideStream *>(g->score_lna_side.get());
}

// However the chunk loop is left -- a launch that raises included -- the operand formed ahead is dropped and the caller's
// stream waits for what has been queued on the side stream.
struct Join {
  const aasr_gmm *g;
  SideStream *ss;
  hipStream_t stream;
  ~Join() {
    gmm_drop_frame_operand(g);
    if (hipEventRecord(ss->lna_done, ss->side) == hipSuccess) (void)hipStreamWaitEvent(stream, ss->lna_done, 0);
  }
};

}  // namespace

// frames per chunk of the two-stream form, 0: the plain sequence
int64_t gmm_score_lna_chunk(const aasr_gmm *g, int64_t F, int64_t pitch, int64_t chunk_frames) {
  if (chunk_frames < 0 || chunk_frames % 512 != 0)
    raise(AASR_ERR_INVALID, "chunk_frames must be 0 or a positive multiple of 512, got %ld", (long)chunk_frames);
  if (!gmm_score_single_track_launch(g, pitch)) return 0;
  if (chunk_frames > 0) return F > chunk_frames ? chunk_frames : 0;
  // automatic: a chunk is a frame block of 512 per CU -- one whole round of the coarse part of the scoring kernel's cut
  // plan (pick_cut_plan) as it stands for the headline; every chunk's own launch picks its plan afresh, so a plan that
  // changes costs time, never bits.  The rest is the last chunk with the fine cuts it gets on its own.  Fewer than two
  // whole rounds: nothing to run the first chunk's LNA pass under
  const int64_t round = (int64_t)(g->num_cus > 0 ? g->num_cus : 256) * 512;
  return F >= 2 * round ? round : 0;
}

void gmm_score_lna_chunked(aasr_gmm *g, const float *d_frames, int64_t F, float *d_scores, int64_t pitch, int normalize,
                           int lnabytes, uint8_t *d_bytes, int64_t chunk_frames, hipStream_t stream) {
  const int64_t chunk = gmm_score_lna_chunk(g, F, pitch, chunk_frames);
  if (F <= 0) return;
  const int S = (int)g->S;
  if (chunk == 0) {
    gmm_score_launch_pitched(g, d_frames, F, d_scores, pitch, stream);
    lna_encode_launch(d_scores, F, S, normalize, lnabytes, nullptr, d_bytes, stream, pitch);
    return;
  }
  SideStream *ss = side_of(g);
  Join join{g, ss, stream};
  // kernels that read a frame operand: formed once, so that nothing lies between two scoring kernels (above); the others
  // (f32 rows, the wave-group kernel) launch one kernel per chunk as it is
  gmm_form_frame_operand(g, d_frames, F, stream);
  // whole chunks first; a remainder joins no chunk (it keeps the cuts -- and below 8192 frames the 4-wave form -- it has alone)
  int c = 0;
  for (int64_t f0 = 0; f0 < F; f0 += chunk, c++) {
    const int64_t n = std::min(chunk, F - f0);
    gmm_score_launch_pitched(g, d_frames + f0 * g->dim, n, d_scores + f0 * pitch, pitch, stream);
    hipEvent_t e = ss->scored[c % kEvents];
    AASR_HIP(hipEventRecord(e, stream));
    AASR_HIP(hipStreamWaitEvent(ss->side, e, 0));
    // the default grid: short workgroups, as many as fit beside the scoring kernel while it runs (one per CU) and the whole
    // chip when it does not (the last chunk's pass).  A grid held to one long-lived workgroup per CU was measured 25 %
    // slower for the step
    lna_encode_launch(d_scores + f0 * pitch, n, S, normalize, lnabytes, nullptr, d_bytes + (size_t)f0 * S * lnabytes,
                      ss->side, pitch);
  }
}

}  // namespace aasr

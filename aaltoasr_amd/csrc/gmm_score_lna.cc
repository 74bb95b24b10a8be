// gmm_score_lna.cc -- scoring and the LNA pass of a batch as one call: frame ranges scored one after another on the
// caller's stream, LNA segments on a side stream beside the scoring launches that follow the ones they wait for.
//
// The two stages want complementary resources: the scoring kernel is bound by the matrix pipe and leaves HBM at an eighth
// of its rate, the LNA pass is bound by vector issue and HBM and leaves the matrix pipe idle.  They fit on a CU together:
// a scoring workgroup puts two waves of 208 allocated VGPRs on every SIMD, and what an LNA segment runs has to fit into the
// 96 and the 32 576 B of LDS that leaves: the multi-frame kernel of the headline's state range (k_state_norm_lna_multi<13,
// 4>: four frame rows per workgroup pass, 94 VGPRs, 13 856 B -- three barriers and one logarithm per wave for four frames
// where the one-frame kernel pays four barriers and a logarithm in every wave per frame) and, for every other S, the
// unmapped one-frame instance (k_state_norm_lna_reg<VPT, false>: at most 96, 64 B).  tests/test_lna_multi_notes.py and
// tests/test_lna_unmapped_notes.py hold the figures; lna_encode_launch_grid chooses, and the bytes do not depend on it.
//
// The schedule is data: plan_score_lna() -- a pure host function -- returns the scoring launches in time order and the LNA
// segments with the launch each waits for; gmm_score_lna_chunked() issues it.  With W whole chunks and a remainder:
//
//   stream:  [operand of all frames] score(rem) E0 score(chunk 0) E1 ... score(chunk W-1) E(W) wait(D)
//   side:    wait(E0) lna(rem) wait(E1) lna(<= share of a chunk) ... wait(E(W)) lna(all that is left) D
//
// so a caller that knows only `stream` sees scores and bytes in stream order, as after the two separate calls.
//   - The remainder -- the frames past the last whole chunk, which pick_cut_plan gives the fine cuts -- is scored FIRST
//     and alone: its many short workgroups end in several rounds, and every round boundary on every CU is an opening for
//     pending LNA workgroups.  Its LNA segment runs beside the first whole chunk, under which nothing could hide before.
//   - Behind every launch but the last at most `share` of a chunk's frames is released, oldest first, and what
//     accumulates is encoded behind the last launch, at full rate on an empty chip.  Beside a scoring kernel an LNA
//     segment runs at 0.88 of the launch's frame rate with the four-frame kernel (0.84 with the one-frame kernel); at a
//     share of 1 workgroups are still pending when the scoring launch ends, take every CU, and the next scoring launch's
//     workgroups are placed one by one as that flood drains.  Measured with the four-frame kernel, holding frames back
//     removes the flood (share 0.9: no LNA kernel runs at the start of a scoring launch; 0.7 with the one-frame kernel),
//     leaves the scoring launches as long as they were, and loses 0.03 ms per step to the longer last pass: the
//     compiled-in share is 1.
//   - The automatic chunk is half a 512-frame block per CU: at the plan's two cuts per block still one whole round of
//     workgroups, with half the window in front under which nothing hides and half the last pass behind.
// Order in time is not frame order; the ranges are disjoint.  Scores do not depend on where the frames are cut (every
// plan and both wave forms of the scoring kernel give identical bits), and an LNA segment writes the bytes of its own
// frames only, whichever workgroup encodes them: the result is that of the plain sequence, bit for bit.
//
// Whether the two kernels really share the CUs is decided by which of them arrives first, and nothing here can order
// that (measured).  When E(c) fires, the next scoring launch is the next packet of the caller's queue and the
// LNA segment the next of the side queue.  An LNA grid that gets ahead -- 20 us are enough -- takes every wave slot; a
// scoring workgroup needs 416 of a SIMD's 512 VGPRs free at once, and the dispatcher refills each slot an LNA workgroup
// leaves with the next one, so the scoring kernel starts when the LNA grid is exhausted: the kernels run one after the
// other, which costs nothing against the plain sequence and gains nothing.  With the scoring kernel ahead, one LNA
// workgroup per CU runs beside it.  On the runtime this was measured on, the wait across queues resolves about 8 us later
// than the one inside a queue, so the scoring kernel is ahead PROVIDED no other kernel lies between two scoring kernels.
// That is why the frame operand of all ranges is formed by one launch in front (gmm_form_frame_operand) where the scoring
// kernel reads one, and why every scoring range begins on a multiple of 512 frames (the operand formed ahead serves only
// such ranges): a per-range k_frame_operand launch between two scoring kernels is exactly the 20 us the LNA grid needs.
// It is an observed latency difference, not a guarantee: another runtime may resolve the race the other way and get the
// serial form.
#include <algorithm>
#include <atomic>
#include <deque>
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

// However the plan's loop is left -- a launch that raises included -- the operand formed ahead is dropped and the caller's
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

// aasr_debug_score_lna_knobs: what the tests set in place of the defaults (a negative field: the default)
std::atomic<int> g_dbg_remainder_first{-1}, g_dbg_share_pct{-1}, g_dbg_chunk_div{-1}, g_dbg_lna_grid{-1};

}  // namespace

// The compiled-in schedule; in the ablation build every rule has its experiment switch, so that it can be timed alone
ScoreLnaKnobs score_lna_default_knobs() {
  static const int rem_env = AASR_EXPERIMENT_ENV("AASR_LNA_REM_FIRST") ? atoi(AASR_EXPERIMENT_ENV("AASR_LNA_REM_FIRST")) : -1;
  static const double share_env = AASR_EXPERIMENT_ENV("AASR_LNA_SHARE") ? atof(AASR_EXPERIMENT_ENV("AASR_LNA_SHARE")) : -1.0;
  static const int div_env = AASR_EXPERIMENT_ENV("AASR_LNA_CHUNK_DIV") ? atoi(AASR_EXPERIMENT_ENV("AASR_LNA_CHUNK_DIV")) : -1;
  static const int grid_env = AASR_EXPERIMENT_ENV("AASR_LNA_GRID") ? atoi(AASR_EXPERIMENT_ENV("AASR_LNA_GRID")) : -1;
  ScoreLnaKnobs k;
  if (rem_env >= 0) k.remainder_first = rem_env != 0;
  if (share_env > 0) k.share = share_env;
  if (div_env >= 1) k.chunk_div = div_env;
  if (grid_env >= 1) k.lna_grid = grid_env;
  if (g_dbg_remainder_first.load() >= 0) k.remainder_first = g_dbg_remainder_first.load() != 0;
  if (g_dbg_share_pct.load() >= 0) k.share = g_dbg_share_pct.load() / 100.0;
  if (g_dbg_chunk_div.load() >= 1) k.chunk_div = g_dbg_chunk_div.load();
  if (g_dbg_lna_grid.load() >= 1) k.lna_grid = g_dbg_lna_grid.load();
  return k;
}

// frames per chunk of the two-stream form, 0: the plain sequence.  No device, no handle
int64_t score_lna_chunk_frames(int64_t F, int cus, int64_t chunk_frames, const ScoreLnaKnobs &k) {
  if (chunk_frames < 0 || chunk_frames % 512 != 0)
    raise(AASR_ERR_INVALID, "chunk_frames must be 0 or a positive multiple of 512, got %ld", (long)chunk_frames);
  if (k.chunk_div < 1 || k.chunk_div > 64 || !(k.share > 0.0) || k.share > 1.0 || k.lna_grid < 1 || k.lna_grid > 1024)
    raise(AASR_ERR_INVALID, "score + LNA schedule: share %g, chunk divisor %d, LNA grid %d", k.share, k.chunk_div, k.lna_grid);
  if (chunk_frames > 0) return F > chunk_frames ? chunk_frames : 0;
  // automatic: a round is a frame block of 512 per CU -- one whole round of the coarse part of the scoring kernel's cut
  // plan (pick_cut_plan) as it stands for the headline at two cuts per block; a chunk is a round over chunk_div (whole
  // 512s), which at chunk_div = 2 is still one whole round of workgroups.  Every launch picks its plan afresh, so a plan
  // that changes costs time, never bits.  Fewer than two whole rounds: the plain sequence, as ever
  const int64_t round = (int64_t)(cus > 0 ? cus : 256) * 512;
  if (F < 2 * round) return 0;
  return std::max<int64_t>(512, round / k.chunk_div / 512 * 512);
}

ScoreLnaPlan plan_score_lna(int64_t F, int cus, int64_t chunk_frames, const ScoreLnaKnobs &k) {
  ScoreLnaPlan p;
  p.chunk = score_lna_chunk_frames(F, cus, chunk_frames, k);
  if (F <= 0) return p;
  if (p.chunk == 0) {
    p.score.push_back({0, F});
    p.lna.push_back({0, F, 0});
    return p;
  }
  const int64_t chunk = p.chunk, whole = F / chunk, rem = F - whole * chunk;
  // the remainder keeps the cuts -- and below 8192 frames the 4-wave form -- it has alone; it joins no chunk
  if (rem > 0 && k.remainder_first) p.score.push_back({whole * chunk, rem});
  for (int64_t c = 0; c < whole; c++) p.score.push_back({c * chunk, chunk});
  if (rem > 0 && !k.remainder_first) p.score.push_back({whole * chunk, rem});
  // scored and not yet encoded, oldest first; neighbours in frame order are one range
  std::deque<ScoreLnaRange> pool;
  const int64_t budget = std::max<int64_t>(1, (int64_t)(k.share * (double)chunk));
  const int n = (int)p.score.size();
  for (int i = 0; i < n; i++) {
    const ScoreLnaRange &s = p.score[i];
    if (!pool.empty() && pool.back().f0 + pool.back().n == s.f0) pool.back().n += s.n;
    else pool.push_back(s);
    int64_t left = i + 1 < n ? budget : F;
    while (left > 0 && !pool.empty()) {
      ScoreLnaRange &r = pool.front();
      const int64_t take = std::min(left, r.n);
      p.lna.push_back({r.f0, take, i});
      left -= take;
      r.f0 += take;
      r.n -= take;
      if (r.n == 0) pool.pop_front();
    }
  }
  return p;
}

int64_t gmm_score_lna_chunk(const aasr_gmm *g, int64_t F, int64_t pitch, int64_t chunk_frames) {
  const int64_t chunk = score_lna_chunk_frames(F, g->num_cus, chunk_frames, score_lna_default_knobs());
  return gmm_score_single_track_launch(g, pitch) ? chunk : 0;
}

void gmm_score_lna_chunked(aasr_gmm *g, const float *d_frames, int64_t F, float *d_scores, int64_t pitch, int normalize,
                           int lnabytes, uint8_t *d_bytes, int64_t chunk_frames, hipStream_t stream) {
  const ScoreLnaKnobs knobs = score_lna_default_knobs();
  const int64_t chunk = gmm_score_lna_chunk(g, F, pitch, chunk_frames);
  if (F <= 0) return;
  const int S = (int)g->S;
  if (chunk == 0) {
    gmm_score_launch_pitched(g, d_frames, F, d_scores, pitch, stream);
    lna_encode_launch(d_scores, F, S, normalize, lnabytes, nullptr, d_bytes, stream, pitch);
    return;
  }
  const ScoreLnaPlan plan = plan_score_lna(F, g->num_cus, chunk, knobs);   // (the chunk as an explicit one: no second choice)
  SideStream *ss = side_of(g);
  Join join{g, ss, stream};
  // kernels that read a frame operand: formed once, so that nothing lies between two scoring kernels (above); the others
  // (f32 rows, the wave-group kernel) launch one kernel per range as it is
  gmm_form_frame_operand(g, d_frames, F, stream);
  size_t next = 0;
  for (size_t i = 0; i < plan.score.size(); i++) {
    const ScoreLnaRange &s = plan.score[i];
    gmm_score_launch_pitched(g, d_frames + s.f0 * g->dim, s.n, d_scores + s.f0 * pitch, pitch, stream);
    // the side stream's wait is queued before the event is recorded again, kEvents launches on
    hipEvent_t e = ss->scored[i % kEvents];
    AASR_HIP(hipEventRecord(e, stream));
    AASR_HIP(hipStreamWaitEvent(ss->side, e, 0));
    // short workgroups, as many as fit beside the scoring kernel while it runs (one per CU) and the whole chip when it
    // does not (the last pass).  A grid held to one long-lived workgroup per CU was measured 25 % slower for the step
    // 
    for (; next < plan.lna.size() && plan.lna[next].wait == (int)i; next++) {
      const ScoreLnaSegment &l = plan.lna[next];
      lna_encode_launch_grid(d_scores + l.f0 * pitch, l.n, S, normalize, lnabytes, nullptr,
                             d_bytes + (size_t)l.f0 * S * lnabytes, ss->side, pitch, nullptr, knobs.lna_grid);
    }
  }
}

}  // namespace aasr

// Diagnostic (tests): the plan of a call, without a handle or a device.  score: (first frame, frames) per scoring launch
// in time order; lna: (first frame, frames, index of the scoring launch waited for) per LNA segment in side-stream order;
// at most `cap` of either are written, the counts are the plan's.  chunk_frames as the public call's (0: automatic, from
// `cus`); remainder_first / share / chunk_div < 0: the compiled-in value.  Returns the frames per chunk (0: the plain
// sequence), -1 for arguments the public call refuses.
extern "C" int64_t aasr_debug_score_lna_plan(int64_t F, int cus, int64_t chunk_frames, int remainder_first, double share,
                                             int chunk_div, int64_t *score, int64_t *lna, int64_t cap, int64_t *n_score,
                                             int64_t *n_lna) {
  int64_t chunk = -1;
  (void)aasr::guarded([&] {
    aasr::ScoreLnaKnobs k = aasr::score_lna_default_knobs();
    if (remainder_first >= 0) k.remainder_first = remainder_first != 0;
    if (share >= 0) k.share = share;
    if (chunk_div >= 0) k.chunk_div = chunk_div;
    const aasr::ScoreLnaPlan p = aasr::plan_score_lna(F, cus, chunk_frames, k);
    for (int64_t i = 0; i < (int64_t)p.score.size() && i < cap && score; i++) {
      score[2 * i] = p.score[i].f0;
      score[2 * i + 1] = p.score[i].n;
    }
    for (int64_t i = 0; i < (int64_t)p.lna.size() && i < cap && lna; i++) {
      lna[3 * i] = p.lna[i].f0;
      lna[3 * i + 1] = p.lna[i].n;
      lna[3 * i + 2] = p.lna[i].wait;
    }
    if (n_score) *n_score = (int64_t)p.score.size();
    if (n_lna) *n_lna = (int64_t)p.lna.size();
    chunk = p.chunk;
  });
  return chunk;
}

// Diagnostic (tests): the schedule of later aasr_gmm_score_lna_pitched_dev calls of this process in place of the
// compiled-in one; a negative argument restores that rule's default.  share in percent; lna_grid in workgroups per CU.
extern "C" void aasr_debug_score_lna_knobs(int remainder_first, int share_percent, int chunk_div, int lna_grid) {
  aasr::g_dbg_remainder_first.store(remainder_first < 0 ? -1 : remainder_first);
  aasr::g_dbg_share_pct.store(share_percent < 1 || share_percent > 100 ? -1 : share_percent);
  aasr::g_dbg_chunk_div.store(chunk_div < 1 || chunk_div > 64 ? -1 : chunk_div);
  aasr::g_dbg_lna_grid.store(lna_grid < 1 || lna_grid > 1024 ? -1 : lna_grid);
}

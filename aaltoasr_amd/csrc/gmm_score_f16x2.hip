// gmm_score_f16x2.hip -- AASR_PREC_F16X2 (the default; what bench.py times): the two-term instances of
// k_gmm_diag_score_pl and k_frame_operand<2> (gmm_score_pl.h; the map of the files: gmm_score.hip), and the phase trace
// of experiment builds, which is of the bench instance.
#include "gmm_score_common.h"

#ifdef AASR_PL_TRACE
#define AASR_PL_TRACE_UNIT 1   // this unit's instances of k_gmm_diag_score_pl carry the trace (gmm_score_pl.h)
namespace aasr {
__device__ unsigned long long g_pl_trace[8][12];
}  // namespace aasr
#endif

#include "gmm_score_pl.h"

namespace aasr {

template bool launch_split<2>(const aasr_gmm *, const TrackLayout &, const float *, int64_t, float *, hipStream_t,
                              const ClusterArgs *, int64_t);
template void form_frame_operand<2>(const aasr_gmm *, const TrackLayout &, const float *, int64_t, hipStream_t);

// Diagnostic (bench.py): milliseconds of ONE k_frame_operand launch over F frames for the layout and arithmetic a scoring
// call would use now -- the launch that precedes k_gmm_diag_score_pl in every scoring call, so that the bench can price
// the scoring kernel on its own duration (HIP events around the call see both).  < 0: the current path forms its frame
// operand inside the kernel.
extern "C" double aasr_debug_frame_operand_ms(aasr_gmm *g, const float *d_frames, int64_t F, int reps, void *stream_v) {
  if (!g || F <= 0 || reps <= 0) return -1.0;
  hipStream_t stream = (hipStream_t)stream_v;
  const TrackLayout &L = g->paired.ok ? g->paired : g->tracks;
  if (!L.ok || !g->use_bf16x3 || g->precision != AASR_PREC_F16X2 || !L.a16h.p || g->cl.enabled) return -1.0;
  const int NW = F >= 8192 ? 8 : 4;
  const int64_t blocks64 = (F + NW * FRAMES_PER_WAVE - 1) / (NW * FRAMES_PER_WAVE) * NW;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
  int64_t stride = 0;
  frame_operand<2>(g, L, d_frames, F, blocks64, stream, &stride);
  (void)hipEventRecord(e0, stream);
  for (int i = 0; i < reps; i++) frame_operand<2>(g, L, d_frames, F, blocks64, stream, &stride);
  (void)hipEventRecord(e1, stream);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return (double)ms / reps;
}

// Diagnostic (tests/test_lna_unmapped_notes.py): dynamic LDS bytes of a workgroup of the bench form -- 39 dimensions
// (five slabs), grouped tracks, two terms -- in its 8-wave (wide) or 4-wave shape; the code object's notes hold only the
// static part
extern "C" int aasr_debug_pl_bench_smem_bytes(int wide) {
  return wide ? PlSmem<5, true, true, 2>::kBytes : PlSmem<5, true, false, 2>::kBytes;
}
}  // namespace aasr

#ifdef AASR_PL_TRACE
// Diagnostic of experiment builds (tools/pl_trace.py): the phase sums of the last traced launch, [wave][interval]
extern "C" int aasr_debug_pl_trace(unsigned long long *out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(aasr::g_pl_trace), sizeof(unsigned long long) * 96) == hipSuccess ? 0 : -1;
}
#endif

// gmm_score_exact.hip -- the forms without the matrix pipe (the map of the files: gmm_score.hip):
//   k_gmm_diag_score_centred, k_outlier_merge    beyond every expanded form's limits; outlier routing (score_outliers,
//                                                hyb_fuse_begin)
//   k_gmm_diag_score_f64[_classes]               AASR_PREC_F64: the reference's arithmetic in double
#include "gmm_score_common.h"

namespace aasr {

// ---------------------------------------------------------------------------
// Centred-form kernel: the numerically safe path.
//
// The expanded (GEMM) form cancels when |mu - pivot| / sigma is large; models
// whose conditioning estimate kappa = max_g sum_d p_gd (mu_gd - v_d)^2 would push
// the f32 error past the 1e-4 budget are scored with the reference's own
// arithmetic shape instead: t = x - mu, acc += (p') t^2 per dimension (all terms
// of one sign, no cancellation), online (max, sum) over a state's components.
// One lane owns one frame (its x vector lives in VGPRs), the Gaussian
// parameters are wave-uniform and arrive through the scalar cache (s_load), so
// the inner loop is 3 VALU instructions per dimension.  The f32 MFMA runs on
// the same lanes as the VALU anyway, so this costs ~1.5x the matrix path, not
// 16x.  Also the fallback for any model the track layouts cannot hold.
// ---------------------------------------------------------------------------
// CL (Gaussian clustering, gmm_cluster.hip): record r belongs to cluster crow[r]; its value counts
// for a frame only where the frame's bit of maskw[word][cluster] is set (the cluster is evaluated
// exactly there), and the result carries no 1e-50 floor (k_cluster_merge applies it).
template <int DIMP, bool CL>
__global__ __launch_bounds__(256) void k_gmm_diag_score_centred(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ recs,
    const int32_t *__restrict__ state_off, const int32_t *__restrict__ split_state,
    float *__restrict__ out, int64_t frame_stride, int64_t state_stride,
    const int32_t *__restrict__ crow, const unsigned long long *__restrict__ maskw, int c1, int64_t n_words,
    float floor_val, int tile_out) {
  // A record = DIMP / 4 groups of 16 floats, group q = [mu x 4][mu_lo x 4][p' x 4][C, pad x 3] of dimensions 4 q .. 4 q + 3
  // (the constant in group 0): the mean as a float pair, mu = mu_hi + mu_lo to 2^-48 -- a mean rounded to one float
  // costs p t ulp(mu)/2, 1e-4 at 14 sigma from a sigma = 0.01 Gaussian.  A group is ONE scalar load of 64 bytes and the
  // groups of consecutive records follow each other in memory, so the kernel walks one stream and fetches a group ahead
  // of the one it computes on (round 6: with [mu][p'][C][mu_lo] a dimension needed three loads from three places, none
  // could be issued early within the scalar registers, and the waves stood at s_waitcnt: 36 % of the vector rate).
  constexpr int NG = DIMP / 4;
  constexpr int REC = 16 * NG;
  typedef float f32x16u __attribute__((ext_vector_type(16), aligned(64)));
  // LDS: first the staging area of the prologue (128 frames x (dim | 1) floats), then -- tile_out -- the results of 16
  // consecutive states for the workgroup's 512 frames ([512][17]), written out as runs of 16 floats per frame row
  extern __shared__ float cen_smem[];
  // each lane owns TWO frames (f, f + 256): one scalar fetch of a Gaussian's
  // parameters feeds 128 frame x Gaussian pairs per wave
  const int tid = threadIdx.x;
  const int64_t f_base = (int64_t)blockIdx.x * 512;
  const int64_t fa = f_base + tid;
  const int64_t fb = fa + 256;
  // The two frames of a lane travel as one <2 x float>: t = x - mu, t*t, fma with p' are
  // v_pk_add / v_pk_mul / v_pk_fma_f32 (two frames per instruction, the scalar operand
  // broadcast) -- 1.5 VALU instructions per frame and dimension instead of 3, same roundings.
  f32x2 x2[DIMP];
  // Prologue: the workgroup's frames are one contiguous run of the frame matrix; it is copied through LDS in four quarters
  // (coalesced loads; a lane then reads its own row, rows an odd number of floats apart: no bank conflicts).  Lanes
  // beyond F take zeros (never stored).
  {
    const int dimo = dim | 1;
#pragma unroll
    for (int qt = 0; qt < 4; qt++) {
      const int64_t f0 = f_base + qt * 128;
      const int nfr = (int)max((int64_t)0, min((int64_t)128, F - f0));
      const int n = nfr * dim;
      const float *src = frames + f0 * dim;
      __syncthreads();
      for (int i = tid; i < n; i += 256) {
        const int fr = i / dim;
        cen_smem[fr * dimo + (i - fr * dim)] = src[i];
      }
      __syncthreads();
      const int row = (tid & 127) < nfr ? (tid & 127) : 0;
      const bool mine = (tid >> 7) == (qt & 1);   // frames f_base + tid (quarters 0, 1) and f_base + 256 + tid (2, 3)
      if (mine) {
        if (qt < 2) {
#pragma unroll
          for (int d = 0; d < DIMP; d++) x2[d].x = (d < dim && nfr > 0) ? cen_smem[row * dimo + d] : 0.0f;
        } else {
#pragma unroll
          for (int d = 0; d < DIMP; d++) x2[d].y = (d < dim && nfr > 0) ? cen_smem[row * dimo + d] : 0.0f;
        }
      }
    }
    __syncthreads();
  }
  const int s_begin = split_state[blockIdx.y], s_end = split_state[blockIdx.y + 1];
  // the 64-frame words of this wave's two frame groups (wave-uniform)
  const int64_t word_a = min((int64_t)blockIdx.x * 8 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_words - 1);
  const int64_t word_b = min(word_a + 4, n_words - 1);
  const int lane_bit = threadIdx.x & 63;
  // the stream of groups: from the first record of the state range on, RING - 1 groups ahead (RING divides the groups of a
  // record, so a group's ring slot is a compile-time constant: no copies between the scalar registers; 12 of them per
  // slot).  One group ahead left the waves waiting on records that come from L2 (whole-model runs: 32 MB of records,
  // 349 -> 296 ms per 10^6 frames x 50 k rows); four ahead covers it.
  constexpr int RING = NG % 5 == 0 ? 5 : NG % 4 == 0 ? 4 : NG % 3 == 0 ? 3 : 2;
  const f32x16u *gp = (const f32x16u *)(recs + (size_t)state_off[s_begin] * REC);
  f32x16u ring[RING];
#pragma unroll
  for (int i = 0; i < RING - 1; i++) ring[i] = gp[i];   // (short ranges: the spare records behind the last one)
  gp += RING - 1;
  for (int s = s_begin; s < s_end; s++) {
    const int r0 = state_off[s], r1 = state_off[s + 1];
    float ma = NEG_BIG_F, sa = 0.0f, mb = NEG_BIG_F, sb = 0.0f;
    for (int r = r0; r < r1; r++) {
      bool on_a = true, on_b = true;
      if (CL) {
        const int c = crow[r];
        on_a = (maskw[word_a * c1 + c] >> lane_bit) & 1ull;
        on_b = (maskw[word_b * c1 + c] >> lane_bit) & 1ull;
      }
      f32x2 acc0 = {0.0f, 0.0f}, acc1 = {0.0f, 0.0f};  // two chains per frame
      float c = 0.0f;
#pragma unroll
      for (int q = 0; q < NG; q++) {
        ring[(q + RING - 1) % RING] = *gp;   // (the spare records behind the last one keep this inside the buffer)
        gp++;
        const f32x16u cur = ring[q % RING];
        if (q == 0) c = cur[12];
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
          const float mu0 = cur[j], mu1 = cur[j + 1];
          const float ml0 = cur[4 + j], ml1 = cur[4 + j + 1];
          const float p0 = cur[8 + j], p1 = cur[8 + j + 1];
          const f32x2 t0 = (x2[4 * q + j] - (f32x2){mu0, mu0}) - (f32x2){ml0, ml0};
          const f32x2 t1 = (x2[4 * q + j + 1] - (f32x2){mu1, mu1}) - (f32x2){ml1, ml1};
          acc0 = __builtin_elementwise_fma(t0 * t0, (f32x2){p0, p0}, acc0);
          acc1 = __builtin_elementwise_fma(t1 * t1, (f32x2){p1, p1}, acc1);
        }
      }
      const float a0 = acc0.x, b0 = acc0.y, a1 = acc1.x, b1 = acc1.y;
      float la = c + (a0 + a1), lb = c + (b0 + b1);  // log2 units
      if (CL) {
        la = on_a ? la : NEG_BIG_F;
        lb = on_b ? lb : NEG_BIG_F;
      }
      const float na = fmaxf(ma, la), nb = fmaxf(mb, lb);
      sa = sa * __builtin_amdgcn_exp2f(ma - na) + __builtin_amdgcn_exp2f(la - na);
      sb = sb * __builtin_amdgcn_exp2f(mb - nb) + __builtin_amdgcn_exp2f(lb - nb);
      ma = na;
      mb = nb;
    }
    float lla = fmaf(ma, LN2_F, __builtin_amdgcn_logf(sa) * LN2_F);
    float llb = fmaf(mb, LN2_F, __builtin_amdgcn_logf(sb) * LN2_F);
    lla = fmaxf(lla, floor_val);
    llb = fmaxf(llb, floor_val);
    if (r1 <= r0) lla = llb = floor_val;
    if (!tile_out) {
      if (fa < F) out[fa * frame_stride + s * state_stride] = lla;
      if (fb < F) out[fb * frame_stride + s * state_stride] = llb;
      continue;
    }
    // frame-major output (state_stride == 1): a lane's values of 16 consecutive states are collected in LDS and leave as
    // runs of 16 floats per frame row -- whole 64-byte half lines where the caller's pitch is a multiple of 16 floats
    const int col = (s - s_begin) & 15;
    cen_smem[tid * 17 + col] = lla;
    cen_smem[(tid + 256) * 17 + col] = llb;
    if (col == 15 || s == s_end - 1) {
      __syncthreads();
      const int c = tid & 15;
      const int64_t s0 = s - col;
      if (c <= col) {
#pragma unroll 4
        for (int r = tid >> 4; r < 512; r += 16) {
          const int64_t f = f_base + r;
          if (f < F) out[f * frame_stride + s0 + c] = cen_smem[r * 17 + c];
        }
      }
      __syncthreads();
    }
  }
}

// scratch budget of the routed passes (outlier / class partial scores); tests shrink it to force
// many passes
double g_score_pass_bytes = 1.0e9;
extern "C" void aasr_debug_set_pass_bytes(double bytes) { g_score_pass_bytes = bytes > 0 ? bytes : 1.0e9; }

template <int DIMP>
static void launch_centred_t(const aasr_gmm *g, const CentredOps &ops, const float *d_frames, int64_t F,
                             float *d_out, hipStream_t stream) {
  const int64_t blocks = (F + 511) / 512;
  // frame-major callers (state_stride == 1) get their values as runs of 32 states per frame row through LDS
  const int tile_out = ops.state_stride == 1 ? 1 : 0;
  const int smem = 4 * std::max(128 * (g->dim | 1), tile_out ? 512 * 17 : 0);
  // State-range cuts: a workgroup keeps its 512 frames in registers and walks the records of its state range, so a cut
  // costs every frame block its prologue again (frames through LDS, ~c records' time) -- R minimises
  // rounds x (records / R + c) over the workgroups the chip holds at once (LDS: two per CU with the output tile).
  const double slots = 4.0 * (g->num_cus > 0 ? g->num_cus : 256);
  const double c_fixed = 6.0;
  int R = 1;
  double best = 1e300;
  for (int r = 1; r <= ops.max_splits; r++) {
    const double rounds = std::ceil((double)blocks * r / slots);
    const double cost = rounds * ((double)std::max<int64_t>(1, ops.n_recs) / r + c_fixed);
    if (cost < best * 0.995) {
      best = cost;
      R = r;
    }
  }
  const int32_t *split = ops.splits + (size_t)(R - 1) * (CENTRED_MAX_SPLITS + 1);
  static bool attr_set[64][2] = {{false}};
  if (!attr_set[g->device & 63][ops.maskw ? 1 : 0]) {
    if (ops.maskw)
      AASR_HIP(hipFuncSetAttribute((const void *)k_gmm_diag_score_centred<DIMP, true>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 512 * 17));
    else
      AASR_HIP(hipFuncSetAttribute((const void *)k_gmm_diag_score_centred<DIMP, false>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 512 * 17));
    attr_set[g->device & 63][ops.maskw ? 1 : 0] = true;
  }
  if (ops.maskw)
    hipLaunchKernelGGL((k_gmm_diag_score_centred<DIMP, true>), dim3((unsigned)blocks, (unsigned)R), dim3(256), smem,
                       stream, d_frames, F, g->dim, ops.recs, ops.state_off, split, d_out, ops.frame_stride,
                       ops.state_stride, ops.crow, ops.maskw, ops.c1, ops.n_words, NEG_BIG_F, tile_out);
  else
    hipLaunchKernelGGL((k_gmm_diag_score_centred<DIMP, false>), dim3((unsigned)blocks, (unsigned)R), dim3(256), smem,
                       stream, d_frames, F, g->dim, ops.recs, ops.state_off, split, d_out, ops.frame_stride,
                       ops.state_stride, (const int32_t *)nullptr, (const unsigned long long *)nullptr, 0, (int64_t)1,
                       ops.floor_val, tile_out);
  AASR_HIP(hipGetLastError());
}

bool launch_centred_ops(const aasr_gmm *g, const CentredOps &ops, int dimp, const float *d_frames,
                               int64_t F, float *d_out, hipStream_t stream) {
  switch (dimp) {
#define AASR_CASE(N)                                             \
  case N:                                                        \
    launch_centred_t<N>(g, ops, d_frames, F, d_out, stream);     \
    return true;
    AASR_CASE(8) AASR_CASE(16) AASR_CASE(24) AASR_CASE(32) AASR_CASE(40) AASR_CASE(48) AASR_CASE(64)
#undef AASR_CASE
    default:
      return false;
  }
}

// The floor of a centred launch whose values take log|det| of an in-place global transform afterwards (k_add_bias, the
// outlier merge): 1e-50 / |det|, so that the floor the reference puts on the TRANSFORMED likelihood is the one that holds
// (floored at 1e-50 first, a value in [1e-50 / |det|, 1e-50] came out as 1e-50 |det| -- visible from log|det| ~ 11 on).
static float outlier_part_floor(const aasr_gmm *g) {
  return std::isfinite(g->out_bias_ln) ? LOG_TINY_F - (float)g->out_bias_ln : LOG_TINY_F;   // (|det| = 0: all at the floor)
}

bool launch_centred(const aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                    hipStream_t stream, int64_t pitch) {
  CentredOps ops{g->centred_recs.p, g->centred_state_off.p, g->centred_splits.p, g->centred_max_splits,
                 pitch > 0 ? pitch : g->S, 1};
  ops.n_recs = (int64_t)g->host.mix_idx.size();
  ops.floor_val = outlier_part_floor(g);   // (k_add_bias follows where log|det| != 0 and floors at 1e-50)
  return launch_centred_ops(g, ops, g->centred_dimp, d_frames, F, d_out, stream);
}

// out[f][map[j]] = log(exp(out[f][map[j]]) + exp(part[j][f])): the matrix path's sum over a
// state's well-conditioned components plus the centred sum over its outliers.  `part` is
// state-major ([Sb][pitch]: the centred kernel's lane = frame stores are coalesced that way); a
// workgroup moves a 64 x 64 tile through LDS so that the update of `out` walks along a frame row.
// Both inputs carry the 1e-50 floor, which the result keeps (floors = 1); in a clustered pass neither
// does (floors = 0).
__global__ __launch_bounds__(256) void k_outlier_merge(float *__restrict__ out, int64_t S,
                                                       const float *__restrict__ part, int64_t pitch,
                                                       int64_t Sb, const int32_t *__restrict__ map,
                                                       int64_t F, int floors, float part_bias) {
  __shared__ float tile[64][65];
  const int64_t f0 = (int64_t)blockIdx.x * 64;
  const int64_t j0 = (int64_t)blockIdx.y * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int jj = w; jj < 64; jj += 4) {
    const int64_t j = j0 + jj, f = f0 + lane;
    tile[jj][lane] = (j < Sb && f < F) ? part[j * pitch + f] : LOG_TINY_F;
  }
  __syncthreads();
  const int64_t j = j0 + lane;
  if (j >= Sb) return;
  const int col = map[j];
  for (int ff = w; ff < 64; ff += 4) {
    const int64_t f = f0 + ff;
    if (f >= F) break;
    float *o = out + f * S + col;
    // part_bias: log|det| of an in-place global transform -- the matrix path carries it at its output, the centred
    // records do not; the floor applies to the share WITH the bias (the partial sums are floored at 1e-50 / |det|,
    // outlier_part_floor), and a share at the floor holds nothing
    float b = tile[lane][ff] + part_bias;
    if (floors) b = fmaxf(b, LOG_TINY_F);
    const float a = *o;
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    float r = hi;
    if (floors) {
      r = merge_floored_shares(a, b);  // a part AT the floor holds nothing
    } else {
      r = hi + log1pf(expf(lo - hi));  // clustered pass: no floors before k_cluster_merge
    }
    *o = r;
  }
}

// Outlier routing (gmm.h): the outlier components of the states that have any, in the centred
// form, merged into the scores the matrix path has already written.
void score_outliers(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, hipStream_t stream,
                    const int32_t *crow, const unsigned long long *maskw, int c1, int64_t n_words, int64_t pitch) {
  if (pitch <= 0) pitch = g->S;
  const int64_t Sb = g->hyb_states;
  if (Sb <= 0) return;
  // passes of at most ~1 GB of partial scores
  int64_t pass = std::max<int64_t>(512, ((int64_t)(g_score_pass_bytes / (double)(Sb * 4))) / 512 * 512);
  if (pass > F) pass = (F + 63) / 64 * 64;
  g->hyb_scratch.ensure((size_t)pass * (size_t)Sb);
  CentredOps ops{g->hyb_recs.p, g->hyb_state_off.p, g->hyb_splits.p, g->hyb_max_splits, 1, pass};
  ops.n_recs = g->hyb_rows;
  ops.crow = crow;
  ops.c1 = c1;
  ops.floor_val = outlier_part_floor(g);
  g->hyb_merge_passes++;
  for (int64_t f0 = 0; f0 < F; f0 += pass) {  // pass is a multiple of 512 frames: whole mask words
    const int64_t n = std::min(pass, F - f0);
    if (maskw) {
      ops.maskw = maskw + (f0 / 64) * c1;
      ops.n_words = n_words - f0 / 64;
    }
    if (!launch_centred_ops(g, ops, g->centred_dimp, d_frames + f0 * g->dim, n, g->hyb_scratch.p, stream))
      raise(AASR_ERR_UNSUPPORTED, "no centred kernel instance for dimension %d", g->dim);
    hipLaunchKernelGGL(k_outlier_merge, dim3((unsigned)((n + 63) / 64), (unsigned)((Sb + 63) / 64)), dim3(256), 0,
                       stream, d_out + f0 * pitch, pitch, g->hyb_scratch.p, pass, Sb, g->hyb_map.p, n, maskw ? 0 : 1,
                       (float)g->out_bias_ln);
    AASR_HIP(hipGetLastError());
  }
}

// Outlier routing with the merge inside the scoring kernel (k_gmm_diag_score_pl<..., HYB>): where the launch that follows
// is the grouped layout's two-term kernel, the outliers' partial sums of all F frames are formed first (state-major, the
// centred kernel's coalesced form) and put on the handle for the launcher; returns false where the merge pass has to do
// it (other layouts / precisions, clustering, more partial sums than a pass holds).  What it returns is an offer: the
// launcher sets hyb_fuse.used where the HYB instance took it, and the callers run the merge pass where none did.
bool hyb_fuse_begin(aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, hipStream_t stream) {
  g->hyb_fuse = aasr_gmm::HybFuse();
  static const int fuse_env = AASR_EXPERIMENT_ENV("AASR_HYB_FUSE") ? atoi(AASR_EXPERIMENT_ENV("AASR_HYB_FUSE")) : 1;   // EXPERIMENT: 0 = merge pass
  const int64_t Sb = g->hyb_states;
  if (!fuse_env || g->hyb_fuse_off || !g->hyb_enabled || Sb <= 0 || !g->hyb_tab.p || g->cl.enabled || g->precision != AASR_PREC_F16X2 ||
      !g->use_bf16x3 || !L.ok || !L.grouped || !L.a16h.p || L.n_pg > 1 || !(g->layout_mask & 1) || L.nk16 <= 0)
    return false;
  const int64_t pass = (F + 63) / 64 * 64;
  if ((double)pass * (double)Sb * 4.0 > g_score_pass_bytes) return false;
  if ((size_t)pass * (size_t)Sb > g->hyb_scratch.n) {
    AASR_HIP(hipDeviceSynchronize());   // growing frees the old buffer
    g->hyb_scratch.ensure((size_t)pass * (size_t)Sb);
  }
  CentredOps ops{g->hyb_recs.p, g->hyb_state_off.p, g->hyb_splits.p, g->hyb_max_splits, 1, pass};
  ops.n_recs = g->hyb_rows;
  ops.floor_val = outlier_part_floor(g);
  if (!launch_centred_ops(g, ops, g->centred_dimp, d_frames, F, g->hyb_scratch.p, stream)) return false;
  g->hyb_fuse.part = g->hyb_scratch.p;
  g->hyb_fuse.pitch = pass;
  return true;
}

// ---------------------------------------------------------------------------
// AASR_PREC_F64: the reference's own arithmetic, operation by operation, in double
// (DiagonalGaussian::compute_log_likelihood, aku/Distributions.cc:1040-1062: ll += d*d*p over the
// dimensions, ll *= -0.5, ll += constant; compute_likelihood :1033-1037 = exp; Mixture::
// compute_likelihood :2078-2086: l += w * lik in component order; HmmSet's 1e-50 clamp
// :497-498).  The build has -ffp-contract=off, so every product and sum is rounded separately as
// in the reference's x86-64 build; what is left against the oracle is the device's exp() and
// log() (<= 1 ulp).  One lane per frame (its vector in VGPRs as doubles), the Gaussian records are
// wave-uniform and arrive through the scalar cache.  A verification / training-side mode:
// ~6 f64 operations per frame, Gaussian and dimension on the vector ALU.
// ---------------------------------------------------------------------------
// CL: Gaussian clustering -- component r belongs to cluster crow[r]; where the frame's bit of
// maskw[word][cluster] is clear the component takes its centre's likelihood, recovered from the
// ranking key the centre kernel stored (key == ll where exp(ll) is a normal double, else the
// denormal's integer multiple of 2^-1074, gmm_cluster.hip lin_key).
template <int DIMP, bool CL>
__global__ __launch_bounds__(256) void k_gmm_diag_score_f64(const double *__restrict__ frames, int64_t F, int dim,
                                                            const double *__restrict__ recs,
                                                            const int32_t *__restrict__ state_off, int64_t S,
                                                            double *__restrict__ out, int linear, double det,
                                                            const int32_t *__restrict__ crow,
                                                            const unsigned long long *__restrict__ maskw, int c1,
                                                            const double *__restrict__ ll64, int64_t Cs, int C) {
  constexpr int REC = 2 * DIMP + 2;  // [mean x DIMP][precision x DIMP][constant, weight]
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t fc = f < F ? f : F - 1;
  double x[DIMP];
#pragma unroll
  for (int d = 0; d < DIMP; d++) x[d] = d < dim ? frames[fc * dim + d] : 0.0;
  const int64_t s_per = (S + gridDim.y - 1) / gridDim.y;
  const int64_t s_begin = (int64_t)blockIdx.y * s_per, s_end = min(S, s_begin + s_per);
  for (int64_t s = s_begin; s < s_end; s++) {
    const int r0 = state_off[s], r1 = state_off[s + 1];
    double l = 0;
    for (int r = r0; r < r1; r++) {
      const double *rec = recs + (size_t)r * REC;
      double ll = 0;
#pragma unroll
      for (int d = 0; d < DIMP; d++) {
        const double t = x[d] - rec[d];
        ll += t * t * rec[DIMP + d];
      }
      ll *= -0.5;
      ll += rec[2 * DIMP];
      // AdaptedGaussian::compute_likelihood = g(A f + b) * |det| (aku/ModelModules.hh:172-173); det = 1 unadapted
      double lik = exp(ll) * det;
      if (CL) {
        const int c = crow[r];
        const bool on = (maskw[(fc >> 6) * c1 + c] >> (fc & 63)) & 1ull;
        if (!on) {  // c < C here: the "no cluster" column C is all ones
          const double key = ll64[fc * Cs + (c < C ? c : 0)];
          lik = key > -1000.0 ? exp(key) : ldexp((key + 2000.0) * 4398046511104.0, -1074);
        }
      }
      l += rec[2 * DIMP + 1] * lik;
    }
    if (l < 1e-50) l = 1e-50;  // also NaN-free: comparisons with NaN are false, as in the reference
    if (f < F) out[f * S + s] = linear ? l : log(l);
  }
}

__global__ void k_f32_to_f64(const float *__restrict__ in, double *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}
__global__ void k_f64_to_f32(const double *__restrict__ in, float *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

// o = b + A f in double, the reference's order (AdaptedFeatureVector::calculate_new_ada_vector,
// aku/ModelModules.hh:208-212)
__global__ void k_affine_frames_f64(const double *__restrict__ x, int64_t F, int dim, const double *__restrict__ A,
                                    const double *__restrict__ b, double *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= F * dim) return;
  const int64_t f = idx / dim;
  const int i = (int)(idx - f * dim);
  double acc = b[i];
  for (int j = 0; j < dim; j++) acc += A[(size_t)i * dim + j] * x[f * dim + j];
  y[idx] = acc;
}

// Per-class model transforms under AASR_PREC_F64 (regression classes: ConstrainedMllr, aku/ModelModules.cc:164-232).
// Every component is an AdaptedGaussian of its class: g(A_c f + b_c) |det_c|, summed in COMPONENT order as
// Mixture::compute_likelihood does -- so the frames of every class are laid out [class][dimension][frame] and a
// record reads its class's values straight from there (coalesced over the lanes, one load per dimension and record):
// a verification mode, an order of magnitude slower than the single-transform kernel.
__global__ void k_affine_frames_f64_classes(const double *__restrict__ x, int64_t F, int dim, int classes,
                                            const double *__restrict__ A, const double *__restrict__ b,
                                            double *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (class, i, f), f fastest
  if (idx >= (int64_t)classes * dim * F) return;
  const int64_t f = idx % F;
  const int64_t ci = idx / F;
  const int i = (int)(ci % dim), c = (int)(ci / dim);
  if (c == 0) {
    y[idx] = x[f * dim + i];
    return;
  }
  // o = b + A f in the reference's order (AdaptedFeatureVector::calculate_new_ada_vector, aku/ModelModules.hh:208-212)
  const double *Ac = A + ((size_t)c * dim + i) * dim;
  double acc = b[(size_t)c * dim + i];
  for (int j = 0; j < dim; j++) acc += Ac[j] * x[f * dim + j];
  y[idx] = acc;
}

template <int DIMP, bool CL>
__global__ __launch_bounds__(256) void k_gmm_diag_score_f64_classes(
    const double *__restrict__ xc, int64_t F, int dim, const double *__restrict__ recs,
    const int32_t *__restrict__ rec_class, const double *__restrict__ class_det,
    const int32_t *__restrict__ state_off, int64_t S, double *__restrict__ out, int linear,
    const int32_t *__restrict__ crow, const unsigned long long *__restrict__ maskw, int c1,
    const double *__restrict__ ll64, int64_t Cs, int C) {
  constexpr int REC = 2 * DIMP + 2;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t fc = f < F ? f : F - 1;
  const int64_t s_per = (S + gridDim.y - 1) / gridDim.y;
  const int64_t s_begin = (int64_t)blockIdx.y * s_per, s_end = min(S, s_begin + s_per);
  for (int64_t s = s_begin; s < s_end; s++) {
    const int r0 = state_off[s], r1 = state_off[s + 1];
    double l = 0;
    for (int r = r0; r < r1; r++) {
      const double *rec = recs + (size_t)r * REC;
      const int c = rec_class[r];
      const double *x = xc + (size_t)c * dim * F + fc;
      double ll = 0;
      for (int d = 0; d < dim; d++) {
        const double t = x[(size_t)d * F] - rec[d];
        ll += t * t * rec[DIMP + d];
      }
      ll *= -0.5;
      ll += rec[2 * DIMP];
      double lik = exp(ll) * class_det[c];
      if (CL) {  // as k_gmm_diag_score_f64: an unselected cluster's members take the (plain) centre's likelihood
        const int cc = crow[r];
        const bool on = (maskw[(fc >> 6) * c1 + cc] >> (fc & 63)) & 1ull;
        if (!on) {
          const double key = ll64[fc * Cs + (cc < C ? cc : 0)];
          lik = key > -1000.0 ? exp(key) : ldexp((key + 2000.0) * 4398046511104.0, -1074);
        }
      }
      l += rec[2 * DIMP + 1] * lik;
    }
    if (l < 1e-50) l = 1e-50;
    if (f < F) out[f * S + s] = linear ? l : log(l);
  }
}

// one pass of at most `n` frames: class frames, then the kernel (masked when the selection tables are given)
static void f64_classes_pass(aasr_gmm *g, const double *d_frames, int64_t n, double *d_out, int linear,
                             const int32_t *crow, const unsigned long long *maskw, int c1, const double *ll64,
                             int64_t Cs, int C, hipStream_t stream) {
  const int nc = g->f64_classes;
  g->f64_class_x.ensure((size_t)nc * g->dim * (size_t)n);
  const int64_t nv = (int64_t)nc * g->dim * n;
  hipLaunchKernelGGL(k_affine_frames_f64_classes, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream, d_frames, n,
                     g->dim, nc, g->f64_class_A.p, g->f64_class_b.p, g->f64_class_x.p);
  AASR_HIP(hipGetLastError());
  const int64_t blocks = (n + 255) / 256;
  int64_t cuts = std::max<int64_t>(1, std::min<int64_t>(g->S, (4 * (int64_t)(g->num_cus > 0 ? g->num_cus : 256) + blocks - 1) / blocks));
  if (cuts > 65535) cuts = 65535;
#define AASR_ARGS g->f64_class_x.p, n, g->dim, g->f64_recs.p, g->f64_rec_class.p, g->f64_class_det.p, \
                  g->f64_state_off.p, g->S, d_out, linear, crow, maskw, c1, ll64, Cs, C
#define AASR_CASE(N)                                                                                              \
  case N:                                                                                                         \
    if (maskw)                                                                                                    \
      hipLaunchKernelGGL((k_gmm_diag_score_f64_classes<N, true>), dim3((unsigned)blocks, (unsigned)cuts), dim3(256), 0, stream, AASR_ARGS); \
    else                                                                                                          \
      hipLaunchKernelGGL((k_gmm_diag_score_f64_classes<N, false>), dim3((unsigned)blocks, (unsigned)cuts), dim3(256), 0, stream, AASR_ARGS); \
    break;
  switch (g->f64_dimp) {
    AASR_CASE(8) AASR_CASE(16) AASR_CASE(24) AASR_CASE(32) AASR_CASE(40) AASR_CASE(48) AASR_CASE(64)
    default:
      raise(AASR_ERR_UNSUPPORTED, "no f64 kernel instance for dimension %d", g->dim);
  }
#undef AASR_CASE
#undef AASR_ARGS
  AASR_HIP(hipGetLastError());
}

static void score_f64_classes_launch(aasr_gmm *g, const double *d_frames, int64_t F, double *d_out, int linear,
                                     hipStream_t stream) {
  // passes of at most ~1 GB of class frames
  int64_t pass = std::max<int64_t>(256, (int64_t)(1.0e9 / ((double)g->f64_classes * g->dim * 8)));
  if (pass > F) pass = F;
  for (int64_t f0 = 0; f0 < F; f0 += pass) {
    const int64_t n = std::min(pass, F - f0);
    f64_classes_pass(g, d_frames + f0 * g->dim, n, d_out + f0 * g->S, linear, nullptr, nullptr, 0, nullptr, 0, 0, stream);
  }
}

// clustered sub-pass under per-class transforms (called by gmm_cluster_score_f64_launch with the RAW frames)
void gmm_f64_classes_masked_launch(aasr_gmm *g, const double *d_frames, int64_t n, double *d_out, int linear,
                                   const int32_t *crow, const unsigned long long *maskw, int c1, const double *ll64,
                                   int64_t Cs, int C, hipStream_t stream) {
  gmm_build_f64(g);
  f64_classes_pass(g, d_frames, n, d_out, linear, crow, maskw, c1, ll64, Cs, C, stream);
}

void gmm_score_f64_launch(aasr_gmm *g, const double *d_frames, int64_t F, double *d_out, int linear,
                          hipStream_t stream) {
  if (F <= 0) return;
  if (g->host.any_full()) raise(AASR_ERR_UNSUPPORTED, "AASR_PREC_F64 is built for diagonal pools");
  if (!g->dim_parts.empty() && (g->cl.enabled || (g->host.n_transforms > 0 && !g->host.global_xform())))
    raise(AASR_ERR_UNSUPPORTED, "AASR_PREC_F64 with clustering or regression classes is built for feature dimensions <= 63");
  gmm_build_f64(g);
  if (g->f64_classes > 0) {
    if (g->cl.enabled) gmm_cluster_score_f64_launch(g, d_frames, d_frames, F, d_out, linear, 1.0, stream);
    else score_f64_classes_launch(g, d_frames, F, d_out, linear, stream);
    return;
  }
  const double *d_raw = d_frames;
  double det = 1.0;
  if (g->host.n_transforms > 0) {  // one global transform: adapted frames, |prod diag A| on every Gaussian
    const int64_t nv = F * g->dim;
    g->f64_xframes.ensure((size_t)nv);
    hipLaunchKernelGGL(k_affine_frames_f64, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream, d_frames, F,
                       g->dim, g->f64_A.p, g->f64_b.p, g->f64_xframes.p);
    AASR_HIP(hipGetLastError());
    d_frames = g->f64_xframes.p;
    det = g->f64_det;
  }
  if (g->cl.enabled) {
    gmm_cluster_score_f64_launch(g, d_raw, d_frames, F, d_out, linear, det, stream);
    return;
  }
  gmm_f64_masked_launch(g, d_frames, F, d_out, linear, det, nullptr, nullptr, 0, nullptr, 0, 0, stream);
}

void gmm_f64_masked_launch(aasr_gmm *g, const double *d_frames, int64_t F, double *d_out, int linear, double det,
                           const int32_t *crow, const unsigned long long *maskw, int c1, const double *ll64,
                           int64_t Cs, int C, hipStream_t stream) {
  gmm_build_f64(g);
  const int64_t blocks = (F + 255) / 256;
  // state-range cuts so that small batches still fill the chip
  int64_t cuts = std::max<int64_t>(1, std::min<int64_t>(g->S, (4 * (int64_t)(g->num_cus > 0 ? g->num_cus : 256) + blocks - 1) / blocks));
  if (cuts > 65535) cuts = 65535;
#define AASR_CASE(N)                                                                                              \
  case N:                                                                                                         \
    if (maskw)                                                                                                    \
      hipLaunchKernelGGL((k_gmm_diag_score_f64<N, true>), dim3((unsigned)blocks, (unsigned)cuts), dim3(256), 0,   \
                         stream, d_frames, F, g->dim, g->f64_recs.p, g->f64_state_off.p, g->S, d_out, linear, det, \
                         crow, maskw, c1, ll64, Cs, C);                                                           \
    else                                                                                                          \
      hipLaunchKernelGGL((k_gmm_diag_score_f64<N, false>), dim3((unsigned)blocks, (unsigned)cuts), dim3(256), 0,  \
                         stream, d_frames, F, g->dim, g->f64_recs.p, g->f64_state_off.p, g->S, d_out, linear, det, \
                         crow, maskw, c1, ll64, Cs, C);                                                           \
    break;
  // wide models (64 < dimension <= 192): the unmasked instance only
#define AASR_WIDE(N)                                                                                              \
  case N:                                                                                                         \
    if (maskw) raise(AASR_ERR_UNSUPPORTED, "AASR_PREC_F64 with clustering is built for feature dimensions <= 63"); \
    hipLaunchKernelGGL((k_gmm_diag_score_f64<N, false>), dim3((unsigned)blocks, (unsigned)cuts), dim3(256), 0,    \
                       stream, d_frames, F, g->dim, g->f64_recs.p, g->f64_state_off.p, g->S, d_out, linear, det,  \
                       crow, maskw, c1, ll64, Cs, C);                                                             \
    break;
  switch (g->f64_dimp) {
    AASR_CASE(8) AASR_CASE(16) AASR_CASE(24) AASR_CASE(32) AASR_CASE(40) AASR_CASE(48) AASR_CASE(64)
    AASR_WIDE(96) AASR_WIDE(128) AASR_WIDE(192)
    default:
      raise(AASR_ERR_UNSUPPORTED, "no f64 kernel instance for dimension %d", g->dim);
  }
#undef AASR_CASE
#undef AASR_WIDE
  AASR_HIP(hipGetLastError());
}

// float entry points under AASR_PREC_F64: frames widened, scores rounded once at the end
void score_f64_for_f32_callers(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, hipStream_t stream) {
  const int64_t nx = F * g->dim, ns = F * g->S;
  g->f64_x.ensure((size_t)nx);
  g->f64_out.ensure((size_t)ns);
  hipLaunchKernelGGL(k_f32_to_f64, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, stream, d_frames, g->f64_x.p, nx);
  gmm_score_f64_launch(g, g->f64_x.p, F, g->f64_out.p, 0, stream);
  hipLaunchKernelGGL(k_f64_to_f32, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream, g->f64_out.p, d_out, ns);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

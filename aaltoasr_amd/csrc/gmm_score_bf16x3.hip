// gmm_score_bf16x3.hip -- AASR_PREC_BF16X3 (the map of the files: gmm_score.hip): the three-term instances of
// k_gmm_diag_score_pl and k_frame_operand<3> (gmm_score_pl.h) up to five K slabs and on multi-pivot layouts, and the
// wave-group kernel k_gmm_diag_score_bf16x3 for six and eight slabs.
#include "gmm_score_pl.h"

namespace aasr {

// WIDE: one workgroup of 8 waves (512 frames) per CU instead of two of 4 waves, so a tile is
// fetched from L2 once per 512 frames -- the L2 -> LDS tile traffic is what the power-capped
// matrix stream pays for (measured: no traffic -6.3 ms, half of it -2.1 ms of 34.9).  The two wave
// groups run the same tile sequence half a tile apart (group 1 lags by one barrier; every wave
// passes two barriers per tile, one in the middle of its stream), which puts one group's
// epilogue under the other group's matrix stream; three tile buffers make the lag legal.
template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS>
__global__ __launch_bounds__(WIDE ? 512 : 256, WIDE ? 1 : 2) void k_gmm_diag_score_bf16x3(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ pivot,
    const uint16_t *__restrict__ apack, const int32_t *__restrict__ split_row,
    const uint16_t *__restrict__ close_mask, const int32_t *__restrict__ sid, int sid_stride,
    float *__restrict__ out, int64_t S, int64_t pitch, float ref_ln, int dbg, ClusterArgs cl) {
  // three bf16 terms only: the two-term fp16 arithmetic (per-column scales, per-dimension clamps: pack_f16x2) lives in
  // k_gmm_diag_score_pl; the NS == 2 paths below are what is left of its first home and know neither
  static_assert(NS == 3, "k_gmm_diag_score_bf16x3 is instantiated for the three-term form only");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int OG = Bf16Smem<NK16, GROUPED, WIDE, NS>::OG;
  constexpr int kTileBytes = Bf16Smem<NK16, GROUPED, WIDE, NS>::kTileBytes;
  constexpr int kTileFloats = kTileBytes / 4;
  constexpr int kOS = Bf16Smem<NK16, GROUPED, WIDE, NS>::kOutStride;
  constexpr int NW = WIDE ? 8 : 4;    // waves per workgroup
  constexpr int NBUF = WIDE ? 3 : 2;  // tile buffers
  // WIDE: slabs before the mid-stream barrier.  Between two barriers one wave of a SIMD runs the slabs behind its
  // mid-stream barrier while its partner runs an epilogue FOLLOWED BY the slabs in front of it, so the partner's
  // stretch is epilogue + JMID slabs of matrix time against (NK16 - JMID) slabs here.  With 30 MFMAs per slab
  // (bf16x3) the epilogue (~1500 cycles: 64 v_exp_f32 at quarter rate + the adds) is the smaller part and the even
  // split is fine; with 12 (f16x2) it is four slabs' worth, so it is paired with ONE slab: 1500 + 384 against 1536
  // cycles and a matrix pipe that is busy 1920 of them (measured: JMID = 3 leaves 59.6 M cycles per launch
  // for 22.9 M of matrix work, the critical wave being epilogue + 36 MFMAs long).
  constexpr int JMID = NS == 2 ? 1 : (NK16 + 1) / 2;
  // f16x2: the fragments of slab j + 1 are requested at the top of slab j into a second register set (12 MFMAs =
  // 384 cycles ahead); the rolling refill of the three-term form would leave them 4 MFMAs
  constexpr int NAB = NS == 2 ? 2 : 1;
  float *abuf0 = (float *)smem_raw;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int group = WIDE ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;
  float *ost = abuf0 + NBUF * kTileFloats + wave * Bf16Smem<NK16, GROUPED, WIDE, NS>::kOutFloatsPerWave;
  const int n = lane & 31;
  const int h = lane >> 5;  // K half of a slab held by this lane AND its row track
  const int64_t f0 = (int64_t)blockIdx.x * (NW * FRAMES_PER_WAVE) + wave * FRAMES_PER_WAVE;

  // ---- frame operand: lane (n, h) holds k = 16*j + 8*h + i, i < 8, of slab j
  u32x4 bq[NK16][NS][2];
#pragma unroll
  for (int nb = 0; nb < 2; nb++) {
    int64_t f = f0 + nb * 32 + n;
    if (f > F - 1) f = F - 1;
    const float *xr = frames + f * dim;
#pragma unroll
    for (int j = 0; j < NK16; j++) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int k = 16 * j + 8 * h + i;
        const int d = (k >> 1) - 1;   // k = 0 / 1: the constant's slots
        const int dc = d >= 0 && d < dim ? d : 0;
        const float xc = xr[dc] - pivot[dc];
        float xq = xc;
        if (NS == 2) xq = fminf(fmaxf(xc, -kF16Clamp), kF16Clamp);  // fp16 range (see the f16x2 note in gmm_score_common.h)
        float val = (k & 1) ? xq * xq : xq;
        if (d < 0) val = (k == 0 || NS == 2) ? 1.0f : 0.0f;
        else if (d >= dim) val = 0.0f;
        v[i] = val;
      }
      if constexpr (NS == 3) {
        unsigned w1[4], w2[4], w3[4];
#pragma unroll
        for (int i = 0; i < 4; i++) split3_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i], w3[i]);
        bq[j][0][nb] = u32x4{w1[0], w1[1], w1[2], w1[3]};
        bq[j][1][nb] = u32x4{w2[0], w2[1], w2[2], w2[3]};
        bq[j][2][nb] = u32x4{w3[0], w3[1], w3[2], w3[3]};
      } else {
        unsigned w1[4], w2[4];
#pragma unroll
        for (int i = 0; i < 4; i++) split2_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i]);
        bq[j][0][nb] = u32x4{w1[0], w1[1], w1[2], w1[3]};
        bq[j][1][nb] = u32x4{w2[0], w2[1], w2[2], w2[3]};
      }
    }
  }

  const int64_t t_begin = split_row[4 * blockIdx.y];
  const int64_t t_end = split_row[4 * blockIdx.y + 4];
  const float *apf = (const float *)apack;
  issue_tile_copy_raw(apf + (size_t)t_begin * kTileFloats, abuf0, kTileFloats, wave, lane, NW);
  if (WIDE && t_begin + 1 < t_end)
    issue_tile_copy_raw(apf + (size_t)(t_begin + 1) * kTileFloats, abuf0 + kTileFloats, kTileFloats, wave, lane, NW);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (WIDE && group == 1) __builtin_amdgcn_s_barrier();  // the lagging group's "end of tile -1"

  float s0 = 0.0f, s1 = 0.0f;
  int closes = split_row[4 * blockIdx.y + 1 + (GROUPED ? 0 : h)];
  const int32_t *my_sid = sid + h * sid_stride;
  int next_sid = GROUPED ? 0 : my_sid[closes];
  float *orow0 = out + (f0 + n) * pitch;  // pitch: row stride of `out` in floats (>= S)
  float *orow1 = out + (f0 + 32 + n) * pitch;
  const bool ok0 = f0 + n < F, ok1 = f0 + 32 + n < F;
  const float floor_val = CL ? cl.floor_val : LOG_TINY_F;
  // this wave's 64 frames are one word of the selection masks; its per-lane bits of tile t
  const unsigned long long *mrow =
      CL ? cl.maskrow + (size_t)(f0 >> 6) * cl.rows_padded + lane : nullptr;
  unsigned long long bits_next = 0;
  if (CL && split_row[4 * blockIdx.y] < split_row[4 * blockIdx.y + 4])
    bits_next = mrow[(size_t)split_row[4 * blockIdx.y] * TILE_ROWS];

  if (AASR_DBG(4)) {  // experiment: de-phase co-resident workgroups
    unsigned hsh = ((unsigned)blockIdx.x + 977u * blockIdx.y) * 2654435761u;
    int bucket = (hsh >> 28) & 15;
    for (int i = 0; i < bucket; i++) __builtin_amdgcn_s_sleep(8);
  }
  if (AASR_DBG(8)) {  // experiment: raise priority of every second workgroup
    if ((blockIdx.x >> 8) & 1) __builtin_amdgcn_s_setprio(2);
  }
  // Close bits of a tile: a VECTOR load issued in the middle of the previous tile's matrix stream
  // and turned into a scalar after that tile's barrier, whose vmcnt(0) covers it.  Two traps are
  // avoided this way: loaded at the top of a tile, the compiler waits for it with vmcnt(0) right
  // behind the tile copy (vmcnt is in issue order; measured 5 ms of 30 in the matrix stream), and a
  // scalar load anywhere in the loop turns every LDS wait of the stream into lgkmcnt(0).
  unsigned mask16_next = t_begin < t_end ? (unsigned)__builtin_amdgcn_readfirstlane((int)close_mask[t_begin]) : 0u;
  unsigned mask_v = 0;
  u32x4 afr[NAB][NS][2];  // A fragments of the current slab, [register set][split][row block]
  if (t_begin < t_end) {
#pragma unroll
    for (int sp = NS - 1; sp >= 0; sp--) {
      afr[0][sp][0] = ((const u32x4 *)abuf0 + lane)[(sp * 2 + 0) * 64];
      afr[0][sp][1] = ((const u32x4 *)abuf0 + lane)[(sp * 2 + 1) * 64];
    }
  }
  int bi = 0;  // buffer of the current tile
  for (int64_t t = t_begin; t < t_end; t++) {
    float *acur = abuf0 + bi * kTileFloats;
    const int bn = bi + 1 < NBUF ? bi + 1 : 0;         // buffer of tile t+1
    const int bnn = bn + 1 < NBUF ? bn + 1 : 0;        // WIDE: buffer of tile t+2 (held tile t-1)
    float *anext = abuf0 + bn * kTileFloats;
    if (!WIDE) {
      if (t + 1 < t_end && !AASR_DBG(256) && !(AASR_DBG(512) && (t & 1)))  // ablations: 256 no tile traffic, 512 half of it
        issue_tile_copy_raw(apf + (size_t)(t + 1) * kTileFloats, anext, kTileFloats, wave, lane, NW);
    } else if (group == 1 && t + 2 < t_end && !AASR_DBG(256)) {
      // both groups are past tile t-1 once the lagging group has passed its end-of-tile barrier
      issue_tile_copy_raw(apf + (size_t)(t + 2) * kTileFloats, abuf0 + bnn * kTileFloats, kTileFloats, wave, lane, NW);
    }
    bi = bn;
    const unsigned mask16 = mask16_next;
    const unsigned mask = GROUPED ? (mask16 & 0xffu) : (h ? (mask16 >> 8) : (mask16 & 0xffu));
    // this tile's selection bits arrived during the previous tile; the next tile's are requested
    // here and waited for by the vmcnt(0) in front of the end-of-tile barrier
    const unsigned long long bits = bits_next;
    if (CL && t + 1 < t_end) bits_next = mrow[(size_t)(t + 1) * TILE_ROWS];

    if (AASR_DBG(32)) __builtin_amdgcn_s_setprio(3);
    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const u32x4 *afrag = (const u32x4 *)acur + lane;  // [slab][split][mb][64 lanes]
    // Rolling A-fragment prefetch.  The products of a slab are ordered by the A split they use,
    // (a3,b1) | (a2,b2) (a2,b1) | (a1,b3) (a1,b2) (a1,b1), so each split's registers fall free as
    // early as possible and are refilled for the NEXT slab right then: every ds_read has 12-20
    // MFMAs (>= 384 cycles) to land and no extra registers are needed.  Left to itself the
    // compiler sinks the reads to their first use (one exposed LDS round trip per slab), hence
    // the full scheduling barriers.  The 2^-16 products still precede the 2^-8 ones of the same
    // A split; the sum already holds earlier slabs, so the order inside a slab is immaterial.
#pragma unroll
    for (int j = 0; j < NK16; j++) {
      if (WIDE && j == JMID) {
        // mid-stream barrier = the other group's end-of-tile barrier
        if (!AASR_DBG(16)) __builtin_amdgcn_s_barrier();
        if (group == 0 && t + 2 < t_end && !AASR_DBG(256))
          issue_tile_copy_raw(apf + (size_t)(t + 2) * kTileFloats, abuf0 + bnn * kTileFloats, kTileFloats, wave, lane, NW);
        __builtin_amdgcn_sched_barrier(0);
      }
      constexpr int kNoSet = 0;
      const int cur = NAB == 2 ? (j & 1) : kNoSet;
      if (NAB == 2 && j + 1 < NK16 && !AASR_DBG(2)) {
#pragma unroll
        for (int sp = NS - 1; sp >= 0; sp--) {
          afr[cur ^ 1][sp][0] = afrag[(((j + 1) * NS + sp) * 2 + 0) * 64];
          afr[cur ^ 1][sp][1] = afrag[(((j + 1) * NS + sp) * 2 + 1) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int grp = 0; grp < NS; grp++) {
        const int sp = NS - 1 - grp;   // A split used by this group: a3, a2, a1 (f16x2: a2, a1)
        const int nprod = grp + 1;     // paired with b1 | b2 b1 | b3 b2 b1
#pragma unroll
        for (int c = 0; c < nprod; c++) {
          const int sb = nprod - 1 - c;
          c00 = mfma_split<NS>(afr[cur][sp][0], bq[j][sb][0], c00);
          c01 = mfma_split<NS>(afr[cur][sp][0], bq[j][sb][1], c01);
          c10 = mfma_split<NS>(afr[cur][sp][1], bq[j][sb][0], c10);
          c11 = mfma_split<NS>(afr[cur][sp][1], bq[j][sb][1], c11);
        }
        __builtin_amdgcn_sched_barrier(0);
        // the aligned word holding tile t+1's bits (the array has a spare element); a 16-bit load
        // would need a zero-extension, which the compiler places -- with its vmcnt wait -- right here
        if (j == (NK16 > 1 ? 1 : 0) && grp == 0) mask_v = ((const uint32_t *)close_mask)[(t + 1) >> 1];
        if (NAB == 1 && j + 1 < NK16 && !AASR_DBG(2)) {
          afr[kNoSet][sp][0] = afrag[(((j + 1) * NS + sp) * 2 + 0) * 64];
          afr[kNoSet][sp][1] = afrag[(((j + 1) * NS + sp) * 2 + 1) * 64];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    if (WIDE && JMID >= NK16) {
      __builtin_amdgcn_s_barrier();
      if (group == 0 && t + 2 < t_end)
        issue_tile_copy_raw(apf + (size_t)(t + 2) * kTileFloats, abuf0 + bnn * kTileFloats, kTileFloats, wave, lane, NW);
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(mask_v) : : "memory");
    if (!AASR_DBG(16)) __builtin_amdgcn_s_barrier();
    mask16_next = (unsigned)__builtin_amdgcn_readfirstlane((int)mask_v);
    mask16_next = ((t + 1) & 1) ? mask16_next >> 16 : mask16_next & 0xffffu;
    if (t + 1 < t_end) {
      // slab 0 of the next tile: in flight while the epilogue runs
      const u32x4 *nfrag = (const u32x4 *)anext + lane;
#pragma unroll
      for (int sp = NS - 1; sp >= 0; sp--) {
        afr[0][sp][0] = nfrag[(sp * 2 + 0) * 64];
        afr[0][sp][1] = nfrag[(sp * 2 + 1) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    if (AASR_DBG(1)) {
      asm volatile("" ::"v"(c00), "v"(c01), "v"(c10), "v"(c11));
      continue;
    }
    if (AASR_DBG(32)) __builtin_amdgcn_s_setprio(0);   // experiment: the epilogue yields to the partner's matrix stream

#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
      const f32x16 &ca = mb ? c10 : c00;
      const f32x16 &cb = mb ? c11 : c01;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float va[4], vb[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          va[e] = ca[4 * q + e];
          vb[e] = cb[4 * q + e];
          if (CL) {
            va[e] = mask_select(va[e], bits, 8 * q + 4 * mb + e);        // k_cluster_expand's bit layout
            vb[e] = mask_select(vb[e], bits, 32 + 8 * q + 4 * mb + e);
          }
        }
        float e0 = __builtin_amdgcn_exp2f(va[0]) + __builtin_amdgcn_exp2f(va[1]);
        float e1 = __builtin_amdgcn_exp2f(va[2]) + __builtin_amdgcn_exp2f(va[3]);
        float g0 = __builtin_amdgcn_exp2f(vb[0]) + __builtin_amdgcn_exp2f(vb[1]);
        float g1 = __builtin_amdgcn_exp2f(vb[2]) + __builtin_amdgcn_exp2f(vb[3]);
        s0 += e0 + e1;
        s1 += g0 + g1;
        if ((mask >> (mb * 4 + q)) & 1) {
          float l0 = fmaf(__builtin_amdgcn_logf(s0), LN2_F, -ref_ln);
          float l1 = fmaf(__builtin_amdgcn_logf(s1), LN2_F, -ref_ln);
          l0 = fmaxf(l0, floor_val);
          l1 = fmaxf(l1, floor_val);
          s0 = 0.0f;
          s1 = 0.0f;
          closes++;
          if (!GROUPED) {
            if (ok0) orow0[next_sid] = l0;
            if (ok1) orow1[next_sid] = l1;
            next_sid = my_sid[closes];
          } else {
            const int pairs_closed = closes;
            const int slot = ((2 * (pairs_closed - 1)) & (OG - 1)) + h;
            ost[n * kOS + slot] = l0;
            ost[(32 + n) * kOS + slot] = l1;
            const int64_t closed = 2 * (int64_t)pairs_closed < S ? 2 * (int64_t)pairs_closed : S;
            if (((2 * pairs_closed) & (OG - 1)) == 0 || 2 * (int64_t)pairs_closed >= S) {
              const int64_t s_base = ((closed - 1) / OG) * OG;
              const int cnt = (int)(closed - s_base);
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              if (OG == 32 && cnt == OG && f0 + FRAMES_PER_WAVE <= F) {
                // 8 lanes x 16 B cover the 32-state group; 8 frame rows per instruction
                const int k4 = lane & 7, r8 = lane >> 3;
                float *op = out + (f0 + r8) * pitch + s_base + 4 * k4;
                const float *ip = ost + r8 * kOS + 4 * k4;  // stride 34: 8-byte aligned
#pragma unroll
                for (int i = 0; i < FRAMES_PER_WAVE / 8; i++) {
                  const f32x2 lo = *(const f32x2 *)(ip + i * 8 * kOS);
                  const f32x2 hi = *(const f32x2 *)(ip + i * 8 * kOS + 2);
                  const f32x4 v = {lo[0], lo[1], hi[0], hi[1]};
                  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
                  *(f32x4u *)(op + (int64_t)i * 8 * pitch) = v;
                }
              } else if (cnt == OG && f0 + FRAMES_PER_WAVE <= F) {
                // 4 lanes x 16 B cover the 16-state group; 16 frame rows per instruction
                const int k4 = lane & 3, r16 = lane >> 2;
                float *op = out + (f0 + r16) * pitch + s_base + 4 * k4;
                const float *ip = ost + r16 * kOS + 4 * k4;
#pragma unroll
                for (int i = 0; i < FRAMES_PER_WAVE / 16; i++) {
                  const f32x4 v = *(const f32x4 *)(ip + i * 16 * kOS);
                  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
                  *(f32x4u *)(op + (int64_t)i * 16 * pitch) = v;
                }
              } else {
                constexpr int RPI = 64 / OG;
                const int k = lane & (OG - 1);
#pragma unroll 4
                for (int i = 0; i < FRAMES_PER_WAVE / RPI; i++) {
                  const int row = i * RPI + lane / OG;
                  const float v = ost[row * kOS + k];
                  if (k < cnt && f0 + row < F) out[(f0 + row) * pitch + s_base + k] = v;
                }
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
            }
          }
        }
      }
    }
  }
  if (WIDE && group == 0) __builtin_amdgcn_s_barrier();  // pairs with the lagging group's last end-of-tile barrier
}

// Row cuts of a launch: `blocks` frame blocks x R cuts are dealt to `slots` resident workgroups in rounds; a workgroup
// costs its tiles plus a fixed part (launch, frame operand, first tile's latency, drain), `overhead` in units of one
// tile's time.  Measured on configs[2] (878 blocks of 512 frames, 782 tiles, 256 slots; ms of the scoring kernel at
// R = 2 / 4 / 8 / 16: 8.51 / 8.68 / 8.94 / 9.20): the fixed part was 6.6 tiles with the operand built in the kernel.
// The former rule -- the R whose last round is fullest -- took R = 9 there (8.86 ms).
static int pick_row_cuts(int64_t blocks, double slots, int64_t tiles, int max_splits, double overhead) {
  static const int force_r = AASR_EXPERIMENT_ENV("AASR_SPLITS") ? atoi(AASR_EXPERIMENT_ENV("AASR_SPLITS")) : 0;
  static const double force_c = AASR_EXPERIMENT_ENV("AASR_CUT_OVERHEAD") ? atof(AASR_EXPERIMENT_ENV("AASR_CUT_OVERHEAD")) : -1.0;
  if (force_r >= 1 && force_r <= max_splits) return force_r;
  if (force_c >= 0) overhead = force_c;
  int R = 1;
  double best = 1e300;
  for (int r = 1; r <= max_splits; r++) {
    const double cost = std::ceil((double)blocks * r / slots) * ((double)tiles / r + overhead);
    if (cost < best * 0.999) {
      best = cost;
      R = r;
    }
  }
  return R;
}

template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS>
static void launch_bf16_t(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                          float *d_out, hipStream_t stream, const ClusterArgs &cl, int64_t pitch) {
  constexpr int NW = WIDE ? 8 : 4;
  const int64_t blocks = (F + NW * FRAMES_PER_WAVE - 1) / (NW * FRAMES_PER_WAVE);
  const int smem = (WIDE ? 3 : 2) * Bf16Smem<NK16, GROUPED, WIDE, NS>::kTileBytes +
                   NW * Bf16Smem<NK16, GROUPED, WIDE, NS>::kOutFloatsPerWave * 4;
  static const int dbg = AASR_EXPERIMENT_ENV("AASR_DBG") ? atoi(AASR_EXPERIMENT_ENV("AASR_DBG")) : 0;
  static bool attr_set[64] = {false};
  auto kern = k_gmm_diag_score_bf16x3<NK16, GROUPED, CL, WIDE, NS>;
  if (!attr_set[g->device & 63]) {
    AASR_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set[g->device & 63] = true;
  }
  const int R = pick_row_cuts(blocks, (WIDE ? 1.0 : 2.0) * (g->num_cus > 0 ? g->num_cus : 256),
                              L.rows_padded / TILE_ROWS, L.max_splits, 6.0);
  const int32_t *split_row = L.splits.p + (size_t)(R - 1) * (L.split_cap + 1) * 4;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)R), dim3(NW * 64), smem, stream, d_frames, F,
                     g->dim, g->d_pivot.p, NS == 3 ? L.a16.p : L.a16h.p, split_row, L.close.p, L.sid.p, L.sid_stride,
                     d_out, g->S, pitch, L.ref_ln - (float)g->out_bias_ln, dbg, cl);
  AASR_HIP(hipGetLastError());
}

template bool launch_split<3>(const aasr_gmm *, const TrackLayout &, const float *, int64_t, float *, hipStream_t,
                              const ClusterArgs *, int64_t);
template void form_frame_operand<3>(const aasr_gmm *, const TrackLayout &, const float *, int64_t, hipStream_t);

}  // namespace aasr

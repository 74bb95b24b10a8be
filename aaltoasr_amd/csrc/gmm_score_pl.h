// gmm_score_pl.h -- the software-pipelined split-operand kernel k_gmm_diag_score_pl with k_frame_operand, the cut
// plans and the launch_split templates (the map of the files: gmm_score.hip).  A header, because two units instantiate
// it: gmm_score_f16x2.hip (launch_split<2>) and gmm_score_bf16x3.hip (launch_split<3>); no kernel instance is in both.
#pragma once
#include "gmm_score_common.h"

namespace aasr {

// ---------------------------------------------------------------------------
// Software-pipelined form of the split-operand kernel (the f16x2 arithmetic runs on it).
//
// With three fp16 products per K slab a wave-tile is 60 MFMAs = 1 920 matrix cycles, and its epilogue -- 64
// v_exp_f32 at quarter rate, the adds, the close logic -- is ~1 600 VALU cycles: no longer the small part.  The
// phase-shifted wave groups of k_gmm_diag_score_bf16x3 (gmm_score_bf16x3.hip) only hide an epilogue under the PARTNER wave's matrix stream, and
// measured that hides about half of it (rocprofv3: 37.9 M cycles per 10^6-frame launch for 22.9 M of matrix work,
// VALU co-executing under 41 % of the MFMA cycles; s_setprio either way changes nothing).  What does hide is VALU
// placed between a wave's OWN MFMAs: an MFMA occupies the matrix pipe for 32 cycles, the in-order wave issues its
// next instructions meanwhile.  So the tile is processed as two half tiles (its two 32-row blocks), and the matrix
// stream of one block carries the exponentials of the other:
//
//     H0(t): 30 MFMAs into block 0 of tile t     ||  2^x and quad sums of block 1 of tile t-1
//            close logic of block 1, tile t-1          (branches, log, staging, stores: not interleaved)
//     H1(t): 30 MFMAs into block 1 of tile t     ||  2^x and quad sums of block 0 of tile t
//            s_waitcnt vmcnt(0); s_barrier; close logic of block 0, tile t
//
// Same 64 accumulator registers (a block is consumed before it is accumulated into again), two accumulator
// chains per phase instead of four (dependent MFMAs 64 cycles apart), one barrier per tile, two tile buffers, all
// waves of a workgroup in step -- no wave groups.  A fragments of the next slab are requested one slab (6 MFMAs)
// ahead into a second register set.  Everything else (operand layout, track epilogue, output groups, row cuts,
// selection masks) is that kernel; results are bit-identical between the 4- and 8-wave forms.
// ---------------------------------------------------------------------------
// Work decomposition of a pipelined-kernel launch (see pick_cut_plan).
struct CutPlan {
  int n_main = 0;        // workgroups of the coarse part: blocks_main frame blocks x r_main cuts
  int blocks_main = 1;
  int blocks_rem = 1;    // frame blocks of the fine part
  int r_main = 1, r_rem = 0;
  const int32_t *split_rem = nullptr;   // cut table row of the fine part
};

// Pivot groups of a launch (nullptr colend: one pivot, the model's)
struct PivotGroups {
  const int32_t *colend = nullptr;   // [groups] one past the group's last output column
  int64_t fop_stride = 0;            // u32x4 elements between the groups' frame-operand images
  // PGF instances (the workgroup forms its group's operand in its prologue): the groups' pivots [groups][dim], their
  // column scales and clamps [groups][3 KH], the slab-constant flag of the layout
  const float *pivots = nullptr;
  const float *tabs = nullptr;
  int sc = 0;
  // HYB instances (outlier routing fused into the close logic, below): hyb_tab[s] = the next state >= s of s's track
  // parity that has outlier components (low 16 bits; 0xffff: none) and its record in the partial sums (high 16 bits);
  // the partial sums [records][pitch] (natural log, state-major, one row of frames per record:
  // k_gmm_diag_score_centred), log|det| of an in-place transform
  const uint32_t *hyb_tab = nullptr;
  const float *hyb_part = nullptr;
  int64_t hyb_pitch = 0;
  float hyb_bias = 0.0f;
};

// ---------------------------------------------------------------------------
// Frame operand of the two-term kernels, one unit: the 8 K-slot values of (frame row xr, slab j, K half h) around `pivot`
// -- (x - pivot), the dimension's clamp and the column's power-of-two scale, the square for the quadratic slots, 1 in the
// constant's slots -- the arithmetic of k_frame_operand (below), shared with the multi-pivot instances of
// k_gmm_diag_score_pl, which form their group's operand in their prologue (round 6: one image per pivot group through
// HBM was 320 B per frame and group, 0.46 ms of a fitted model's 11.1).  f16tab: [2 KH] column scales, [KH] clamps.
// ---------------------------------------------------------------------------
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void fop_unit_f16(const float *__restrict__ xr, int dim, const float *__restrict__ pivot,
                                             const float *__restrict__ f16tab, int KH, int j, int h, int sc,
                                             unsigned w1[4], unsigned w2[4]) {
  const int k0 = 16 * j + 8 * h;
  const int d0 = sc ? 7 * j + (h ? 3 : -1) : (k0 >> 1) - 1;
  const bool whole = !sc && d0 >= 0 && d0 + 4 <= dim;   // uniform per K half
  float v[8];
  if (whole) {
    const f32x4u a = *(const f32x4u *)(xr + d0);
    const f32x4u b = *(const f32x4u *)(pivot + d0);
    const f32x4u c = *(const f32x4u *)(f16tab + 2 * KH + d0);
    const f32x4u e0 = *(const f32x4u *)(f16tab + k0);
    const f32x4u e1 = *(const f32x4u *)(f16tab + k0 + 4);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float xc = a[i] - b[i];
      const float xq = fminf(fmaxf(xc, -c[i]), c[i]);   // fp16 range: the dimension's clamp (pack_f16x2)
      v[2 * i] = xq * (i < 2 ? e0[2 * i] : e1[2 * i - 4]);
      v[2 * i + 1] = (xq * xq) * (i < 2 ? e0[2 * i + 1] : e1[2 * i - 3]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int k = k0 + i;
      const int d = (sc ? (h == 0 && i < 2) : k < 2) ? -1 : d0 + (i >> 1);
      const int dc = d >= 0 && d < dim ? d : 0;
      const float xc = xr[dc] - pivot[dc];
      const float lim = f16tab[2 * KH + dc];
      const float xq = fminf(fmaxf(xc, -lim), lim);
      float val = (k & 1) ? xq * xq : xq;
      if (d < 0) val = 1.0f;   // the constant and its remainder
      else if (d >= dim) val = 0.0f;
      v[i] = val * f16tab[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) split2_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i]);
}

template <int NK16, bool GROUPED, bool WIDE, int NS>
struct PlSmem {
  static constexpr int kTileBytes = NK16 * NS * 2 * 64 * 16;
  static constexpr int NBUF = WIDE ? 3 : 2;   // tile buffers (the 8-wave form's lagging group needs the third)
  static constexpr bool kBig = WIDE && GROUPED && NBUF * kTileBytes + 8 * FRAMES_PER_WAVE * 34 * 4 <= 160 * 1024;
  static constexpr int OG = kBig ? 32 : 16;
  static constexpr int kOutStride = kBig ? 34 : 20;
  static constexpr int kOutFloatsPerWave = GROUPED ? FRAMES_PER_WAVE * kOutStride : 0;
  // Padding no kernel touches (until round 6: a side table of 64 bytes per tile buffer).  It stays because workgroups per
  // CU by LDS is floor(160 KB / kBytes), and without it seven instances sit exactly on a divisor and would gain a resident
  // workgroup (NK16 = 5, GROUPED, 4 waves, three terms: 82 048 -> 81 920 B = 80 KB, one workgroup per CU -> two): a change
  // of behaviour that would have to be measured, not a deletion.  Table: profiles/scoring_unit_kernel_digests.txt.
  static constexpr int kPadBytes = NBUF * 64;
  static constexpr int kBytes = NBUF * kTileBytes + (WIDE ? 8 : 4) * kOutFloatsPerWave * 4 + kPadBytes;
};

// AASR_PL_TRACE (experiment builds only, tools/pl_trace.py): where one workgroup's waves spend their cycles.  Every wave of
// workgroup AASR_PL_TRACE_BLOCK reads the shader clock (s_memtime) at the phase boundaries of its tile loop and sums the
// intervals: [0] H0 matrix phase, [1] close logic behind H0, [2] H1 matrix phase, [3] the tile barrier (wait + the next
// tile's copy issue; the lagging group passes it inside H0: its time is taken out of [0]), [4] fragment prefetch + close
// logic behind H1, [5] the part of [3] spent in s_barrier, [6] the part of [3] spent in s_waitcnt vmcnt(0), [7] whole kernel, [8] tiles, [9] / [10] of interval 4: the fragment prefetch, the close logic of block 0.  Reading the clock waits for every outstanding scalar and LDS
// operation, so the traced launch runs slower than the product kernel (the tool reports by how much).
#ifdef AASR_PL_TRACE_UNIT
// (AASR_PL_TRACE_UNIT and g_pl_trace are defined by the one unit that traces, in front of this header: gmm_score_f16x2.hip
// under an AASR_PL_TRACE build; the three-term unit compiles the kernel without the trace)
#ifndef AASR_PL_TRACE_BLOCK
#define AASR_PL_TRACE_BLOCK 300
#endif
#define PL_TRACE_DECL unsigned long long tr_tiles = 0, tr_sub[3] = {0, 0, 0}, tr_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tr_prev = __builtin_readcyclecounter(), tr_t0 = tr_prev, tr_bar = 0, tr_vm = 0
#define PL_TRACE(k) do { const unsigned long long tr_now = __builtin_readcyclecounter(); tr_acc[k] += tr_now - tr_prev; tr_prev = tr_now; } while (0)
#else
#define PL_TRACE_DECL
#define PL_TRACE(k)
#endif
// Issue priorities of the matrix phases (s_setprio; found with the phase trace above).  4-wave form: priority 1 inside a
// matrix phase, 0 in the close logic, so the wave's matrix instructions do not queue behind the other wave's vector, LDS
// and store instructions (-0.9 % on configs[2], priority 1 and 3 alike).  8-wave form: the two waves of a SIMD share the
// matrix pipe whenever their matrix phases overlap, and at equal priority the arbiter gives the older wave -- the leading
// group's -- two thirds of it: it ran ahead through its H1 and then waited ~1 200 cycles per tile at the barrier.  So the
// leading group takes priority 2 in H0 and 1 in H1, the lagging group the reverse, and both reach the barrier together:
// configs[1] 18.77 -> 18.14 ms.  Measured against it and lost (round 5): the reverse assignment 18.60, the lagging group
// higher throughout 19.3, priorities 1 / 0 18.44 (3 / 1 the same as 2 / 1).
// HYB (GROUPED, two terms, one pivot, unmasked; round 6): outlier routing without a merge pass.  The Gaussians the matrix
// layout left out (null rows) are summed per state by k_gmm_diag_score_centred BEFORE this launch, into a state-major
// buffer; a lane that closes such a state adds the buffer's value for its frame -- the arithmetic of k_outlier_merge,
// the same bits -- in front of the store.  The values are fetched a state ahead: per track parity a table says which state
// comes next and where its sums are; a state's two values (frames n, 32 + n) and the table entry of the state after it are
// requested when the previous one is consumed, so the close logic waits for global memory only where such states follow
// each other within a tile's time (the launcher leaves models where they are dense to the engine parts).  (k_outlier_merge's read-modify-write of one column of the score matrix
// touches a line per frame: 20 us per state and 449 280 frames, more than the gather of a model with engine parts from
// ~100 states on.)
template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS, bool PGF = false, bool HYB = false>
__global__ __launch_bounds__(WIDE ? 512 : 256, WIDE ? 1 : 2) void k_gmm_diag_score_pl(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ pivot,
    const uint16_t *__restrict__ apack, const int32_t *__restrict__ split_row,
    const uint16_t *__restrict__ close_mask, const int32_t *__restrict__ sid, int sid_stride,
    float *__restrict__ out, int64_t S, int64_t pitch, float ref_ln, int dbg, ClusterArgs cl,
    const u32x4 *__restrict__ fop, CutPlan plan, PivotGroups pg) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  typedef PlSmem<NK16, GROUPED, WIDE, NS> SM;
  // work item -> (frame block, row cut): the first n_main workgroups take the coarse cuts of the frame blocks that fill
  // whole rounds of the chip, the rest the fine cuts of the remaining blocks (pick_cut_plan); within either part the cut
  // is the slow index, so the workgroups resident at one time stream the same rows
  int blk, cut;
  if ((int)blockIdx.x < plan.n_main) {
    cut = (int)blockIdx.x / plan.blocks_main;
    blk = (int)blockIdx.x - cut * plan.blocks_main;
  } else {
    const int b = (int)blockIdx.x - plan.n_main;
    cut = b / plan.blocks_rem;
    blk = plan.blocks_main + (b - cut * plan.blocks_rem);
    split_row = plan.split_rem;
  }
  blk = __builtin_amdgcn_readfirstlane(blk);
  cut = __builtin_amdgcn_readfirstlane(cut);
  PL_TRACE_DECL;
  constexpr int OG = SM::OG;
  constexpr int kTileFloats = SM::kTileBytes / 4;
  constexpr int kOS = SM::kOutStride;
  constexpr int NW = WIDE ? 8 : 4;
  constexpr int NPROD = NS * (NS + 1) / 2;       // products kept per slab: 3 (f16x2), 6 (bf16x3)
  constexpr int MPH = NK16 * NPROD * 2;          // MFMAs per phase (one 32-row block, two frame blocks)
  float *abuf0 = (float *)smem_raw;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  constexpr int NBUF = SM::NBUF;
  float *ost = abuf0 + NBUF * kTileFloats + wave * SM::kOutFloatsPerWave;
  // A tile's rows into tile buffer `b`: the tile copy in the scalar-base form of the LDS-DMA instruction: the tile's address is wave-uniform, so the base goes
  // in a scalar register pair (two scalar additions per instruction) and the lanes carry ONE constant 32-bit offset,
  // 16 * lane, for the whole launch -- no 64-bit per-lane address to form and to send to the address unit per instruction
  // (against the generic per-lane pointers of issue_tile_copy_raw: configs[1] 17.94 -> 17.84 ms, configs[2] 10.42 ->
  // 10.38 ms per step, alternating runs on one box; two registers fewer).  (Round 5 also spread the copy
  // instructions over the slabs of the H0 that follows the barrier instead of issuing them behind it -- the barrier interval
  // of the phase trace fell from ~550 to ~260 cycles and H0 grew by as much: an LDS-DMA instruction costs the issuing wave
  // 100-150 cycles wherever it stands; 1 % slower with twelve more registers, removed.  The whole copy issued by the
  // leading group alone, whose close logic follows the barrier: +0.7 %, removed.)
  const unsigned lane_off16 = (unsigned)lane * 16u;
  auto issue_tile = [&](int64_t tile, int b) {
    constexpr int kChunks = kTileFloats / 4 / 64;   // 1 KB instructions per tile
    const char *gbase = (const char *)((const float *)apack + (size_t)tile * kTileFloats);
    const unsigned lbase = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(abuf0 + b * kTileFloats));
    // a wave takes CONSECUTIVE 1 KB pieces: one scalar base, one M0, the pieces told apart by the instruction's immediate
    // offset (it moves the global and the LDS address alike); against a base and an M0 per instruction: configs[1]
    // 17.91 -> 17.82 ms, three alternating runs on one box.  Tiles of more than 4 pieces per wave take a piece per round.
    constexpr int kRounds = (kChunks + NW - 1) / NW;
    if (kRounds <= 4) {
      const int w = __builtin_amdgcn_readfirstlane(wave);
      const int c0 = w * kRounds;   // pieces c0 .. c0 + kRounds - 1 (the last waves may run past the tile: guarded)
      const unsigned long long sb = (unsigned long long)(uintptr_t)gbase + (unsigned long long)c0 * 1024ull;
      const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)sb);
      const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(sb >> 32));
      const unsigned long long sbase = (unsigned long long)lo | ((unsigned long long)hi << 32);
      const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(lbase + (unsigned)c0 * 1024u));
      const int cnt = kChunks - c0 < kRounds ? kChunks - c0 : kRounds;   // wave-uniform
      // (one statement per count: M0 must hold between the instructions)
      if (cnt >= 4)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\tglobal_load_lds_dwordx4 %1, %2 offset:3072"
                     : : "s"(dst), "v"(lane_off16), "s"(sbase) : "memory", "m0");
      else if (cnt == 3)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048"
                     : : "s"(dst), "v"(lane_off16), "s"(sbase) : "memory", "m0");
      else if (cnt == 2)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024"
                     : : "s"(dst), "v"(lane_off16), "s"(sbase) : "memory", "m0");
      else if (cnt == 1)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(dst), "v"(lane_off16), "s"(sbase) : "memory", "m0");
    } else {
#pragma unroll
      for (int k = 0; k < kRounds; k++) {
        const int c = __builtin_amdgcn_readfirstlane(wave) + k * NW;   // wave-uniform
        if (c < kChunks) {
          const unsigned long long sb = (unsigned long long)(uintptr_t)gbase + (unsigned long long)c * 1024ull;
          const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)sb);
          const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(sb >> 32));
          const unsigned long long sbase = (unsigned long long)lo | ((unsigned long long)hi << 32);
          const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(lbase + (unsigned)c * 1024u));
          asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(dst), "v"(lane_off16), "s"(sbase) : "memory", "m0");
        }
      }
    }
  };
  // 8-wave form: waves 4-7 pass the tile's barrier in front of their H0 instead of at the end of H1, so they run
  // nearly a whole tile behind waves 0-3 -- the two waves of a SIMD then never sit in their close logic (or at
  // the barrier) at the same time, one of them always has MFMAs to issue.  Three tile buffers make the lag legal: the
  // copy of tile t + 2 is issued by every wave right behind its barrier t (all waves are past tile t - 1 there) and
  // has landed at barrier t + 1, before the lagging group's first read of it.
  // (The barrier in front of slab 0 / 1 / 2 of H0, configs[2], ms of the scoring stage on one box: 8.47 / 8.55 / 8.53.)
  const int group = WIDE ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;
  auto matrix_prio = [&](int phase) {   // see "Issue priorities" above the kernel
    if (WIDE) {
      if ((group == 1) == (phase == 1)) __builtin_amdgcn_s_setprio(2);
      else __builtin_amdgcn_s_setprio(1);
    } else {
      __builtin_amdgcn_s_setprio(1);
    }
  };
  const int n = lane & 31;
  const int h = lane >> 5;  // K half of a slab held by this lane AND its row track
  const int64_t f0 = (int64_t)blk * (NW * FRAMES_PER_WAVE) + wave * FRAMES_PER_WAVE;

  // The first two tiles are requested before anything else: they land while the frame operand is being built.
  const int64_t t_begin = split_row[4 * cut];
  const int64_t t_end = split_row[4 * cut + 4];
  if (t_begin < t_end) issue_tile(t_begin, 0);
  if (t_begin + 1 < t_end) issue_tile(t_begin + 1, 1);
  // pivot groups (multi-pivot layouts, gmm.h TrackLayout::n_pg): a row cut lies inside ONE group -- its rows are expanded
  // around that group's pivot, so the workgroup takes that group's image of the frame operand, and the group's columns end
  // at its own limit (its last line goes out partly filled, the next group starts on a whole line)
  int pgi = 0;
  if (pg.colend) {
    pgi = split_row[4 * cut + 3];
    if (!PGF) fop += (size_t)pgi * pg.fop_stride;
    S = pg.colend[pgi];
  }

  // ---- frame operand: lane (n, h) holds k = 16*j + 8*h + i, i < 8, of slab j -- split into its terms ONCE per launch by
  // k_frame_operand (below the kernel) and fetched here with 16-byte loads, 64 lanes x 16 B contiguous per instruction.
  // Built in place (one 4-byte load per K slot at a lane-dependent address, ~2 000 instructions) it cost every workgroup
  // ~20 us -- six tiles' time in front of every row cut, paid R times per frame.
  u32x4 bq[NK16][NS][2];
  if constexpr (PGF && NS == 2) {
    // multi-pivot layouts: the group's image is formed here, around the group's pivot (fop_unit_f16 = k_frame_operand's
    // arithmetic: the same bits), instead of being fetched -- one image per group and launch through HBM cost more than
    // the ~800 instructions a row cut pays for it
    const float *pv = pg.pivots + (size_t)pgi * dim;
    const float *tab = pg.tabs + (size_t)pgi * (3 * 8 * NK16);
#pragma unroll
    for (int nb = 0; nb < 2; nb++) {
      int64_t f = f0 + nb * 32 + n;
      if (f > F - 1) f = F - 1;
      const float *xr = frames + f * dim;
#pragma unroll
      for (int j = 0; j < NK16; j++) {
        unsigned w1[4], w2[4];
        fop_unit_f16(xr, dim, pv, tab, 8 * NK16, j, h, pg.sc, w1, w2);
        bq[j][0][nb] = u32x4{w1[0], w1[1], w1[2], w1[3]};
        bq[j][1][nb] = u32x4{w2[0], w2[1], w2[2], w2[3]};
      }
    }
  } else {
    const u32x4 *bw = fop + ((size_t)blk * NW + wave) * (NK16 * NS * 2 * 64) + lane;
#pragma unroll
    for (int j = 0; j < NK16; j++)
#pragma unroll
      for (int sp = 0; sp < NS; sp++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++) bq[j][sp][nb] = bw[((j * NS + sp) * 2 + nb) * 64];
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  PL_TRACE(6);
  float s0 = 0.0f, s1 = 0.0f;
  int closes = split_row[4 * cut + 1 + (GROUPED ? 0 : h)];
  // HYB: the next state of this lane's track that has outlier components, and its two values
  int hyb_st = 0x7fffffff;
  float hyb_v0 = LOG_TINY_F, hyb_v1 = LOG_TINY_F;
  uint32_t hyb_e_next = 0xffffu;   // the table entry of the state AFTER hyb_st (requested together with hyb_st's values)
  // ... whose values are requested BEHIND the next tile barrier, not where hyb_st is consumed: the barrier waits for every
  // outstanding vector-memory operation of the wave (the tile copy's), and a request issued in the close logic in front
  // of it made all eight waves wait for its latency (+13 % with such a state in every tenth column)
  uint32_t hyb_pend = 0xffffu;
  auto hyb_issue = [&](uint32_t e) {   // e: table entry of the state to take next (0xffff in the low half: none)
    hyb_st = 0x7fffffff;
    hyb_e_next = 0xffffu;
    if ((e & 0xffffu) != 0xffffu) {
      hyb_st = (int)(e & 0xffffu);
      const float *pr = pg.hyb_part + (int64_t)(e >> 16) * pg.hyb_pitch;
      const int64_t fa = f0 + n < F ? f0 + n : F - 1, fb = f0 + 32 + n < F ? f0 + 32 + n : F - 1;   // (never stored past F)
      hyb_v0 = pr[fa];
      hyb_v1 = pr[fb];
      if (hyb_st + 2 < (int)S) hyb_e_next = pg.hyb_tab[hyb_st + 2];
    }
  };
  if constexpr (HYB) {
    const int from = 2 * closes + h;   // the first state of this lane's track (parity h) in this row cut
    hyb_issue(from < (int)S ? pg.hyb_tab[from] : 0xffffu);
  }
  const int32_t *my_sid = sid + h * sid_stride;
  int next_sid = GROUPED ? 0 : my_sid[closes];
  float *orow0 = out + (f0 + n) * pitch;  // pitch: row stride of `out` in floats (>= S)
  float *orow1 = out + (f0 + 32 + n) * pitch;
  const bool ok0 = f0 + n < F, ok1 = f0 + 32 + n < F;
  const float floor_val = CL ? cl.floor_val : LOG_TINY_F;
  const unsigned long long *mrow =
      CL ? cl.maskrow + (size_t)(f0 >> 6) * cl.rows_padded + lane : nullptr;

  // a staged group of `cnt` (<= OG) columns from s_base on goes out: whole 16-byte pieces, 128 (64) bytes per frame row
  auto flush_group = [&](const int64_t s_base, const int cnt) {
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
  };

  // close logic of one 32-row block: P[nb][q] = this lane's sum of 2^x over quad q for frame block nb
  auto commit = [&](const float (&P)[2][4], unsigned nib) {
    if (AASR_DBG(128)) {   // ablation: no close logic
      asm volatile("" ::"v"(P[0][0]), "v"(P[0][1]), "v"(P[0][2]), "v"(P[0][3]), "v"(P[1][0]), "v"(P[1][1]), "v"(P[1][2]), "v"(P[1][3]));
      return;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      s0 += P[0][q];
      s1 += P[1][q];
      if ((nib >> q) & 1) {
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
          if constexpr (HYB) {
            const int stc = 2 * (pairs_closed - 1) + h;
            if ((hyb_pend & 0xffffu) != 0xffffu && stc == (int)(hyb_pend & 0xffffu)) {   // (closes before the barrier came)
              hyb_issue(hyb_pend);
              hyb_pend = 0xffffu;
            }
            if (stc == hyb_st) {
              // k_outlier_merge's arithmetic: out = log(exp(out) + exp(part)); a part AT the floor holds nothing (the
              // partial sums are floored at 1e-50 / |det|, outlier_part_floor: the floor applies after the bias)
              l0 = merge_floored_shares(l0, fmaxf(hyb_v0 + pg.hyb_bias, LOG_TINY_F));
              l1 = merge_floored_shares(l1, fmaxf(hyb_v1 + pg.hyb_bias, LOG_TINY_F));
              hyb_pend = hyb_e_next;
              hyb_st = 0x7fffffff;
            }
          }
          const int slot = ((2 * (pairs_closed - 1)) & (OG - 1)) + h;
          ost[n * kOS + slot] = l0;
          ost[(32 + n) * kOS + slot] = l1;
          const int64_t closed = 2 * (int64_t)pairs_closed < S ? 2 * (int64_t)pairs_closed : S;
          if (((2 * pairs_closed) & (OG - 1)) == 0 || 2 * (int64_t)pairs_closed >= S) {
            const int64_t s_base = ((closed - 1) / OG) * OG;
            flush_group(s_base, (int)(closed - s_base));
          }
        }
      }
    }
  };

  // element `k` (0..31) of a block's exponentials: frame block nb = k / 16, quad q, element e; the quad's four
  // values are summed pairwise as k_gmm_diag_score_bf16x3 does, (x0 + x1) + (x2 + x3)
  float t0 = 0.0f, t1 = 0.0f;
  auto epi_step = [&](int k, int mb, const f32x16 &c0, const f32x16 &c1, unsigned long long bits, float (&P)[2][4]) {
    const int nb = k >> 4, q = (k >> 2) & 3, e = k & 3;
    float v = nb ? c1[4 * q + e] : c0[4 * q + e];
    if (CL) v = mask_select(v, bits, 32 * nb + 8 * q + 4 * mb + e);  // k_cluster_expand's bit layout
    // pinned where it is written: left as a builtin the compiler sinks all 32 exponentials of a phase into the
    // close logic that consumes P, i.e. out from under the matrix stream (s_nop: a VALU read of a transcendental's
    // result needs one wait state, and the hazard recogniser does not look inside assembly)
    float x;
    if (AASR_DBG(64)) asm volatile("v_mov_b32 %0, %1" : "=v"(x) : "v"(v));   // ablation: no transcendentals
    else asm volatile("v_exp_f32 %0, %1\n\ts_nop 0" : "=v"(x) : "v"(v));
    // the pair sums ride in the stream as well (left to the compiler they gather behind the phase's last MFMA).
    // (Round 4: the additions run one element behind the exponentials, so that no instruction reads a transcendental's
    // result right behind it and the s_nop can go -- measured 1 % SLOWER, 8.60 against 8.51 ms on configs[2]; kept as is.)
    if (e == 0) t0 = x;
    else if (e == 1) asm volatile("v_add_f32 %0, %1, %2" : "=v"(t0) : "v"(t0), "v"(x));
    else if (e == 2) t1 = x;
    else {
      asm volatile("v_add_f32 %0, %1, %2" : "=v"(t1) : "v"(t1), "v"(x));
      asm volatile("v_add_f32 %0, %1, %2" : "=v"(P[nb][q]) : "v"(t0), "v"(t1));
    }
  };

  // one phase: the MFMAs of 32-row block MB of the tile in `acur` into (n0, n1), carrying the exponentials of the
  // other block's accumulators (o0, o1, selection bits obits) into P
  u32x4 afr[2][NS];  // A fragments [register set][split] of the block being accumulated
  auto load_frags = [&](const float *tile, int j, int mb, int set) {
    const u32x4 *afrag = (const u32x4 *)tile + lane;  // [slab][split][mb][64 lanes]
#pragma unroll
    for (int sp = NS - 1; sp >= 0; sp--) afr[set][sp] = afrag[((j * NS + sp) * 2 + mb) * 64];
  };

  int lane_zero = 0;
  asm volatile("" : "+v"(lane_zero));   // a zero the compiler cannot see through
  f32x16 cA0 = {0}, cA1 = {0}, cB0 = {0}, cB1 = {0};
  unsigned long long bits_cur = 0, bits_prev = 0;
  unsigned mask_cur = 0, mask_prev = 0;
  unsigned mask_v = 0;
  if (t_begin < t_end) {
    mask_cur = (unsigned)__builtin_amdgcn_readfirstlane((int)close_mask[t_begin]);
    if (CL) bits_cur = mrow[(size_t)t_begin * TILE_ROWS];
    load_frags(abuf0, 0, 0, 0);
  }
  int bi = 0;
  for (int64_t t = t_begin; t < t_end; t++) {
    float *acur = abuf0 + bi * kTileFloats;
    const int bn = bi + 1 < NBUF ? bi + 1 : 0, bnn = bn + 1 < NBUF ? bn + 1 : 0;
    float *anext = abuf0 + bn * kTileFloats;
    // tile t + 2 goes where tile t - 1 was (three buffers), or into tile t's own buffer when every wave is done
    // with it at the barrier (two buffers, no lagging group)
    // (Read by nothing since the side table of round 4's mixed layout went; with this copy of the index gone the register
    // allocator colours the loop's scalar registers differently -- the same instructions, other register numbers.  It
    // stays so that the kernels are byte for byte the ones that were measured.)
    const int bcur = bi;
    (void)bcur;
    bi = bn;
    // barrier t of this wave: its share of tile t + 1 has landed, and every wave is past tile t - 1
    auto tile_barrier = [&]() {
#ifdef AASR_PL_TRACE_UNIT
      const unsigned long long tb0 = __builtin_readcyclecounter();
#endif
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(mask_v) : : "memory");
#ifdef AASR_PL_TRACE_UNIT
      const unsigned long long tb1 = __builtin_readcyclecounter();
      tr_vm += tb1 - tb0;
#endif
      if (!AASR_DBG(16)) __builtin_amdgcn_s_barrier();
#ifdef AASR_PL_TRACE_UNIT
      const unsigned long long tb2 = __builtin_readcyclecounter();
      tr_acc[5] += tb2 - tb1;   // (the s_barrier itself; the tile count moves to the host side)
#endif
      if (t + 2 < t_end) issue_tile(t + 2, bnn);
      if constexpr (HYB) {
        if ((hyb_pend & 0xffffu) != 0xffffu) {
          hyb_issue(hyb_pend);
          hyb_pend = 0xffffu;
        }
      }
#ifdef AASR_PL_TRACE_UNIT
      tr_bar += __builtin_readcyclecounter() - tb0;
#endif
    };
    // close bits and selection bits of tile t+1: vector loads waited for by the vmcnt(0) in front of the barrier (an
    // aligned 32-bit word: the array has a spare element).  It has to stay a VECTOR load -- as a scalar load it would turn
    // every LDS wait of the stream into lgkmcnt(0) -- and it has to stay a load the COMPILER knows: the first version
    // issued it through inline assembly, and the compiler, for which the result was ready at the asm statement, copied
    // the register before the value had landed (one wave group's close bits were garbage in ~1 workgroup of 6 000 per
    // launch, found by the 10^6-frame test).  The opaque zero keeps the address a vector value.
    mask_v = ((const uint32_t *)close_mask)[((t + 1) >> 1) + lane_zero];
    unsigned long long bits_next = 0;
    if (CL && t + 1 < t_end) bits_next = mrow[(size_t)(t + 1) * TILE_ROWS];

    float P[2][4];
    PL_TRACE(4);  // (what ran since the end of the previous tile's H1: its barrier excluded below)
    matrix_prio(0);
    // ---------------- H0: block 0 of tile t  ||  exponentials of block 1 of tile t-1
    {
      int mi = 0;
#pragma unroll
      for (int j = 0; j < NK16; j++) {
        const int cur = j & 1;
        if (WIDE && j == 0) {
          if (group == 1) tile_barrier();
          __builtin_amdgcn_sched_barrier(0);
        }
        if (j + 1 < NK16) load_frags(acur, j + 1, 0, cur ^ 1);
        else load_frags(acur, 0, 1, cur ^ 1);     // slab 0 of block 1, for H1
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int grp = 0; grp < NS; grp++) {
          const int sp = NS - 1 - grp;
#pragma unroll
          for (int c = 0; c <= grp; c++) {
            const int sb = grp - c;
#pragma unroll
            for (int nb = 0; nb < 2; nb++) {
              if (j == 0 && grp == 0 && c == 0) {
                const f32x16 z = {0};
                if (nb == 0) cA0 = mfma_split<NS>(afr[cur][sp], bq[j][sb][0], z);
                else cA1 = mfma_split<NS>(afr[cur][sp], bq[j][sb][1], z);
              } else {
                if (nb == 0) cA0 = mfma_split<NS>(afr[cur][sp], bq[j][sb][0], cA0);
                else cA1 = mfma_split<NS>(afr[cur][sp], bq[j][sb][1], cA1);
              }
#pragma unroll
              for (int k = mi * 32 / MPH; k < (mi + 1) * 32 / MPH; k++) epi_step(k, 1, cB0, cB1, bits_prev, P);
              mi++;
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    PL_TRACE(0);
    if (t > t_begin) commit(P, (GROUPED ? mask_prev : (h ? mask_prev >> 8 : mask_prev)) >> 4 & 0xfu);
    PL_TRACE(1);
    matrix_prio(1);
    // ---------------- H1: block 1 of tile t  ||  exponentials of block 0 of tile t
    {
      int mi = 0;
      constexpr int set0 = NK16 & 1;   // the register set H0 left slab 0 of block 1 in
#pragma unroll
      for (int j = 0; j < NK16; j++) {
        const int cur = (j + set0) & 1;
        if (j + 1 < NK16) {
          load_frags(acur, j + 1, 1, cur ^ 1);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int grp = 0; grp < NS; grp++) {
          const int sp = NS - 1 - grp;
#pragma unroll
          for (int c = 0; c <= grp; c++) {
            const int sb = grp - c;
#pragma unroll
            for (int nb = 0; nb < 2; nb++) {
              if (j == 0 && grp == 0 && c == 0) {
                const f32x16 z = {0};
                if (nb == 0) cB0 = mfma_split<NS>(afr[cur][sp], bq[j][sb][0], z);
                else cB1 = mfma_split<NS>(afr[cur][sp], bq[j][sb][1], z);
              } else {
                if (nb == 0) cB0 = mfma_split<NS>(afr[cur][sp], bq[j][sb][0], cB0);
                else cB1 = mfma_split<NS>(afr[cur][sp], bq[j][sb][1], cB1);
              }
#pragma unroll
              for (int k = mi * 32 / MPH; k < (mi + 1) * 32 / MPH; k++) epi_step(k, 0, cA0, cA1, bits_cur, P);
              mi++;
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    PL_TRACE(2);
#ifdef AASR_PL_TRACE_UNIT
    tr_tiles++;
#endif
    // end of tile: the leading group's barrier
    if (!WIDE || group == 0) tile_barrier();
    else asm volatile("" : "+v"(mask_v));
#ifdef AASR_PL_TRACE_UNIT
    const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
    if (t + 1 < t_end) {
      load_frags(anext, 0, 0, 0);   // slab 0 of the next tile's block 0: in flight during the close logic
      __builtin_amdgcn_sched_barrier(0);
    }
#ifdef AASR_PL_TRACE_UNIT
    const unsigned long long ts1 = __builtin_readcyclecounter();
    tr_sub[0] += ts1 - ts0;   // fragment prefetch (issue)
#endif
    commit(P, (GROUPED ? mask_cur : (h ? mask_cur >> 8 : mask_cur)) & 0xfu);
#ifdef AASR_PL_TRACE_UNIT
    tr_sub[1] += __builtin_readcyclecounter() - ts1;   // close logic of block 0
#endif
    mask_prev = mask_cur;
    bits_prev = bits_cur;
    {
      const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane((int)mask_v);
      mask_cur = ((t + 1) & 1) ? w >> 16 : w & 0xffffu;
    }
    bits_cur = bits_next;
  }
  // drain: block 1 of the last tile
  if (t_begin < t_end) {
    float P[2][4];
#pragma unroll
    for (int k = 0; k < 32; k++) epi_step(k, 1, cB0, cB1, bits_prev, P);
    commit(P, (GROUPED ? mask_prev : (h ? mask_prev >> 8 : mask_prev)) >> 4 & 0xfu);
  }
#ifdef AASR_PL_TRACE_UNIT
  if ((int)blockIdx.x == AASR_PL_TRACE_BLOCK && lane == 0) {
    PL_TRACE(4);
    // the lagging group's barrier sits inside H0, the leading group's behind H1 (inside interval 4)
    if (WIDE && group == 1) tr_acc[0] -= tr_bar;
    else tr_acc[4] -= tr_bar;
    tr_acc[3] = tr_bar;
    tr_acc[6] = tr_vm;   // (of interval 3: the wait for the wave's own vector-memory operations, tile copy share and stores)
    tr_acc[7] = tr_prev - tr_t0;
    for (int k = 0; k < 8; k++) g_pl_trace[wave & 7][k] = tr_acc[k];
    g_pl_trace[wave & 7][8] = tr_tiles;
    g_pl_trace[wave & 7][9] = tr_sub[0];
    g_pl_trace[wave & 7][10] = tr_sub[1];
  }
#endif
}

// ---------------------------------------------------------------------------
// Frame operand of the split-term kernels, formed once per launch: for every block of 64 frames the K x 64 operand in
// the register layout of k_gmm_diag_score_pl -- [block][slab j][term][frame half nb][lane (n, h)] x 8 halves, K slot
// k = 16 j + 8 h + i -- so that a wave's prologue is NK16 * NS * 2 coalesced 16-byte loads.  Per value the arithmetic of
// the former in-kernel prologue: (x - pivot), the dimension's clamp and the column's power-of-two scale (f16x2), the
// square for odd k, 1 in the constant's slot(s), then the two fp16 / three bf16 terms.  Frames past the end repeat the
// last one (their results are never stored).  One thread per (frame, slab, K half).
// ---------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(256) void k_frame_operand(const float *__restrict__ frames, int64_t F, int dim,
                                                       const float *__restrict__ pivot, const float *__restrict__ f16tab,
                                                       int nk16, u32x4 *__restrict__ out, int64_t n_units, int n_pg,
                                                       int64_t pg_stride, int sc) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(tid & 63);
  const int64_t unit = tid >> 6;   // (block of 64 frames, frame half, slab)
  if (unit >= n_units) return;
  const int j = (int)(unit % nk16);
  const int nb = (int)((unit / nk16) & 1);
  const int64_t blk = unit / (2 * nk16);
  const int n = lane & 31, h = lane >> 5;
  const int KH = 8 * nk16;
  int64_t f = blk * 64 + nb * 32 + n;
  if (f > F - 1) f = F - 1;
  const float *xr = frames + f * dim;
  // the thread's 8 K slots are four (linear, quadratic) pairs: pair u = k / 2 is the constant's two slots for u = 0 and
  // dimension u - 1 otherwise (the K order at the top of the split-term kernels), so a thread handles 4 consecutive
  // dimensions d0 .. d0 + 3 (three and the constant in the first slab's first half).  Where they all exist the frame
  // components, pivots and clamps come as one 16-byte load each, the column scales as two (rows are 4-byte aligned; the
  // tables' loads are the same for every lane of a K half)
  // Slab-constant layout (sc, TrackLayout::sc): slab j = its constant's two slots, then dimensions 7 j .. 7 j + 6 -- the
  // first K half holds the constant and three dimensions, the second four.
  const int k0 = 16 * j + 8 * h;
  const int d0 = sc ? 7 * j + (h ? 3 : -1) : (k0 >> 1) - 1;
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  const bool whole = !sc && d0 >= 0 && d0 + 4 <= dim;   // uniform per K half
  float x[4];
  if (whole) {
    const f32x4u a = *(const f32x4u *)(xr + d0);
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = a[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = xr[d0 + i >= 0 && d0 + i < dim ? d0 + i : 0];
  }
  u32x4 *o = out + ((size_t)(blk * nk16 + j) * NS * 2 + nb) * 64 + lane;   // + term * 2 * 64
  // one image per pivot group (multi-pivot layouts; n_pg = 1 otherwise): the frame is read once
  for (int g = 0; g < n_pg; g++, pivot += dim, f16tab += (NS == 2 ? 3 * KH : 0), o += pg_stride) {
    float v[8];
    if (whole) {
      const f32x4u b = *(const f32x4u *)(pivot + d0);
      f32x4u c = {0, 0, 0, 0}, e0 = {1, 1, 1, 1}, e1 = {1, 1, 1, 1};
      if (NS == 2) {
        c = *(const f32x4u *)(f16tab + 2 * KH + d0);
        e0 = *(const f32x4u *)(f16tab + k0);
        e1 = *(const f32x4u *)(f16tab + k0 + 4);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float xc = x[i] - b[i];
        float xq = xc;
        if (NS == 2) xq = fminf(fmaxf(xc, -c[i]), c[i]);   // fp16 range: the dimension's clamp (pack_f16x2)
        float lin = xq, quad = xq * xq;
        if (NS == 2) {   // the columns' power-of-two scales (the rows carry their inverses): exact
          lin *= i < 2 ? e0[2 * i] : e1[2 * i - 4];
          quad *= i < 2 ? e0[2 * i + 1] : e1[2 * i - 3];
        }
        v[2 * i] = lin;
        v[2 * i + 1] = quad;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int k = k0 + i;
        // (the constant's slots: the first two of the plain layout, the first two of every slab of the slab-constant one)
        const int d = (sc ? (h == 0 && i < 2) : k < 2) ? -1 : d0 + (i >> 1);
        const int dc = d >= 0 && d < dim ? d : 0;
        const float xc = x[i >> 1] - pivot[dc];
        float xq = xc;
        if (NS == 2) {  // fp16 range: the dimension's clamp (see the f16x2 note in gmm_score_common.h and pack_f16x2)
          const float lim = f16tab[2 * KH + dc];
          xq = fminf(fmaxf(xc, -lim), lim);
        }
        float val = (k & 1) ? xq * xq : xq;
        if (d < 0) val = (k == 0 || NS == 2) ? 1.0f : 0.0f;   // the constant and (f16x2) its remainder
        else if (d >= dim) val = 0.0f;
        if (NS == 2) val *= f16tab[k];   // the column's power-of-two scale (the rows carry its inverse): exact
        v[i] = val;
      }
    }
    if constexpr (NS == 3) {
      unsigned w1[4], w2[4], w3[4];
#pragma unroll
      for (int i = 0; i < 4; i++) split3_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i], w3[i]);
      o[0] = u32x4{w1[0], w1[1], w1[2], w1[3]};
      o[2 * 64] = u32x4{w2[0], w2[1], w2[2], w2[3]};
      o[4 * 64] = u32x4{w3[0], w3[1], w3[2], w3[3]};
    } else {
      // (the unit's arithmetic lives in fop_unit_f16, shared with the kernels that form their operand themselves; `v`
      // above is the three-term form's)
      unsigned w1[4], w2[4];
      fop_unit_f16(xr, dim, pivot, f16tab, KH, j, h, sc, w1, w2);
      o[0] = u32x4{w1[0], w1[1], w1[2], w1[3]};
      o[2 * 64] = u32x4{w2[0], w2[1], w2[2], w2[3]};
    }
  }
}

// frame operand of `blocks64` blocks of 64 frames into the handle's scratch (grown as needed)
template <int NS>
static const u32x4 *frame_operand(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                                  int64_t blocks64, hipStream_t stream, int64_t *pg_stride) {
  const size_t per_block = (size_t)L.nk16 * NS * 2 * 64;   // u32x4 per 64 frames
  const int n_pg = L.n_pg > 1 ? L.n_pg : 1;
  const size_t image = (size_t)blocks64 * per_block;       // u32x4 per pivot group
  if (image * n_pg * 4 > g->fop_scratch.n) {
    AASR_HIP(hipDeviceSynchronize());   // growing frees the old buffer
    g->fop_scratch.ensure(image * n_pg * 4);
  }
  const int64_t n_units = blocks64 * 2 * L.nk16;
  hipLaunchKernelGGL(k_frame_operand<NS>, dim3((unsigned)((n_units * 64 + 255) / 256)), dim3(256), 0, stream, d_frames, F,
                     g->dim, L.n_pg > 1 ? L.pg_pivot.p : g->d_pivot.p,
                     NS == 2 ? (L.n_pg > 1 ? L.pg_tab.p : L.f16tab.p) : nullptr, L.nk16, (u32x4 *)g->fop_scratch.p, n_units,
                     n_pg, (int64_t)image, (NS == 2 && L.sc) ? 1 : 0);
  AASR_HIP(hipGetLastError());
  *pg_stride = (int64_t)image;
  return (const u32x4 *)g->fop_scratch.p;
}

// Two-level plan: the workgroups of a launch run in rounds of `slots`, and a uniform R leaves the last round partly
// empty (configs[2]: 878 blocks x 2 cuts = 6.86 rounds of 256).  So the frame blocks that fill whole rounds at a coarse
// cut count go first, and the remaining blocks are cut finer so that THEIR last round is nearly full too: configs[2]
// 768 blocks x 2 cuts (6 rounds) + 110 blocks x 16 cuts (6.9 short rounds) instead of 7 long ones.  Same cost model as
// pick_row_cuts; falls back to the uniform plan when that is no better.
static CutPlan pick_cut_plan(int64_t blocks, double slots_d, int64_t tiles, int max_splits, double overhead,
                             const int32_t *splits_base, int min_splits = 1, int split_cap = TRACK_MAX_SPLITS) {
  static const int force_r = AASR_EXPERIMENT_ENV("AASR_SPLITS") ? atoi(AASR_EXPERIMENT_ENV("AASR_SPLITS")) : 0;
  static const double force_c = AASR_EXPERIMENT_ENV("AASR_CUT_OVERHEAD") ? atof(AASR_EXPERIMENT_ENV("AASR_CUT_OVERHEAD")) : -1.0;
  static const int two_level = AASR_EXPERIMENT_ENV("AASR_TWO_LEVEL") ? atoi(AASR_EXPERIMENT_ENV("AASR_TWO_LEVEL")) : 1;
  if (force_c >= 0) overhead = force_c;
  const int64_t slots = (int64_t)slots_d;
  CutPlan best;
  double best_cost = 1e300;
  auto row = [&](int r) { return splits_base + (size_t)(r - 1) * (split_cap + 1) * 4; };
  for (int r1 = min_splits; r1 <= max_splits; r1++) {   // (multi-pivot layouts: every pivot group is at least one cut)
    if (force_r >= min_splits && force_r <= max_splits && r1 != force_r) continue;
    // uniform
    const double uni = std::ceil((double)blocks * r1 / slots_d) * ((double)tiles / r1 + overhead);
    if (uni < best_cost * 0.999) {
      best_cost = uni;
      best = CutPlan();
      best.n_main = (int)(blocks * r1);
      best.blocks_main = (int)blocks;
      best.r_main = r1;
    }
    if (!two_level || (force_r >= 1 && force_r <= max_splits)) continue;
    // whole rounds at r1, the rest at r2
    const int64_t rounds = blocks * r1 / slots;
    if (rounds < 1 || (rounds * slots) % r1 != 0) continue;
    const int64_t bm = rounds * slots / r1;
    const int64_t rem = blocks - bm;
    if (rem <= 0) continue;
    for (int r2 = r1 + 1; r2 <= max_splits; r2++) {
      const double cost = (double)rounds * ((double)tiles / r1 + overhead) +
                          std::ceil((double)rem * r2 / slots_d) * ((double)tiles / r2 + overhead);
      if (cost < best_cost * 0.995) {
        best_cost = cost;
        best.n_main = (int)(bm * r1);
        best.blocks_main = (int)bm;
        best.blocks_rem = (int)rem;
        best.r_main = r1;
        best.r_rem = r2;
        best.split_rem = row(r2);
      }
    }
  }
  return best;
}

// the wave-group kernel's launcher (gmm_score_bf16x3.hip): three terms beyond five slabs, never instantiated with NS = 2
template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS>
static void launch_bf16_t(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                          float *d_out, hipStream_t stream, const ClusterArgs &cl, int64_t pitch);

// The three-term bf16 arithmetic on the pipelined kernel as well, up to 39 dimensions (five slabs: with six the 8-wave
// instance spills).  Round 3 measured it SLOWER there than on the wave-group kernel (33.2 against 32.4 ms per 10^6 frames);
// with the wave groups' priorities crossed per phase it is the faster one: 31.08 against 31.65 ms, two alternating runs
// on one box.  Six and eight slabs stay on k_gmm_diag_score_bf16x3.
// One launch of instance <..., PGF, HYB> of the pipelined kernel under `plan`: the dynamic LDS size is registered once per
// device and instance; `fop` / `pg` are what tells the three forms apart (launch_pl_t).
template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS, bool PGF, bool HYB>
static void launch_pl_instance(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, float *d_out,
                               hipStream_t stream, const ClusterArgs &cl, int64_t pitch, const u32x4 *fop,
                               const CutPlan &plan, const PivotGroups &pg) {
  constexpr int NW = WIDE ? 8 : 4;
  const int smem = PlSmem<NK16, GROUPED, WIDE, NS>::kBytes;
  static const int dbg = AASR_EXPERIMENT_ENV("AASR_DBG") ? atoi(AASR_EXPERIMENT_ENV("AASR_DBG")) : 0;
  static bool attr_set[64] = {false};
  auto kern = k_gmm_diag_score_pl<NK16, GROUPED, CL, WIDE, NS, PGF, HYB>;
  if (!attr_set[g->device & 63]) {
    AASR_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set[g->device & 63] = true;
  }
  const int32_t *split_row = L.splits.p + (size_t)(plan.r_main - 1) * (L.split_cap + 1) * 4;
  const unsigned n_items = (unsigned)(plan.n_main + (plan.r_rem ? plan.blocks_rem * plan.r_rem : 0));
  hipLaunchKernelGGL(kern, dim3(n_items), dim3(NW * 64), smem, stream, d_frames, F,
                     g->dim, g->d_pivot.p, NS == 3 ? L.a16.p : L.a16h.p, split_row, L.close.p, L.sid.p, L.sid_stride,
                     d_out, g->S, pitch, L.ref_ln - (float)g->out_bias_ln, dbg, cl, fop, plan, pg);
  AASR_HIP(hipGetLastError());
}

template <int NK16, bool GROUPED, bool CL, bool WIDE, int NS>
static void launch_pl_t(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                        float *d_out, hipStream_t stream, const ClusterArgs &cl, int64_t pitch) {
  constexpr int NW = WIDE ? 8 : 4;
  const int64_t blocks = (F + NW * FRAMES_PER_WAVE - 1) / (NW * FRAMES_PER_WAVE);
  const bool multi = L.n_pg > 1;   // pivot groups: every group at least one cut, its own frame operand
  const CutPlan plan = pick_cut_plan(blocks, (WIDE ? 1.0 : 2.0) * (g->num_cus > 0 ? g->num_cus : 256),
                                     L.rows_padded / TILE_ROWS, L.max_splits, 3.0, L.splits.p, multi ? L.n_pg : 1, L.split_cap);
  PivotGroups pg;
  if constexpr (GROUPED && NS == 2) {
    // multi-pivot layouts: the workgroups form their group's frame operand themselves (no k_frame_operand launch)
    static const int pgf_env = AASR_EXPERIMENT_ENV("AASR_PGF") ? atoi(AASR_EXPERIMENT_ENV("AASR_PGF")) : 1;   // EXPERIMENT: 0 = images through HBM
    if (multi && pgf_env && L.pg_tab.p) {
      pg.colend = L.pg_colend.p;
      pg.pivots = L.pg_pivot.p;
      pg.tabs = L.pg_tab.p;
      pg.sc = L.sc ? 1 : 0;
      launch_pl_instance<NK16, GROUPED, CL, WIDE, NS, true, false>(g, L, d_frames, F, d_out, stream, cl, pitch, nullptr, plan, pg);
      return;
    }
  }
  const u32x4 *fop = nullptr;
  const aasr_gmm::FopAhead &ah = g->fop_ahead;
  if (!multi && ah.frames && ah.ns == NS && d_frames >= ah.frames) {
    // an operand formed ahead (form_frame_operand below) that covers this call's frames from a 512-frame boundary on: its
    // image is whole 512-frame blocks, so the blocks of either wave form that begin there lie inside it
    const int64_t off = d_frames - ah.frames, unit = (int64_t)512 * g->dim;
    if (off % unit == 0 && off / g->dim + F <= ah.F) {
      fop = (const u32x4 *)g->fop_scratch.p + (size_t)(off / g->dim / 64) * ((size_t)L.nk16 * NS * 2 * 64);
      pg.fop_stride = ah.stride;
    }
  }
  if (!fop) {
    g->fop_ahead = aasr_gmm::FopAhead();   // (the launch below rewrites the scratch an operand formed ahead lives in)
    fop = frame_operand<NS>(g, L, d_frames, F, blocks * NW, stream, &pg.fop_stride);
  }
  if (multi) pg.colend = L.pg_colend.p;
  if constexpr (GROUPED && NS == 2 && !CL) {
    // outlier routing with the merge in the close logic: the launcher has put the outliers' partial sums on the handle
    if (!multi && g->hyb_fuse.part && g->hyb_tab.p) {
      pg.hyb_tab = g->hyb_tab.p;
      pg.hyb_part = g->hyb_fuse.part;
      pg.hyb_pitch = g->hyb_fuse.pitch;
      pg.hyb_bias = (float)g->out_bias_ln;
      g->hyb_fuse.used = true;   // (the callers run the merge pass where no launch took the partial sums)
      g->hyb_fused_launches++;
      launch_pl_instance<NK16, GROUPED, CL, WIDE, NS, false, true>(g, L, d_frames, F, d_out, stream, cl, pitch, fop, plan, pg);
      return;
    }
  }
  launch_pl_instance<NK16, GROUPED, CL, WIDE, NS, false, false>(g, L, d_frames, F, d_out, stream, cl, pitch, fop, plan, pg);
}

// the 8-wave form needs three tile buffers + eight staging areas in 160 KB of LDS
template <int N, int NS>
static constexpr bool wide_ok() {
  if (NS == 2) return PlSmem<N, true, true, NS>::kBytes <= 160 * 1024;
  // (three terms: the wave-group kernel, or -- multi-pivot layouts -- the pipelined one: room for either)
  return 3 * Bf16Smem<N, true, true, NS>::kTileBytes + 8 * Bf16Smem<N, true, true, NS>::kOutFloatsPerWave * 4 <= 160 * 1024 &&
         PlSmem<N, true, true, NS>::kBytes <= 160 * 1024;
}

// One instance choice of launch_split: NS = 2 and three terms up to five slabs on the software-pipelined kernel, three
// terms beyond on the wave-group kernel -- or, on a multi-pivot layout (grouped by construction), on the pipelined one,
// which takes the groups' operand images
template <int N, int NS, bool GR, bool CLF, bool WD>
static void launch_split_instance(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, float *d_out,
                                  hipStream_t stream, const ClusterArgs &cl, int64_t pitch) {
  if constexpr (NS == 2 || N <= 5)
    launch_pl_t<N, GR, CLF, WD, NS>(g, L, d_frames, F, d_out, stream, cl, pitch);
  else if (L.n_pg > 1) {
    if constexpr (GR) launch_pl_t<N, true, CLF, WD, NS>(g, L, d_frames, F, d_out, stream, cl, pitch);
  } else
    launch_bf16_t<N, GR, CLF, WD, NS>(g, L, d_frames, F, d_out, stream, cl, pitch);
}

// GROUPED from the layout
template <int N, int NS, bool CLF, bool WD>
static void launch_split_tracks(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, float *d_out,
                                hipStream_t stream, const ClusterArgs &cl, int64_t pitch) {
  if (L.grouped) launch_split_instance<N, NS, true, CLF, WD>(g, L, d_frames, F, d_out, stream, cl, pitch);
  else launch_split_instance<N, NS, false, CLF, WD>(g, L, d_frames, F, d_out, stream, cl, pitch);
}

// CL from the masks, WIDE from the batch size and the LDS budget
template <int N, int NS>
static void launch_split_n(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, float *d_out,
                           hipStream_t stream, const ClusterArgs *cl, int64_t pitch, bool wide) {
  const ClusterArgs none;
  if (cl && NS == 2 && wide && wide_ok<N, NS>()) {
    // masked (clustered) runs: the bf16x3 8-wave form with masks needs 254 VGPRs + spills and was measured slower, so it
    // keeps 4-wave workgroups; the f16x2 kernel has the registers
    if constexpr (NS == 2) launch_split_tracks<N, NS, true, true>(g, L, d_frames, F, d_out, stream, *cl, pitch);
  } else if (cl) {
    launch_split_tracks<N, NS, true, false>(g, L, d_frames, F, d_out, stream, *cl, pitch);
  } else if (wide && wide_ok<N, NS>()) {
    launch_split_tracks<N, NS, false, true>(g, L, d_frames, F, d_out, stream, none, pitch);
  } else {
    launch_split_tracks<N, NS, false, false>(g, L, d_frames, F, d_out, stream, none, pitch);
  }
}

// The frame operand of F frames of a one-pivot layout, formed ahead of the scoring calls that use it (launch_pl_t takes it
// for calls inside the range): whole 512-frame blocks, which covers the blocks of the 8-wave and of the 4-wave form.
template <int NS>
void form_frame_operand(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, hipStream_t stream) {
  g->fop_ahead = aasr_gmm::FopAhead();
  if (F <= 0 || L.n_pg > 1) return;
  int64_t stride = 0;
  frame_operand<NS>(g, L, d_frames, F, (F + 511) / 512 * 8, stream, &stride);
  g->fop_ahead.frames = d_frames;
  g->fop_ahead.F = F;
  g->fop_ahead.stride = stride;
  g->fop_ahead.ns = NS;
}

// NS = 3: three bf16 terms (AASR_PREC_BF16X3); NS = 2: two fp16 terms (AASR_PREC_F16X2)
template <int NS>
bool launch_split(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                  float *d_out, hipStream_t stream, const ClusterArgs *cl, int64_t pitch) {
  if (pitch <= 0) pitch = g->S;
  if (NS == 3 ? !L.a16.p : !L.a16h.p) return false;
  // AASR_BF16_WIDE=0 selects the 4-wave workgroups
  static const int wide_env = AASR_EXPERIMENT_ENV("AASR_BF16_WIDE") ? atoi(AASR_EXPERIMENT_ENV("AASR_BF16_WIDE")) : -1;
  // small batches (a decoder's per-utterance blocks) fill the chip better with 256-frame workgroups
  const bool wide = (wide_env >= 0 ? wide_env : (F >= 8192 ? 1 : 0)) != 0;
  switch (L.nk16) {
    case 1: launch_split_n<1, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 2: launch_split_n<2, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 3: launch_split_n<3, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 4: launch_split_n<4, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 5: launch_split_n<5, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 6: launch_split_n<6, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    case 8: launch_split_n<8, NS>(g, L, d_frames, F, d_out, stream, cl, pitch, wide); return true;
    default: return false;
  }
}

}  // namespace aasr

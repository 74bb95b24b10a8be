// gmm_score_f32.hip -- the f32 MFMA scoring kernels (the map of the files: gmm_score.hip):
//   k_gmm_diag_score           LDS-staged epilogue: any layout (diagnostic) and the per-Gaussian view; launch_diag
//   k_gmm_diag_score_tracks    AASR_PREC_F32: track layouts, in-register epilogue; launch_tracks
#include "gmm_score_common.h"

namespace aasr {

// finished state log-likelihoods are buffered per wave and written OUT_GROUP
// consecutive states at a time: 32 contiguous bytes per frame row
constexpr int OUT_GROUP = 8;

template <int NKK>
struct ScoreSmem {
  // [2 buffers][NKK/2][64 lanes][4] floats
  static constexpr int kTileFloats = (NKK / 2) * 64 * 4;
  static constexpr int kStageFloatsPerWave = CHUNK_ROWS * FRAMES_PER_WAVE;
  // per-wave output transposition buffer: OUT_GROUP finished states x 64 frames
  static constexpr int kOutFloatsPerWave = OUT_GROUP * FRAMES_PER_WAVE;
  static constexpr int kBytes =
      (2 * kTileFloats + WAVES_PER_BLOCK * (kStageFloatsPerWave + kOutFloatsPerWave)) * 4;
};

// Reduce rows [a, b) of the staged chunk for this lane's frame, 16 rows at a
// time, merging into the running (m, s) pair:  sum_r 2^v_r = s * 2^m.
__device__ __forceinline__ void reduce_rows(const float *stage_col, int a, int b,
                                            float &m, float &s) {
  for (int r0 = a; r0 < b; r0 += 16) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      int r = r0 + i;
      int rc = r < b ? r : b - 1;
      float x = stage_col[rc * FRAMES_PER_WAVE];
      v[i] = r < b ? x : NEG_BIG_F;
    }
    float gm = v[0];
#pragma unroll
    for (int i = 1; i < 16; i++) gm = fmaxf(gm, v[i]);
    float mn = fmaxf(m, gm);
    float acc = s * __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
    for (int i = 0; i < 16; i++) acc += __builtin_amdgcn_exp2f(v[i] - mn);
    m = mn;
    s = acc;
  }
}

// MODE 0: per-state mixture log-likelihoods (segmented log-sum-exp)
// MODE 1: raw per-row log-likelihoods (pool view), out[f][row]
template <int NKK, int MODE>
__global__ __launch_bounds__(256, 2) void k_gmm_diag_score(
    const float *__restrict__ frames, int64_t F, int dim,
    const float *__restrict__ pivot, const float *__restrict__ apack,
    int64_t tiles, const int32_t *__restrict__ chunk_seg_begin,
    const uint32_t *__restrict__ seg_desc, const int32_t *__restrict__ seg_out,
    float *__restrict__ out, int64_t out_cols, int64_t rows, int dbg) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *smem = (float *)smem_raw;
  constexpr int kTileFloats = ScoreSmem<NKK>::kTileFloats;
  float *abuf0 = smem;
  float *abuf1 = smem + kTileFloats;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  float *stage = smem + 2 * kTileFloats + wave * ScoreSmem<NKK>::kStageFloatsPerWave;

  const int n = lane & 31;   // MFMA column (frame within a 32-block)
  const int h = lane >> 5;   // K parity held by this lane
  const int64_t f0 = (int64_t)blockIdx.x * FRAMES_PER_BLOCK + wave * FRAMES_PER_WAVE;

  // ---- frame operand: B[kk][nb] = h ? x'^2 : x'  (kk<dim), 1 at kk==dim/h==0
  float bf[NKK][2];
#pragma unroll
  for (int nb = 0; nb < 2; nb++) {
    int64_t f = f0 + nb * 32 + n;
    if (f > F - 1) f = F - 1;
    const float *xr = frames + f * dim;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) {
      const int kc = kk < dim ? kk : 0;
      const float xc = xr[kc] - pivot[kc];
      float v = h ? xc * xc : xc;
      if (kk == dim) v = h ? 0.0f : 1.0f;
      if (kk > dim) v = 0.0f;
      bf[kk][nb] = v;
    }
  }

  float carry_m = NEG_BIG_F, carry_s = 0.0f;
  float *ost = smem + 2 * kTileFloats + WAVES_PER_BLOCK * ScoreSmem<NKK>::kStageFloatsPerWave +
               wave * ScoreSmem<NKK>::kOutFloatsPerWave;
  int n_closed = 0;  // states finished so far == index of the next state (MODE 0)

  // prologue: tile 0 -> buffer 0
  issue_tile_copy(apack, abuf0, kTileFloats, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int64_t my_frame = f0 + lane;  // epilogue: lane <-> frame
  const bool frame_ok = my_frame < F;

  for (int64_t t = 0; t < tiles; t++) {
    float *acur = (t & 1) ? abuf1 : abuf0;
    float *anext = (t & 1) ? abuf0 : abuf1;
    // Buffer `anext` was last read by the MFMA loop of tile t-1; every wave is
    // past the barrier that followed that loop, so it can be refilled now.
    if (t + 1 < tiles)
      issue_tile_copy(apack + (size_t)(t + 1) * kTileFloats, anext, kTileFloats, wave, lane);

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const f32x4 *afrag = (const f32x4 *)acur + lane;
    // A fragments are fetched two kk-pairs ahead of their MFMAs
    f32x4 a0 = afrag[0];
    f32x4 a1 = afrag[(NKK / 2 > 1 ? 1 : 0) * 64];
#pragma unroll
    for (int q = 0; q < NKK / 2; q++) {
      const int qn = (q + 2 < NKK / 2) ? q + 2 : NKK / 2 - 1;
      f32x4 a2 = afrag[qn * 64];
      const f32x4 av = a0;  // {mb0 kk0, mb0 kk1, mb1 kk0, mb1 kk1}
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bf[2 * q][0], c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bf[2 * q][1], c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bf[2 * q][0], c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bf[2 * q][1], c11, 0, 0, 0);
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bf[2 * q + 1][0], c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bf[2 * q + 1][1], c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bf[2 * q + 1][0], c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bf[2 * q + 1][1], c11, 0, 0, 0);
      a0 = a1;
      a1 = a2;
    }

    // One barrier per tile, here: (a) every wave has finished reading `acur`,
    // (b) every wave's share of tile t+1 has landed (the global_load_lds were
    // issued before this tile's MFMAs; the only other outstanding vector-memory
    // ops are the previous tile's output stores, long retired).  The epilogue
    // below then runs without any inter-wave synchronisation and its stores
    // stay in flight across the next MFMA phase.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    if (AASR_DBG(1)) {  // ablation: MFMA only (keep the accumulators live)
      asm volatile("" ::"v"(c00), "v"(c01), "v"(c10), "v"(c11));
      continue;
    }
    // ---- epilogue, one 32-row chunk at a time
#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
      const f32x16 &ca = mb ? c10 : c00;
      const f32x16 &cb = mb ? c11 : c01;
      // C layout: lane (n,h), reg i -> row 8*(i/4) + 4*h + (i%4), col n
#pragma unroll
      for (int i = 0; i < 16; i++) {
        int row = 8 * (i >> 2) + 4 * h + (i & 3);
        stage[row * FRAMES_PER_WAVE + n] = ca[i];
        stage[row * FRAMES_PER_WAVE + 32 + n] = cb[i];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const float *col = stage + lane;
      const int64_t chunk = t * 2 + mb;
      if (MODE == 0) {
        const int sb = chunk_seg_begin[chunk];
        const int se = chunk_seg_begin[chunk + 1];
        for (int si = sb; si < se; si++) {
          const uint32_t d = seg_desc[si];
          const int a = d & 0xff, b = (d >> 8) & 0xff;
          const bool cont = (d >> 16) & 1, open = (d >> 17) & 1;
          float m = cont ? carry_m : NEG_BIG_F;
          float s = cont ? carry_s : 0.0f;
          reduce_rows(col, a, b, m, s);
          if (open) {
            carry_m = m;
            carry_s = s;
          } else {
            float lg = __builtin_amdgcn_logf(s);  // log2
            float ll = fmaf(m, LN2_F, lg * LN2_F);
            ll = fmaxf(ll, LOG_TINY_F);
            // states close in index order: buffer [frame][k], k = n_closed % 8
            const int k = n_closed & (OUT_GROUP - 1);
            ost[lane * OUT_GROUP + k] = ll;
            n_closed++;
            if ((n_closed & (OUT_GROUP - 1)) == 0 || n_closed == (int)out_cols) {
              const int cnt = ((n_closed - 1) & (OUT_GROUP - 1)) + 1;
              const int s_base = n_closed - cnt;
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              const int kk2 = lane & (OUT_GROUP - 1);
#pragma unroll
              for (int i = 0; i < FRAMES_PER_WAVE / (64 / OUT_GROUP); i++) {
                const int j = i * (64 / OUT_GROUP) + (lane / OUT_GROUP);
                const float v = ost[j * OUT_GROUP + kk2];
                if (kk2 < cnt && f0 + j < F) out[(f0 + j) * out_cols + s_base + kk2] = v;
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
            }
          }
        }
      } else {
        const int64_t rbase = chunk * CHUNK_ROWS;
        if (frame_ok) {
          for (int r = 0; r < CHUNK_ROWS; r++) {
            if (rbase + r < rows)
              out[my_frame * out_cols + rbase + r] = col[r * FRAMES_PER_WAVE] * LN2_F;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int NKK, int MODE>
static void launch_t(const aasr_gmm *g, const PackedRows &pr, const float *d_frames,
                     int64_t F, float *d_out, int64_t out_cols, hipStream_t stream) {
  if (F <= 0) return;
  const int64_t blocks = (F + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  int smem = ScoreSmem<NKK>::kBytes;
  static const int dbg = AASR_EXPERIMENT_ENV("AASR_DBG") ? atoi(AASR_EXPERIMENT_ENV("AASR_DBG")) : 0;
  if (dbg & 2) smem = 100 * 1024;  // ablation: one workgroup per CU
  static bool attr_set[64] = {false};
  auto kern = k_gmm_diag_score<NKK, MODE>;
  if (!attr_set[g->device & 63]) {
    AASR_HIP(hipFuncSetAttribute((const void *)kern,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set[g->device & 63] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), smem, stream, d_frames, F,
                     g->dim, g->d_pivot.p, pr.a.p, pr.tiles, pr.chunk_seg_begin.p,
                     pr.seg_desc.p, pr.seg_out.p, d_out, out_cols, pr.rows, dbg);
  AASR_HIP(hipGetLastError());
}

template <int MODE>
void launch_diag(const aasr_gmm *g, const PackedRows &pr, const float *d_frames,
                 int64_t F, float *d_out, int64_t out_cols, hipStream_t stream) {
  switch (pr.nkk) {
#define AASR_CASE(N)                                                    \
  case N:                                                               \
    launch_t<N, MODE>(g, pr, d_frames, F, d_out, out_cols, stream);     \
    return;
    AASR_CASE(8) AASR_CASE(14) AASR_CASE(20) AASR_CASE(26) AASR_CASE(32) AASR_CASE(40)
    AASR_CASE(48) AASR_CASE(64)
#undef AASR_CASE
    default:
      break;
  }
  raise(AASR_ERR_UNSUPPORTED, "no kernel instance for K/2 = %d", pr.nkk);
}
template void launch_diag<0>(const aasr_gmm *, const PackedRows &, const float *, int64_t, float *, int64_t, hipStream_t);
template void launch_diag<1>(const aasr_gmm *, const PackedRows &, const float *, int64_t, float *, int64_t, hipStream_t);

// Diagnostic (not part of the public ABI): resident workgroups per CU the
// runtime predicts for the NKK=40 scoring kernel.
extern "C" int aasr_debug_score_occupancy(void) {
  int nb = -1;
  auto kern = k_gmm_diag_score<40, 0>;
  (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            ScoreSmem<40>::kBytes);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, 256,
                                                   ScoreSmem<40>::kBytes) != hipSuccess)
    return -1;
  return nb;
}

// ---------------------------------------------------------------------------
// Track layouts: in-register epilogue (see gmm_build_tracks()).
//
// The host lays every state on one of the two row tracks that lane halves
// h = 0 / 1 hold in their accumulator registers and folds a fixed reference
// 2^ref into the constants, so the epilogue is 16 v_exp_f32 + 16 adds per
// accumulator block with no LDS round trip, no running maximum and one 16-bit
// close mask per tile.  On gfx950 the f32 MFMA executes on the same lanes as
// the VALU (SQ_VALU_MFMA_COEXEC_CYCLES = 0), so every VALU instruction removed
// from the epilogue is matrix time won back.
//   GROUPED: states 2j/2j+1 finish together; results are transposed through a
//            wave-private LDS buffer and written 32 consecutive states (128 B)
//            per frame row with 16-byte stores.
//   !GROUPED: the tracks close states independently; results are stored per
//            state (4-byte scatter, one store instruction per 32 frames).
// The row range can be cut (blockIdx.y) so that the grid has no tail round.
// ---------------------------------------------------------------------------
template <int NKK, bool GROUPED>
struct TrackSmem {
  static constexpr int OG = TRACK_OUT_GROUP;
  static constexpr int kTileFloats = (NKK / 2) * 64 * 4;
  static constexpr int kOutStride = OG + 4;  // 16-byte aligned rows for ds_read_b128
  static constexpr int kOutFloatsPerWave = GROUPED ? FRAMES_PER_WAVE * kOutStride : 0;
  static constexpr int kBytes = (2 * kTileFloats + WAVES_PER_BLOCK * kOutFloatsPerWave) * 4;
};

template <int NKK, bool GROUPED, bool CL>
__global__ __launch_bounds__(256, 2) void k_gmm_diag_score_tracks(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ pivot,
    const float *__restrict__ apack, const int32_t *__restrict__ split_row,
    const uint16_t *__restrict__ close_mask, const int32_t *__restrict__ sid, int sid_stride,
    float *__restrict__ out, int64_t S, int64_t pitch, float ref_ln, int dbg, ClusterArgs cl) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *smem = (float *)smem_raw;
  constexpr int OG = TRACK_OUT_GROUP;
  constexpr int kTileFloats = TrackSmem<NKK, GROUPED>::kTileFloats;
  constexpr int kOS = TrackSmem<NKK, GROUPED>::kOutStride;
  float *abuf0 = smem;
  float *abuf1 = smem + kTileFloats;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  float *ost = smem + 2 * kTileFloats + wave * TrackSmem<NKK, GROUPED>::kOutFloatsPerWave;
  const int n = lane & 31;
  const int h = lane >> 5;
  const int64_t f0 = (int64_t)blockIdx.x * FRAMES_PER_BLOCK + wave * FRAMES_PER_WAVE;

  float bf[NKK][2];
#pragma unroll
  for (int nb = 0; nb < 2; nb++) {
    int64_t f = f0 + nb * 32 + n;
    if (f > F - 1) f = F - 1;
    const float *xr = frames + f * dim;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) {
      const int kc = kk < dim ? kk : 0;
      const float xc = xr[kc] - pivot[kc];
      float v = h ? xc * xc : xc;
      if (kk == dim) v = h ? 0.0f : 1.0f;
      if (kk > dim) v = 0.0f;
      bf[kk][nb] = v;
    }
  }

  // this workgroup's share of the rows: tiles [t_begin, t_end)
  const int64_t t_begin = split_row[4 * blockIdx.y];
  const int64_t t_end = split_row[4 * blockIdx.y + 4];
  issue_tile_copy_raw(apack + (size_t)t_begin * kTileFloats, abuf0, kTileFloats, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float s0 = 0.0f, s1 = 0.0f;  // running sum_k 2^(v_k) of this lane's open state, frames n / 32+n
  // closes so far on this lane's track (GROUPED: pairs closed, same on both tracks)
  int closes = split_row[4 * blockIdx.y + 1 + (GROUPED ? 0 : h)];
  const int32_t *my_sid = sid + h * sid_stride;
  int next_sid = GROUPED ? 0 : my_sid[closes];
  float *orow0 = out + (f0 + n) * pitch;       // !GROUPED: this lane's two output rows
  float *orow1 = out + (f0 + 32 + n) * pitch;
  const bool ok0 = f0 + n < F, ok1 = f0 + 32 + n < F;
  const float floor_val = CL ? cl.floor_val : LOG_TINY_F;
  // this wave's 64 frames are one word of the selection masks; its per-lane bits of tile t
  const unsigned long long *mrow =
      CL ? cl.maskrow + (size_t)(f0 >> 6) * cl.rows_padded + lane : nullptr;
  unsigned long long bits_next = 0;
  if (CL && split_row[4 * blockIdx.y] < split_row[4 * blockIdx.y + 4])
    bits_next = mrow[(size_t)split_row[4 * blockIdx.y] * TILE_ROWS];

  // close bits of the next tile are requested (scalar) right after the barrier, one tile ahead
  unsigned pair_next = t_begin < t_end ? sload_close_pair(close_mask, t_begin) : 0u;
  for (int64_t t = t_begin; t < t_end; t++) {
    const int par = (int)((t - t_begin) & 1);
    float *acur = par ? abuf1 : abuf0;
    float *anext = par ? abuf0 : abuf1;
    if (t + 1 < t_end)
      issue_tile_copy_raw(apack + (size_t)(t + 1) * kTileFloats, anext, kTileFloats, wave, lane);
    const unsigned mask16 = close16_of_pair(pair_next, t);
    // GROUPED: both tracks carry the same bits -> wave-uniform branch
    const unsigned mask = GROUPED ? (mask16 & 0xffu) : (h ? (mask16 >> 8) : (mask16 & 0xffu));
    // this tile's selection bits arrived during the previous tile; the next tile's are requested
    // here and waited for by the vmcnt(0) in front of the end-of-tile barrier
    const unsigned long long bits = bits_next;
    if (CL && t + 1 < t_end) bits_next = mrow[(size_t)(t + 1) * TILE_ROWS];

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const f32x4 *afrag = (const f32x4 *)acur + lane;
    f32x4 a0 = afrag[0];
    f32x4 a1 = afrag[(NKK / 2 > 1 ? 1 : 0) * 64];
#pragma unroll
    for (int q = 0; q < NKK / 2; q++) {
      // fetched two kk-pairs ahead; the scheduling barriers keep the compiler from sinking the
      // read to its first use (which exposes one LDS round trip per 8 MFMAs)
      const int qn = (q + 2 < NKK / 2) ? q + 2 : NKK / 2 - 1;
      __builtin_amdgcn_sched_barrier(0);
      f32x4 a2 = afrag[qn * 64];
      __builtin_amdgcn_sched_barrier(0);
      const f32x4 av = a0;
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bf[2 * q][0], c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bf[2 * q][1], c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bf[2 * q][0], c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bf[2 * q][1], c11, 0, 0, 0);
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bf[2 * q + 1][0], c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bf[2 * q + 1][1], c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bf[2 * q + 1][0], c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bf[2 * q + 1][1], c11, 0, 0, 0);
      a0 = a1;
      a1 = a2;
    }

    // One barrier per tile: every wave is done reading `acur` and every wave's
    // share of tile t+1 has landed; the epilogue then needs no inter-wave sync.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < t_end) pair_next = sload_close_pair(close_mask, t + 1);

    if (AASR_DBG(1)) {  // ablation: MFMA only
      asm volatile("" ::"v"(c00), "v"(c01), "v"(c10), "v"(c11));
      continue;
    }

#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
      const f32x16 &ca = mb ? c10 : c00;
      const f32x16 &cb = mb ? c11 : c01;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        // this lane's quad q of the block: accumulator registers 4q .. 4q+3
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
            next_sid = my_sid[closes];  // list is padded by one entry
          } else {
            const int pairs_closed = closes;
            const int slot = ((2 * (pairs_closed - 1)) & (OG - 1)) + h;
            ost[n * kOS + slot] = l0;
            ost[(32 + n) * kOS + slot] = l1;
            const int64_t closed = 2 * (int64_t)pairs_closed < S ? 2 * (int64_t)pairs_closed : S;
            if ((((2 * pairs_closed) & (OG - 1)) == 0 || 2 * (int64_t)pairs_closed >= S) &&
                !AASR_DBG(16)) {
              const int64_t s_base = ((closed - 1) / OG) * OG;
              const int cnt = (int)(closed - s_base);
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              if (cnt == OG && f0 + FRAMES_PER_WAVE <= F) {
                // full group: each lane moves 4 consecutive states (16 B) of one
                // frame row; 8 lanes cover the 32-state group, 8 rows per instruction
                const int k4 = lane & 7, r8 = lane >> 3;
                float *op = out + (f0 + r8) * pitch + s_base + 4 * k4;
                const float *ip = ost + r8 * kOS + 4 * k4;
#pragma unroll
                for (int i = 0; i < FRAMES_PER_WAVE / 8; i++) {
                  const f32x4 v = *(const f32x4 *)(ip + i * 8 * kOS);
                  // rows of the [F x S] output are only 4-byte aligned
                  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
                  *(f32x4u *)(op + (int64_t)i * 8 * pitch) = v;
                }
              } else {
                constexpr int RPI = 64 / OG;  // frame rows per store instruction
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
}

template <int NKK, bool GROUPED, bool CL>
static void launch_tracks_t(const aasr_gmm *g, const TrackLayout &L, const float *d_frames,
                            int64_t F, float *d_out, hipStream_t stream, const ClusterArgs &cl,
                            int64_t pitch) {
  const int64_t blocks = (F + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  const int smem = TrackSmem<NKK, GROUPED>::kBytes;
  static const int dbg = AASR_EXPERIMENT_ENV("AASR_DBG") ? atoi(AASR_EXPERIMENT_ENV("AASR_DBG")) : 0;
  static bool attr_set[64] = {false};
  auto kern = k_gmm_diag_score_tracks<NKK, GROUPED, CL>;
  if (!attr_set[g->device & 63]) {
    AASR_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set[g->device & 63] = true;
  }
  // Row-range cuts: pick the number of cuts R that leaves the smallest tail
  // round on the chip (2 workgroups per CU resident), preferring fewer cuts.
  static const int force_r = AASR_EXPERIMENT_ENV("AASR_SPLITS") ? atoi(AASR_EXPERIMENT_ENV("AASR_SPLITS")) : 0;
  const double slots = 2.0 * (g->num_cus > 0 ? g->num_cus : 256);
  int R = 1;
  double best_eff = 0;
  for (int r = 1; r <= L.max_splits; r++) {
    double x = (double)blocks * r / slots;
    double eff = x / std::ceil(x);
    if (eff > best_eff + 0.005) {
      best_eff = eff;
      R = r;
    }
  }
  if (force_r >= 1 && force_r <= L.max_splits) R = force_r;
  const int32_t *split_row = L.splits.p + (size_t)(R - 1) * (L.split_cap + 1) * 4;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)R), dim3(256), smem, stream, d_frames, F,
                     g->dim, g->d_pivot.p, L.rows.a.p, split_row, L.close.p, L.sid.p, L.sid_stride,
                     d_out, g->S, pitch, L.ref_ln - (float)g->out_bias_ln, dbg, cl);
  AASR_HIP(hipGetLastError());
}

bool launch_tracks(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                   float *d_out, hipStream_t stream, const ClusterArgs *cl, int64_t pitch) {
  if (pitch <= 0) pitch = g->S;
  const ClusterArgs none;
  switch (L.rows.nkk) {
#define AASR_CASE(N)                                                                        \
  case N:                                                                                   \
    if (cl) {                                                                               \
      if (L.grouped) launch_tracks_t<N, true, true>(g, L, d_frames, F, d_out, stream, *cl, pitch); \
      else launch_tracks_t<N, false, true>(g, L, d_frames, F, d_out, stream, *cl, pitch);          \
    } else {                                                                                \
      if (L.grouped) launch_tracks_t<N, true, false>(g, L, d_frames, F, d_out, stream, none, pitch); \
      else launch_tracks_t<N, false, false>(g, L, d_frames, F, d_out, stream, none, pitch);        \
    }                                                                                       \
    return true;
    AASR_CASE(8) AASR_CASE(14) AASR_CASE(20) AASR_CASE(26) AASR_CASE(32) AASR_CASE(40)
    AASR_CASE(48) AASR_CASE(64)
#undef AASR_CASE
    default:
      return false;
  }
}

}  // namespace aasr

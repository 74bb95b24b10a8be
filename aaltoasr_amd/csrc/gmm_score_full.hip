// gmm_score_full.hip -- full-covariance pools (the map of the files: gmm_score.hip): k_gmm_full_score (f32),
// k_gmm_full_score_bf16x3 (two fp16 / three bf16 terms), gmm_full_launch, gmm_full_masked_launch.
#include "gmm_score_common.h"

namespace aasr {

// ---------------------------------------------------------------------------
// Full-covariance kernel (see gmm_build_fullcov()).
//
// Same frame-stationary skeleton; the streamed rows are the rows of
// sqrt(log2e/2) * R^-1 of every mixture component (Sigma = R R^T), K = dim + 1.
// The accumulators hold y = R^-1 (x - mu); the epilogue squares and sums them
// per component (one FMA per value), turns each finished component into
// 2^(C_g - |y|^2 + ref) and adds it to its state's running sum.  Two
// independent row tracks, results stored per state.
// ---------------------------------------------------------------------------
// CL (Gaussian clustering over a full-covariance pool, gmm_cluster.hip): a component counts for a frame only where
// the selection bit of its rows is set (all rows of a component belong to one cluster; the bit of its last row is
// tested where the component closes), and the result carries no 1e-50 floor (k_cluster_merge applies it).
template <int NKK, bool CL>
__global__ __launch_bounds__(256, 2) void k_gmm_full_score(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ pivot,
    const float *__restrict__ apack, const int32_t *__restrict__ split_row,
    const uint32_t *__restrict__ close_mask, const float *__restrict__ gconst, int g_stride,
    const int32_t *__restrict__ sid, int s_stride, float *__restrict__ out, int64_t S, float ref_ln,
    ClusterArgs cl) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *smem = (float *)smem_raw;
  constexpr int kTileFloats = (NKK / 2) * 64 * 4;
  float *abuf0 = smem;
  float *abuf1 = smem + kTileFloats;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int n = lane & 31;
  const int h = lane >> 5;
  const int64_t f0 = (int64_t)blockIdx.x * FRAMES_PER_BLOCK + wave * FRAMES_PER_WAVE;

  // B[kk][nb]: K index k = 2*kk + h -> x'_k (k < dim), 1 (k == dim), 0 beyond
  float bf[NKK][2];
#pragma unroll
  for (int nb = 0; nb < 2; nb++) {
    int64_t f = f0 + nb * 32 + n;
    if (f > F - 1) f = F - 1;
    const float *xr = frames + f * dim;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) {
      const int k = 2 * kk + h;
      const int kc = k < dim ? k : 0;
      float v = xr[kc] - pivot[kc];
      if (k == dim) v = 1.0f;
      if (k > dim) v = 0.0f;
      bf[kk][nb] = v;
    }
  }

  const int64_t t_begin = split_row[8 * blockIdx.y];
  const int64_t t_end = split_row[8 * blockIdx.y + 8];
  issue_tile_copy(apack + (size_t)t_begin * kTileFloats, abuf0, kTileFloats, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float q0 = 0.0f, q1 = 0.0f;  // |y|^2 of the open component, frames n / 32+n
  float s0 = 0.0f, s1 = 0.0f;  // sum over finished components of the open state
  int ks = split_row[8 * blockIdx.y + 1 + h];
  int kg = split_row[8 * blockIdx.y + 3 + h];
  const int32_t *my_sid = sid + h * s_stride;
  const float *my_gc = gconst + h * g_stride;
  int next_sid = my_sid[ks];
  float next_gc = my_gc[kg];
  float *orow0 = out + (f0 + n) * S;
  float *orow1 = out + (f0 + 32 + n) * S;
  const bool ok0 = f0 + n < F, ok1 = f0 + 32 + n < F;
  const float floor_val = CL ? cl.floor_val : LOG_TINY_F;
  const unsigned long long *mrow = CL ? cl.maskrow + (size_t)(f0 >> 6) * cl.rows_padded + lane : nullptr;
  const int etest = (dim - 1) & 3;   // element of a component's last quad that holds its last row

  for (int64_t t = t_begin; t < t_end; t++) {
    const int par = (int)((t - t_begin) & 1);
    float *acur = par ? abuf1 : abuf0;
    float *anext = par ? abuf0 : abuf1;
    if (t + 1 < t_end)
      issue_tile_copy(apack + (size_t)(t + 1) * kTileFloats, anext, kTileFloats, wave, lane);
    unsigned long long bits = 0;
    if (CL) bits = mrow[(size_t)t * TILE_ROWS];   // k_cluster_expand's per-lane word of this tile
    const unsigned m32 = sload_close32(close_mask, t);
    const unsigned gmask = h ? ((m32 >> 8) & 0xffu) : (m32 & 0xffu);
    const unsigned smask = h ? ((m32 >> 24) & 0xffu) : ((m32 >> 16) & 0xffu);

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const f32x4 *afrag = (const f32x4 *)acur + lane;
    f32x4 a0 = afrag[0];
    f32x4 a1 = afrag[(NKK / 2 > 1 ? 1 : 0) * 64];
#pragma unroll
    for (int q = 0; q < NKK / 2; q++) {
      const int qn = (q + 2 < NKK / 2) ? q + 2 : NKK / 2 - 1;
      f32x4 a2 = afrag[qn * 64];
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
      const f32x16 &ca = mb ? c10 : c00;
      const f32x16 &cb = mb ? c11 : c01;
#pragma unroll
      for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
          q0 = fmaf(ca[4 * q + e], ca[4 * q + e], q0);
          q1 = fmaf(cb[4 * q + e], cb[4 * q + e], q1);
        }
        if ((gmask >> (mb * 4 + q)) & 1) {
          float e0 = __builtin_amdgcn_exp2f(next_gc - q0);
          float e1 = __builtin_amdgcn_exp2f(next_gc - q1);
          if (CL) {
            e0 = ((bits >> (8 * q + 4 * mb + etest)) & 1ull) ? e0 : 0.0f;
            e1 = ((bits >> (32 + 8 * q + 4 * mb + etest)) & 1ull) ? e1 : 0.0f;
          }
          s0 += e0;
          s1 += e1;
          q0 = 0.0f;
          q1 = 0.0f;
          kg++;
          next_gc = my_gc[kg];
          if ((smask >> (mb * 4 + q)) & 1) {
            float l0 = fmaf(__builtin_amdgcn_logf(s0), LN2_F, -ref_ln);
            float l1 = fmaf(__builtin_amdgcn_logf(s1), LN2_F, -ref_ln);
            l0 = fmaxf(l0, floor_val);
            l1 = fmaxf(l1, floor_val);
            if (ok0) orow0[next_sid] = l0;
            if (ok1) orow1[next_sid] = l1;
            s0 = 0.0f;
            s1 = 0.0f;
            ks++;
            next_sid = my_sid[ks];
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The same kernel on the bf16 matrix pipe (AASR_PREC_BF16X3): rows and frames as
// three bf16 terms, six products per slab accumulated in f32 -- the scheme of
// k_gmm_diag_score_bf16x3 (rolling A-fragment prefetch ordered by split, tile
// copy through inline assembly, close bits requested mid-stream one tile ahead).
// K = dim + 1 padded to a multiple of 16, K index = column of R^-1 | bias.
// ---------------------------------------------------------------------------
// NS = 2 (AASR_PREC_F16X2): rows and frames as two fp16 terms, three products per slab -- half the matrix
// instructions.  State-level error ~2x the three-term form's at the same conditioning (tools/exp_fullcov_f16.py), so
// a pool takes it only below FULL_KAPPA_LIMIT_F16 (gmm.h); the frame operand is clamped to +-kFullF16Clamp.
// CL (Gaussian clustering over a full-covariance pool): a component counts for a frame only where its cluster's bit of
// the tile's per-lane word (k_cluster_expand) is set; no floor on the states -- the merge adds the centres.
template <int NK16, int NS, bool CL = false>
__global__ __launch_bounds__(256, 2) void k_gmm_full_score_bf16x3(
    const float *__restrict__ frames, int64_t F, int dim, const float *__restrict__ pivot,
    const uint16_t *__restrict__ apack, const int32_t *__restrict__ split_row,
    const uint32_t *__restrict__ close_mask, const float *__restrict__ gc_tile,
    const int32_t *__restrict__ sid_tile, float *__restrict__ out, int64_t S, float ref_ln, ClusterArgs cl,
    const float *__restrict__ f16scale) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int kTileFloats = NK16 * NS * 2 * 64 * 16 / 4;
  float *abuf0 = (float *)smem_raw;
  float *abuf1 = abuf0 + kTileFloats;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int n = lane & 31;
  const int h = lane >> 5;
  const int64_t f0 = (int64_t)blockIdx.x * FRAMES_PER_BLOCK + wave * FRAMES_PER_WAVE;

  // frame operand: lane (n, h) holds k = 16*j + 8*h + i, i < 8: x'_k (k < dim), 1 (k == dim), 0 beyond
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
        const int kc = k < dim ? k : 0;
        float val = xr[kc] - pivot[kc];
        // two fp16 terms: the column's power-of-two scale (the factor rows carry its inverse: exact), then the fp16 range
        if (NS == 2) val = fminf(fmaxf(val * f16scale[kc], -kFullF16Clamp), kFullF16Clamp);
        if (k == dim) val = 1.0f;
        if (k > dim) val = 0.0f;
        v[i] = val;
      }
      unsigned w1[4], w2[4], w3[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if constexpr (NS == 3) split3_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i], w3[i]);
        else split2_pair(v[2 * i], v[2 * i + 1], w1[i], w2[i]);
      }
      bq[j][0][nb] = u32x4{w1[0], w1[1], w1[2], w1[3]};
      bq[j][1][nb] = u32x4{w2[0], w2[1], w2[2], w2[3]};
      if constexpr (NS == 3) bq[j][2][nb] = u32x4{w3[0], w3[1], w3[2], w3[3]};
    }
  }

  const int64_t t_begin = split_row[8 * blockIdx.y];
  const int64_t t_end = split_row[8 * blockIdx.y + 8];
  const float *apf = (const float *)apack;
  issue_tile_copy_raw(apf + (size_t)t_begin * kTileFloats, abuf0, kTileFloats, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float q0 = 0.0f, q1 = 0.0f;  // |y|^2 of the open component, frames n / 32+n
  float s0 = 0.0f, s1 = 0.0f;  // sum over finished components of the open state
  // this track's closing constants / state indices of a tile, by quad position
  const f32x4 *gct = (const f32x4 *)(gc_tile + h * 8);
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const i32x4 *sdt = (const i32x4 *)(sid_tile + h * 8);
  float *orow0 = out + (f0 + n) * S;
  float *orow1 = out + (f0 + 32 + n) * S;
  const bool ok0 = f0 + n < F, ok1 = f0 + 32 + n < F;
  const float floor_val = CL ? cl.floor_val : LOG_TINY_F;
  const unsigned long long *mrow = CL ? cl.maskrow + (size_t)(f0 >> 6) * cl.rows_padded + lane : nullptr;
  const int etest = (dim - 1) & 3;   // element of a component's last quad that holds its last row

  unsigned m32_next = t_begin < t_end ? (unsigned)__builtin_amdgcn_readfirstlane((int)close_mask[t_begin]) : 0u;
  unsigned mask_v = 0;
  u32x4 afr[NS][2];
  if (t_begin < t_end) {
#pragma unroll
    for (int sp = NS - 1; sp >= 0; sp--) {
      afr[sp][0] = ((const u32x4 *)abuf0 + lane)[(sp * 2 + 0) * 64];
      afr[sp][1] = ((const u32x4 *)abuf0 + lane)[(sp * 2 + 1) * 64];
    }
  }
  for (int64_t t = t_begin; t < t_end; t++) {
    const int par = (int)((t - t_begin) & 1);
    float *acur = par ? abuf1 : abuf0;
    float *anext = par ? abuf0 : abuf1;
    if (t + 1 < t_end)
      issue_tile_copy_raw(apf + (size_t)(t + 1) * kTileFloats, anext, kTileFloats, wave, lane);
    // fetched with the tile: they land under the matrix stream, the epilogue never waits on memory
    const f32x4 gca = gct[4 * t], gcb = gct[4 * t + 1];
    const i32x4 sda = sdt[4 * t], sdb = sdt[4 * t + 1];
    const float gcv[8] = {gca.x, gca.y, gca.z, gca.w, gcb.x, gcb.y, gcb.z, gcb.w};
    const int sdv[8] = {sda.x, sda.y, sda.z, sda.w, sdb.x, sdb.y, sdb.z, sdb.w};
    unsigned long long bits = 0;
    if (CL) bits = mrow[(size_t)t * TILE_ROWS];   // k_cluster_expand's per-lane word of this tile
    const unsigned m32 = m32_next;
    const unsigned gmask = h ? ((m32 >> 8) & 0xffu) : (m32 & 0xffu);
    const unsigned smask = h ? ((m32 >> 24) & 0xffu) : ((m32 >> 16) & 0xffu);

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const u32x4 *afrag = (const u32x4 *)acur + lane;  // [slab][split][mb][64 lanes]
#pragma unroll
    for (int j = 0; j < NK16; j++) {
#pragma unroll
      for (int grp = 0; grp < NS; grp++) {
        const int sp = NS - 1 - grp;  // a3 | a2 | a1
        const int nprod = grp + 1;    // b1 | b2 b1 | b3 b2 b1
#pragma unroll
        for (int c = 0; c < nprod; c++) {
          const int sb = nprod - 1 - c;
          c00 = mfma_split<NS>(afr[sp][0], bq[j][sb][0], c00);
          c01 = mfma_split<NS>(afr[sp][0], bq[j][sb][1], c01);
          c10 = mfma_split<NS>(afr[sp][1], bq[j][sb][0], c10);
          c11 = mfma_split<NS>(afr[sp][1], bq[j][sb][1], c11);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j == 0 && grp == 0) mask_v = close_mask[t + 1];  // the array has one spare element
        if (j + 1 < NK16) {
          afr[sp][0] = afrag[(((j + 1) * NS + sp) * 2 + 0) * 64];
          afr[sp][1] = afrag[(((j + 1) * NS + sp) * 2 + 1) * 64];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(mask_v) : : "memory");
    __builtin_amdgcn_s_barrier();
    m32_next = (unsigned)__builtin_amdgcn_readfirstlane((int)mask_v);
    if (t + 1 < t_end) {
      const u32x4 *nfrag = (const u32x4 *)anext + lane;
#pragma unroll
      for (int sp = NS - 1; sp >= 0; sp--) {
        afr[sp][0] = nfrag[(sp * 2 + 0) * 64];
        afr[sp][1] = nfrag[(sp * 2 + 1) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
    }

#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
      const f32x16 &ca = mb ? c10 : c00;
      const f32x16 &cb = mb ? c11 : c01;
#pragma unroll
      for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
          q0 = fmaf(ca[4 * q + e], ca[4 * q + e], q0);
          q1 = fmaf(cb[4 * q + e], cb[4 * q + e], q1);
        }
        if ((gmask >> (mb * 4 + q)) & 1) {
          float e0 = __builtin_amdgcn_exp2f(gcv[mb * 4 + q] - q0);
          float e1 = __builtin_amdgcn_exp2f(gcv[mb * 4 + q] - q1);
          if (CL) {
            e0 = ((bits >> (8 * q + 4 * mb + etest)) & 1ull) ? e0 : 0.0f;
            e1 = ((bits >> (32 + 8 * q + 4 * mb + etest)) & 1ull) ? e1 : 0.0f;
          }
          s0 += e0;
          s1 += e1;
          q0 = 0.0f;
          q1 = 0.0f;
          if ((smask >> (mb * 4 + q)) & 1) {
            float l0 = fmaf(__builtin_amdgcn_logf(s0), LN2_F, -ref_ln);
            float l1 = fmaf(__builtin_amdgcn_logf(s1), LN2_F, -ref_ln);
            l0 = fmaxf(l0, floor_val);
            l1 = fmaxf(l1, floor_val);
            if (ok0) orow0[sdv[mb * 4 + q]] = l0;
            if (ok1) orow1[sdv[mb * 4 + q]] = l1;
            s0 = 0.0f;
            s1 = 0.0f;
          }
        }
      }
    }
  }
}

// Row-range cuts of a full-covariance launch: the number of cuts that leaves the smallest tail round on the chip (two
// workgroups per CU resident), preferring fewer cuts
static int pick_full_cuts(const aasr_gmm *g, int64_t blocks) {
  const double slots = 2.0 * (g->num_cus > 0 ? g->num_cus : 256);
  int R = 1;
  double best_eff = 0;
  for (int r = 1; r <= g->full.max_splits; r++) {
    double x = (double)blocks * r / slots;
    double eff = x / std::ceil(x);
    if (x < 1.0) eff = x;
    if (eff > best_eff + 0.005) {
      best_eff = eff;
      R = r;
    }
  }
  return R;
}

template <int NK16, int NS = 3, bool CL = false>
static void launch_full_bf16_t(const aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                               hipStream_t stream, const ClusterArgs &cl = ClusterArgs()) {
  const FullLayout &L = g->full;
  const int64_t blocks = (F + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  const int smem = 2 * NK16 * NS * 2 * 64 * 16;
  const int R = pick_full_cuts(g, blocks);
  const int32_t *split_row = L.splits.p + (size_t)(R - 1) * (TRACK_MAX_SPLITS + 1) * 8;
  hipLaunchKernelGGL((k_gmm_full_score_bf16x3<NK16, NS, CL>), dim3((unsigned)blocks, (unsigned)R), dim3(256), smem,
                     stream, d_frames, F, g->dim, g->d_pivot.p, NS == 2 ? L.a16h.p : L.a16.p, split_row, L.close.p,
                     L.gc_tile.p, L.sid_tile.p, d_out, g->S, L.ref_ln, cl, NS == 2 ? L.f16scale.p : nullptr);
  AASR_HIP(hipGetLastError());
}

template <int NKK, bool CL = false>
static void launch_full_t(const aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                          hipStream_t stream, const ClusterArgs &cl = ClusterArgs()) {
  const FullLayout &L = g->full;
  const int64_t blocks = (F + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  const int smem = 2 * (NKK / 2) * 64 * 4 * 4;
  const int R = pick_full_cuts(g, blocks);
  const int32_t *split_row = L.splits.p + (size_t)(R - 1) * (TRACK_MAX_SPLITS + 1) * 8;
  hipLaunchKernelGGL((k_gmm_full_score<NKK, CL>), dim3((unsigned)blocks, (unsigned)R), dim3(256), smem, stream,
                     d_frames, F, g->dim, g->d_pivot.p, L.rows.a.p, split_row, L.close.p, L.gconst.p,
                     L.g_stride, L.sid.p, L.s_stride, d_out, g->S, L.ref_ln, cl);
  AASR_HIP(hipGetLastError());
}

void gmm_full_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                     hipStream_t stream) {
  if (!g->full.ok) raise(AASR_ERR_UNSUPPORTED, "full-covariance layout was not built for this model");
  if (g->use_bf16x3 && g->precision == AASR_PREC_F16X2 && g->full.a16h.p) {
    switch (g->full.nk16) {
      case 1: launch_full_bf16_t<1, 2>(g, d_frames, F, d_out, stream); return;
      case 2: launch_full_bf16_t<2, 2>(g, d_frames, F, d_out, stream); return;
      case 3: launch_full_bf16_t<3, 2>(g, d_frames, F, d_out, stream); return;
      case 4: launch_full_bf16_t<4, 2>(g, d_frames, F, d_out, stream); return;
      default: break;
    }
  }
  if (g->use_bf16x3 && g->full.a16.p) {
    switch (g->full.nk16) {
      case 1: launch_full_bf16_t<1>(g, d_frames, F, d_out, stream); return;
      case 2: launch_full_bf16_t<2>(g, d_frames, F, d_out, stream); return;
      case 3: launch_full_bf16_t<3>(g, d_frames, F, d_out, stream); return;
      case 4: launch_full_bf16_t<4>(g, d_frames, F, d_out, stream); return;
      default: break;
    }
  }
  switch (g->full.rows.nkk) {
#define AASR_CASE(N)                                   \
  case N:                                              \
    launch_full_t<N>(g, d_frames, F, d_out, stream);   \
    return;
    AASR_CASE(8) AASR_CASE(14) AASR_CASE(20) AASR_CASE(26) AASR_CASE(32)
#undef AASR_CASE
    default:
      raise(AASR_ERR_UNSUPPORTED, "no full-covariance kernel instance for K/2 = %d", g->full.rows.nkk);
  }
}

// Gaussian clustering over a full-covariance pool: the exact part of every state on the f32 factor-row kernel with
// the selection masks (the fp16 / bf16 matrix forms where the rows are packed for them, else the f32 kernel), no floor -- the merge adds the centres.
void gmm_full_masked_launch(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                            const unsigned long long *maskrow, hipStream_t stream) {
  if (!g->full.ok) raise(AASR_ERR_UNSUPPORTED, "full-covariance layout was not built for this model");
  ClusterArgs cl;
  cl.maskrow = maskrow;
  cl.rows_padded = g->full.rows_padded;
  cl.floor_val = NEG_BIG_F;
  // the matrix-pipe forms of the rows (two fp16 / three bf16 terms) with the masks, where they are packed
  if (g->use_bf16x3 && g->precision == AASR_PREC_F16X2 && g->full.a16h.p) {
    switch (g->full.nk16) {
      case 1: launch_full_bf16_t<1, 2, true>(g, d_frames, F, d_out, stream, cl); return;
      case 2: launch_full_bf16_t<2, 2, true>(g, d_frames, F, d_out, stream, cl); return;
      case 3: launch_full_bf16_t<3, 2, true>(g, d_frames, F, d_out, stream, cl); return;
      case 4: launch_full_bf16_t<4, 2, true>(g, d_frames, F, d_out, stream, cl); return;
      default: break;
    }
  }
  if (g->use_bf16x3 && g->full.a16.p) {
    switch (g->full.nk16) {
      case 1: launch_full_bf16_t<1, 3, true>(g, d_frames, F, d_out, stream, cl); return;
      case 2: launch_full_bf16_t<2, 3, true>(g, d_frames, F, d_out, stream, cl); return;
      case 3: launch_full_bf16_t<3, 3, true>(g, d_frames, F, d_out, stream, cl); return;
      case 4: launch_full_bf16_t<4, 3, true>(g, d_frames, F, d_out, stream, cl); return;
      default: break;
    }
  }
  switch (g->full.rows.nkk) {
#define AASR_CASE(N)                                                  \
  case N:                                                             \
    launch_full_t<N, true>(g, d_frames, F, d_out, stream, cl);        \
    return;
    AASR_CASE(8) AASR_CASE(14) AASR_CASE(20) AASR_CASE(26) AASR_CASE(32)
#undef AASR_CASE
    default:
      raise(AASR_ERR_UNSUPPORTED, "no full-covariance kernel instance for K/2 = %d", g->full.rows.nkk);
  }
}

}  // namespace aasr

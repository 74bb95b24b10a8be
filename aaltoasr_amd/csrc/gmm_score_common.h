// gmm_score_common.h -- what more than one file of the scoring unit uses (the map of the files: gmm_score.hip): vector
// types and constants, the ablation switch, the tile copies and close-bit loads, the clustering hook, the split-operand
// helpers, the wave-group kernel's LDS plan, and the launchers that are called across the files.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "gmm.h"

namespace aasr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define LN2_F 0.69314718055994530942f
#define LOG2E_F 1.4426950408889634074f
// log(1e-50): HmmSet clamps state likelihoods at util::tiny_for_log
// (aku/HmmSet.cc:497-498, aku/util.hh:131)
#define LOG_TINY_F (-115.12925464970228f)
#define NEG_BIG_F (-3.0e38f)
// Kernel ablations (AASR_DBG=bits: 1 matrix stream only, 2 no A-fragment reads, 16 no barriers,
// 256 / 512 no / half of the tile copies, 4 / 8 scheduling experiments) exist only in a build made
// with AASR_BUILD_ABLATION=1 (-DAASR_ABLATION=1); the product kernels carry none of the branches.
#ifndef AASR_ABLATION
#define AASR_ABLATION 0
#endif
#if AASR_ABLATION
#define AASR_DBG(bits) (dbg & (bits))
#else
#define AASR_DBG(bits) false
#endif

__device__ __forceinline__ void issue_tile_copy(const float *__restrict__ gtile,
                                                float *lds_buf, int tile_floats,
                                                int wave, int lane) {
  // 16 bytes per lane per issue; the LDS destination of a global_load_lds is
  // wave-uniform base + lane*16, i.e. lane-linear -- exactly the packed layout.
  const int chunks = tile_floats / 4;  // 16-byte pieces
  for (int c0 = wave * 64; c0 < chunks; c0 += WAVES_PER_BLOCK * 64) {
    const float *src = gtile + (size_t)(c0 + lane) * 4;
    float *dst = lds_buf + (size_t)c0 * 4;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)src,
        (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
  }
}

// The same copy issued through inline assembly, i.e. invisible to the compiler's wait-count
// bookkeeping.  The builtin is modelled as a FLAT access that touches LDS and global memory at
// once; while one is outstanding the compiler degrades EVERY s_waitcnt lgkmcnt(n) to
// lgkmcnt(0), which serialises the A-fragment prefetch of the matrix stream against LDS latency.
// Callers must order the copy themselves: s_waitcnt vmcnt(0) + barrier before the tile is read.
__device__ __forceinline__ void issue_tile_copy_raw(const float *__restrict__ gtile, float *lds_buf,
                                                    int tile_floats, int wave, int lane,
                                                    int nwaves = WAVES_PER_BLOCK) {
  const int chunks = tile_floats / 4;
  for (int c0 = wave * 64; c0 < chunks; c0 += nwaves * 64) {
    const float *src = gtile + (size_t)(c0 + lane) * 4;
    // the LDS offset is the low half of the generic address (the aperture sits in the high half): no
    // addrspacecast, whose null check the compiler mis-selects in some instantiations
    const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(lds_buf + (size_t)c0 * 4));
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(dst), "v"(src) : "memory", "m0");
  }
}

// Per-tile close bits through the scalar cache (SMEM, lgkmcnt).  A vector load here is a trap:
// its result is needed as a scalar, the compiler waits for it with s_waitcnt vmcnt(0), and
// vmcnt counts in issue order -- so the wave would sit until the tile copy issued just before
// it has landed (measured: 5 ms of 30 in the bf16x3 matrix stream).  t is wave-uniform.
typedef const __attribute__((address_space(4))) uint32_t *cmask32_ptr;
__device__ __forceinline__ unsigned sload_close_pair(const uint16_t *close_mask, int64_t t) {
  return ((cmask32_ptr)close_mask)[__builtin_amdgcn_readfirstlane((int)(t >> 1))];
}
// Bits of tile t out of a word requested earlier; the empty asm keeps the compiler from doing the
// extraction (and therefore the lgkmcnt wait) right behind the request.
__device__ __forceinline__ unsigned close16_of_pair(unsigned pair, int64_t t) {
  asm volatile("" : "+s"(pair));
  return (t & 1) ? pair >> 16 : pair & 0xffffu;
}
__device__ __forceinline__ unsigned sload_close16(const uint16_t *close_mask, int64_t t) {
  return close16_of_pair(sload_close_pair(close_mask, t), t);
}
__device__ __forceinline__ unsigned sload_close32(const uint32_t *close_mask, int64_t t) {
  return ((cmask32_ptr)close_mask)[__builtin_amdgcn_readfirstlane((int)t)];
}

// Gaussian-clustering hook of the track kernels (CL = true; see gmm_cluster.hip).
// One bit per (packed row, frame): 1 = use the Gaussian's exact value, 0 = the row
// contributes nothing here (its cluster centre is added by k_cluster_merge).
// k_cluster_expand stores the bits PER LANE: lane (n, h) of the wave that owns frames
// f0 .. f0+63 holds, for one tile, the 64 accumulator values {mb, q, e, side}
// (rows 32 mb + 8q + 4h + e, frames f0 + 32 side + n), so maskrow[word][tile][lane] is one
// 64-bit word with bit ((mb*4 + q)*4 + e)*2 + side.  A wave fetches its 512 bytes for the NEXT
// tile with one coalesced vector load issued in the middle of the matrix stream; the first
// version read ready-made 64-lane masks through the scalar cache (6 GB per 10^6 frames that
// missed it: +7.6 ms of exposed waits).
struct ClusterArgs {
  const unsigned long long *maskrow = nullptr;
  int64_t rows_padded = 0;
  float floor_val = LOG_TINY_F;
};

// The table is read-only for the whole launch: addressing it through the
// constant address space lets the compiler use scalar loads (plain global loads
// are not scalarised in a kernel that also stores).
// value if this lane's bit `idx` (compile-time) of the tile's word is set, a large negative
// exponent otherwise
__device__ __forceinline__ float mask_select(float x, unsigned long long bits, int idx) {
  const unsigned half = idx < 32 ? (unsigned)bits : (unsigned)(bits >> 32);
  // two instructions per value: the bit sign-extended to a lane mask (v_bfe_i32), then a bitfield
  // insert picks x or the constant (v_bfi_b32) -- and / compare / select is three
  const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)half, idx & 31, 1);
  const unsigned r = (__builtin_bit_cast(unsigned, x) & m) | (__builtin_bit_cast(unsigned, NEG_BIG_F) & ~m);
  return __builtin_bit_cast(float, r);
}

// ---------------------------------------------------------------------------
// bf16x3 variant of the track kernel (AASR_PREC_BF16X3).
//
// The f32 MFMA shares its lanes with the VALU and runs at 1/16 of the bf16
// matrix rate.  Here both operands are split into three bf16 terms
// (x = x1 + x2 + x3, 8 significant bits each, so the split is exact to 2^-24) and
// the six products of order <= 2^-16 are accumulated in f32 by
// v_mfma_f32_32x32x16_bf16:  a1b3 + a2b2 + a3b1 + a1b2 + a2b1 + a1b1, i.e. six
// K = 16 MFMAs per 16 values of K -- 0.375x the matrix cycles of the f32 form,
// f32-class accuracy (dropped terms are 2^-24 relative; every MFMA rounds once
// per 16 products instead of once per product), and the bf16 pipe co-executes
// with the VALU epilogue of the other wave on the SIMD.
// K order (constant first, then interleaved): k = 0: the constant (B = 1), k = 1: the constant's remainder (f16x2; B = 1),
// k = 2 + 2 d: linear term of dimension d, k = 3 + 2 d: its quadratic term, zero beyond; K = 16 NK16 >= 2 dim + 2.  A
// dimension's two terms -- p mu' x' and -p/2 x'^2, each as large as the conditioning estimates say and of opposite sign
// -- meet inside ONE matrix instruction, whose 16 products are summed before the f32 accumulator rounds, and the chain
// starts from the constant (which holds -kappa/2): the running sum then moves from C towards the result by
// (kappa_d - z_d^2)/2 per dimension and never leaves their range.  (Until round 5 the order was all linear terms, the
// constant, then all quadratic terms: the accumulator climbed to the linear terms' sum, ~kappa + sqrt(kappa) |z| log2
// units, and every later instruction rounded at that magnitude -- the dominant error of both split forms on models
// fitted to data, 1.6e-4 on visible values where this order gives 6e-5.)
// ---------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned bf16_bits_rne(float x) {
  unsigned u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// three-term split of two floats, packed pairwise (lo = first value)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned &p1, unsigned &p2,
                                            unsigned &p3) {
  unsigned a1 = bf16_bits_rne(x0), b1 = bf16_bits_rne(x1);
  float r0 = x0 - __uint_as_float(a1 << 16), r1 = x1 - __uint_as_float(b1 << 16);
  unsigned a2 = bf16_bits_rne(r0), b2 = bf16_bits_rne(r1);
  r0 -= __uint_as_float(a2 << 16);
  r1 -= __uint_as_float(b2 << 16);
  unsigned a3 = bf16_bits_rne(r0), b3 = bf16_bits_rne(r1);
  p1 = a1 | (b1 << 16);
  p2 = a2 | (b2 << 16);
  p3 = a3 | (b3 << 16);
}

// ---------------------------------------------------------------------------
// f16x2 variant (AASR_PREC_F16X2): the same kernel with both operands carried as TWO fp16 terms
// (hi = fp16(x), lo = fp16(x - hi): 22 significant bits) and the three products hi*hi, hi*lo, lo*hi
// accumulated in f32 by v_mfma_f32_32x32x16_f16 -- half the matrix instructions of the bf16x3 form.
// What it gives up is 2 bits per operand: measured on 10^7 states of the configs[1] model the worst
// state-level error is 3.4e-5 against 1.9e-5 (tools/exp_fp16_split.py), and the error grows with the
// model's conditioning estimate as the other forms' does, so it is only chosen below tighter limits
// (KAPPA_LIMIT_F16, gmm.h); models above them keep the bf16x3 form.  The constant rides in TWO K slots
// (k = 2 dim and k = 2 dim + 1, the frame operand is 1 in both): 44 bits, so the largest term of the sum
// loses nothing.  fp16 range: the frame operand is clamped to |x - pivot| <= kF16Clamp (its square stays
// finite); load-time eligibility guarantees that a frame that far out is at the 1e-50 floor either way.
// ---------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <int NS>
__device__ __forceinline__ f32x16 mfma_split(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
  if constexpr (NS == 3)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// two-term fp16 split of two floats, packed pairwise (lo half = first value)
__device__ __forceinline__ void split2_pair(float x0, float x1, unsigned &p1, unsigned &p2) {
  const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
  const _Float16 l0 = (_Float16)(x0 - (float)h0), l1 = (_Float16)(x1 - (float)h1);
  p1 = __builtin_bit_cast(unsigned, (f16x2){h0, h1});
  p2 = __builtin_bit_cast(unsigned, (f16x2){l0, l1});
}

template <int NK16, bool GROUPED, bool WIDE = false, int NS = 3>
struct Bf16Smem {
  static constexpr int kTileBytes = NK16 * NS * 2 * 64 * 16;
  // States per output group.  4-wave form: 16 (LDS budget of 2 workgroups per CU).  8-wave form: 32
  // where three tile buffers + eight staging areas of stride 34 still fit 160 KB -- a group is then
  // a whole 128-byte L2 line of a padded output row, written by one store instruction.
  static constexpr bool kBig = WIDE && GROUPED && 3 * kTileBytes + 8 * FRAMES_PER_WAVE * 34 * 4 <= 160 * 1024;
  static constexpr int OG = kBig ? 32 : 16;
  static constexpr int kOutStride = kBig ? 34 : 20;
  static constexpr int kOutFloatsPerWave = GROUPED ? FRAMES_PER_WAVE * kOutStride : 0;
};

// log(exp(a) + exp(b)) for a state's two shares (matrix rows / outlier components, both with the 1e-50 floor, which the
// result keeps; a share AT the floor holds nothing).  The hardware's 2^x and log2 (1 ulp): 2e-7 on the result -- the
// library's expf / log1pf cost ~120 instructions per value, a seventh of the scoring kernel's time where 10 % of the
// states take this path in its close logic (k_gmm_diag_score_pl<..., HYB>); k_outlier_merge uses the same expression.
__device__ __forceinline__ float merge_floored_shares(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  float r = hi;
  if (lo > LOG_TINY_F) r = fmaf(__builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f((lo - hi) * LOG2E_F)), LN2_F, hi);
  return fmaxf(r, LOG_TINY_F);
}

// operand set of the centred kernel: the whole model, or the outlier components only
struct CentredOps {
  const float *recs;
  const int32_t *state_off, *splits;
  int max_splits;
  int64_t frame_stride, state_stride;  // out[f * frame_stride + s * state_stride]
  // Gaussian clustering: cluster of every record, selection bits [words][c1]; null = unmasked
  const int32_t *crow = nullptr;
  const unsigned long long *maskw = nullptr;
  int c1 = 0;
  int64_t n_words = 1;
  float floor_val = LOG_TINY_F;  // NEG_BIG_F: no floor (clustered passes, per-Gaussian view)
  int64_t n_recs = 0;            // records of the operand set (the launcher's cost model; 0: unknown)
};

// ---------------------------------------------------------------------------
// Launchers called across the files (every kernel instance is instantiated in the one file named here).
// ---------------------------------------------------------------------------
// gmm_score_f32.hip
template <int MODE>
void launch_diag(const aasr_gmm *g, const PackedRows &pr, const float *d_frames,
                 int64_t F, float *d_out, int64_t out_cols, hipStream_t stream);
bool launch_tracks(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                   float *d_out, hipStream_t stream, const ClusterArgs *cl = nullptr,
                   int64_t pitch = 0);
// gmm_score_pl.h, instantiated by gmm_score_f16x2.hip (NS = 2) and gmm_score_bf16x3.hip (NS = 3)
template <int NS>
bool launch_split(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F,
                  float *d_out, hipStream_t stream, const ClusterArgs *cl = nullptr, int64_t pitch = 0);
template <int NS>
void form_frame_operand(const aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, hipStream_t stream);
// gmm_score_exact.hip
extern double g_score_pass_bytes;
bool launch_centred_ops(const aasr_gmm *g, const CentredOps &ops, int dimp, const float *d_frames,
                        int64_t F, float *d_out, hipStream_t stream);
bool launch_centred(const aasr_gmm *g, const float *d_frames, int64_t F, float *d_out,
                    hipStream_t stream, int64_t pitch = 0);
void score_outliers(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, hipStream_t stream,
                    const int32_t *crow = nullptr, const unsigned long long *maskw = nullptr, int c1 = 0,
                    int64_t n_words = 1, int64_t pitch = 0);
bool hyb_fuse_begin(aasr_gmm *g, const TrackLayout &L, const float *d_frames, int64_t F, hipStream_t stream);
void score_f64_for_f32_callers(aasr_gmm *g, const float *d_frames, int64_t F, float *d_out, hipStream_t stream);

}  // namespace aasr

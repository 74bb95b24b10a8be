// lna_encode.hip -- per-frame state normalisation + LNA packing on device.
//
// Replaces the tail of the phone_probs frame loop (aku/phone_probs.cc:224-262;
// PPToolbox: aku/PhoneProbsToolbox.cc:84-131):
//   obs[i] = (float) state_likelihood(i);  Z = sum_i (double) obs[i]
//   if (no-normalization || Z == 0) Z = 1
//   obs[i] = (float) safe_log(obs[i] / Z)            (floor log(1e-50))
//   2-byte: obs < -36.008 -> FF FF, else big-endian (int)(-1820*obs + .5)
//   4-byte: little-endian float
// The input here is the LOG state likelihood (float32, >= log(1e-50)), so the
// reference's float storage of the LINEAR likelihood is emulated:
//   ll <  ln(2^-150)            -> (float)lik == 0  -> output log(1e-50)
//   ln(2^-150) <= ll < ln(2^-126) -> denormal: q = rint(lik * 2^149) quanta
//   otherwise                   -> normal float, relative rounding 6e-8 (kept)
//
// One workgroup per frame; HBM-bound: S*(4 in + lnabytes out) bytes per frame.
// (A wave-per-frame variant without workgroup barriers was measured 2.5 ms slower
// on 449 280 x 3125: it reads the row three times with 4-byte loads.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "lna_device.h"

namespace aasr {

__global__ __launch_bounds__(256) void k_state_norm_lna(
    const float *__restrict__ loglik, int64_t F, int S, int64_t in_pitch, int normalize,
    int lnabytes, float *__restrict__ lp_out, uint8_t *__restrict__ bytes_out) {
  __shared__ double red[8];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    const float *row = loglik + f * in_pitch;
    double logz = 0.0;
    if (normalize) {
      // pass 1: max of the float-cast log-likelihoods
      double m = -INFINITY;
      for (int i = tid; i < S; i += 256) {
        double v = float_cast_loglik(row[i]);
        m = v > m ? v : m;
      }
      m = wave_reduce_max(m);
      if (lane == 0) red[wave] = m;
      __syncthreads();
      m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
      __syncthreads();
      if (m > -INFINITY) {
        // pass 2: Z / exp(m) accumulated in double
        double z = 0.0;
        for (int i = tid; i < S; i += 256) {
          double v = float_cast_loglik(row[i]);
          z += (double)expf((float)(v - m));
        }
        z = wave_reduce_sum(z);
        if (lane == 0) red[4 + wave] = z;
        __syncthreads();
        z = (red[4] + red[5]) + (red[6] + red[7]);
        __syncthreads();
        logz = m + log(z);
      }  // all zero -> Z = 1 (phone_probs.cc:231-232)
    }
    // pass 3: normalise, cast, pack
    for (int i = tid; i < S; i += 256) {
      double v = float_cast_loglik(row[i]);
      double lpd = v - logz;
      if (!(lpd >= LOG_TINY_D)) lpd = LOG_TINY_D;  // safe_log floor (also -inf)
      float lp = (float)lpd;
      int64_t o = f * (int64_t)S + i;
      if (lp_out) lp_out[o] = lp;
      if (bytes_out) {
        if (lnabytes == 4) {
          ((float *)bytes_out)[o] = lp;
        } else {
          unsigned short code;
          if ((double)lp < -36.008) {
            code = 0xffff;
          } else {
            int temp = (int)(-1820.0 * (double)lp + .5);
            unsigned b0 = (temp >> 8) & 255, b1 = temp & 255;
            code = (unsigned short)(b0 | (b1 << 8));  // big-endian on disk
          }
          ((unsigned short *)bytes_out)[o] = code;
        }
      }
    }
  }
}


// Register-resident variant for S <= 256*VPT: one global read of the row, the
// three passes (max, sum, pack) run on registers.
// MAPPED = false (no column map: state i is column i) keeps no col[] and reads row[tid + 256 * j]: VPT registers
// fewer, which puts the <13> instance under the 96 VGPRs that two scoring waves leave free on a SIMD
// (gmm_score_lna_chunked, tests/test_lna_unmapped_notes.py).
template <int VPT, bool MAPPED>
__global__ __launch_bounds__(256) void k_state_norm_lna_reg(
    const float *__restrict__ loglik, int64_t F, int S, int64_t in_pitch, int normalize, int lnabytes,
    float *__restrict__ lp_out, uint8_t *__restrict__ bytes_out, const int32_t *__restrict__ colmap) {
  __shared__ double red[8];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // the launcher takes the smallest instance that covers S: S > 256 * (the next smaller instance's VPT)
  constexpr int JSAFE = VPT == 4 ? 0 : VPT == 8 ? 4 : VPT == 10 ? 8 : VPT == 13 ? 10 : VPT == 16 ? 13 : 0;
  // colmap (engine-internal score layout of a routed model, gmm_engine_colmap): state i sits in column colmap[i] of a
  // score row; the same for every frame, so a thread looks its columns up once
  int col[MAPPED ? VPT : 1];
  if constexpr (MAPPED) {
#pragma unroll
    for (int j = 0; j < VPT; j++) {
      const int i = tid + 256 * j;
      col[j] = (colmap && (j < JSAFE || i < S)) ? colmap[i] : i;
    }
  }
  // a workgroup walks frames blockIdx.x, + gridDim.x, ...; the next frame's row is requested
  // before this one is reduced (the four barriers of a frame leave nothing else to hide the
  // load latency behind)
  float vn[VPT];
  {
    const float *row = loglik + (int64_t)blockIdx.x * in_pitch;
#pragma unroll
    for (int j = 0; j < VPT; j++) {
      const int i = tid + 256 * j;
      vn[j] = ((j < JSAFE || i < S) && (int64_t)blockIdx.x < F) ? row[MAPPED ? col[j] : i] : -INFINITY;
    }
  }
  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    float v[VPT];
#pragma unroll
    for (int j = 0; j < VPT; j++) v[j] = vn[j];
    if (f + gridDim.x < F) {
      const float *row = loglik + (f + gridDim.x) * in_pitch;
#pragma unroll
      for (int j = 0; j < VPT; j++) {
        const int i = tid + 256 * j;
        vn[j] = (j < JSAFE || i < S) ? row[MAPPED ? col[j] : i] : -INFINITY;
      }
    }
    lna_row_from_registers<VPT, JSAFE>(v, S, tid, wave, lane, red, normalize, lnabytes, f, true, lp_out, bytes_out);
  }
}

// Q frame rows per workgroup pass: the production call (2-byte codes, no float output, no column map) with what a frame
// pays per pass -- the barriers, the two LDS exchanges, the final combines, the double-precision log -- paid once for
// Q frames.  Beside a scoring workgroup the four waves of this kernel are the youngest on their SIMDs and every barrier
// is a round trip between four starved waves; k_state_norm_lna_reg pays four per frame and evaluates log(z) in all four
// waves for the same frame.  Here group g = blockIdx.x + k gridDim.x holds frames Q g ... Q g + Q - 1 and
//   - the maxima of the Q frames cross LDS together (one barrier), then the Q sums (one barrier);
//   - wave q alone forms logz of frame q (Q = 4: one log per wave and pass instead of four) and all read it after the
//     third barrier;
//   - frame q's registers are dead once it is packed, and the next group's frame q is requested right there: one
//     register set, Q * VPT values, no second one for the prefetch.
// Every rounding step is where lna_row_from_registers' fast path has it (fmaxf over j, the xor butterfly, four wave values;
// the sum in j order from 0.0 in double, wave_reduce_sum's butterfly, (r0 + r1) + (r2 + r3); (double)mr + log(z); the
// packing expression and lna_store), so the bytes are those of k_state_norm_lna_reg.
// The fast path's test -- every mr_q >= -51 -- is taken from LDS values and is uniform over the workgroup.  A pass with a
// frame that fails it is only noted (a bit per pass in LDS) and its rows are left alone; a second loop behind the first
// reads the rows of such passes again, one after another, into one row of registers and hands each to
// lna_row_from_registers itself (all 256 threads with the same frame: its barrier count depends on the frame).  Inside
// the first loop that routine would need its registers on top of the Q rows, and a path that redefines the rows makes the
// compiler keep two sets of them; behind it, it has the register file to itself.  A last group with fewer than Q frames
// clamps the frame index -- a valid row, computed again -- and suppresses the store; no branch around a barrier.
// Registers: Q * VPT = 52 values, 27 the loop never writes (of them 15 hold constants of log()) and up to 25 of working
// set at the logarithm do not fit the 96 that two scoring waves leave on a SIMD.  The last row of a pass therefore waits
// in LDS from its maximum to its packing -- each thread its own VPT slots, 13 312 B, no barrier owed -- which is 13 LDS
// stores and 26 loads per thread and pass: <13, 4> 94 VGPRs, <13, 2> 76, no scratch (tests/test_lna_multi_notes.py).
template <int VPT, int JSAFE>
struct LnaMultiRow {
  // State tid + 256 j of a row as (a uniform base, four elements on) + (the lane's offset) + (a constant): the load takes its
  // base from scalar registers and one 32-bit offset register serves every j.  Elements that may lie beyond S (j >= JSAFE)
  // read the row's last state instead -- no branch, no 64-bit lane address -- and are replaced by -inf.
  static __device__ __forceinline__ void load(float (&v)[VPT], const float *__restrict__ row, int S, int tid) {
#pragma unroll
    for (int j = 0; j < VPT; j++) {
      if (j < JSAFE) {
        v[j] = (row + 1024 * (j >> 2))[tid + 256 * (j & 3)];
      } else {
        const int i = tid + 256 * j;
        const float x = *(const float *)((const char *)row + 4u * (unsigned)std::min(i, S - 1));
        v[j] = i < S ? x : -INFINITY;
      }
    }
  }
};

// wave_reduce_max / wave_reduce_sum of lna_device.h, the same partners in the same order -- so the same bits in every
// lane -- with the five steps inside a half wave as ds_swizzle (xor mode: no lane-index register each)
template <int O>
__device__ __forceinline__ float lna_xor_lane(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x1f | (O << 10)));
}
template <int O>
__device__ __forceinline__ double lna_xor_lane(double x) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)u, 0x1f | (O << 10));
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(u >> 32), 0x1f | (O << 10));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float lna_multi_reduce_max(float v) {
  float u = __shfl_xor(v, 32, 64);
  v = u > v ? u : v;
  u = lna_xor_lane<16>(v); v = u > v ? u : v;
  u = lna_xor_lane<8>(v); v = u > v ? u : v;
  u = lna_xor_lane<4>(v); v = u > v ? u : v;
  u = lna_xor_lane<2>(v); v = u > v ? u : v;
  u = lna_xor_lane<1>(v); v = u > v ? u : v;
  return v;
}
__device__ __forceinline__ double lna_multi_reduce_sum(double v) {
  v += __shfl_xor(v, 32, 64);
  v += lna_xor_lane<16>(v);
  v += lna_xor_lane<8>(v);
  v += lna_xor_lane<4>(v);
  v += lna_xor_lane<2>(v);
  v += lna_xor_lane<1>(v);
  return v;
}

__device__ __forceinline__ float lna_uniform(float x) {   // a value every lane holds, into a scalar register
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
__device__ __forceinline__ double lna_uniform(double x) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

constexpr int kLnaMultiMaxPasses = 2048;   // passes of one workgroup whose kind the kernel can note (the launcher's grid)

template <int VPT, int Q>
__global__ __launch_bounds__(256, 5) void k_state_norm_lna_multi(   // 5 waves per SIMD: at most 96 VGPRs (gmm_score_lna.cc)
    const float *__restrict__ loglik, int64_t F, int S, int64_t in_pitch, int normalize, uint8_t *__restrict__ bytes_out) {
  static_assert(Q >= 2 && Q <= 4, "wave q forms frame q's normaliser");
  __shared__ double red[8];      // lna_row_from_registers' (the passes with a frame off the fast path)
  __shared__ float smax[Q][4];
  __shared__ double ssum[Q][4];
  __shared__ double slogz[Q];
  __shared__ unsigned offfast[kLnaMultiMaxPasses / 32];   // bit p: pass p of this workgroup has a frame off the fast path
  __shared__ float parked[VPT][256];                      // a thread's values of the pass's last row (its own slots)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int JSAFE = VPT == 4 ? 0 : VPT == 8 ? 4 : VPT == 10 ? 8 : VPT == 13 ? 10 : VPT == 16 ? 13 : 0;
  constexpr int P = Q - 1;       // the parked row
  using Row = LnaMultiRow<VPT, JSAFE>;
  const int64_t G = (F + Q - 1) / Q;
  if ((int64_t)blockIdx.x >= G) return;   // uniform over the workgroup
  if (tid < kLnaMultiMaxPasses / 32) offfast[tid] = 0u;
  float v[Q][VPT];
#pragma unroll
  for (int q = 0; q < Q; q++) Row::load(v[q], loglik + std::min<int64_t>((int64_t)blockIdx.x * Q + q, F - 1) * in_pitch, S, tid);
  __syncthreads();
  bool any_off = false;
  int pass = 0;
  for (int64_t g = blockIdx.x;; pass++) {
    const int64_t gn = g + gridDim.x;     // the group whose rows are requested during this pass
    // the Q maxima; the last row first: from there to its packing it waits in LDS, which leaves its registers to the
    // sums and the logarithm (every thread reads back what it wrote itself: no barrier is owed to this)
#pragma unroll
    for (int qq = 0; qq < Q; qq++) {
      const int q = (qq + P) % Q;
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < VPT; j++) m = fmaxf(m, v[q][j]);
      m = lna_multi_reduce_max(m);
      if (lane == 0) smax[q][wave] = m;
      if (q == P) {
#pragma unroll
        for (int j = 0; j < VPT; j++) parked[j][tid] = v[P][j];
      }
    }
    __syncthreads();
    float mr[Q];   // the same in every lane: kept in scalar registers
    bool fast = true;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      mr[q] = lna_uniform(fmaxf(fmaxf(smax[q][0], smax[q][1]), fmaxf(smax[q][2], smax[q][3])));
      fast = fast && mr[q] >= -51.0f;
    }
    if (!normalize || !fast) __syncthreads();   // uniform: smax[] has been read before the next pass writes it
    if (fast) {   // from LDS values: uniform over the workgroup, as every barrier below
      if (normalize) {   // uniform over the grid
#pragma unroll
        for (int q = 0; q < Q; q++) {
          double z = 0.0;
#pragma unroll
          for (int j = 0; j < VPT; j++) {
            const float x = q == P ? parked[j][tid] : v[q][j];
            z += (double)__builtin_amdgcn_exp2f((x - mr[q]) * 1.44269504088896340736f);
          }
          z = lna_multi_reduce_sum(z);
          if (lane == 0) ssum[q][wave] = z;
          __builtin_amdgcn_sched_barrier(0);   // one frame's chain at a time: the register file holds the rows already
        }
        __syncthreads();
        if (wave < Q) {   // wave-uniform, no barrier inside
          const double z = (ssum[wave][0] + ssum[wave][1]) + (ssum[wave][2] + ssum[wave][3]);
          const float m = fmaxf(fmaxf(smax[wave][0], smax[wave][1]), fmaxf(smax[wave][2], smax[wave][3]));
          const double lz = (double)m + log(z);
          if (lane == 0) slogz[wave] = lz;
        }
        __syncthreads();
      }
    } else {
      // left to the second loop below, which has the register file to itself
      if (tid == 0) offfast[pass >> 5] |= 1u << (pass & 31);
      any_off = true;
    }
    const bool more = gn < G;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int64_t f = g * Q + q;
      if (q == P) {
#pragma unroll
        for (int j = 0; j < VPT; j++) v[P][j] = parked[j][tid];
      }
      if (fast && f < F) {   // uniform; the clamped rows of a short last group are not stored
        const double logz = normalize ? lna_uniform(slogz[q]) : 0.0;
        unsigned short *out = (unsigned short *)bytes_out + f * (int64_t)S;   // uniform: a scalar base, 32-bit lane offsets
#pragma unroll
        for (int j = 0; j < VPT; j++) {
          const int i = tid + 256 * j;
          if (j < JSAFE || i < S) {
            const float lp = fmaxf((float)((double)v[q][j] - logz), (float)LOG_TINY_D);
            lna_store(lp, 2, tid + 256 * (j & 7), nullptr, (uint8_t *)(out + 2048 * (j >> 3)));
          }
        }
      }
      // frame q's registers are dead: the next group's frame q goes into them (a load moved above the packing would need
      // a second set).  The one place rows are loaded inside the loop, for both kinds of pass
      __builtin_amdgcn_sched_barrier(0);
      if (more) Row::load(v[q], loglik + std::min<int64_t>(gn * Q + q, F - 1) * in_pitch, S, tid);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!more) break;
    g = gn;
  }
  if (!any_off) return;   // uniform
  // The passes with a frame the fast path's test refuses (rare): their Q frames one after another through the one-frame
  // routine, every thread with the same frame -- its barrier count depends on the frame
  __syncthreads();
  pass = 0;
  for (int64_t g = blockIdx.x; g < G; g += gridDim.x, pass++) {
    const unsigned bits = __builtin_amdgcn_readfirstlane(offfast[pass >> 5]);
    if (!((bits >> (pass & 31)) & 1u)) continue;
#pragma nounroll
    for (int q = 0; q < Q; q++) {
      const int64_t f = g * Q + q;
      float w[VPT];
      Row::load(w, loglik + std::min<int64_t>(f, F - 1) * in_pitch, S, tid);
      lna_row_from_registers<VPT, JSAFE>(w, S, tid, wave, lane, red, normalize, 2, f, f < F, nullptr, bytes_out);
    }
  }
}

// AASR_PREC_F64: the tail of the phone_probs frame loop as written (aku/phone_probs.cc:224-233), from the
// LINEAR state likelihoods in double: obs = (float) lik; Z = sum of (double) obs (Z == 0 or -N: 1);
// obs = (float) safe_log(obs / Z) with the division and the logarithm in double.  Against the
// reference only the order of the Z sum (a tree here, i = 0, 1, ... there) and the device's log()
// can differ, by ~1e-16 relative before the rounding to float.
__global__ __launch_bounds__(256) void k_state_norm_lna_f64(const double *__restrict__ lik, int64_t F, int S,
                                                            int normalize, int lnabytes, float *__restrict__ lp_out,
                                                            uint8_t *__restrict__ bytes_out) {
  __shared__ double red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    const double *row = lik + f * (int64_t)S;
    double z = 1.0;
    if (normalize) {
      double part = 0.0;
      for (int i = tid; i < S; i += 256) part += (double)(float)row[i];
      part = wave_reduce_sum(part);
      __syncthreads();  // red[] of the previous frame has been read
      if (lane == 0) red[wave] = part;
      __syncthreads();
      z = (red[0] + red[1]) + (red[2] + red[3]);
      if (z == 0) z = 1.0;
    }
    for (int i = tid; i < S; i += 256) {
      const float o = (float)row[i];
      const double q = (double)o / z;
      const float lp = (float)(q < 1e-50 ? LOG_TINY_D : log(q));
      lna_store(lp, lnabytes, f * (int64_t)S + i, lp_out, bytes_out);
    }
  }
}

void lna_encode_f64_launch(const double *d_lik, int64_t F, int S, int normalize, int lnabytes, float *d_lp,
                           uint8_t *d_bytes, hipStream_t stream) {
  if (F <= 0 || S <= 0) return;
  const int64_t blocks = std::min<int64_t>(F, 8192);
  hipLaunchKernelGGL(k_state_norm_lna_f64, dim3((unsigned)blocks), dim3(256), 0, stream, d_lik, F, S, normalize, lnabytes,
                     d_lp, d_bytes);
  AASR_HIP(hipGetLastError());
}

// Frames per workgroup pass of the production call where an instance of k_state_norm_lna_multi exists; 1: the one-frame
// kernel.  aasr_debug_lna_frames_per_pass sets it for the process (tests, A/B runs); a negative value: the default
constexpr int kLnaFramesPerPass = 4;
static std::atomic<int> g_dbg_lna_frames_per_pass{-1};

static int lna_frames_per_pass() {
  const int q = g_dbg_lna_frames_per_pass.load();
  return q < 0 ? kLnaFramesPerPass : q;
}

template <int VPT>
static void launch_lna_reg(unsigned blocks, hipStream_t stream, const float *d_loglik, int64_t F, int S, int64_t in_pitch,
                           int normalize, int lnabytes, float *d_lp, uint8_t *d_bytes, const int32_t *d_colmap) {
  if (d_colmap)
    hipLaunchKernelGGL((k_state_norm_lna_reg<VPT, true>), dim3(blocks), dim3(256), 0, stream, d_loglik, F, S, in_pitch,
                       normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else
    hipLaunchKernelGGL((k_state_norm_lna_reg<VPT, false>), dim3(blocks), dim3(256), 0, stream, d_loglik, F, S, in_pitch,
                       normalize, lnabytes, d_lp, d_bytes, d_colmap);
}

// The launch with the workgroups per CU of the register-resident instances given (the chunked score + LNA step, whose
// passes run beside a scoring kernel: gmm_score_lna.cc).  Which workgroup encodes a frame changes no byte of it.
void lna_encode_launch_grid(const float *d_loglik, int64_t F, int S, int normalize,
                            int lnabytes, float *d_lp, uint8_t *d_bytes, hipStream_t stream, int64_t in_pitch,
                            const int32_t *d_colmap, int wgs_per_cu) {
  if (wgs_per_cu < 1 || wgs_per_cu > 1024) raise(AASR_ERR_INVALID, "LNA grid of %d workgroups per CU", wgs_per_cu);
  if (in_pitch <= 0) in_pitch = S;  // row stride of the input in floats
  if (F <= 0 || S <= 0) return;
  if (d_colmap && S > 256 * 16) raise(AASR_ERR_UNSUPPORTED, "a column map needs the register-resident LNA kernels (S <= 4096)");
  int64_t blocks = F < (1 << 20) ? F : (1 << 20);
  // register-resident variants: a few workgroups per CU, each walking many frames with the next
  // row prefetched
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  // 32 per CU.  Historical figure, taken when the kernel held 4 waves per SIMD with the column map in registers: 2.56 ms at
  // 4 per CU, 2.16 at 32, flat above.  The unmapped <13> instance (90 VGPRs) holds 5; re-measured with it in the chunked
  // score + LNA step, where the passes run beside a scoring kernel: 64, 128 and 256 per CU are within 0.03 ms of 32 per
  // step and never faster in all four alternating runs, so 32 stays for every caller.
  if (S <= 256 * 16) blocks = std::min<int64_t>(blocks, (int64_t)cus * wgs_per_cu);
  // The production call on a model of the <13> range: Q frames per pass (k_state_norm_lna_multi), the same bytes, for
  // the stand-alone pass and the chunked step alike.  Its grid counts groups of Q frames, and the rule was measured again
  // for them in the chunked step (Q = 4, per step, two runs each): 8 per CU 9.69 / 9.71 ms, 16 9.63 / 9.63, 32 9.57 /
  // 9.57, 64 9.57 / 9.58, 128 9.57 / 9.58: 32 again -- and never so few workgroups that one walks more
  // passes than it can note the kind of
  const int q = lna_frames_per_pass();
  if (q > 1 && lnabytes == 2 && !d_lp && d_bytes && !d_colmap && S > 256 * 10 && S <= 256 * 13) {
    const int64_t groups = (F + q - 1) / q;
    const int64_t least = (groups + kLnaMultiMaxPasses - 1) / kLnaMultiMaxPasses;
    const unsigned ng = (unsigned)std::min<int64_t>(groups, std::max<int64_t>(least, (int64_t)cus * wgs_per_cu));
    if (q == 4)
      hipLaunchKernelGGL((k_state_norm_lna_multi<13, 4>), dim3(ng), dim3(256), 0, stream, d_loglik, F, S, in_pitch, normalize,
                         d_bytes);
    else
      hipLaunchKernelGGL((k_state_norm_lna_multi<13, 2>), dim3(ng), dim3(256), 0, stream, d_loglik, F, S, in_pitch, normalize,
                         d_bytes);
    AASR_HIP(hipGetLastError());
    return;
  }
  const unsigned nb = (unsigned)blocks;
  if (S <= 256 * 4)
    launch_lna_reg<4>(nb, stream, d_loglik, F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else if (S <= 256 * 8)
    launch_lna_reg<8>(nb, stream, d_loglik, F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else if (S <= 256 * 10)
    launch_lna_reg<10>(nb, stream, d_loglik, F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else if (S <= 256 * 13)
    launch_lna_reg<13>(nb, stream, d_loglik, F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else if (S <= 256 * 16)
    launch_lna_reg<16>(nb, stream, d_loglik, F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes, d_colmap);
  else
    hipLaunchKernelGGL(k_state_norm_lna, dim3(nb), dim3(256), 0, stream, d_loglik,
                       F, S, in_pitch, normalize, lnabytes, d_lp, d_bytes);
  AASR_HIP(hipGetLastError());
}

void lna_encode_launch(const float *d_loglik, int64_t F, int S, int normalize,
                       int lnabytes, float *d_lp, uint8_t *d_bytes, hipStream_t stream, int64_t in_pitch,
                       const int32_t *d_colmap) {
  lna_encode_launch_grid(d_loglik, F, S, normalize, lnabytes, d_lp, d_bytes, stream, in_pitch, d_colmap, 32);
}

}  // namespace aasr

// Diagnostic (tests, A/B runs): frames per workgroup pass of later LNA launches of this process -- 1: the one-frame kernel
// k_state_norm_lna_reg, 2 or 4: k_state_norm_lna_multi where the call qualifies; negative: the compiled-in value.  Any
// other value is ignored.  The bytes do not depend on it.
extern "C" void aasr_debug_lna_frames_per_pass(int q) {
  if (q < 0) aasr::g_dbg_lna_frames_per_pass.store(-1);
  else if (q == 1 || q == 2 || q == 4) aasr::g_dbg_lna_frames_per_pass.store(q);
}

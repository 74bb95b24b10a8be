// fst_conf.hip -- the device passes of the FST decoder's confidence: the best acoustic value of every frame and its
// per-utterance sum, and the best different hypothesis among a search's surviving tokens (layout: fst_conf.h).
#include "fst_conf.h"

#include <climits>

namespace aasr {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t float_image(float x) {  // unsigned order = float order (as in fst_search.hip)
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float image_float(uint32_t m) { return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m); }

// the running best of a 4-byte row: the reference's `if (x > best) best = x` over ascending columns, in any order
struct Best {
  float v;
  int32_t col;  // -1: the start value
};
__device__ __forceinline__ void take(Best &b, float x, int32_t col) {
  if (x > b.v || (x == b.v && col < b.col)) {
    b.v = x;
    b.col = col;
  }
}

template <int BYTES>
__device__ __forceinline__ uint32_t word_min(uint32_t w) {  // the smallest code of four row bytes
  if (BYTES == 2) {
    const uint32_t s = __builtin_bswap32(w);  // big-endian codes: bytes b0 b1 b2 b3 -> (b0 b1) (b2 b3)
    return min(s >> 16, s & 0xffffu);
  }
  return min(min(w & 0xffu, (w >> 8) & 0xffu), min((w >> 16) & 0xffu, w >> 24));
}

}  // namespace

template <int BYTES>
__global__ __launch_bounds__(FSTC_THREADS) void k_fst_frame_best(const FstFrameBestParams p, const int64_t total) {
  const int lane = threadIdx.x & 63, lpr = p.lanes_per_row, sub = lane & (lpr - 1);
  int64_t f = ((int64_t)blockIdx.x * (FSTC_THREADS / 64) + (threadIdx.x >> 6)) * (64 / lpr) + lane / lpr;
  const bool live = f < total;
  if (!live) f = total - 1;  // (the lanes past the last row sweep it once more and write nothing: every lane shuffles)
  int32_t lo = 0, hi = p.n_utt - 1;  // the last utterance whose first frame is <= f: the one that holds f
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (p.frame_off[mid] <= f)
      lo = mid;
    else
      hi = mid - 1;
  }
  const size_t row_bytes = (size_t)p.n_models * BYTES;
  const uintptr_t s = (uintptr_t)p.lna + (size_t)(p.row0[lo] + (f - p.frame_off[lo])) * row_bytes, e = s + row_bytes;
  Best best{FSTC_ACU_START, -1};
  uint32_t code = 0xffffffffu;
  for (uintptr_t a = (s & ~(uintptr_t)15) + (uintptr_t)sub * 16; a < e; a += (uintptr_t)lpr * 16) {
    if (a >= s && a + 16 <= e) {
      const uint4 q = *reinterpret_cast<const uint4 *>(a);
      if (BYTES == 4) {
        const int32_t c = (int32_t)((a - s) >> 2);
        take(best, __uint_as_float(q.x), c);
        take(best, __uint_as_float(q.y), c + 1);
        take(best, __uint_as_float(q.z), c + 2);
        take(best, __uint_as_float(q.w), c + 3);
      } else {
        code = min(code, min(min(word_min<BYTES>(q.x), word_min<BYTES>(q.y)), min(word_min<BYTES>(q.z), word_min<BYTES>(q.w))));
      }
    } else {  // a ragged end of the row: its elements one by one
      const uintptr_t b0 = a > s ? a : s, b1 = a + 16 < e ? a + 16 : e;
      for (uintptr_t b = b0; b < b1; b += BYTES) {
        if (BYTES == 4) {
          take(best, *reinterpret_cast<const float *>(b), (int32_t)((b - s) >> 2));
        } else if (BYTES == 2) {
          const uint8_t *q = reinterpret_cast<const uint8_t *>(b);
          code = min(code, ((uint32_t)q[0] << 8) | q[1]);
        } else {
          code = min(code, (uint32_t) * reinterpret_cast<const uint8_t *>(b));
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if (o < lpr) {  // (the same for every lane: the row's lanes are lpr neighbours)
      if (BYTES == 4) {
        const float v = __shfl_xor(best.v, o, 64);
        const int32_t c = __shfl_xor(best.col, o, 64);
        take(best, v, c);
      } else {
        code = min(code, (uint32_t)__shfl_xor((int)code, o, 64));
      }
    }
  }
  if (live && sub == 0) p.frame_best[f] = BYTES == 4 ? best.v : p.decode[code];  // (a row has at least one model: code is one)
}

// one wave per utterance: 64 maxima per coalesced load, then the reference's chain over them, the same in every lane
__global__ __launch_bounds__(FSTC_THREADS) void k_fst_frame_sum(const FstFrameBestParams p) {
  const int lane = threadIdx.x & 63;
  const int32_t u = (int32_t)(blockIdx.x * (FSTC_THREADS / 64) + (threadIdx.x >> 6));
  if (u >= p.n_utt) return;  // (the whole wave)
  const int64_t end = p.frame_off[u + 1];
  float sum = 0.0f;  // FstConfidenceWithPhoneLoop::run: m_best_acu_score = 0, += per frame
  for (int64_t base = p.frame_off[u]; base < end; base += 64) {
    const float v = base + lane < end ? p.frame_best[base + lane] : 0.0f;
    const int n = end - base < 64 ? (int)(end - base) : 64;
    for (int j = 0; j < n; j++) sum = __fadd_rn(sum, __shfl(v, j, 64));
  }
  if (lane == 0) p.sum[u] = sum;
}

namespace {

__device__ __forceinline__ u64 wave_max(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t h = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), o, 64), l = (uint32_t)__shfl_xor((int)(uint32_t)k, o, 64);
    const u64 n = ((u64)h << 32) | l;
    k = n > k ? n : k;
  }
  return k;
}

}  // namespace

__global__ __launch_bounds__(FSTC_THREADS) void k_fst_conf_tokens(const FstParams p, FstConfRecord *rec) {
  __shared__ u64 s_key[FSTC_THREADS / 64];
  __shared__ uint32_t s_img[FSTC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t u = (int32_t)blockIdx.x;
  int32_t n = p.result[u].n_tokens;
  n = n < 0 ? 0 : (n > p.cap_tok ? p.cap_tok : n);
  const int32_t *t_node = p.t_node + (size_t)u * p.cap_tok, *t_hist = p.t_hist + (size_t)u * p.cap_tok;
  const float *t_lp = p.t_lp + (size_t)u * p.cap_tok;

  // the best end-node token: k_fst_search's key, the log-probability's image above the complement of the token's index
  u64 k = 0;
  for (int32_t i = tid; i < n; i += FSTC_THREADS) {
    if (p.node_end[t_node[i]]) {
      const u64 c = ((u64)float_image(t_lp[i]) << 32) | (uint32_t)~(uint32_t)i;
      k = c > k ? c : k;
    }
  }
  k = wave_max(k);
  if (lane == 0) s_key[w] = k;
  __syncthreads();
  k = 0;
#pragma unroll
  for (int i = 0; i < FSTC_THREADS / 64; i++) k = s_key[i] > k ? s_key[i] : k;
  FstConfRecord r;
  r.best_final_hist = 0;
  r.best_final_n_words = 0;
  r.has_final = 0;
  r.has_different = 0;
  r.best_final_lp = FSTC_NONE;
  r.best_different_lp = FSTC_NONE;
  if (k == 0) {  // (the whole workgroup)
    if (tid == 0) rec[u] = r;
    return;
  }
  const int32_t ib = (int32_t)~(uint32_t)k;
  const int32_t hist = t_hist[ib];
  uint32_t m = 0;  // the image of no float that a search produces
  for (int32_t i = tid; i < n; i += FSTC_THREADS) {
    if (t_hist[i] != hist) {
      const uint32_t x = float_image(t_lp[i]);
      m = x > m ? x : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = (uint32_t)__shfl_xor((int)m, o, 64);
    m = x > m ? x : m;
  }
  if (lane == 0) s_img[w] = m;
  __syncthreads();
  if (tid == 0) {
    m = 0;
    for (int i = 0; i < FSTC_THREADS / 64; i++) m = s_img[i] > m ? s_img[i] : m;
    r.best_final_hist = hist;
    r.best_final_n_words = hist == 0 ? 0 : p.result[u].n_words;
    r.has_final = 1;
    r.best_final_lp = t_lp[ib];
    if (m) {
      r.has_different = 1;
      r.best_different_lp = image_float(m);
    }
    rec[u] = r;
  }
}

void fst_frame_best_launch(const FstFrameBestParams &p, int64_t total_frames, hipStream_t st) {
  if (p.n_utt <= 0) return;
  if (total_frames > 0) {
    // lanes per row: the power of two, 8 ... 64, that covers the row's 16-byte chunks (one more when it starts off the grid)
    FstFrameBestParams q = p;
    const size_t chunks = ((size_t)p.n_models * (size_t)p.lnabytes + 15) / 16 + 1;
    q.lanes_per_row = chunks > 32 ? 64 : chunks > 16 ? 32 : chunks > 8 ? 16 : 8;
    const int64_t rows_per_group = (int64_t)(FSTC_THREADS / 64) * (64 / q.lanes_per_row);
    const dim3 grid((unsigned)((total_frames + rows_per_group - 1) / rows_per_group)), block(FSTC_THREADS);
    if (p.lnabytes == 4)
      hipLaunchKernelGGL(k_fst_frame_best<4>, grid, block, 0, st, q, total_frames);
    else if (p.lnabytes == 2)
      hipLaunchKernelGGL(k_fst_frame_best<2>, grid, block, 0, st, q, total_frames);
    else
      hipLaunchKernelGGL(k_fst_frame_best<1>, grid, block, 0, st, q, total_frames);
  }
  hipLaunchKernelGGL(k_fst_frame_sum, dim3((unsigned)((p.n_utt + FSTC_THREADS / 64 - 1) / (FSTC_THREADS / 64))), dim3(FSTC_THREADS), 0, st, p);
}

void fst_conf_tokens_launch(const FstParams &p, FstConfRecord *rec, int32_t n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_fst_conf_tokens, dim3((unsigned)n_launch), dim3(FSTC_THREADS), 0, st, p, rec);
}

}  // namespace aasr

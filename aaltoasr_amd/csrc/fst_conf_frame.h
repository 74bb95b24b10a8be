// fst_conf_frame.h -- the device bodies of the FST decoder's confidence, shared by the batch passes (fst_conf.hip:
// k_fst_frame_best, k_fst_conf_tokens) and the streaming entry (fst_conf_stream.hip: k_fst_conf_chunk).  One copy of
// the frame-best row sweep and of the token record; rules: fst_conf.h.  Included by device code only.
#pragma once
#include "fst_conf.h"
#include "fst_frame.h"

namespace aasr {

namespace {

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

// The best acoustic value of the row at bytes [s, e), swept by lpr neighbouring lanes of a wave (lpr a power of two,
// this lane the sub-th of them): 16-byte chunks on the address space's 16-byte grid, the ragged ends element by element,
// nothing outside the row read.  Every lane of the wave calls it (the lanes shuffle); every lane of the row gets the value.
template <int BYTES>
__device__ __forceinline__ float fst_row_best(uintptr_t s, uintptr_t e, int sub, int lpr, const float *decode) {
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
  return BYTES == 4 ? best.v : decode[code];  // (a row has at least one model: code is one)
}

// lanes per row: the power of two, 8 ... 64, that covers the row's 16-byte chunks (one more when it starts off the grid)
inline int fst_lanes_per_row(int32_t n_models, int32_t lnabytes) {
  const size_t chunks = ((size_t)n_models * (size_t)lnabytes + 15) / 16 + 1;
  return chunks > 32 ? 64 : chunks > 16 ? 32 : chunks > 8 ? 16 : 8;
}

__device__ __forceinline__ u64 wave_max(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t h = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), o, 64), l = (uint32_t)__shfl_xor((int)(uint32_t)k, o, 64);
    const u64 n = ((u64)h << 32) | l;
    k = n > k ? n : k;
  }
  return k;
}

// the record's LDS: 48 bytes of wave results
struct FstConfLds {
  u64 key[FSTC_THREADS / 64];
  uint32_t img[FSTC_THREADS / 64];
};

// The token record of utterance (session) u over the tokens its search left: t_node, t_lp, t_hist, result[u].n_tokens.
// Every lane of the workgroup calls it; result[u] and the tokens must be visible to every lane (a barrier behind the
// lane that wrote them).
__device__ __forceinline__ void fst_conf_record(const FstParams &p, int32_t u, FstConfLds &s, FstConfRecord *rec) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t n = p.result[u].n_tokens;
  n = n < 0 ? 0 : (n > p.cap_tok ? p.cap_tok : n);
  const int32_t *t_node = p.t_node + (size_t)u * p.cap_tok, *t_hist = p.t_hist + (size_t)u * p.cap_tok;
  const float *t_lp = p.t_lp + (size_t)u * p.cap_tok;

  // the best end-node token: k_fst_search's key, the log-probability's image above the complement of the token's index
  u64 k = 0;
  for (int32_t i = tid; i < n; i += FSTC_THREADS) {
    if (p.node_end[t_node[i]]) {
      const u64 c = cand_key(t_lp[i], i);
      k = c > k ? c : k;
    }
  }
  k = wave_max(k);
  if (lane == 0) s.key[w] = k;
  __syncthreads();
  k = 0;
#pragma unroll
  for (int i = 0; i < FSTC_THREADS / 64; i++) k = s.key[i] > k ? s.key[i] : k;
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
  if (lane == 0) s.img[w] = m;
  __syncthreads();
  if (tid == 0) {
    m = 0;
    for (int i = 0; i < FSTC_THREADS / 64; i++) m = s.img[i] > m ? s.img[i] : m;
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

}  // namespace

}  // namespace aasr

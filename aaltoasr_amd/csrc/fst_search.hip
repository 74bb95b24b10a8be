// fst_search.hip -- the FST decoder's token pass: one workgroup per utterance, the frame loop inside (layout, phases
// and the reference's line numbers: fst_search.h).
#include "fst_search.h"

namespace aasr {

namespace {

typedef unsigned long long u64;
constexpr u64 FST_EMPTY = ~0ull;

__device__ __forceinline__ uint32_t float_image(float x) {  // unsigned order = float order
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 cand_key(float lp, int32_t c) { return ((u64)float_image(lp) << 32) | (uint32_t)~(uint32_t)c; }

// the tables are written with atomics only and read past the lane's cache
__device__ __forceinline__ u64 table_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void table_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t mix(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

// slot of key in an open-addressing table of mask + 1 entries, inserting it when absent (*made = 1); -1: table full
__device__ __forceinline__ int32_t table_slot(u64 *keys, uint32_t mask, u64 key, int *made) {
  uint32_t s = mix(key) & mask;
  for (uint32_t n = 0; n <= mask; n++) {
    const u64 cur = atomicCAS(&keys[s], FST_EMPTY, key);
    if (cur == FST_EMPTY) {
      *made = 1;
      return (int32_t)s;
    }
    if (cur == key) return (int32_t)s;
    s = (s + 1) & mask;
  }
  return -1;
}

// exclusive scan of v over the workgroup; total: the sum.  Every lane calls it.
__device__ __forceinline__ int block_scan(int v, int *s_wave, int &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(incl, o, 64);
    if (lane >= o) incl += n;
  }
  __syncthreads();  // (the totals of the previous call are read)
  if (lane == 63) s_wave[w] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < FST_THREADS / 64; i++) {
    const int x = s_wave[i];
    if (i < w) base += x;
    total += x;
  }
  return base + incl - v;
}

__device__ __forceinline__ float acoustic(const FstParams &p, const uint8_t *row, int32_t pdf) {
  if (p.lnabytes == 4) return reinterpret_cast<const float *>(row)[pdf];
  if (p.lnabytes == 2) return p.decode[((uint32_t)row[2 * pdf] << 8) | row[2 * pdf + 1]];
  return p.decode[row[pdf]];
}

}  // namespace

__global__ __launch_bounds__(FST_THREADS) void k_fst_search(const FstParams p) {
  __shared__ unsigned s_hist[256];
  __shared__ int s_wave[FST_THREADS / 64];
  __shared__ u64 s_best, s_best_final;
  __shared__ int s_flag, s_nhist, s_bin, s_rem;

  const int tid = threadIdx.x;
  const int32_t u = (int32_t)blockIdx.x;
  const int32_t T = p.n_frames[u];
  int32_t *t_node = p.t_node + (size_t)u * p.cap_tok, *t_dur = p.t_dur + (size_t)u * p.cap_tok;
  int32_t *t_hist = p.t_hist + (size_t)u * p.cap_tok, *t_off = p.t_off + (size_t)u * (p.cap_tok + 1);
  float *t_lp = p.t_lp + (size_t)u * p.cap_tok;
  float *c_lp = p.c_lp + (size_t)u * p.cap_cand;
  int32_t *c_tok = p.c_tok + (size_t)u * p.cap_cand, *c_node = p.c_node + (size_t)u * p.cap_cand;
  int32_t *c_dur = p.c_dur + (size_t)u * p.cap_cand, *c_hist = p.c_hist + (size_t)u * p.cap_cand;
  int32_t *c_slot = p.c_slot + (size_t)u * p.cap_cand;
  u64 *w_key = p.w_key + (size_t)u * p.cap_cand;
  u64 *r_key = p.r_key + (size_t)u * p.cap_recomb, *r_val = p.r_val + (size_t)u * p.cap_recomb;
  u64 *h_key = p.h_key + (size_t)u * p.cap_hist;
  const uint32_t r_mask = (uint32_t)p.cap_recomb - 1, h_mask = (uint32_t)p.cap_hist - 1;

  for (int32_t i = tid; i < p.cap_recomb; i += FST_THREADS) {
    table_store(&r_key[i], FST_EMPTY);
    table_store(&r_val[i], 0);
  }
  for (int32_t i = tid; i < p.cap_hist; i += FST_THREADS) table_store(&h_key[i], FST_EMPTY);
  if (tid == 0) {
    t_node[0] = p.initial;  // FstSearch_tmpl.hh:45-51
    t_lp[0] = 0.0f;
    t_dur[0] = 0;
    t_hist[0] = 0;
    s_flag = 0;
    s_nhist = 0;
  }
  int32_t n_act = 1, status = FST_OK;
  const int64_t K = (int64_t)p.token_limit + 1;
  __threadfence();
  __syncthreads();

  for (int32_t t = 0; t < T; t++) {
    // (1) offsets of the tokens' arcs among the frame's candidates
    int64_t total = 0;
    for (int32_t base = 0; base < n_act; base += FST_THREADS) {
      const int32_t i = base + tid;
      int deg = 0;
      if (i < n_act) {
        const int32_t node = t_node[i];
        deg = p.arc_begin[node + 1] - p.arc_begin[node];
      }
      int tot;
      const int ex = block_scan(deg, s_wave, tot);
      if (i < n_act) t_off[i] = (int32_t)(total + ex);  // (garbage past cap_cand is never read: the frame ends below)
      total += tot;
    }
    if (total == 0) {
      status = FST_NO_TOKENS;
      n_act = 0;
      break;
    }
    if (total > p.cap_cand) {
      status = FST_OVERFLOW_CANDIDATES;
      n_act = 0;
      break;
    }
    const int32_t n_cand = (int32_t)total;
    if (tid == 0) s_best = 0;
    __syncthreads();

    // (2) every candidate's log-probability, FstSearch_tmpl.hh:198-218, and the frame's best
    const uint8_t *row = p.lna + (size_t)(p.row0[u] + t) * (size_t)p.n_models * (size_t)p.lnabytes;
    u64 my_best = 0;
    for (int32_t c = tid; c < n_cand; c += FST_THREADS) {
      int32_t lo = 0, hi = n_act - 1;  // the last token whose offset is <= c
      while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (t_off[mid] <= c)
          lo = mid;
        else
          hi = mid - 1;
      }
      const int32_t node = t_node[lo];
      const int32_t a = p.arc_begin[node] + (c - t_off[lo]);
      const int32_t tgt = p.arc_tgt[a];
      float lp = __fadd_rn(t_lp[lo], __fmul_rn(p.transition_scale, p.arc_lp[a]));
      const int32_t tp = p.node_pdf[tgt];
      if (tp >= 0) lp = __fadd_rn(lp, acoustic(p, row, tp));
      if (tgt != node) {
        const int32_t sp = p.node_pdf[node];
        if (sp >= 0) {
          float dl = 0.0f;
          if (p.dur_slot) {
            const int32_t sl = p.dur_slot[sp];
            if (sl >= 0) dl = p.dur_table[(size_t)sl * (size_t)(p.D + 1) + (size_t)t_dur[lo]];
          }
          lp = __fadd_rn(lp, __fmul_rn(p.duration_scale, dl));
        }
      }
      c_lp[c] = lp;
      c_tok[c] = lo;
      const u64 k = cand_key(lp, c);
      my_best = k > my_best ? k : my_best;
    }
    if (my_best) atomicMax(&s_best, my_best);
    __syncthreads();
    const int32_t best_c = (int32_t)~(uint32_t)s_best;
    const float thr = __fsub_rn(c_lp[best_c], p.beam);

    // (3) the candidates within the beam: history, then recombination on (node, history)
    for (int32_t c = tid; c < n_cand; c += FST_THREADS) {
      const float lp = c_lp[c];
      int32_t slot = -1;
      if (lp > thr || c == best_c) {
        const int32_t i = c_tok[c];
        const int32_t node = t_node[i];
        const int32_t a = p.arc_begin[node] + (c - t_off[i]);
        const int32_t tgt = p.arc_tgt[a];
        const int32_t word = p.arc_word[a];
        const int32_t dur = tgt != node ? (p.node_pdf[node] >= 0 ? 1 : t_dur[i]) : t_dur[i] + 1;
        int32_t hist = t_hist[i];
        if (word >= 0) {
          int made = 0;
          const int32_t s = table_slot(h_key, h_mask, ((u64)(uint32_t)hist << 32) | (uint32_t)word, &made);
          if (made) atomicAdd(&s_nhist, 1);
          if (s < 0) atomicOr(&s_flag, 2);
          hist = s + 1;
        }
        c_node[c] = tgt;
        c_dur[c] = dur;
        c_hist[c] = hist;
        int made = 0;
        slot = table_slot(r_key, r_mask, ((u64)(uint32_t)tgt << 32) | (uint32_t)hist, &made);
        if (slot < 0)
          atomicOr(&s_flag, 1);
        else
          atomicMax(&r_val[slot], cand_key(lp, c));
      }
      c_slot[c] = slot;
    }
    __threadfence();
    __syncthreads();
    if (s_flag || s_nhist > p.cap_hist - p.cap_hist / 4) {  // (the history table is kept at most three quarters full)
      status = (s_flag & 1) ? FST_OVERFLOW_RECOMB : FST_OVERFLOW_HISTORY;
      n_act = 0;
      break;
    }

    // (4) the winners' keys in candidate order
    int32_t n_win = 0;
    for (int32_t base = 0; base < n_cand; base += FST_THREADS) {
      const int32_t c = base + tid;
      int win = 0;
      u64 k = 0;
      if (c < n_cand && c_slot[c] >= 0) {
        k = cand_key(c_lp[c], c);
        win = table_load(&r_val[c_slot[c]]) == k;
      }
      int tot;
      const int ex = block_scan(win, s_wave, tot);
      if (win) w_key[n_win + ex] = k;
      n_win += tot;
    }
    __syncthreads();
    for (int32_t c = tid; c < n_cand; c += FST_THREADS) {  // the table is empty again for the next frame
      const int32_t s = c_slot[c];
      if (s >= 0) {
        table_store(&r_key[s], FST_EMPTY);
        table_store(&r_val[s], 0);
      }
    }

    // (5) the token limit: the K-th largest key, FstSearch_tmpl.hh:101-102 (K = limit + 1)
    u64 kth = 0;
    if ((int64_t)n_win > K) {
      u64 prefix = 0;
      int32_t remaining = (int32_t)K;
      for (int shift = 56; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();
        for (int32_t j = tid; j < n_win; j += FST_THREADS) {
          const u64 k = w_key[j];
          if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          int32_t acc = 0, b = 255;
          for (; b > 0; b--) {
            if (acc + (int32_t)s_hist[b] >= remaining) break;
            acc += (int32_t)s_hist[b];
          }
          s_bin = b;
          s_rem = remaining - acc;
        }
        __syncthreads();
        prefix |= (u64)(unsigned)s_bin << shift;
        remaining = s_rem;
        __syncthreads();
      }
      kth = prefix;
    }

    // (6) the selected winners are the next frame's tokens
    int32_t n_new = 0;
    for (int32_t base = 0; base < n_win; base += FST_THREADS) {
      const int32_t j = base + tid;
      u64 k = 0;
      int sel = 0;
      if (j < n_win) {
        k = w_key[j];
        sel = k >= kth;
      }
      int tot;
      const int ex = block_scan(sel, s_wave, tot);
      if (sel) {
        const int32_t c = (int32_t)~(uint32_t)k, o = n_new + ex;
        t_node[o] = c_node[c];
        t_lp[o] = c_lp[c];
        t_dur[o] = c_dur[c];
        t_hist[o] = c_hist[c];
      }
      n_new += tot;
    }
    n_act = n_new;
    __threadfence();
    __syncthreads();
  }

  // result, FstSearch_tmpl.hh:151-176: the best token, the best token at an end node and its words
  if (tid == 0) {
    s_best = 0;
    s_best_final = 0;
  }
  __syncthreads();
  for (int32_t i = tid; i < n_act; i += FST_THREADS) {
    const u64 k = cand_key(t_lp[i], i);
    atomicMax(&s_best, k);
    if (p.node_end[t_node[i]]) atomicMax(&s_best_final, k);
  }
  __syncthreads();
  if (tid == 0) {
    FstResult r;
    r.status = status;
    r.n_tokens = n_act;
    r.n_words = 0;
    r.logprob = -1.0f;
    r.best_lp = s_best ? t_lp[(int32_t)~(uint32_t)s_best] : -9999999.0f;
    r.best_final_lp = -9999999.9f;
    if (s_best_final) {
      const int32_t i = (int32_t)~(uint32_t)s_best_final;
      r.logprob = r.best_final_lp = t_lp[i];
      int32_t n = 0;
      for (int32_t h = t_hist[i]; h > 0 && n <= p.cap_hist; h = (int32_t)(table_load(&h_key[h - 1]) >> 32)) n++;
      int32_t *words = p.res_words + (size_t)u * p.cap_words;
      if (n <= p.cap_words) {  // (a path has at most one word per frame: always)
        int32_t at = n;
        for (int32_t h = t_hist[i]; h > 0 && at > 0; h = (int32_t)(table_load(&h_key[h - 1]) >> 32))
          words[--at] = (int32_t)(uint32_t)table_load(&h_key[h - 1]);
        r.n_words = n;
      } else {
        r.n_words = -1;
      }
    }
    p.result[u] = r;
  }
}

void fst_search_launch(const FstParams &p, int32_t n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_fst_search, dim3((unsigned)n_launch), dim3(FST_THREADS), 0, st, p);
}

}  // namespace aasr

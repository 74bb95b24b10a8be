// fst_frame.h -- the device body of the FST token pass, shared by its entries: k_fst_search (fst_search.hip, an
// utterance's whole frame loop in one launch), k_fst_search_chunk (fst_stream.hip, the frames of one feed of a
// session) and, through fst_chunk.h, k_fst_conf_chunk (fst_conf_stream.hip).  One copy of the arithmetic: the start of a
// search, the six phases of a frame and the result block are the functions below, forced inline into the kernels.
// Layout, phases and the reference's line numbers: fst_search.h.
// Included by device code only.
#pragma once
#include "fst_search.h"

namespace aasr {

namespace {

typedef unsigned long long u64;
constexpr u64 FST_EMPTY = ~0ull;

// the workgroup's LDS (1 072 bytes): the radix select's histogram, the scans' wave totals, the best keys, flags
struct FstLds {
  unsigned hist[256];
  int wave[FST_THREADS / 64];
  u64 best, best_final;
  int flag, nhist, bin, rem;
};

// one utterance's (one session's) slices of the batch's buffers
struct FstUtt {
  int32_t *t_node, *t_dur, *t_hist, *t_off;
  float *t_lp, *c_lp;
  int32_t *c_tok, *c_node, *c_dur, *c_hist, *c_slot;
  u64 *w_key, *r_key, *r_val, *h_key;
};

__device__ __forceinline__ FstUtt fst_utt(const FstParams &p, int32_t u) {
  FstUtt m;
  m.t_node = p.t_node + (size_t)u * p.cap_tok;
  m.t_dur = p.t_dur + (size_t)u * p.cap_tok;
  m.t_hist = p.t_hist + (size_t)u * p.cap_tok;
  m.t_off = p.t_off + (size_t)u * (p.cap_tok + 1);
  m.t_lp = p.t_lp + (size_t)u * p.cap_tok;
  m.c_lp = p.c_lp + (size_t)u * p.cap_cand;
  m.c_tok = p.c_tok + (size_t)u * p.cap_cand;
  m.c_node = p.c_node + (size_t)u * p.cap_cand;
  m.c_dur = p.c_dur + (size_t)u * p.cap_cand;
  m.c_hist = p.c_hist + (size_t)u * p.cap_cand;
  m.c_slot = p.c_slot + (size_t)u * p.cap_cand;
  m.w_key = p.w_key + (size_t)u * p.cap_cand;
  m.r_key = p.r_key + (size_t)u * p.cap_recomb;
  m.r_val = p.r_val + (size_t)u * p.cap_recomb;
  m.h_key = p.h_key + (size_t)u * p.cap_hist;
  return m;
}

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

// The start of a search: both tables empty, one token at the initial node (FstSearch_tmpl.hh:45-51).  Every lane calls it;
// the workgroup is synchronised when it returns.
__device__ __forceinline__ void fst_start(const FstParams &p, const FstUtt &m, FstLds &s) {
  const int tid = threadIdx.x;
  for (int32_t i = tid; i < p.cap_recomb; i += FST_THREADS) {
    table_store(&m.r_key[i], FST_EMPTY);
    table_store(&m.r_val[i], 0);
  }
  for (int32_t i = tid; i < p.cap_hist; i += FST_THREADS) table_store(&m.h_key[i], FST_EMPTY);
  if (tid == 0) {
    m.t_node[0] = p.initial;
    m.t_lp[0] = 0.0f;
    m.t_dur[0] = 0;
    m.t_hist[0] = 0;
    s.flag = 0;
    s.nhist = 0;
  }
  __threadfence();
  __syncthreads();
}

// One frame over the acoustic row `row`: n_act tokens in, n_act tokens out.  FST_OK, or the status that ends the search
// (n_act is 0 then).  Every lane calls it and every lane gets the same answer; the workgroup is synchronised on FST_OK.
__device__ __forceinline__ int32_t fst_frame(const FstParams &p, const FstUtt &m, FstLds &s, const uint8_t *row, int32_t &n_act) {
  const int tid = threadIdx.x;
  int32_t *t_node = m.t_node, *t_dur = m.t_dur, *t_hist = m.t_hist, *t_off = m.t_off;
  float *t_lp = m.t_lp, *c_lp = m.c_lp;
  int32_t *c_tok = m.c_tok, *c_node = m.c_node, *c_dur = m.c_dur, *c_hist = m.c_hist, *c_slot = m.c_slot;
  u64 *w_key = m.w_key, *r_key = m.r_key, *r_val = m.r_val, *h_key = m.h_key;
  const uint32_t r_mask = (uint32_t)p.cap_recomb - 1, h_mask = (uint32_t)p.cap_hist - 1;
  const int64_t K = (int64_t)p.token_limit + 1;

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
    const int ex = block_scan(deg, s.wave, tot);
    if (i < n_act) t_off[i] = (int32_t)(total + ex);  // (garbage past cap_cand is never read: the frame ends below)
    total += tot;
  }
  if (total == 0) {
    n_act = 0;
    return FST_NO_TOKENS;
  }
  if (total > p.cap_cand) {
    n_act = 0;
    return FST_OVERFLOW_CANDIDATES;
  }
  const int32_t n_cand = (int32_t)total;
  if (tid == 0) s.best = 0;
  __syncthreads();

  // (2) every candidate's log-probability, FstSearch_tmpl.hh:198-218, and the frame's best
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
  if (my_best) atomicMax(&s.best, my_best);
  __syncthreads();
  const int32_t best_c = (int32_t)~(uint32_t)s.best;
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
        const int32_t sl = table_slot(h_key, h_mask, ((u64)(uint32_t)hist << 32) | (uint32_t)word, &made);
        if (made) atomicAdd(&s.nhist, 1);
        if (sl < 0) atomicOr(&s.flag, 2);
        hist = sl + 1;
      }
      c_node[c] = tgt;
      c_dur[c] = dur;
      c_hist[c] = hist;
      int made = 0;
      slot = table_slot(r_key, r_mask, ((u64)(uint32_t)tgt << 32) | (uint32_t)hist, &made);
      if (slot < 0)
        atomicOr(&s.flag, 1);
      else
        atomicMax(&r_val[slot], cand_key(lp, c));
    }
    c_slot[c] = slot;
  }
  __threadfence();
  __syncthreads();
  if (s.flag || s.nhist > p.cap_hist - p.cap_hist / 4) {  // (the history table is kept at most three quarters full)
    n_act = 0;
    return (s.flag & 1) ? FST_OVERFLOW_RECOMB : FST_OVERFLOW_HISTORY;
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
    const int ex = block_scan(win, s.wave, tot);
    if (win) w_key[n_win + ex] = k;
    n_win += tot;
  }
  __syncthreads();
  for (int32_t c = tid; c < n_cand; c += FST_THREADS) {  // the table is empty again for the next frame
    const int32_t sl = c_slot[c];
    if (sl >= 0) {
      table_store(&r_key[sl], FST_EMPTY);
      table_store(&r_val[sl], 0);
    }
  }

  // (5) the token limit: the K-th largest key, FstSearch_tmpl.hh:101-102 (K = limit + 1)
  u64 kth = 0;
  if ((int64_t)n_win > K) {
    u64 prefix = 0;
    int32_t remaining = (int32_t)K;
    for (int shift = 56; shift >= 0; shift -= 8) {
      s.hist[tid] = 0;
      __syncthreads();
      for (int32_t j = tid; j < n_win; j += FST_THREADS) {
        const u64 k = w_key[j];
        if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s.hist[(unsigned)(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        int32_t acc = 0, b = 255;
        for (; b > 0; b--) {
          if (acc + (int32_t)s.hist[b] >= remaining) break;
          acc += (int32_t)s.hist[b];
        }
        s.bin = b;
        s.rem = remaining - acc;
      }
      __syncthreads();
      prefix |= (u64)(unsigned)s.bin << shift;
      remaining = s.rem;
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
    const int ex = block_scan(sel, s.wave, tot);
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
  return FST_OK;
}

// the words of history id h, oldest first, into words[cap]: their number, or -1 when they do not fit.  One lane.
__device__ __forceinline__ int32_t fst_history_words(const FstParams &p, const FstUtt &m, int32_t h0, int32_t *words, int32_t cap) {
  int32_t n = 0;
  for (int32_t h = h0; h > 0 && n <= p.cap_hist; h = (int32_t)(table_load(&m.h_key[h - 1]) >> 32)) n++;
  if (n > cap) return -1;  // (a path has at most one word per frame: never)
  int32_t at = n;
  for (int32_t h = h0; h > 0 && at > 0; h = (int32_t)(table_load(&m.h_key[h - 1]) >> 32))
    words[--at] = (int32_t)(uint32_t)table_load(&m.h_key[h - 1]);
  return n;
}

// The result, FstSearch_tmpl.hh:151-176: the best token, the best token at an end node and its words, into result[u] and
// res_words.  Every lane calls it; s.best holds the best token's key (0: no token) for lane 0 when it returns.
__device__ __forceinline__ void fst_result(const FstParams &p, const FstUtt &m, FstLds &s, int32_t u, int32_t status, int32_t n_act) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    s.best = 0;
    s.best_final = 0;
  }
  __syncthreads();
  for (int32_t i = tid; i < n_act; i += FST_THREADS) {
    const u64 k = cand_key(m.t_lp[i], i);
    atomicMax(&s.best, k);
    if (p.node_end[m.t_node[i]]) atomicMax(&s.best_final, k);
  }
  __syncthreads();
  if (tid == 0) {
    FstResult r;
    r.status = status;
    r.n_tokens = n_act;
    r.n_words = 0;
    r.logprob = -1.0f;
    r.best_lp = s.best ? m.t_lp[(int32_t)~(uint32_t)s.best] : -9999999.0f;
    r.best_final_lp = -9999999.9f;
    if (s.best_final) {
      const int32_t i = (int32_t)~(uint32_t)s.best_final;
      r.logprob = r.best_final_lp = m.t_lp[i];
      r.n_words = fst_history_words(p, m, m.t_hist[i], p.res_words + (size_t)u * p.cap_words, p.cap_words);
    }
    p.result[u] = r;
  }
}

}  // namespace

}  // namespace aasr

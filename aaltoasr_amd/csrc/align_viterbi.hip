// align_viterbi.hip -- the forced aligner's Viterbi search on the device (aku/Viterbi.cc,
// aku/Lattice.cc and the window loop of aku/align.cc:viterbi_align), one wave64 per utterance.
//
// What is restated exactly, arithmetic and types included:
//   * cells hold a float log-probability; "unused" is the finite sentinel -1e24 (Lattice.hh INF);
//   * pruning of the previous frame from both range ends by the probability beam (float sum) and
//     the state beam (fill_transition_probs), against m_best_log_prob / m_best_position as they
//     stand -- after a move these are the values from before the renormalisation, as in the
//     reference;
//   * transitions: the reference pushes from sources in ascending position, transitions in .ph
//     order, replacing on a strict '>'; here each target pulls, and keeps the largest value, on a
//     tie the smallest source, on a further tie that source's first transition: the same winner;
//   * observation: lik = (float)exp((double)ll) (HmmSet::state_likelihood stored in a float),
//     best over the live range in float, (float)(safe_log(lik) - best_log), added in float, the
//     best cell by strict '>' in ascending position, cells below -1e24 floored;
//   * compute_best_path with the forced end, move() with its renormalisation of the last kept
//     frame, and the retry with doubled beams when the forced end falls outside the window or range.
// Layout: the lattice is a ring of swins frames (slot = absolute frame mod swins) of `width`
// cells each; a frame's cells are stored from its range start at creation (its origin), so a move
// copies nothing: it only advances the frame and position bases.  Back-pointers are the source's
// distance below the target (uint8: the topology's largest target offset is <= 255).  The previous
// frame's cells live in LDS.
#include <hip/hip_runtime.h>

#include <cmath>

#include "align.h"
#include "common.h"

namespace aasr {

#define AL_INF 1e24f

__device__ __forceinline__ double al_safe_log(double x) { return x < 1e-50 ? log(1e-50) : log(x); }

__device__ __forceinline__ double al_ll(const AlignParams &P, int64_t row, int state) {
  if (P.f64) return ((const double *)P.scores)[row * P.pitch + state];
  return (double)((const float *)P.scores)[row * P.pitch + state];
}

// first lane (lowest position) whose predicate holds, over a range striped in chunks of 64
__device__ __forceinline__ int wave_min_int(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_float(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct AlShared {
  AlignRun R;
  int o_prev, s_prev, e_prev;  // previous frame: storage origin, range
  int flag;
};

__global__ __launch_bounds__(64) void k_align_viterbi(AlignParams P, int32_t windows) {
  extern __shared__ float lds[];
  __shared__ AlShared sh;
  const int u = blockIdx.x, lane = threadIdx.x;
  const AlignUttDev U = P.utt[u];
  float *prev = lds, *curb = lds + P.width, *likb = lds + 2 * P.width;
  float *cells = P.cells + U.cells_begin;
  uint8_t *back = P.back + U.cells_begin;
  int32_t *meta = P.meta + 3 * U.meta_begin;
  int32_t *path = P.path + U.meta_begin;
  const int32_t *trs = P.tr_state + U.pos_begin;
  const int32_t *inb = P.in_begin + U.pos_begin;
  const int32_t *lines = P.line_states + U.line_begin;
  const int W = P.width, SW = P.swins;

  if (lane == 0) sh.R = P.run[u];
  __syncthreads();
  if (sh.R.status != ALIGN_ACTIVE) return;

#define R sh.R
#define FAIL(code)            \
  do {                        \
    if (lane == 0) {          \
      R.status = ALIGN_ERROR; \
      R.error = (code);       \
    }                         \
    __syncthreads();          \
    goto done;                \
  } while (0)

  for (int w = 0; w < windows; w++) {
    if (R.status != ALIGN_ACTIVE) break;
    __syncthreads();
    if (R.fresh) {  // Viterbi::reset + viterbi_align's start
      if (lane == 0) {
        R.fresh = 0;
        R.acc = 0;
        R.fin = 0;
        R.best = -AL_INF;
        R.bestpos = -1;
        R.wstart = U.start_frame;
        R.ffr = U.start_frame;
        R.cur = 0;
        R.base = 0;
        R.loaded = 0;
        R.line = 0;
        R.tr_eof = 0;
        R.lim = SW;
        R.committed = 0;
      }
      __syncthreads();
    }
    // window borders (align.cc:77-86)
    int wend = R.wstart + SW;
    bool last_window = false;
    if (U.end_frame > 0) {
      if (R.wstart >= U.end_frame) {
        if (lane == 0) R.status = ALIGN_OK;
        __syncthreads();
        break;
      }
      if (wend >= U.end_frame) {
        wend = U.end_frame;
        last_window = true;
      }
    }
    int last_frame = wend - R.wstart;
    __syncthreads();
    // Viterbi::fill_transcription: whole HMMs until m_last_position positions are loaded
    if (lane == 0) {
      int size = R.loaded - R.base;
      if (size == 0) {
        R.line = 0;
        R.tr_eof = U.n_lines <= 0;
      }
      while (!R.tr_eof && size < R.lim) {
        const int n = lines[R.line];
        size += n;
        R.loaded += n;
        R.line++;
        R.tr_eof = R.line >= U.n_lines;
      }
      if (R.lim > size) R.lim = size;
    }
    __syncthreads();
    if (R.loaded - R.base <= 0) FAIL(1);  // empty transcription
    if (R.cur == 0) {  // lattice frame 0: position 0 with log-probability 0
      if (lane == 0) {
        const int s0 = R.wstart % SW;
        meta[3 * s0] = R.base;
        meta[3 * s0 + 1] = R.base;
        meta[3 * s0 + 2] = R.base + 1;
        cells[(int64_t)s0 * W] = 0.f;
        back[(int64_t)s0 * W] = 0;
        prev[0] = 0.f;
        sh.o_prev = R.base;
        sh.s_prev = R.base;
        sh.e_prev = R.base + 1;
        R.acc = al_safe_log(exp(al_ll(P, U.row0 + (R.ffr - U.start_frame), trs[R.base])));
        R.ffr++;
        R.cur = 1;
      }
      __syncthreads();
    } else {  // the last filled frame from the ring
      const int sl = (R.wstart + R.cur - 1) % SW;
      const int o = meta[3 * sl], s = meta[3 * sl + 1], e = meta[3 * sl + 2];
      for (int p = s + lane; p < e; p += 64) prev[p - o] = cells[(int64_t)sl * W + (p - o)];
      if (lane == 0) {
        sh.o_prev = o;
        sh.s_prev = s;
        sh.e_prev = e;
      }
      __syncthreads();
    }
    bool eof_hit = false;
    while (R.cur < last_frame) {
      if (R.ffr >= U.eof_frame) {  // FeatureGenerator::eof after generate()
        last_frame = R.cur;
        eof_hit = true;
        break;
      }
      const int t = R.cur;
      const float beam = (float)R.beam;
      const int sbeam = R.sbeam;
      const float B = R.best;
      const int bp = R.bestpos;
      const int o = sh.o_prev, s = sh.s_prev, e = sh.e_prev;
      const bool prev0 = (t - 1) == 0;  // lattice frame 0: every cell has from < 0
      // prune at the beginning
      int ns = INT_MAX;
      for (int c = s; c < e && ns == INT_MAX; c += 64) {
        const int p = c + lane;
        bool keep = false;
        if (p < e) {
          const float v = prev[p - o];
          const bool unused = prev0 && v == -AL_INF;
          keep = !(unused || v + beam < B || p + sbeam < bp);
        }
        const unsigned long long m = __ballot(keep);
        if (m) ns = c + __ffsll((long long)m) - 1;
      }
      if (ns == INT_MAX) FAIL(2);
      // prune at the end
      int ne = -1;
      for (int c = e - 1; c >= ns && ne < 0; c -= 64) {
        const int p = c - lane;
        bool keep = false;
        if (p >= ns) {
          const float v = prev[p - o];
          const bool unused = prev0 && v == -AL_INF;
          keep = !(unused || v + beam < B || p - sbeam > bp);
        }
        const unsigned long long m = __ballot(keep);
        if (m) ne = c - (__ffsll((long long)m) - 1) + 1;
      }
      if (ne < 0) FAIL(2);
      // transitions, pulled by the targets: one pass over [ns, tmax] finds each target's best source
      // (its incoming list is ordered by source position, then transition), its likelihood, and whether
      // any source reaches it.  The new frame is stored from ns: ns <= ts and te - ns <= width.
      const int lim_abs = R.base + R.lim;
      const int tmax = min(ne - 1 + P.max_off, lim_abs - 1);
      if (tmax - ns + 1 > W) FAIL(4);
      const int slot = (R.wstart + t) % SW;
      const int64_t row = U.row0 + (R.ffr - U.start_frame);
      int first = INT_MAX, last = -1;
      float bestlik = -1.f;
      for (int p = ns + lane; p <= tmax; p += 64) {
        const int k0 = inb[p], k1 = inb[p + 1];
        const int st = trs[p];
        float cand = 0.f;
        int from = -1;
        for (int k = k0; k < k1; k++) {
          const int q = p - P.in_delta[k];
          if (q < ns || q >= ne) continue;
          const float v = prev[q - o] + P.in_logp[k];
          if (from < 0 || v > cand) {
            cand = v;
            from = q;
          }
        }
        if (from >= 0) {
          first = min(first, p);
          last = max(last, p);
          const float lik = (float)exp(al_ll(P, row, st));
          bestlik = fmaxf(bestlik, lik);
          curb[p - ns] = cand;
          likb[p - ns] = lik;
          back[(int64_t)slot * W + (p - ns)] = (uint8_t)(p - from);
        } else {
          likb[p - ns] = -1.f;  // marks a target no source reaches
        }
      }
      const int ts = wave_min_int(first), te = wave_max_int(last) + 1;
      if (te <= ts) FAIL(3);
      bestlik = wave_max_float(bestlik);
      // normalised observation probabilities of the new range (same lanes as above: no barrier)
      const float best_log = (float)al_safe_log((double)bestlik);
      float bv = -AL_INF;
      int bpos = INT_MAX;
      int hole = 0;
      for (int p = ns + lane; p < te; p += 64) {
        if (p < ts) continue;
        const float lik = likb[p - ns];
        if (lik < 0.f) {
          hole = 1;
          continue;
        }
        const float sp = (float)(al_safe_log((double)lik) - (double)best_log);
        float v = curb[p - ns] + sp;
        if (v > bv) {
          bv = v;
          bpos = p;
        }
        if (v < -AL_INF) v = -AL_INF;
        curb[p - ns] = v;
        cells[(int64_t)slot * W + (p - ns)] = v;
      }
      if (wave_max_int(hole)) FAIL(5);
      // best cell: largest value, smallest position on a tie
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int op = __shfl_xor(bpos, off, 64);
        if (ov > bv || (ov == bv && op < bpos)) {
          bv = ov;
          bpos = op;
        }
      }
      if (bpos == INT_MAX) FAIL(6);
      __syncthreads();
      if (lane == 0) {
        const int sp = (R.wstart + t - 1) % SW;
        meta[3 * sp + 1] = ns;
        meta[3 * sp + 2] = ne;
        meta[3 * slot] = ns;
        meta[3 * slot + 1] = ts;
        meta[3 * slot + 2] = te;
        R.acc += (double)best_log;
        R.best = bv;
        R.bestpos = bpos;
        sh.o_prev = ns;
        sh.s_prev = ts;
        sh.e_prev = te;
        R.ffr++;
        R.cur++;
      }
      {
        float *tmp = prev;
        prev = curb;
        curb = tmp;
      }
      __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    {
      const bool vlast = last_window || eof_hit;
      // Viterbi::compute_best_path (lane 0 walks the back-pointers)
      if (lane == 0) {
        sh.flag = 0;
        const int f = R.cur - 1;
        const int sl = (R.wstart + f) % SW;
        const int e = meta[3 * sl + 2], s = meta[3 * sl + 1];
        int pos;
        if (P.force_end && vlast) {
          pos = R.base + R.lim - 1;
          if (R.lim - 1 < (R.loaded - R.base) - 1 || !(pos >= s && pos < e)) sh.flag = 1;
        } else {
          pos = R.bestpos;
        }
        if (!sh.flag) {
          if (!(pos >= s && pos < e)) pos = e - 1;  // the reference reports the states lost here
          R.fin = (double)cells[(int64_t)sl * W + (pos - meta[3 * sl])];
          path[f] = pos;
          for (int g = f; g > 0; g--) {
            const int sg = (R.wstart + g) % SW;
            const int og = meta[3 * sg];
            if (pos < og || pos - og >= W) {  // a path off the stored band (the reference asserts here)
              sh.flag = 2;
              break;
            }
            const int from = pos - (int)back[(int64_t)sg * W + (pos - og)];
            pos = from < R.base ? R.base : from;  // Lattice::move's from-pointer fix-up
            path[g - 1] = pos;
          }
        }
      }
      __syncthreads();
      if (sh.flag == 2) FAIL(7);
      if (sh.flag) {  // the forced end is out of the window or range: retry with doubled beams
        if (lane == 0) {
          R.n_fail++;
          R.beam *= 2;
          R.sbeam *= 2;
          if (R.beam <= P.maxbeam)
            R.fresh = 1;
          else
            R.status = ALIGN_GAVE_UP;
        }
        __syncthreads();
        continue;
      }
      if (eof_hit) {
        last_window = true;
        wend = R.wstart + last_frame;
      }
      int target = P.target;
      if (last_window) target = wend - R.wstart;
      if (R.wstart + target > wend) target = wend - R.wstart;
      const int ob = R.wstart - U.start_frame;
      for (int f = lane; f < target; f += 64)
        if (ob + f < U.n_out) P.out[U.out_begin + ob + f] = path[f];
      __syncthreads();
      if (lane == 0) {
        R.committed = min(ob + target, U.n_out);
        R.wstart += target;
        sh.flag = last_window && R.wstart >= U.end_frame;
        if (sh.flag) R.status = ALIGN_OK;
      }
      __syncthreads();
      if (sh.flag) break;
      // Viterbi::move(target, path[target]) -- the ring keeps its cells; bases advance
      const int position = path[target];
      if (lane == 0) {
        R.base = position;
        R.cur -= target;
        // kept frames lose the positions below the new base
        for (int f = 0; f < R.cur; f++) {
          const int sl = (R.wstart + f) % SW;
          if (meta[3 * sl + 1] < position) meta[3 * sl + 1] = position;
        }
        const int f = R.cur - 1;
        const int sl = (R.wstart + f) % SW;
        sh.o_prev = meta[3 * sl];
        sh.s_prev = meta[3 * sl + 1];
        sh.e_prev = meta[3 * sl + 2];
      }
      __syncthreads();
      {
        const int f = R.cur - 1;
        const int sl = (R.wstart + f) % SW;
        const int o = sh.o_prev, s = sh.s_prev, e = sh.e_prev;
        const int pp = path[f + target];
        if (pp < s || pp >= e) FAIL(8);
        const float lp = prev[pp - o];
        for (int p = s + lane; p < e; p += 64) {
          const float v = prev[p - o] - lp;
          prev[p - o] = v;
          cells[(int64_t)sl * W + (p - o)] = v;
        }
        __syncthreads();
        if (lane == 0) {
          R.acc += (double)lp;
          R.fin = 0;
        }
      }
      __syncthreads();
    }
  }
done:
  __syncthreads();
  if (lane == 0) P.run[u] = R;
#undef R
#undef FAIL
}

void align_launch(const AlignParams &p, int32_t n_utt, int32_t windows, hipStream_t stream) {
  if (n_utt <= 0) return;
  const size_t lds = (size_t)3 * p.width * sizeof(float);
  hipLaunchKernelGGL(k_align_viterbi, dim3((unsigned)n_utt), dim3(64), lds, stream, p, windows);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr

// hmmnet_fb.hip -- forward-backward over HMM networks: aku/HmmNetBaumWelch.cc's fill_backward_probabilities
// (:817-1020), backward_propagate_epsilon_arcs (:1023-1075), create_segmented_lattice (:1078-1419) and
// get_arc_score (:1917-1942) in dense form.  Layout and launch shape: hmmnet_fb.h.
//
// Every sum is a gather by one lane over an index list in ascending order (a node's out-arcs, its in-arcs, a
// pdf's arcs, an epsilon level's nodes), so there are no atomics and the same input gives the same bytes.
// All arithmetic is double.
#include <hip/hip_runtime.h>

#include "hmmnet_fb.h"

namespace aasr {

namespace {

// util::logadd
__device__ __forceinline__ double fb_plus(double a, double b) {
  double d = a - b;
  if (d > 0) {
    b = a;
    d = -d;
  }
  return b + log1p(exp(d));
}

__device__ __forceinline__ double fb_join(double v, double x, bool viterbi) {
  if (v <= FB_ZERO) return x;
  return viterbi ? (v < x ? x : v) : fb_plus(v, x);
}

// One utterance's view of the blobs: the bases and the network's offsets into them (32-bit, so the view stays in
// scalar registers).
struct FbView {
  const int32_t *I;
  const double *F;
  const FbNetDev *op;
  const void *scores;
  int64_t pitch, row0;
  int32_t f64, N, A;
  double ac_scale, bw_beam;
  bool viterbi;
  const double *beta;  // (T + 1) x N, rows after the epsilon closure
  const double *best;  // T
};

__device__ __forceinline__ double fb_state_ll(const FbView &v, int32_t t, int32_t pdf) {
  const int64_t i = (v.row0 + t) * v.pitch + pdf;
  return v.f64 ? ((const double *)v.scores)[i] : (double)((const float *)v.scores)[i];
}

// get_arc_score of an emitting arc: static score + ac_scale * safe_log(likelihood * prob), zero at the floor
__device__ __forceinline__ double fb_arc_score(const FbView &v, int32_t a, int32_t t) {
  const double s = fb_state_ll(v, t, v.I[v.op->em_pdf + a]) + v.F[v.op->em_logp + a];
  if (s <= FB_LOG_TINY) return FB_ZERO;
  return v.F[v.op->em_static + a] + v.ac_scale * s;
}

// the arc's backward score at frame t before pruning: beta[t + 1][target] + arc score, zero when either is
__device__ __forceinline__ double fb_raw(const FbView &v, int32_t a, int32_t t) {
  const double b = v.beta[(int64_t)(t + 1) * v.N + v.I[v.op->em_tgt + a]];
  if (b <= FB_ZERO) return FB_ZERO;
  const double s = fb_arc_score(v, a, t);
  if (s <= FB_ZERO) return FB_ZERO;
  const double x = b + s;
  return x > FB_ZERO ? x : FB_ZERO;
}

__device__ __forceinline__ bool fb_kept(const FbView &v, double x, double best) {
  return x > FB_ZERO && !(x - best < -v.bw_beam);
}

// what FrameScores::get_score returns to the forward pass: zero for a pruned arc and, in Viterbi mode, for
// every arc but the first best one of its source node
__device__ __forceinline__ double fb_value(const FbView &v, int32_t a, int32_t t) {
  const double best = v.best[t];
  const double x = fb_raw(v, a, t);
  if (!fb_kept(v, x, best)) return FB_ZERO;
  if (v.viterbi) {
    const int32_t n = v.I[v.op->em_src + a];
    double bv = FB_ZERO;
    int32_t ba = -1;
    for (int32_t o = v.I[v.op->em_begin + n]; o < v.I[v.op->em_begin + n + 1]; o++) {
      const double y = o == a ? x : fb_raw(v, o, t);
      if (!fb_kept(v, y, best)) continue;
      if (y > bv) {
        bv = y;
        ba = o;
      }
    }
    if (ba != a) return FB_ZERO;
  }
  return x;
}

// backward_propagate_epsilon_arcs on the row w, level by level; ends with a barrier
__device__ __forceinline__ void fb_close_backward(const FbView &v, double *w, int32_t n_bl) {
  for (int32_t l = 0; l < n_bl; l++) {
    for (int32_t i = v.I[v.op->bl_begin + l] + (int32_t)threadIdx.x; i < v.I[v.op->bl_begin + l + 1]; i += FB_THREADS) {
      const int32_t n = v.I[v.op->bl_nodes + i];
      double x = w[n];
      for (int32_t e = v.I[v.op->eo_begin + n]; e < v.I[v.op->eo_begin + n + 1]; e++) {
        const double b = w[v.I[v.op->ep_tgt + e]];
        if (b <= FB_ZERO) continue;
        x = fb_join(x, b + v.F[v.op->ep_score + e], v.viterbi);
      }
      w[n] = x;
    }
    __syncthreads();
  }
}

}  // namespace

template <bool kLds>
__global__ __launch_bounds__(FB_THREADS) void k_hmmnet_fb(FbParams p) {
  __shared__ double s_red[FB_THREADS];
  __shared__ double s_nodes[kLds ? 2 * FB_LDS_NODES : 1];
  const int32_t tid = (int32_t)threadIdx.x;
  const int32_t u = p.list[blockIdx.x];
  const FbUttDev &ud = p.utt[u];
  const FbNetDev &nd = ud.net;
  const int32_t N = nd.n_nodes, A = nd.n_em, T = ud.T;
  FbView v;
  v.I = p.ints;
  v.F = p.doubles;
  v.op = &nd;
  v.scores = p.scores;
  v.pitch = p.pitch;
  v.row0 = ud.row0;
  v.f64 = p.f64;
  v.N = N;
  v.A = A;
  v.ac_scale = p.ac_scale;
  v.bw_beam = p.bw_beam;
  v.viterbi = p.mode == FB_MODE_VITERBI;
  double *beta = p.work + ud.beta;
  double *best = p.work + ud.best;
  double *arc0 = p.work + ud.arcs, *arc1 = arc0 + A;
  v.beta = beta;
  v.best = best;
  double *w0, *w1;
  if constexpr (kLds) {
    w0 = s_nodes;
    w1 = s_nodes + FB_LDS_NODES;
  } else {
    w0 = p.work + ud.nodes;
    w1 = w0 + N;
  }
  FbResult &res = p.result[u];
  double *occ = p.want_pdf_occ ? p.occ + ud.occ : nullptr;
  double *trocc = p.want_tr_occ ? p.trocc + ud.trocc : nullptr;
  int32_t *path = p.path ? p.path + ud.path : nullptr;
  const int32_t P = nd.n_pdf, K = nd.n_tr;

  // ---- backward: beta row T is the closure of the final node, then frame by frame from the last ----
  for (int32_t n = tid; n < N; n += FB_THREADS) w0[n] = n == nd.final_node ? 0.0 : FB_ZERO;
  __syncthreads();
  fb_close_backward(v, w0, nd.n_bl);
  for (int32_t n = tid; n < N; n += FB_THREADS) beta[(int64_t)T * N + n] = w0[n];
  __syncthreads();
  for (int32_t t = T - 1; t >= 0; t--) {
    double m = FB_ZERO;
    for (int32_t a = tid; a < A; a += FB_THREADS) {
      const double x = fb_raw(v, a, t);
      arc0[a] = x;
      m = x > m ? x : m;
    }
    s_red[tid] = m;
    __syncthreads();
    for (int32_t s = FB_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) s_red[tid] = s_red[tid + s] > s_red[tid] ? s_red[tid + s] : s_red[tid];
      __syncthreads();
    }
    const double fbest = s_red[0];
    if (tid == 0) best[t] = fbest;
    for (int32_t n = tid; n < N; n += FB_THREADS) {
      double x = FB_ZERO;
      for (int32_t a = v.I[v.op->em_begin + n]; a < v.I[v.op->em_begin + n + 1]; a++) {
        const double y = arc0[a];
        if (!fb_kept(v, y, fbest)) continue;
        x = fb_join(x, y, v.viterbi);
      }
      w0[n] = x;
    }
    __syncthreads();
    fb_close_backward(v, w0, nd.n_bl);
    for (int32_t n = tid; n < N; n += FB_THREADS) beta[(int64_t)t * N + n] = w0[n];
    __syncthreads();
  }
  const double total = beta[nd.initial];
  if (tid == 0) {
    res.backward_total = total;
    res.forward_total = FB_ZERO;
    res.attempts += 1;
  }
  if (total <= FB_ZERO) {  // the initial node was not reached: the caller may widen the backward beam
    if (tid == 0) res.status = FB_FAILED_BACKWARD;
    return;
  }
  const double limit = total - p.fw_beam;
  if (occ)
    for (int64_t i = tid; i < (int64_t)T * P; i += FB_THREADS) occ[i] = 0.0;
  if (trocc)
    for (int32_t k = tid; k < K; k += FB_THREADS) trocc[k] = 0.0;
  __syncthreads();

  // ---- forward, Viterbi mode: the reference's single token, walked by one lane ----
  if (v.viterbi) {
    if (tid == 0) {
      int32_t node = nd.initial;
      double alpha = 0.0;
      bool alive = true;
      for (int32_t t = 0; t < T && alive; t++) {
        for (;;) {  // the best arc among all out-arcs; an epsilon arc moves the token and the choice is made again
          double bt = FB_ZERO;
          int32_t be = -1;
          for (int32_t e = v.I[v.op->eo_begin + node]; e < v.I[v.op->eo_begin + node + 1]; e++) {
            const double b = beta[(int64_t)t * N + v.I[v.op->ep_tgt + e]];
            if (b <= FB_ZERO) continue;
            const double tot = alpha + b + v.F[v.op->ep_score + e];
            if (tot < limit) continue;
            if (tot > bt) {
              bt = tot;
              be = e;
            }
          }
          for (int32_t a = v.I[v.op->em_begin + node]; a < v.I[v.op->em_begin + node + 1]; a++) {
            const double x = fb_value(v, a, t);
            if (x <= FB_ZERO || alpha + x < limit) continue;
            if (alpha + x > bt) {
              bt = alpha + x;
              be = -1;
            }
          }
          if (be < 0) break;
          alpha += v.F[v.op->ep_score + be];
          node = v.I[v.op->ep_tgt + be];
        }
        int32_t taken = -1;
        for (int32_t a = v.I[v.op->em_begin + node]; a < v.I[v.op->em_begin + node + 1]; a++) {
          const double x = fb_value(v, a, t);
          if (x > FB_ZERO && !(alpha + x < limit)) taken = a;
        }
        if (taken < 0) {
          alive = false;
          break;
        }
        alpha += fb_arc_score(v, taken, t);
        node = v.I[v.op->em_tgt + taken];
        if (occ) occ[(int64_t)t * P + v.I[v.op->em_slot + taken]] = 1.0;
        if (trocc) trocc[v.I[v.op->em_trslot + taken]] += 1.0;
        if (path) path[t] = taken;
      }
      res.status = alive ? FB_OK : FB_FAILED_FORWARD;
      if (alive) res.forward_total = alpha;
    }
    return;
  }

  // ---- forward, Baum-Welch mode ----
  double *al = w0, *nx = w1;
  for (int32_t n = tid; n < N; n += FB_THREADS) al[n] = n == nd.initial ? 0.0 : FB_ZERO;
  __syncthreads();
  for (int32_t t = 0; t < T; t++) {
    // epsilon closure: an arc is followed when alpha[source] + its backward value stays within the beam
    for (int32_t l = 0; l < nd.n_fl; l++) {
      for (int32_t i = v.I[v.op->fl_begin + l] + tid; i < v.I[v.op->fl_begin + l + 1]; i += FB_THREADS) {
        const int32_t n = v.I[v.op->fl_nodes + i];
        const double b = beta[(int64_t)t * N + n];
        double x = al[n];
        if (b > FB_ZERO)
          for (int32_t k = v.I[v.op->ei_begin + n]; k < v.I[v.op->ei_begin + n + 1]; k++) {
            const int32_t e = v.I[v.op->ei_arcs + k];
            const double as = al[v.I[v.op->ep_src + e]];
            if (as <= FB_ZERO) continue;
            if (as + b + v.F[v.op->ep_score + e] < limit) continue;
            x = fb_join(x, as + v.F[v.op->ep_score + e], false);
          }
        al[n] = x;
      }
      __syncthreads();
    }
    for (int32_t a = tid; a < A; a += FB_THREADS) {
      double fs = FB_ZERO, tot = FB_ZERO;
      const double as = al[v.I[v.op->em_src + a]];
      if (as > FB_ZERO) {
        const double x = fb_value(v, a, t);
        if (x > FB_ZERO && !(as + x < limit)) {
          fs = as + fb_arc_score(v, a, t);
          tot = as + x;
        }
      }
      arc0[a] = fs;
      arc1[a] = tot;
    }
    __syncthreads();
    for (int32_t n = tid; n < N; n += FB_THREADS) {
      double x = FB_ZERO;
      for (int32_t k = v.I[v.op->in_begin + n]; k < v.I[v.op->in_begin + n + 1]; k++) {
        const double y = arc0[v.I[v.op->in_arcs + k]];
        if (y > FB_ZERO) x = fb_join(x, y, false);
      }
      nx[n] = x;
    }
    if (occ)
      for (int32_t q = tid; q < P; q += FB_THREADS) {
        double g = 0.0;
        for (int32_t k = v.I[v.op->pdf_begin + q]; k < v.I[v.op->pdf_begin + q + 1]; k++) {
          const double y = arc1[v.I[v.op->pdf_arcs + k]];
          if (y > FB_ZERO) g += exp(y - total);
        }
        occ[(int64_t)t * P + q] = g;
      }
    if (trocc)
      for (int32_t q = tid; q < K; q += FB_THREADS) {
        double g = 0.0;
        for (int32_t k = v.I[v.op->tr_begin + q]; k < v.I[v.op->tr_begin + q + 1]; k++) {
          const double y = arc1[v.I[v.op->tr_arcs + k]];
          if (y > FB_ZERO) g += exp(y - total);
        }
        trocc[q] += g;
      }
    __syncthreads();
    double *sw = al;
    al = nx;
    nx = sw;
  }
  // the total over the tokens alive after the last frame (:1389-1416), in node order
  if (tid == 0) {
    double ft = FB_ZERO;
    for (int32_t n = 0; n < N; n++)
      if (al[n] > FB_ZERO) ft = fb_join(ft, al[n], false);
    s_red[0] = ft;
    res.forward_total = ft;
    res.status = ft > FB_ZERO ? FB_OK : FB_FAILED_FORWARD;
  }
  __syncthreads();
  const double ft = s_red[0];
  if (ft <= FB_ZERO) return;
  // occupancies were taken against the backward total; the lattice's own total is the forward one
  const double scale = exp(total - ft);
  if (occ)
    for (int64_t i = tid; i < (int64_t)T * P; i += FB_THREADS) occ[i] *= scale;
  if (trocc)
    for (int32_t k = tid; k < K; k += FB_THREADS) trocc[k] *= scale;
}

void hmmnet_fb_launch(const FbParams &p, int32_t n_list, bool lds_form, hipStream_t stream) {
  if (n_list <= 0) return;
  if (lds_form)
    hipLaunchKernelGGL(k_hmmnet_fb<true>, dim3((unsigned)n_list), dim3(FB_THREADS), 0, stream, p);
  else
    hipLaunchKernelGGL(k_hmmnet_fb<false>, dim3((unsigned)n_list), dim3(FB_THREADS), 0, stream, p);
}

}  // namespace aasr

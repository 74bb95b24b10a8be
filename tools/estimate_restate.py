"""estimate_restate.py -- NumPy restatement of aku/estimate.cc --ml over diagonal pools, the yardstick of the native
estimate tool (csrc/estimate.cc): readers and writers of the four dump files of stats (.gks, .mcs, .phs, .lls) in the
diagonal (mode 1) and the full-statistics (mode 3) form, the accumulation in double, the ML update, the pool edits
(--delete, --mremove, --split), the model writers, and HmmSet::estimate_mllt in double with the Gaussians taken in
order.

Every scalar operation is an IEEE double operation in the reference's order, so that the host parts of the native tool
can be compared with ==.  LAPACK++'s own fused operations are not modelled.  The MLLT part uses
np.linalg.inv for the dim x dim inverses: against it the native code is compared with a bound, not with ==.

    python tools/estimate_restate.py BASE LIST OUT [-t] [--minvar V] [--mllt]     (a plain --ml round, for a look)
"""
from __future__ import annotations

import math
import struct
import sys

import numpy as np

ML, FULL = 1, 3   # PDF_ML_STATS, PDF_ML_STATS | PDF_ML_FULL_STATS
MAX_MLLT_ITER, MAX_MLLT_A_ITER = 7, 80


def tri(d: int) -> int:
    return d * (d + 1) // 2


# ---- the dump files ------------------------------------------------------------------------------

def write_gks(path, dim, mode, gaussians):
    """gaussians: per pool entry None (nothing accumulated) or (feacount, gamma, sum_x [dim], sum_xx) with sum_xx [dim]
    (mode 1) or the packed lower triangle (mode 3); the values are narrowed to float as the reference's writer does."""
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", len(gaussians), dim, mode))
        for g, st in enumerate(gaussians):
            f.write(struct.pack("<i", g))
            if st is not None:
                fc, gamma, sx, sxx = st
                f.write(struct.pack("<iidd", 0, int(fc), float(gamma), 0.0))
                f.write(np.asarray(sx, np.float32).tobytes())
                f.write(np.asarray(sxx, np.float32).tobytes())
            f.write(struct.pack("<i", -1))


def write_mcs(path, mode, mixtures):
    """mixtures: per mixture None or (pointers, gammas, mixture_ll)"""
    with open(path, "w") as f:
        f.write("%d\n%d\n" % (len(mixtures), mode))
        for i, st in enumerate(mixtures):
            f.write("%d\n" % i)
            if st is not None:
                ptr, gam, ll = st
                f.write("0 %d" % len(ptr) + "".join(" %d %.10g" % (p, g) for p, g in zip(ptr, gam)) + " 0 %.10g\n" % ll)
            f.write("-1\n")


def write_phs(path, n_transitions, lines):
    """lines: (source state, target offset, occupancy) of the accumulated transitions"""
    with open(path, "w") as f:
        f.write("%d\n" % n_transitions)
        for s, t, occ in lines:
            f.write("%d %d %g\n" % (s, t, occ))


def write_lls(path, items):
    with open(path, "w") as f:
        for k, v in items:
            f.write("%s: %.12g\n" % (k, v))


def write_model(base, mean, var, mixtures, hmms, self_prob=None):
    """A small model's three files.  mixtures: per state (pointers, weights); hmms: (label, [state ...]); every state
    has a self loop and a step to the next state (the last: out of the HMM), self_prob[state] the loop's probability."""
    G, d = np.shape(mean)
    with open(base + ".gk", "w") as f:
        f.write("%d %d variable\n" % (G, d))
        for g in range(G):
            f.write("diag " + " ".join("%.17g" % x for x in list(mean[g]) + list(var[g])) + "\n")
    with open(base + ".mc", "w") as f:
        f.write("%d\n" % len(mixtures))
        for ptr, w in mixtures:
            f.write("%d" % len(ptr) + "".join(" %d %.17g" % (p, x) for p, x in zip(ptr, w)) + "\n")
    with open(base + ".ph", "w") as f:
        f.write("PHONE\n%d\n" % len(hmms))
        for h, (label, states) in enumerate(hmms):
            n = len(states)
            f.write("%d %d %s\n-1 -2 %s\n0 1 2 1\n1 0\n" % (h + 1, n + 2, label, " ".join(map(str, states))))
            for s, st in enumerate(states):
                p = 0.6 if self_prob is None else self_prob[st]
                f.write("%d 2 %d %.17g %d %.17g\n" % (s + 2, s + 2, p, 1 if s == n - 1 else s + 3, 1 - p))


def frame_statistics(x, gamma, full):
    """(feacount, sum gamma, sum gamma x, sum gamma x^2 or the packed lower triangle of sum gamma x x^T) of frames x"""
    x, gamma = np.asarray(x, np.float64), np.asarray(gamma, np.float64)
    sx = (gamma[:, None] * x).sum(0)
    if full:
        r, c = np.tril_indices(x.shape[1])
        sxx = (gamma[:, None] * x[:, r] * x[:, c]).sum(0)
    else:
        sxx = (gamma[:, None] * x * x).sum(0)
    return len(x), float(gamma.sum()), sx, sxx


# ---- the model -----------------------------------------------------------------------------------

class Model:
    """HmmSet as estimate sees it: the pool, the mixtures (state s emits mixture s), the HMMs and the transitions
    numbered in state order, with the accumulators."""

    def __init__(self, base=None, gk=None, mc=None, ph=None):
        gk, mc, ph = gk or base + ".gk", mc or base + ".mc", ph or base + ".ph"
        tok = open(gk).read().split()
        n, self.dim, kind = int(tok[0]), int(tok[1]), tok[2]
        pos, d = 3, self.dim
        self.mean, self.var = [], []
        for _ in range(n):
            if kind == "variable":
                assert tok[pos] == "diag", "only diagonal Gaussians"
                pos += 1
            else:
                assert kind == "diagonal_cov", "only diagonal Gaussians"
            self.mean.append([float(x) for x in tok[pos:pos + d]])
            self.var.append([float(x) for x in tok[pos + d:pos + 2 * d]])
            pos += 2 * d
        tok = open(mc).read().split()
        pos = 1
        self.pointers, self.weights = [], []
        for _ in range(int(tok[0])):
            k = int(tok[pos])
            pos += 1
            self.pointers.append([int(tok[pos + 2 * i]) for i in range(k)])
            w = [float(tok[pos + 2 * i + 1]) for i in range(k)]
            pos += 2 * k
            self.weights.append(self._normalized(w))
        tok = open(ph).read().split()
        assert tok[0] == "PHONE"
        pos = 2
        self.hmms, info = [], {}
        for _ in range(int(tok[1])):
            states, label = int(tok[pos + 1]) - 2, tok[pos + 2]
            pos += 5
            pdfs = [int(x) for x in tok[pos:pos + states]]
            pos += states
            load = [p not in info for p in pdfs]
            for p in pdfs:
                info.setdefault(p, [])
            for _s in range(-2, states):
                source, k = int(tok[pos]) - 2, int(tok[pos + 1])
                pos += 2
                for _t in range(k):
                    target, prob = int(tok[pos]), float(tok[pos + 1])
                    pos += 2
                    if source >= 0 and load[source]:
                        off = states - source if target == 1 else target - 2 - source
                        info[pdfs[source]].append([pdfs[source], off, prob])
            self.hmms.append((label, pdfs))
        self.n_states = max(info) + 1 if info else 0
        self.transitions, self.state_transitions = [], []
        for s in range(self.n_states):
            self.state_transitions.append([])
            for tr in info.get(s, []):
                self.state_transitions[s].append(len(self.transitions))
                self.transitions.append(tr)
        # accumulators
        self.mode = 0
        self.acc = [None] * n          # per Gaussian: None or dict(feacount, gamma, sum_x, sum_xx, accumulated)
        self.mix_acc = [None] * len(self.pointers)   # per mixture: None or dict(gamma [size at creation], ll, accumulated)
        self.trans_acc = None
        self.trans_accumulated = None
        self.sums = {}
        self.minvar = 0.1

    @staticmethod
    def _normalized(w):
        s = 0.0
        for x in w:
            s += x
        return [x / s for x in w]

    # -- accumulation (HmmSet::accumulate_*_from_dump)
    def add_dump(self, base, transitions=False):
        self._add_gks(base + ".gks")
        self._add_mcs(base + ".mcs")
        if transitions:
            self._add_phs(base + ".phs")
        try:
            for line in open(base + ".lls"):
                if ":" in line:
                    k, v = line.rstrip("\n").split(":", 1)
                    if v:
                        self.sums[k] = self.sums.get(k, 0.0) + float(v) if k in self.sums else float(v)
        except OSError:
            pass

    def _xx(self):
        return tri(self.dim) if self.mode & 2 else self.dim

    def _add_gks(self, path):
        b = open(path, "rb").read()
        n, dim, mode = struct.unpack_from("<iii", b, 0)
        assert n == len(self.mean) and dim == self.dim
        if self.mode == 0:
            self.mode = mode
        pos, d, xx = 12, self.dim, self._xx()
        while pos + 4 <= len(b):
            g, = struct.unpack_from("<i", b, pos)
            pos += 4
            assert 0 <= g < n
            if self.acc[g] is None:
                self.acc[g] = dict(feacount=0, gamma=0.0, sum_x=[0.0] * d, sum_xx=[0.0] * xx, accumulated=False)
            a = self.acc[g]
            ap, = struct.unpack_from("<i", b, pos)
            pos += 4
            while ap >= 0:
                assert ap == 0
                fc, gamma, _aux = struct.unpack_from("<idd", b, pos)
                pos += 20
                assert fc >= 0
                a["feacount"] += fc
                a["gamma"] += gamma
                a["accumulated"] = True
                sx = np.frombuffer(b, np.float32, d, pos)
                pos += 4 * d
                sxx = np.frombuffer(b, np.float32, xx, pos)
                pos += 4 * xx
                for i in range(d):
                    a["sum_x"][i] += float(sx[i])
                for i in range(xx):
                    a["sum_xx"][i] += float(sxx[i])
                ap, = struct.unpack_from("<i", b, pos)
                pos += 4

    def _add_mcs(self, path):
        tok = open(path).read().split()
        assert int(tok[0]) == len(self.pointers)
        if self.mode == 0:
            self.mode = int(tok[1])
        pos = 2
        while pos < len(tok):
            m = int(tok[pos])
            pos += 1
            if self.mix_acc[m] is None:
                self.mix_acc[m] = dict(gamma=[0.0] * len(self.pointers[m]), ll=0.0, accumulated=False)
            a = self.mix_acc[m]
            ap = int(tok[pos])
            pos += 1
            while ap >= 0:
                sz = int(tok[pos])
                pos += 1
                assert sz == len(self.pointers[m])
                for i in range(sz):
                    assert int(tok[pos]) == self.pointers[m][i]
                    a["gamma"][i] += float(tok[pos + 1])
                    pos += 2
                a["ll"] += float(tok[pos + 1])
                pos += 2
                a["accumulated"] = True
                ap = int(tok[pos])
                pos += 1

    def _add_phs(self, path):
        try:
            tok = open(path).read().split()
        except OSError:
            return
        T = len(self.transitions)
        if self.trans_acc is None:
            self.trans_acc, self.trans_accumulated = [0.0] * T, [False] * T
        assert int(tok[0]) == T
        pos, last = 1, None
        for t in range(T):
            if pos + 3 <= len(tok):
                last = (int(tok[pos]), int(tok[pos + 1]), float(tok[pos + 2]))
                pos += 3
            elif t == 0:
                break    # premature EOF (no transition information)
            # (past the end of the file the reference's reader keeps the values of the last line)
            s, off, occ = last
            at = [i for i, tr in enumerate(self.transitions) if tr[0] == s and tr[1] == off][0]
            self.trans_acc[at] += occ
            self.trans_accumulated[at] = True

    # -- the ML update
    def accumulated(self, g):
        return self.acc[g] is not None and self.acc[g]["accumulated"]

    def estimate_gaussians(self):
        d = self.dim
        for g in range(len(self.mean)):
            if not self.accumulated(g):
                continue
            a = self.acc[g]
            inv = 1 / a["gamma"]
            mean = [a["sum_x"][i] * inv for i in range(d)]
            if self.mode & 2:
                var = [a["sum_xx"][tri(i) + i] * inv - mean[i] * mean[i] for i in range(d)]
            else:
                var = [a["sum_xx"][i] / a["gamma"] - mean[i] * mean[i] for i in range(d)]
            self.mean[g] = mean
            self.var[g] = [v if not v < self.minvar else self.minvar for v in var]

    def estimate_mixtures(self):
        for s in range(self.n_states):
            a = self.mix_acc[s]
            if a is None or not a["accumulated"]:
                continue
            total = 0.0
            for i in range(len(self.weights[s])):
                total += a["gamma"][i]
            self.weights[s] = [a["gamma"][i] / total for i in range(len(self.weights[s]))]

    def estimate_transitions(self):
        if self.trans_acc is None:
            return
        for s in range(self.n_states):
            total = np.float32(0.0)
            for t in self.state_transitions[s]:
                total = np.float32(float(total) + self.trans_acc[t])
            if total > 0.0:
                for t in self.state_transitions[s]:
                    p = self.trans_acc[t] / float(total)
                    self.transitions[t][2] = p if not p < .001 else .001

    # -- the pool edits
    def occupancy(self, g):
        return self.acc[g]["gamma"] if self.accumulated(g) else -1

    def _delete(self, index_map):
        keep = [i for i, m in enumerate(index_map) if m >= 0]
        self.mean, self.var, self.acc = [self.mean[i] for i in keep], [self.var[i] for i in keep], [self.acc[i] for i in keep]

    def _update_components(self, m, cmap):
        ptr, w = [], []
        for p, x in zip(self.pointers[m], self.weights[m]):
            if cmap[p] >= 0:
                ptr.append(cmap[p])
                w.append(x)
        self.pointers[m], self.weights[m] = ptr, self._normalized(w)

    def delete_gaussians(self, minocc):
        n = len(self.mean)
        imap = list(range(n))
        for i in range(n):
            occ = self.occupancy(i)
            if occ < minocc and occ >= 0:
                for j in range(i + 1, n):
                    imap[j] -= 1
                imap[i] = -1
        for m in range(len(self.pointers)):
            if any(imap[p] >= 0 for p in self.pointers[m]):
                continue
            max_w, max_i = -1, -1
            for p, w in zip(self.pointers[m], self.weights[m]):
                if w > max_w:
                    max_w, max_i = w, p
            new = 0
            for j in range(max_i - 1, -1, -1):
                if imap[j] >= 0:
                    new = imap[j] + 1
                    break
            imap[max_i] = new
            for j in range(max_i + 1, n):
                if imap[j] >= 0:
                    imap[j] += 1
        self._delete(imap)
        for m in range(len(self.pointers)):
            self._update_components(m, imap)
        return imap

    def remove_mixture_components(self, min_weight):
        n = len(self.mean)
        count = [0] * n
        for m in range(len(self.pointers)):
            while True:
                w = self.weights[m]
                k = min(range(len(w)), key=lambda i: (w[i], i))   # the first of the smallest
                if w[k] > min_weight:
                    break
                del self.pointers[m][k]
                del w[k]
                self.weights[m] = self._normalized(w)
            for p in self.pointers[m]:
                count[p] += 1
        imap, cur = [], 0
        for i in range(n):
            if count[i] == 0:
                imap.append(-1)
            else:
                imap.append(cur)
                cur += 1
        if cur < n:
            self._delete(imap)
            for m in range(len(self.pointers)):
                self._update_components(m, imap)
        return imap

    def split_gaussians(self, minocc=0.0, maxg=0, numgauss=-1, splitalpha=1.0):
        """-> (splits, the occupancy limit the search ended with, steps of the search)"""
        if minocc < 1.0:
            minocc = 1.0
        order = [g for g in range(len(self.mean)) if self.accumulated(g) and self.acc[g]["gamma"] >= 0]
        order.sort(key=lambda g: -self.acc[g]["gamma"])    # stable: a tie goes to the lower index
        P = len(self.pointers)
        pdf_occ, limit, sum_occ = [], [], 0.0
        for p in range(P):
            occ_sum, lim = 0.0, 0
            for k in range(len(self.pointers[p])):
                occ = self.mix_acc[p]["gamma"][k]
                occ_sum += occ
                lim += int(math.floor(occ / (minocc / 2.0)))
            pdf_occ.append(occ_sum)
            limit.append(lim)
            sum_occ += occ_sum
        mixg, steps = 0.0, 0
        if numgauss > 0:
            if len(self.mean) >= numgauss:
                return 0, mixg, steps
            mixg = 10 * self.dim
            temp = sum_occ / float(P)
            mixg = math.pow(temp, splitalpha) / (temp / mixg)
            interval, growing = mixg, True
            for _ in range(30):
                total = 0
                for p in range(P):
                    k = int(math.floor(math.pow(pdf_occ[p], splitalpha) / mixg))
                    k = min(k, limit[p])
                    total += max(min(k, maxg), len(self.pointers[p]))
                if total > (1 + .001) * numgauss:
                    if growing:
                        mixg *= 2
                        interval = mixg / 2.0
                    else:
                        mixg += interval / 2.0
                elif total < numgauss:
                    growing = False
                    mixg -= interval / 2.0
                else:
                    break
                steps += 1
                if not growing:
                    interval /= 2.0
        splits = 0
        for g in order:
            ok, users = True, []
            for p in range(P):
                if g in self.pointers[p]:
                    if (numgauss > 0 and math.pow(pdf_occ[p], splitalpha) / (len(self.pointers[p]) + 1) < mixg) or \
                            len(self.pointers[p]) >= maxg or self.acc[g]["gamma"] < minocc:
                        ok = False
                        break
                    users.append(p)
            if not ok:
                continue
            sd = [0.2 * math.sqrt(v) for v in self.var[g]]
            m1 = [m - s for m, s in zip(self.mean[g], sd)]
            m2 = [m + s for m, s in zip(self.mean[g], sd)]
            self.mean[g] = m1
            self.mean.append(m2)
            self.var.append(list(self.var[g]))
            self.acc.append(self.acc[g])
            new = len(self.mean) - 1
            for p in users:
                k = self.pointers[p].index(g)
                c = self.weights[p][k]
                self.weights[p][k] = 0.5 * c
                self.pointers[p].append(new)
                self.weights[p].append(0.5 * c)
            splits += 1
        return splits, mixg, steps

    # -- the writers: the tokens of the three files ("%g": an ostream of default precision)
    def gk_tokens(self):
        out = [str(len(self.mean)), str(self.dim), "variable"]
        for m, v in zip(self.mean, self.var):
            out += ["diag"] + ["%g" % x for x in m] + ["%g" % x for x in v]
        return out

    def mc_tokens(self):
        out = [str(len(self.pointers))]
        for s in range(self.n_states):
            out.append(str(len(self.pointers[s])))
            for p, w in zip(self.pointers[s], self.weights[s]):
                out += [str(p), "%g" % w]
        return out

    def ph_tokens(self):
        out = ["PHONE", str(len(self.hmms))]
        for h, (label, pdfs) in enumerate(self.hmms):
            ns = len(pdfs)
            out += [str(h + 1), str(ns + 2), label, "-1", "-2"] + [str(p) for p in pdfs] + "0 1 2 1 1 0".split()
            for s in range(ns):
                tr = self.state_transitions[pdfs[s]]
                out += [str(s + 2), str(len(tr))]
                for t in tr:
                    target = self.transitions[t][1] + 2 + s
                    out += [str(1 if target == ns + 2 else target), "%g" % self.transitions[t][2]]
        return out

    def write(self, base):
        for ext, tok in ((".gk", self.gk_tokens()), (".mc", self.mc_tokens()), (".ph", self.ph_tokens())):
            open(base + ext, "w").write(" ".join(tok) + "\n")

    def summary_lines(self, name):
        return [name] + ["  %s: %.12g" % (k, self.sums[k]) for k in sorted(self.sums)]

    # -- MLLT over the model's mode-3 statistics
    def mllt_arrays(self):
        G, d = len(self.mean), self.dim
        ok = np.array([self.accumulated(g) for g in range(G)])
        gamma, sx, sxx = np.zeros(G), np.zeros((G, d)), np.zeros((G, tri(d)))
        for g in range(G):
            if ok[g]:
                gamma[g], sx[g], sxx[g] = self.acc[g]["gamma"], self.acc[g]["sum_x"], self.acc[g]["sum_xx"]
        return gamma, sx, sxx, ok


# ---- MLLT ----------------------------------------------------------------------------------------

def unpack_lower(p, d):
    m = np.zeros(p.shape[:-1] + (d, d), p.dtype)
    r, c = np.tril_indices(d)
    m[..., r, c] = p
    m[..., c, r] = p
    return m


def covariances(gamma, sum_x, sum_xx, ok, dtype=np.float64):
    """S_g = M2_g (1 / gamma_g) - mean_g mean_g^T as packed lower triangles; zero where ok is false"""
    G, d = sum_x.shape
    out = np.zeros((G, tri(d)), dtype)
    r, c = np.tril_indices(d)
    for g in range(G):
        if ok[g]:
            inv = 1 / dtype(gamma[g])
            mean = sum_x[g].astype(dtype) * inv
            out[g] = sum_xx[g].astype(dtype) * inv - mean[r] * mean[c]
    return out


def variances(A, cov):
    """var_gi = a_i S_g a_i^T from packed covariances, in the dtype of cov"""
    d = A.shape[0]
    S = unpack_lower(cov, d)
    A = A.astype(cov.dtype)
    return np.einsum("ij,gjk,ik->gi", A, S, A)


def variance_bound(A, cov):
    """sum_jk |a_ij S_jk a_ik| per (g, i)"""
    d = A.shape[0]
    return np.einsum("ij,gjk,ik->gi", np.abs(A), np.abs(unpack_lower(cov, d)), np.abs(A))


def update_rows(A, g_inv, beta, iterations=1):
    """aku/HmmSet.cc:955-980: every row from the cofactors of the previous A"""
    A = np.array(A, np.float64)
    d = A.shape[0]
    for _ in range(iterations):
        At = A.T.copy()
        C = abs(np.linalg.det(At)) * np.linalg.inv(At)
        for i in range(d):
            row = g_inv[i].T @ C[i]
            A[i] = row * math.sqrt(beta / float(C[i] @ row))
    return A


def estimate_mllt(gamma, sum_x, sum_xx, ok, minvar=0.1, order=None):
    """HmmSet::estimate_mllt in double, the Gaussians' sums taken in `order` (default: pool order)
    -> (A, mean [G x d], var [G x d]); rows of Gaussians without statistics are zero"""
    G, d = sum_x.shape
    order = [g for g in (range(G) if order is None else order) if ok[g]]
    cov = covariances(gamma, sum_x, sum_xx, ok)
    S = unpack_lower(cov, d)
    A = np.eye(d)
    beta = 0.0
    for g in order:
        beta += gamma[g]

    def floored(A):
        v = variances(A, cov)
        return np.where(v < minvar, minvar, v)

    for _ in range(MAX_MLLT_ITER):
        var = floored(A)
        Gm = np.zeros((d, d, d))
        for g in order:
            Gm += (gamma[g] / var[g])[:, None, None] * S[g]
        g_inv = np.array([np.linalg.inv(Gm[i]) for i in range(d)])
        A = update_rows(A, g_inv, beta, MAX_MLLT_A_ITER)
        A = A * (1 / math.pow(abs(np.linalg.det(A)), 1 / float(d)))
    var = floored(A)
    mean = np.zeros((G, d))
    for g in order:
        mean[g] = A @ (sum_x[g] * (1 / gamma[g]))
    var[~np.asarray(ok, bool)] = 0
    return A, mean, var


def mllt_objective(A, gamma, var, ok):
    """sum_g gamma_g (log |det A| - 1/2 sum_i log var_gi) over the Gaussians with statistics"""
    ok = np.asarray(ok, bool)
    return float(np.sum(gamma[ok] * (math.log(abs(np.linalg.det(A))) - 0.5 * np.sum(np.log(var[ok]), axis=1))))


def main(argv):
    if len(argv) < 4:
        print(__doc__)
        return 2
    m = Model(argv[1])
    trans = "-t" in argv
    if "--minvar" in argv:
        m.minvar = float(argv[argv.index("--minvar") + 1])
    for base in open(argv[2]).read().split():
        m.add_dump(base, trans)
    if trans:
        m.estimate_transitions()
    if "--mllt" in argv:
        gamma, sx, sxx, ok = m.mllt_arrays()
        A, mean, var = estimate_mllt(gamma, sx, sxx, ok, m.minvar)
        for g in range(len(m.mean)):
            if ok[g]:
                m.mean[g], m.var[g] = list(mean[g]), list(var[g])
        np.set_printoptions(precision=6, suppress=True, linewidth=200)
        print(A)
    else:
        m.estimate_gaussians()
    m.estimate_mixtures()
    m.write(argv[3])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

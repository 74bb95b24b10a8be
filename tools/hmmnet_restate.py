"""hmmnet_restate.py -- NumPy restatement, in double, of the forward-backward pass over an HMM network
(csrc/hmmnet_fb.hip): aku/HmmNetBaumWelch.cc's fill_backward_probabilities, backward_propagate_epsilon_arcs,
create_segmented_lattice and get_arc_score in dense form.

The input is the network as plain lists and the state log-likelihood rows; nothing here touches the device
or the library.  Next to the totals and occupancies it reports how many arcs the beams pruned and the
smallest distance of any pruning comparison from its threshold, so a test can choose inputs on which a
rounding difference cannot flip a decision.

    net = Net(n_nodes, initial, final, emitting=[(src, tgt, pdf, logp, static, transition)], eps=[(src, tgt, score)])
    r = forward_backward(net, ll, fw_beam=15, bw_beam=200, ac_scale=1.0, viterbi=False)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

ZERO = -1e15                      # HmmNetBaumWelch::LLType::zero()
LOG_TINY = math.log(1e-50)        # util::tiny_for_log
OK, FAILED_BACKWARD, FAILED_FORWARD = 1, 2, 3


def plus(a: float, b: float) -> float:
    """util::logadd"""
    d = a - b
    if d > 0:
        b, d = a, -d
    return b + math.log1p(math.exp(d))


@dataclass
class Net:
    n_nodes: int
    initial: int
    final: int
    emitting: list            # (src, tgt, pdf, logp, static, transition)
    eps: list                 # (src, tgt, score)

    def __post_init__(self):
        N = self.n_nodes
        self.out_em = [[] for _ in range(N)]
        self.in_em = [[] for _ in range(N)]
        for a, e in enumerate(self.emitting):
            self.out_em[e[0]].append(a)
            self.in_em[e[1]].append(a)
        self.out_eps = [[] for _ in range(N)]
        self.in_eps = [[] for _ in range(N)]
        for a, e in enumerate(self.eps):
            self.out_eps[e[0]].append(a)
            self.in_eps[e[1]].append(a)
        # height: longest epsilon path leaving a node; depth: longest epsilon path entering it
        self.height = [0] * N
        self.depth = [0] * N
        memo_h, memo_d = {}, {}

        def h(n):
            if n not in memo_h:
                memo_h[n] = max([1 + h(self.eps[a][1]) for a in self.out_eps[n]], default=0)
            return memo_h[n]

        def d(n):
            if n not in memo_d:
                memo_d[n] = max([1 + d(self.eps[a][0]) for a in self.in_eps[n]], default=0)
            return memo_d[n]

        for n in range(N):
            self.height[n] = h(n)
            self.depth[n] = d(n)
        self.by_height = sorted((n for n in range(N) if self.height[n] > 0), key=lambda n: (self.height[n], n))
        self.by_depth = sorted((n for n in range(N) if self.depth[n] > 0), key=lambda n: (self.depth[n], n))
        self.pdfs = sorted({e[2] for e in self.emitting})
        self.transitions = sorted({e[5] for e in self.emitting})


@dataclass
class Result:
    status: int = OK
    backward_total: float = ZERO
    forward_total: float = ZERO
    pdf_occ: np.ndarray = None       # [T x len(net.pdfs)]
    tr_occ: np.ndarray = None        # [len(net.transitions)]
    pruned: int = 0                  # arcs dropped by either beam
    min_margin: float = math.inf     # smallest |comparison - threshold| of any pruning decision
    path: list = field(default_factory=list)   # Viterbi: the emitting arc of each frame


def arc_score(e, row, ac_scale):
    s = float(row[e[2]]) + e[3]
    if s <= LOG_TINY:
        return ZERO
    return e[4] + ac_scale * s


def _close_backward(net, beta, viterbi):
    for n in net.by_height:
        v = beta[n]
        for a in net.out_eps[n]:
            _, tgt, sc = net.eps[a]
            if beta[tgt] <= ZERO:
                continue
            x = beta[tgt] + sc
            if v <= ZERO:
                v = x
            else:
                v = max(v, x) if viterbi else plus(v, x)
        beta[n] = v


class _Backward:
    """beta rows after the epsilon closure (row T: before any frame) and the per-frame best."""

    def __init__(self, net, ll, bw_beam, ac_scale, viterbi, res):
        T, N = ll.shape[0], net.n_nodes
        self.net, self.ll, self.beam, self.ac, self.vit = net, ll, bw_beam, ac_scale, viterbi
        self.beta = np.full((T + 1, N), ZERO)
        self.best = np.full(T, ZERO)
        self.beta[T, net.final] = 0.0
        _close_backward(net, self.beta[T], viterbi)
        for t in range(T - 1, -1, -1):
            bs = [self.raw(a, t) for a in range(len(net.emitting))]
            self.best[t] = max([x for x in bs if x > ZERO], default=ZERO)
            for a, x in enumerate(bs):
                if x > ZERO:
                    res.min_margin = min(res.min_margin, abs(x - self.best[t] + bw_beam))
                    res.pruned += x - self.best[t] < -bw_beam
            row = self.beta[t]
            for n in range(N):
                v = ZERO
                for a in net.out_em[n]:
                    x = bs[a]
                    if x <= ZERO or x - self.best[t] < -bw_beam:
                        continue
                    if v <= ZERO:
                        v = x
                    else:
                        v = max(v, x) if viterbi else plus(v, x)
                row[n] = v
            _close_backward(net, row, viterbi)

    def raw(self, a, t):
        e = self.net.emitting[a]
        b = self.beta[t + 1, e[1]]
        if b <= ZERO:
            return ZERO
        s = arc_score(e, self.ll[t], self.ac)
        if s <= ZERO:
            return ZERO
        x = b + s
        return x if x > ZERO else ZERO

    def value(self, a, t):
        """the arc's backward score at frame t as the forward pass sees it: ZERO when pruned (and, in
        Viterbi mode, when it is not the best arc of its source node)"""
        x = self.raw(a, t)
        if x <= ZERO or x - self.best[t] < -self.beam:
            return ZERO
        if self.vit:
            src = self.net.emitting[a][0]
            bestv, besta = ZERO, -1
            for o in self.net.out_em[src]:
                y = self.raw(o, t)
                if y <= ZERO or y - self.best[t] < -self.beam:
                    continue
                if y > bestv:
                    bestv, besta = y, o
            if besta != a:
                return ZERO
        return x


def forward_backward(net: Net, ll, fw_beam=15.0, bw_beam=200.0, ac_scale=1.0, viterbi=False) -> Result:
    ll = np.asarray(ll, dtype=np.float64)
    T, N = ll.shape[0], net.n_nodes
    res = Result()
    res.pdf_occ = np.zeros((T, len(net.pdfs)))
    res.tr_occ = np.zeros(len(net.transitions))
    bw = _Backward(net, ll, bw_beam, ac_scale, viterbi, res)
    total = bw.beta[0, net.initial]
    res.backward_total = float(total)
    if total <= ZERO:
        res.status = FAILED_BACKWARD
        return res
    limit = total - fw_beam
    slot = {p: i for i, p in enumerate(net.pdfs)}
    trslot = {k: i for i, k in enumerate(net.transitions)}

    def check(x):
        res.min_margin = min(res.min_margin, abs(x - limit))
        if x < limit:
            res.pruned += 1
            return False
        return True

    if viterbi:
        node, alpha = net.initial, 0.0
        for t in range(T):
            while True:
                best_tot, best_arc, best_eps = ZERO, -1, False
                for a in net.out_eps[node]:
                    _, tgt, sc = net.eps[a]
                    if bw.beta[t, tgt] <= ZERO:
                        continue
                    tot = alpha + bw.beta[t, tgt] + sc
                    if tot < limit:
                        continue
                    if tot > best_tot:
                        best_tot, best_arc, best_eps = tot, a, True
                for a in net.out_em[node]:
                    v = bw.value(a, t)
                    if v <= ZERO or alpha + v < limit:
                        continue
                    if alpha + v > best_tot:
                        best_tot, best_arc, best_eps = alpha + v, a, False
                if best_arc >= 0 and best_eps:
                    alpha += net.eps[best_arc][2]
                    node = net.eps[best_arc][1]
                    continue
                break
            taken = -1
            for a in net.out_em[node]:
                v = bw.value(a, t)
                if v > ZERO and alpha + v >= limit:
                    taken = a
            if taken < 0:
                res.status = FAILED_FORWARD
                return res
            e = net.emitting[taken]
            alpha += arc_score(e, ll[t], ac_scale)
            node = e[1]
            res.path.append(taken)
            res.pdf_occ[t, slot[e[2]]] = 1.0
            res.tr_occ[trslot[e[5]]] += 1.0
        res.forward_total = float(alpha)
        return res

    alpha = np.full(N, ZERO)
    alpha[net.initial] = 0.0
    occ = []                                        # (t, arc, total score)
    for t in range(T):
        for n in net.by_depth:
            v = alpha[n]
            for a in net.in_eps[n]:
                src, _, sc = net.eps[a]
                if alpha[src] <= ZERO or bw.beta[t, n] <= ZERO:
                    continue
                if not check(alpha[src] + bw.beta[t, n] + sc):
                    continue
                x = alpha[src] + sc
                v = x if v <= ZERO else plus(v, x)
            alpha[n] = v
        nxt = np.full(N, ZERO)
        for a, e in enumerate(net.emitting):
            if alpha[e[0]] <= ZERO:
                continue
            v = bw.value(a, t)
            if v <= ZERO:
                continue
            tot = alpha[e[0]] + v
            if not check(tot):
                continue
            x = alpha[e[0]] + arc_score(e, ll[t], ac_scale)
            nxt[e[1]] = x if nxt[e[1]] <= ZERO else plus(nxt[e[1]], x)
            occ.append((t, a, tot))
        alpha = nxt
    alive = [x for x in alpha if x > ZERO]
    if not alive:
        res.status = FAILED_FORWARD
        return res
    tot = alive[0]
    for x in alive[1:]:
        tot = plus(tot, x)
    res.forward_total = float(tot)
    for t, a, x in occ:
        g = math.exp(x - tot)
        e = net.emitting[a]
        res.pdf_occ[t, slot[e[2]]] += g
        res.tr_occ[trslot[e[5]]] += g
    return res


def brute_force(net: Net, ll, ac_scale=1.0, viterbi=False):
    """Every path from the initial to the final node that emits exactly T frames: (log of the sum, or the
    best, of the path scores).  For networks of a few nodes only."""
    ll = np.asarray(ll, dtype=np.float64)
    T = ll.shape[0]
    scores = []

    def walk(node, t, acc):
        if t == T and node == net.final:
            scores.append(acc)
        for a in net.out_eps[node]:
            walk(net.eps[a][1], t, acc + net.eps[a][2])
        if t < T:
            for a in net.out_em[node]:
                e = net.emitting[a]
                s = arc_score(e, ll[t], ac_scale)
                if s > ZERO:
                    walk(e[1], t + 1, acc + s)

    walk(net.initial, 0, 0.0)
    if not scores:
        return ZERO
    if viterbi:
        return max(scores)
    m = max(scores)
    return m + math.log(sum(math.exp(s - m) for s in scores))

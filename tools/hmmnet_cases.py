"""hmmnet_cases.py -- small HMM networks in the text FST format of HmmNetBaumWelch::read_fst, written out for
the tests of the network reader and the forward-backward kernel and for tools/bench_logl.py, with a parser of
its own (nothing of the library) that turns the text into the restatement's Net.

The model behind every case has one state per HMM: state s has the transitions 2 s (self, probability
self_prob[s]) and 2 s + 1 (next, 1 - self_prob[s]), the numbering HmmSet::read_ph gives them.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import hmmnet_restate as RS  # noqa: E402


def self_probs(num_states: int, seed: int = 5) -> np.ndarray:
    return np.round(np.random.default_rng(seed).uniform(0.3, 0.8, num_states), 3)


def write_ph(path: str, self_prob) -> None:
    """A legacy PHONE file with one state per HMM (HmmSet::read_legacy_ph)."""
    with open(path, "w") as f:
        f.write("PHONE\n%d\n" % len(self_prob))
        for s, p in enumerate(self_prob):
            f.write("%d 3 h%d\n-1 -2 %d\n0 1 2 1.0\n1 0\n2 2 2 %.3f 1 %.3f\n" % (s + 1, s, s, p, 1 - p))


def parse(text: str, self_prob) -> "RS.Net":
    """The restatement's Net of a network text; arcs in file order."""
    initial = final = -1
    em, eps, n = [], [], 0
    for line in text.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "I":
            initial = int(f[1])
        elif f[0] == "F":
            final = int(f[1])
        elif f[0] == "T":
            src, tgt = int(f[1]), int(f[2])
            n = max(n, src + 1, tgt + 1)
            label = f[3] if len(f) > 3 and f[3] != "," else ""
            score = float(np.float32(f[5])) if len(f) > 5 else 0.0          # str::str2float goes through float
            if label == "" or label[0] == "#":
                eps.append((src, tgt, score))
            else:
                tr = int(label.split(";")[0])
                s = tr // 2
                p = self_prob[s] if tr % 2 == 0 else 1 - self_prob[s]
                # the .ph file carries three decimals
                p = float("%.3f" % p)
                em.append((src, tgt, s, math.log(p), score, tr))
    return RS.Net(max(n, initial + 1, final + 1), initial, final, em, eps)


class Builder:
    def __init__(self):
        self.lines = []
        self.n = 0

    def node(self) -> int:
        self.n += 1
        return self.n - 1

    def emit(self, src, tgt, tr, static=None, label=""):
        if static is None and not label:
            self.lines.append("T %d %d %d" % (src, tgt, tr))
        else:
            self.lines.append("T %d %d %d%s , %s" % (src, tgt, tr, label, repr(float(static or 0.0))))

    def eps(self, src, tgt, score=None, label=None):
        if score is None and label is None:
            self.lines.append("T %d %d" % (src, tgt))
        else:
            self.lines.append("T %d %d %s , %s" % (src, tgt, label or ",", repr(float(score or 0.0))))

    def state(self, s, nxt=None, static=None, rng=None):
        """A node with state s's self loop and its next transition into `nxt` (a new node when None) -> (node, nxt)"""
        n = self.node()
        nxt = self.node() if nxt is None else nxt
        st = (lambda: None) if static is None else (lambda: round(float(rng.uniform(-static, static)), 3))
        self.emit(n, n, 2 * s, st())
        self.emit(n, nxt, 2 * s + 1, st())
        return n, nxt

    def text(self, initial, final) -> str:
        return "#FSTBasic MaxPlus\nI %d\nF %d\n" % (initial, final) + "\n".join(self.lines) + "\n"


def chain(states, static=None, seed=0) -> str:
    """(a): initial -eps-> a left-to-right chain; the last state's next transition enters the final node"""
    rng = np.random.default_rng(seed)
    b = Builder()
    init = b.node()
    nodes = [b.node() for _ in states]
    fin = b.node()
    b.eps(init, nodes[0])
    st = (lambda: None) if static is None else (lambda: round(float(rng.uniform(-static, static)), 3))
    for i, s in enumerate(states):
        b.emit(nodes[i], nodes[i], 2 * s, st())
        b.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else fin, 2 * s + 1, st())
    return b.text(init, fin)


def fan(num_states, branches, length, seed=0, static=None, eps_scores=False) -> str:
    """(b), (c): the initial node's epsilon arcs fan out into `branches` parallel chains of `length` states that
    merge again in one node, which an epsilon arc joins to the final node"""
    rng = np.random.default_rng(seed)
    b = Builder()
    init, merge, fin = b.node(), b.node(), b.node()
    for _ in range(branches):
        nodes = [b.node() for _ in range(length)]
        b.eps(init, nodes[0], round(float(rng.uniform(-1, 0)), 3) if eps_scores else None)
        st = (lambda: None) if static is None else (lambda: round(float(rng.uniform(-static, static)), 3))
        for i in range(length):
            s = int(rng.integers(0, num_states))
            b.emit(nodes[i], nodes[i], 2 * s, st())
            b.emit(nodes[i], nodes[i + 1] if i + 1 < length else merge, 2 * s + 1, st())
    b.eps(merge, fin)
    return b.text(init, fin)


def deep_eps(num_states, seed=0, tail_score=-0.7) -> str:
    """(d): epsilon chains three deep at the start, in the middle (two routes of different depth into one node) and
    into the final node, the last arc with a nonzero static score"""
    rng = np.random.default_rng(seed)
    b = Builder()
    s = lambda: int(rng.integers(0, num_states))
    init, e1, e2, e3 = b.node(), b.node(), b.node(), b.node()
    b.eps(init, e1, -0.25)
    b.eps(e1, e2, label="#w1")
    b.eps(e2, e3, -0.5)
    a, a2 = b.state(s())
    b.eps(e3, a)
    m, x1, x2 = b.node(), b.node(), b.node()     # a2 has no self loop: routes of depth 1 and 3 into m
    b.eps(a2, m, -0.3)
    b.eps(a2, x1, -0.1)
    b.eps(x1, x2, -0.2)
    b.eps(x2, m, -0.4)
    c, c2 = b.state(s())
    b.eps(m, c)
    d, _ = b.state(s(), c2)                      # a parallel state into the same node
    b.eps(m, d, -0.6)
    t1 = b.node()
    g, _ = b.state(s(), t1)
    b.eps(c2, g)
    t2, t3, fin = b.node(), b.node(), b.node()
    b.eps(t1, t2, -0.15)
    b.eps(t2, t3)
    b.eps(t3, fin, tail_score)
    return b.text(init, fin)


def scores(T, num_states, seed, spread=3.0) -> np.ndarray:
    """synthetic state log-likelihood rows [T x num_states], double"""
    return np.random.default_rng(seed).normal(-8.0, spread, (T, num_states))

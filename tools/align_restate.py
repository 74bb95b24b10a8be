"""align_restate.py -- restatement of the alignment that stats --networks -M vit -a writes (csrc/stats.cc,
aku/stats.cc:59-70, 116-131, 179-188 with HmmNetBaumWelch.cc:763-768): from the best path of
hmmnet_restate.forward_backward(..., viterbi=True).path, the arcs' labels, the range's first frame and the frame
rate to the text of the file -- and an enumeration of a small network's paths of its own, which returns the best
path and its gap to the runner-up, so a test can require inputs on which no rounding decides the path.

Nothing here touches the device or the library.

    labels = arc_labels(text)                       # per emitting arc in file order, as the network file has them
    r = RS.forward_backward(HC.parse(text, sp), ll, viterbi=True)
    alignment_text(r.path, labels, first_frame, frame_rate)
    engine_arcs(net)[a]                             # arc a of the restatement in the numbering of csrc/hmmnet.h
    best, gap = best_two_paths(net, ll)
"""
from __future__ import annotations

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import hmmnet_restate as RS  # noqa: E402


def arc_labels(text: str) -> list:
    """The label of every emitting arc of a network text, in file order: the input label and, after ';', the
    output label (LatticeLabel's constructor, HmmNetBaumWelch.cc:418-462)."""
    out = []
    for line in text.splitlines():
        f = line.split()
        if len(f) < 4 or f[0] != "T" or f[3] == "," or f[3][0] == "#":
            continue
        label = f[3]
        if len(f) > 4 and f[4] != ",":
            label += ";" + f[4]
        out.append(label)
    return out


def frame_label(label: str) -> str:
    """What a frame on the arc is called: the label without its '#' end marks, or "fields[2].fields[1]" where it
    splits at ';' into three fields or more (mixture;state;phone;...)."""
    label = label.replace("#", "")
    f = label.split(";")
    return f[2] + "." + f[1] if len(f) >= 3 else label


def segments(path, labels, first_frame: int) -> list:
    """(start frame, end frame, label) of every run of one label text; the last run ends one frame past the range,
    the reference's own "+1" (aku/stats.cc:184-186)."""
    out = []
    start, cur = -1, None
    for t, a in enumerate(path):
        name = frame_label(labels[a])
        if start < 0:
            start, cur = first_frame + t, name
        elif name != cur:
            out.append((start, first_frame + t, cur))
            start, cur = first_frame + t, name
    if start >= 0:
        out.append((start, first_frame + len(path) + 1, cur))
    return out


def alignment_text(path, labels, first_frame: int, frame_rate: float) -> str:
    mult = int(np.float32(16000) / np.float32(frame_rate))        # print_alignment_line: (int)(16000 / fr), fr a float
    return "".join("%d %d %s\n" % (a * mult, b * mult, name) for a, b, name in segments(path, labels, first_frame))


def engine_arcs(net: "RS.Net") -> list:
    """csrc/hmmnet.h numbers the emitting arcs by source node, a node's arcs in file order: -> per arc of the
    restatement (file order) its number there."""
    order = sorted(range(len(net.emitting)), key=lambda a: (net.emitting[a][0], a))
    out = [0] * len(order)
    for k, a in enumerate(order):
        out[a] = k
    return out


def best_two_paths(net: "RS.Net", ll, ac_scale: float = 1.0):
    """Every path from the initial to the final node that emits exactly T frames, epsilon arcs included, walked one
    by one (a branch is left when the final node can no longer be reached in the frames that remain).
    -> (the emitting arcs of the best path, its score minus the runner-up's; inf with one path), or (None, 0.0)
    without any.  Two routes of epsilon arcs under the same emitting arcs are two paths.  Small networks only."""
    ll = np.asarray(ll, dtype=np.float64)
    T, N = ll.shape[0], net.n_nodes
    INF = 1 << 30
    need = [INF] * N                     # fewest emitting arcs from a node to the final node
    need[net.final] = 0
    changed = True
    while changed:
        changed = False
        for e in net.eps:
            if need[e[1]] < need[e[0]]:
                need[e[0]], changed = need[e[1]], True
        for e in net.emitting:
            if need[e[1]] + 1 < need[e[0]]:
                need[e[0]], changed = need[e[1]] + 1, True
    found = []                           # (score, arcs), the two best so far

    def keep(score, arcs):
        found.append((score, tuple(arcs)))
        found.sort(key=lambda p: -p[0])
        del found[2:]

    arcs = []

    def walk(node, t, acc):
        if need[node] > T - t:
            return
        if t == T and node == net.final:
            keep(acc, arcs)
        for a in net.out_eps[node]:
            walk(net.eps[a][1], t, acc + net.eps[a][2])
        if t < T:
            for a in net.out_em[node]:
                e = net.emitting[a]
                s = RS.arc_score(e, ll[t], ac_scale)
                if s > RS.ZERO:
                    arcs.append(a)
                    walk(e[1], t + 1, acc + s)
                    arcs.pop()

    walk(net.initial, 0, 0.0)
    if not found:
        return None, 0.0
    return list(found[0][1]), (found[0][0] - found[1][0] if len(found) > 1 else float("inf"))


SIX = ("I 0\nF 5\nT 0 1 , , -0.2\nT 0 2 #b , -0.9\nT 1 1 2\nT 1 3 3 , 0.4\nT 2 2 8\nT 2 3 9\nT 3 4 10 , -0.3\n"
       "T 3 5 11\nT 4 4 4\nT 4 5 5\n")           # the six-node network of tests/test_hmmnet_host.py


def path_cases() -> list:
    """The inputs of the path tests, (name, network text, frames, score seed), over the one-state-per-HMM model of
    hmmnet_cases (state s: transitions 2 s and 2 s + 1, HMM h<s>): the six-node network with epsilon arcs and
    plain labels; a left-to-right chain of 12 labelled states; two parallel branches of four states that share
    their first and last pdf under different labels (11 nodes)."""
    import hmmnet_cases as HC

    def labelled(b, nodes, states, last, tag):
        for i, s in enumerate(states):
            lab = ";0;%s%d" % (tag, s)
            b.emit(nodes[i], nodes[i], 2 * s, 0.0, lab)
            b.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else last, 2 * s + 1, 0.0, lab + "#")

    b = HC.Builder()
    init = b.node()
    nodes = [b.node() for _ in range(12)]
    fin = b.node()
    b.eps(init, nodes[0])
    labelled(b, nodes, [9, 2, 21, 5, 14, 0, 33, 7, 18, 3, 26, 11], fin, "h")
    chain = b.text(init, fin)
    b = HC.Builder()
    init, merge, fin = b.node(), b.node(), b.node()
    for tag, states, score in (("h", [4, 17, 8, 23], -0.4), ("g", [4, 30, 12, 23], -0.1)):
        nodes = [b.node() for _ in states]
        b.eps(init, nodes[0], score)
        labelled(b, nodes, states, merge, tag)
    b.eps(merge, fin)
    branches = b.text(init, fin)
    return [("six", SIX, 7, 101), ("six", SIX, 12, 102), ("chain", chain, 16, 103), ("chain", chain, 20, 104),      # (75582 paths at 20 frames: still enumerable)
            ("branches", branches, 9, 105), ("branches", branches, 17, 106)]

"""fst_restate.py -- the FST token pass of csrc/fst_search.hip restated in NumPy float32: the yardstick of its tests.

It follows the reference's decoder/src/Fst.cc (reader), FstAcoustics.cc (duration tables, :60-101),
LnaReaderCircular.cc (:168-198, the three LNA decodings) and FstSearch_tmpl.hh (:45-51 start, :179-239 propagation,
:54-113 selection, :151-176 result) operation by operation, every float32 operation rounded on its own.  Where the
reference's std::sort leaves the order of equal log-probabilities open, the rule here is "the earlier candidate in
propagation order wins" (a stable sort), and `ties` reports every tie that could change an output:

    ("limit", frame)   equal log-probabilities across the token-limit boundary
    ("dur", frame)     duplicates of one (node, words) with equal log-probability and different durations
    ("final",)         best end-node tokens of equal log-probability with different words

The tests use inputs for which the report is empty.  logf / lgammaf are the C library's (ctypes), as in the reference.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import struct

import numpy as np

F32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.lgammaf.restype = ctypes.c_float
_libm.lgammaf.argtypes = [ctypes.c_float]

OK, NO_TOKENS = 0, 1


class FstReadError(ValueError):
    pass


class Net:
    """arc_begin (nodes + 1), arc_tgt, arc_lp (float32), arc_word (-1: none), node_pdf, node_end, initial, symbols (bytes)"""

    def __init__(self):
        self.arc_begin = self.arc_tgt = self.arc_lp = self.arc_word = self.node_pdf = self.node_end = None
        self.initial = -1
        self.symbols = []


def _atoi(b: bytes) -> int:
    s = b.lstrip(b" \t\n\v\f\r")
    i, sign = 0, 1
    if s[:1] in (b"+", b"-"):
        sign = -1 if s[:1] == b"-" else 1
        i = 1
    v = 0
    while i < len(s) and 48 <= s[i] <= 57:
        v = v * 10 + s[i] - 48
        i += 1
    return sign * v


def _strtod(b: bytes) -> float:
    """the longest prefix strtod accepts (decimal forms, inf, nan); 0.0 when none"""
    import re
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?(?:inf(?:inity)?|nan|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?))", b, re.I)
    return float(m.group(1)) if m else 0.0


def _split(line: bytes) -> list:
    """str::split(line, " ", true): runs of spaces are one delimiter, a trailing delimiter adds an empty field"""
    fields, begin, end, pending = [], 0, 0, False
    while begin < len(line):
        pending = False
        while end < len(line):
            if line[end:end + 1] == b" ":
                pending = True
                break
            end += 1
        fields.append(line[begin:end])
        end += 1
        while end < len(line) and line[end:end + 1] == b" ":
            end += 1
        begin = end
    if pending:
        fields.append(b"")
    return fields


def read_fst(data: bytes) -> Net:
    """Fst::read (Fst.cc:10-103) on the bytes of a file.  Raises FstReadError with the reference's message."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    header = lines[0] if lines else b""
    if header != b"#FSTBasic MaxPlus":
        raise FstReadError("Unknown header '%s'." % header.decode("latin-1"))
    pdf, end, arcs, initial = [], [], [], -1
    sym_id, symbols = {}, []

    def grow(n):
        while len(pdf) <= n:
            pdf.append(-1)
            end.append(0)
            arcs.append([])

    for line in lines[1:]:
        text = line.decode("latin-1")
        if line == b"":     # (read_line ends at a line of no bytes only at the end of the file; a bare newline is "Too few fields")
            raise FstReadError("Too few fields '%s'." % text)
        f = _split(line)
        if len(f) < 2:
            raise FstReadError("Too few fields '%s'." % text)
        first = _atoi(f[1])
        if first < 0:
            raise FstReadError("Negative node index '%s'." % text)
        grow(first)
        if f[0] == b"I":
            initial = first
            if len(f) > 2:
                raise FstReadError("Too many fields for I: '%s'." % text)
            continue
        if f[0] == b"F":
            end[first] = 1
            if len(f) > 2:
                raise FstReadError("Too many fields for F: '%s'." % text)
            continue
        if f[0] != b"T":
            raise FstReadError("Weird type indicator: '%s'." % f[0].decode("latin-1"))
        if len(f) < 3 or len(f) > 6:
            raise FstReadError("Weird number of fields for T: '%s'." % text)
        second = _atoi(f[2])
        if second < 0:
            raise FstReadError("Negative node index '%s'." % text)
        grow(second)
        word = -1
        if len(f) >= 5 and f[4] != b",":
            if f[4] not in sym_id:
                sym_id[f[4]] = len(symbols)
                symbols.append(f[4])
            word = sym_id[f[4]]
        lp = F32(_strtod(f[5])) if len(f) >= 6 else F32(0)
        arcs[first].append((second, lp, word))
        p = _atoi(f[3]) if len(f) >= 4 else -1     # (the reference reads a field that is not there; here: no pdf)
        if pdf[second] == -1:
            pdf[second] = p
        elif pdf[second] != p:
            raise FstReadError("Conflicting emission_pdf_indices for node %d: %d != %d." % (second, pdf[second], p))
    if initial < 0:
        raise FstReadError("No initial node.")
    net = Net()
    net.arc_begin = np.zeros(len(pdf) + 1, np.int32)
    for i, a in enumerate(arcs):
        net.arc_begin[i + 1] = net.arc_begin[i] + len(a)
    flat = [x for a in arcs for x in a]
    net.arc_tgt = np.array([x[0] for x in flat], np.int32)
    net.arc_lp = np.array([x[1] for x in flat], np.float32)
    net.arc_word = np.array([x[2] for x in flat], np.int32)
    net.node_pdf = np.array(pdf, np.int32)
    net.node_end = np.array(end, np.int32)
    net.initial = initial
    net.symbols = symbols
    return net


def read_durations(text: str, by_state: bool = False):
    """FstAcoustics::duration_read (:60-89): (a, b) float32 tables.  As the reference builds them (resize(n), then
    push_back) the file's values sit at [n, 2n) behind n zeros; by_state: at [0, n), as was evidently meant."""
    tok = text.split()
    if int(tok[0]) != 4:
        raise ValueError("FstAcoustics: invalid format")
    n = int(tok[1])
    a, b = [], []
    for i in range(n):
        if int(tok[2 + 3 * i]) != i:
            raise ValueError("FstAcoustics: invalid format")
        a.append(F32(float(tok[3 + 3 * i])))
        b.append(F32(float(tok[4 + 3 * i])))
    if by_state:
        return np.array(a, np.float32), np.array(b, np.float32)
    z = [F32(0)] * n
    return np.array(z + a, np.float32), np.array(z + b, np.float32)


def duration_logprob(a_tab, b_tab, pdf: int, d: int) -> np.float32:
    """FstAcoustics::duration_logprob (:91-101); a pdf past the tables (where the reference reads out of bounds) is 0"""
    if a_tab is None or pdf >= len(a_tab):
        return F32(0)
    a = F32(a_tab[pdf])
    if a <= 0:
        return F32(0)
    b = F32(b_tab[pdf])
    logf, lgammaf = (lambda x: F32(_libm.logf(float(x)))), (lambda x: F32(_libm.lgammaf(float(x))))
    const = F32(F32(F32(-a) * logf(b)) - lgammaf(a))
    with np.errstate(all="ignore"):
        return F32(F32(F32(F32(a - F32(1)) * logf(F32(d))) - F32(F32(d) / b)) + const)


def decode_lna(raw: bytes, n_models: int, lnabytes: int) -> np.ndarray:
    """LnaReaderCircular::go_to (:168-198) on the frames behind the 5-byte header: float32 [frames, n_models]"""
    u = np.frombuffer(raw, np.uint8)
    frames = len(u) // (n_models * lnabytes)
    u = u[:frames * n_models * lnabytes]
    if lnabytes == 4:
        return u.view("<f4").reshape(frames, n_models).copy()
    if lnabytes == 2:
        v = u.reshape(frames, n_models, 2).astype(np.float64)
        return ((v[:, :, 0] * 256 + v[:, :, 1]) / -1820.0).astype(np.float32)
    return (u.reshape(frames, n_models).astype(np.float64) / -24.0).astype(np.float32)


def read_lna(path: str):
    data = open(path, "rb").read()
    n_models, lnabytes = struct.unpack(">iB", data[:5])
    return decode_lna(data[5:], n_models, lnabytes), lnabytes


class Result:
    def __init__(self):
        self.status = OK
        self.tokens = []            # (node, logprob float32, dur, words tuple of ids), descending
        self.words = ()
        self.logprob = F32(-1.0)
        self.best_logprob = F32(-9999999.0)
        self.best_final_logprob = F32(-9999999.9)
        self.ties = []
        # what the device's capacities have to hold: the most candidates of one frame; the most distinct (node, words)
        # among one frame's candidates within the beam; the distinct word sequences made by such candidates
        self.max_candidates = 0
        self.max_keys = 0
        self.histories = set()
        self.last_keys = 1          # distinct (node, words) among ALL candidates of the last frame
        self.frames_done = 0

    def text(self, symbols) -> bytes:
        return b" ".join(symbols[w] for w in self.words)


def search(net: Net, ac: np.ndarray, beam=2600.0, token_limit=5000, duration_scale=3.0, transition_scale=1.0,
           durations=None) -> Result:
    """ac: float32 [frames, models] as decode_lna gives them; durations: (a, b) of read_durations or None."""
    beam, dscale, tscale = F32(beam), F32(duration_scale), F32(transition_scale)
    a_tab, b_tab = durations if durations is not None else (None, None)
    res = Result()
    tokens = [(net.initial, F32(0), 0, ())]
    with np.errstate(all="ignore"):
        for t in range(ac.shape[0]):
            cand = []
            for (node, lp0, dur0, words0) in tokens:
                src_pdf = int(net.node_pdf[node])
                for a in range(int(net.arc_begin[node]), int(net.arc_begin[node + 1])):
                    tgt = int(net.arc_tgt[a])
                    lp = F32(lp0 + F32(tscale * net.arc_lp[a]))
                    dur, words = dur0, words0
                    if net.node_pdf[tgt] >= 0:
                        lp = F32(lp + ac[t, net.node_pdf[tgt]])
                    if tgt != node:
                        if src_pdf >= 0:
                            lp = F32(lp + F32(dscale * duration_logprob(a_tab, b_tab, src_pdf, dur)))
                            dur = 1
                    else:
                        dur += 1
                    if net.arc_word[a] >= 0:
                        words = words + (int(net.arc_word[a]),)
                    cand.append((tgt, lp, dur, words))
            res.max_candidates = max(res.max_candidates, len(cand))
            if not cand:
                res.status = NO_TOKENS
                tokens = []
                break
            order = sorted(range(len(cand)), key=lambda i: -float(cand[i][1]))   # stable: the earlier candidate first
            top = cand[order[0]][1]
            inside = [i for i in range(len(cand)) if cand[i][1] > F32(top - beam) or i == order[0]]
            res.max_keys = max(res.max_keys, len({(cand[i][0], cand[i][3]) for i in inside}))
            res.histories.update(cand[i][3] for i in inside if cand[i][3])
            res.last_keys = len({(c[0], c[3]) for c in cand})
            seen, kept = {}, []
            for i in order:
                key = (cand[i][0], cand[i][3])
                if key in seen:
                    j = seen[key]
                    if cand[j][1] == cand[i][1] and cand[j][2] != cand[i][2]:
                        res.ties.append(("dur", t))
                    continue
                if len(kept) == token_limit + 1:
                    if cand[i][1] == cand[kept[-1]][1] and cand[i][1] > F32(cand[kept[0]][1] - beam):
                        res.ties.append(("limit", t))
                    break
                seen[key] = i
                kept.append(i)
            best = cand[kept[0]][1]
            n = 1
            while n < len(kept) and cand[kept[n]][1] > F32(best - beam):
                n += 1
            tokens = [cand[i] for i in kept[:n]]
            res.frames_done = t + 1
    res.tokens = tokens
    if tokens:
        res.best_logprob = tokens[0][1]
    finals = [tk for tk in tokens if net.node_end[tk[0]]]
    if finals:
        res.words, res.logprob, res.best_final_logprob = finals[0][3], finals[0][1], finals[0][1]
        if any(tk[1] == finals[0][1] and tk[3] != finals[0][3] for tk in finals[1:]):
            res.ties.append(("final",))
    return res


def write_fst(net_lines: list) -> bytes:
    return b"#FSTBasic MaxPlus\n" + b"".join(l + b"\n" for l in net_lines)


def random_net(rng, n_nodes: int, n_models: int, max_deg: int = 6, p_word: float = 0.1, n_words: int = 7) -> bytes:
    """A random network in the file's text form: self-loops, non-emitting nodes, symbols also on self-loops, end nodes."""
    pdf = [-1 if rng.random() < 0.2 else int(rng.integers(0, n_models)) for _ in range(n_nodes)]
    lines = [b"I 0"]
    for s in range(n_nodes):
        for _ in range(int(rng.integers(0, max_deg + 1))):
            t = s if rng.random() < 0.25 else int(rng.integers(0, n_nodes))
            sym = b"w%d" % int(rng.integers(0, n_words)) if rng.random() < p_word else b","
            lines.append(b"T %d %d %d %s %.6f" % (s, t, pdf[t], sym, -float(rng.random()) * 5))
    for s in range(n_nodes):
        if rng.random() < 0.3:
            lines.append(b"F %d" % s)
    return write_fst(lines)

"""dur_est_restate.py -- restatement of the dur_est tool (csrc/dur_est.cc; aku/dur_est.cc with the line reader of
aku/PhnReader.cc:82-134, 293-399): the duration histograms of state-numbered .phn files and their gamma fits, with
a .phn reader of its own.  Nothing here touches the library.

The fit repeats estimate_gamma_models (aku/dur_est.cc:62-120) operation for operation in IEEE double.  lgamma is
the C library's, through ctypes (math.lgamma is CPython's own implementation and rounds differently), and log is
math.log, which calls the C library's: both sides run the same operations, so the four printed decimals are
compared as bytes.

    table = histograms(hmm_states, num_states, files, maxdur=100, skip=0)
    hist_text(table, skip); dur_text(table, skip, mincount)
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]
lgamma = _libm.lgamma

FRAME_RATE = 125.0            # PhnReader's default: Recipe::Info::init_phn_files without a feature generator


def _atoi(s: str) -> int:
    s = s.lstrip(" \t")
    k = 1 if s[:1] in ("+", "-") else 0
    j = k
    while j < len(s) and s[j].isdigit():
        j += 1
    return int(s[:j]) if j > k else 0


def _fields(text: str, n: int) -> list:
    """str::split(" \\t", group = true, n): fields end at a blank, the blanks after it are skipped, the n-th field
    takes the rest"""
    out, at = [], 0
    while at < len(text):
        if len(out) == n - 1:
            out.append(text[at:])
            break
        stop = at
        while stop < len(text) and text[stop] not in " \t":
            stop += 1
        out.append(text[at:stop])
        at = stop + 1
        while at < len(text) and text[at] in " \t":
            at += 1
    return out


class PhnLines:
    """PhnReader as dur_est drives it: open, set_frame_limits, set_line_limits, then line after line."""

    def __init__(self, path: str):
        self.rows = open(path).read().split("\n")
        self.pos = 0
        self.line_no = 0
        self.first = self.last = self.last_line = 0
        self.spf = np.float32(16000) / np.float32(FRAME_RATE)

    def next(self):
        """(start, end, label, state) or None"""
        if self.last_line > 0 and self.line_no >= self.last_line:
            return None
        while self.pos < len(self.rows) and self.rows[self.pos] == "":
            self.pos += 1
        if self.pos >= len(self.rows):
            return None
        text = self.rows[self.pos]
        self.pos += 1
        start = end = state = -1
        if text[0].isdigit():
            f = _fields(text, 4)
            if len(f) < 3:
                raise ValueError("invalid start or end time: " + text)
            start = int(np.float32(int(f[0])) / self.spf)      # (int)(long / float samples per frame)
            end = int(np.float32(int(f[1])) / self.spf)
            head = f[2]
            dot = head.find(".")
            if dot >= 0:
                state = _atoi(head[dot + 1:])
                head = head[:dot] + head[dot + 2:]
            if start > end:
                raise ValueError("invalid start or end time: " + text)
        else:
            head = _fields(text, 2)[0]
        if self.last > 0:
            if start >= self.last:
                return None
            if end >= self.last:
                end = self.last
        if self.first > 0 and 0 <= start < self.first:
            start = self.first
        self.line_no += 1
        return start, end, head.split(",")[0], state

    def set_frame_limits(self, first: int, last: int) -> None:
        self.first, self.last = first, last
        while True:
            pos, line_no = self.pos, self.line_no
            row = self.next()
            if row is None:
                return
            if row[1] < 0 or row[1] > first:
                self.pos, self.line_no = pos, line_no           # back to the line's start
                return

    def set_line_limits(self, first_line: int, last_line: int) -> None:
        self.last_line = last_line
        while self.line_no < first_line:                        # first_line lines are consumed
            if self.next() is None:
                return


def file_lines(path: str, start_time: float = 0.0, end_time: float = 0.0, start_line: int = 0, end_line: int = 0):
    """The lines dur_est counts of one file -- every line after the one that init_utterance_segmentation takes --
    or None when that first line is not there."""
    rd = PhnLines(path)
    if start_time > 0 or end_time > 0:
        st, en = np.float32(start_time), np.float32(end_time)   # Recipe::Info keeps floats
        rd.set_frame_limits(int(st * np.float32(FRAME_RATE)), int(en * np.float32(FRAME_RATE)))
    if start_line > 0 or end_line > 0:
        rd.set_line_limits(start_line, end_line)
    if rd.next() is None:
        return None
    out = []
    while True:
        row = rd.next()
        if row is None:
            return out
        out.append(row)


def histograms(hmm_states: dict, num_states: int, files: list, maxdur: int = 100, skip: int = 0) -> np.ndarray:
    """hmm_states[label]: the state index of every state of the HMM; files: dicts of file_lines' arguments.
    -> table [num_states x maxdur], table[s][d - 1] lines of d frames (d capped at maxdur)"""
    table = np.zeros((num_states, maxdur), np.int64)
    for f in files:
        for start, end, label, state in file_lines(**f) or []:
            if state == -1:
                raise ValueError("Collecting duration statistics requires phn files with state numbers!")
            s = hmm_states[label][state]
            if s < skip:
                continue
            d = min(end - start, maxdur)
            assert d > 0
            table[s, d - 1] += 1
    return table


def hist_text(table, skip: int = 0) -> str:
    return "".join("%d " % i + "".join("%d " % c for c in table[i]) + "\n" for i in range(skip, len(table)))


def _nll(a: float, mean_log: float, log_mean: float) -> float:
    return a * (1 + log_mean - math.log(a)) + lgamma(a) + (1 - a) * mean_log


def fit_gamma(hist):
    """estimate_gamma_models: (a, b), or None with fewer than two points"""
    hist = [int(c) for c in hist]
    count = float(sum(hist))
    if count < 2:
        return None
    mean = 0.0
    for i, c in enumerate(hist):
        mean += float((i + 1) * c)
    mean /= count
    var = 0.0
    for i, c in enumerate(hist):
        var += (i + 1 - mean) * (i + 1 - mean) * c
    var = max(var / (count - 1), 0.25)
    log_mean = math.log(mean)
    mean_log = 0.0
    for i, c in enumerate(hist):
        mean_log += math.log(i + 1) * c
    mean_log /= count
    r = (math.sqrt(5) - 1) / 2
    a = 1.0
    b = 2 * max(mean * mean / var, 1.5) - 1
    x1 = a + (1 - r) * (b - a)
    x2 = a + r * (b - 1)                     # b - 1, as the reference computes it
    x1v, x2v = _nll(x1, mean_log, log_mean), _nll(x2, mean_log, log_mean)
    while b - a > 0.01:
        if x2v > x1v:
            b = x2
            x2, x2v = x1, x1v
            x1 = a + (1 - r) * (b - a)
            x1v = _nll(x1, mean_log, log_mean)
        else:
            a = x1
            x1, x1v = x2, x2v
            x2 = b - (1 - r) * (b - a)
            x2v = _nll(x2, mean_log, log_mean)
    a_out = (a + b) / 2
    return a_out, mean / a_out


def dur_text(table, skip: int = 0, mincount: int = 10) -> str:
    out = "4\n%d\n" % len(table)
    for i, hist in enumerate(table):
        fit = None if i < skip or int(hist.sum()) < mincount else fit_gamma(hist)
        a, b = fit if fit else (0.0, 0.0)
        out += "%d %.4f %.4f\n" % (i, a, b)
    return out

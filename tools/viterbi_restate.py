"""viterbi_restate.py -- the forced aligner in plain Python: a restatement of the reference's windowed beam search
(aku/Viterbi.cc fill / fill_transition_probs / fill_observation_probs / compute_best_path / move, aku/Lattice.cc
move, aku/Lattice.hh cells and ranges, the window loop of aku/align.cc:viterbi_align and the retry loop of its main),
to compare csrc/align_viterbi.hip against at the kernel's own interface.

It follows the reference's algorithm, not the kernel's layout: sources push to their targets in ascending position
and .ph transition order and replace on a strict '>', a frame's cells are a dictionary, and a move really re-bases the
lattice and the transcription.  There is no ring, no per-slot origin and no pull.  The arithmetic is the one the
header of align_viterbi.hip lists: float32 cells with the -1e24 sentinel, lik = float32(exp(float64(ll))), the best
likelihood in float32, float32(safe_log(lik) - best_log), cells floored at -1e24, unused() = from < 0 and
log_prob == -1e24, the accumulated and final log-probabilities in double, and
target = int(float32(swins) * (float32(1) - float32(overlap))).

Besides the kernel's own outputs (positions, loglik, status, n_fail) the result carries what a test needs to show
that an input is fair and that it reached the path it is meant for: min_margin, max_abs_cell, max_abs_term, max_span,
moves, attempt_moves, kept_one, frames_past_first_ring, pruned_front, pruned_back, exact_ties, aborts (see Result).

Limit: this restatement is not compared with the reference binary (oracle/_ref/align_refmain), which needs the
device library for its likelihoods; tests/test_align_gpu.py's tool-parity test remains the link to that binary.  Its
independent check is tests/test_viterbi_restate_host.py: with one window and wide beams it gives the path of
global_viterbi below, a plain dynamic programme in double.

Nothing here touches the device or the library.

    trans = [[(off, np.float32(np.log(p))) for off, p in topo.transitions(s)] for s in range(S)]
    r = align(states, line_states, trans, rows, start_frame, end_frame, eof_frame,
              swins=16, beam=20.0, sbeam=3, maxbeam=200.0, overlap=0.4)
    r.positions, r.loglik, r.status, r.n_fail, r.min_margin, ...
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

ALIGN_ACTIVE, ALIGN_OK, ALIGN_GAVE_UP, ALIGN_ERROR = 0, 1, 2, 3

F32 = np.float32
INF = F32(1e24)                       # Lattice.hh INF: the "unused" log-probability is -INF, a finite float
TINY = 1e-50                          # util::tiny_for_log


def safe_log(x: float) -> float:
    return math.log(TINY) if x < TINY else math.log(x)


def ulp32(x: float) -> float:
    """the spacing of float32 at |x|"""
    return float(np.spacing(F32(abs(x))))


def window_target(swins: int, overlap: float) -> int:
    """frames committed by a window that is not the last: (int)(win_size * (1 - overlap)), all in float"""
    return int(F32(swins) * (F32(1) - F32(overlap)))


def global_viterbi(ll, states, trans, force_end=True):
    """Plain DP over positions: V[t, p] = max_q V[t-1, q] + log a(q -> p) + ll[t, p], V[0, 0] = 0."""
    T, P = ll.shape[0], len(states)
    V = np.full(P, -np.inf)
    V[0] = 0.0
    back = np.zeros((T, P), np.int64)
    for t in range(1, T):
        best = np.full(P, -np.inf)
        arg = np.zeros(P, np.int64)
        for q in range(P):
            if V[q] == -np.inf:
                continue
            for off, lp in trans[states[q]]:
                p = q + off
                if p < P and V[q] + lp > best[p]:
                    best[p] = V[q] + lp
                    arg[p] = q
        V = best + ll[t, states]
        back[t] = arg
    pos = np.zeros(T, np.int64)
    pos[-1] = P - 1 if force_end else int(np.argmax(V))
    for t in range(T - 1, 0, -1):
        pos[t - 1] = back[t, pos[t]]
    return pos


@dataclass
class Result:
    positions: np.ndarray = None      # committed absolute transcription position per frame (of the last attempt)
    loglik: float = 0.0               # accumulated + final log-probability
    status: int = ALIGN_ACTIVE
    n_fail: int = 0                   # times the forced end was missed; each one doubled the beams
    # counters, summed over every attempt
    min_margin: float = math.inf      # smallest non-zero |a - b| over the comparisons that decide something: both
                                      # beam scans, replace-or-keep between two sources, best cell
    max_abs_cell: float = 0.0         # largest |log-probability| a cell held
    max_abs_term: float = 0.0         # largest |term| added into the double log-likelihood
    max_span: int = 0                 # widest (new range end - pruned previous range start) of any frame
    frames: int = 0                   # lattice frames filled
    moves: int = 0
    attempt_moves: int = 0            # ... of the last attempt alone
    kept_one: int = 0                 # moves that left one frame
    frames_past_first_ring: int = 0   # filled frames at swins or more frames after start_frame
    pruned_front: int = 0             # cells dropped by the scan from the range start
    pruned_back: int = 0              # ... and from the range end
    exact_ties: int = 0               # comparisons with a == b between two distinct candidates
    aborts: int = 0                   # the reference would assert or read out of bounds here: not a test input
    abort_reason: str = ""
    froms_ok: bool = True             # every from-pointer written lay in the previous frame's final range
    target: int = 0

    def same(self, other: "Result") -> bool:
        a, b = dict(self.__dict__), dict(other.__dict__)
        pa, pb = a.pop("positions"), b.pop("positions")
        return a == b and np.array_equal(pa, pb)


class _Abort(Exception):
    pass


class _Retry(Exception):
    pass


class _Empty(Exception):
    pass


@dataclass
class Search:
    """The search of one utterance.  step(n) runs n window steps (a retry's restart is part of the next step), so a
    caller can cut a run where it likes; nothing outside this object is read or written."""
    states: list                      # HMM state per transcription position
    line_states: list                 # positions each transcript line adds (0: none)
    trans: list                       # per HMM state: [(target offset, float32 log prob)] in .ph order
    rows: np.ndarray                  # score rows, row 0 = feature frame start_frame; float32 or float64
    start_frame: int
    end_frame: int                    # 0: to the end of the audio
    eof_frame: int
    swins: int
    beam: float
    sbeam: int
    maxbeam: float
    overlap: float
    no_force_end: bool = False
    res: Result = field(default_factory=Result)

    def __post_init__(self):
        self.res.target = self.target = window_target(self.swins, self.overlap)
        self.trans = [[(int(o), F32(lp)) for o, lp in v] for v in self.trans]
        self.fresh = True
        self.out = []
        self.acc = 0.0
        self.fin = 0.0

    # -- bookkeeping ---------------------------------------------------------------------------
    def _margin(self, a, b):
        d = abs(float(a) - float(b))
        if d != 0.0 and d < self.res.min_margin:
            self.res.min_margin = d

    def _cell_seen(self, v):
        if v != -INF:
            self.res.max_abs_cell = max(self.res.max_abs_cell, abs(float(v)))

    def _term(self, v):
        self.res.max_abs_term = max(self.res.max_abs_term, abs(float(v)))

    def _ll(self, frame, state) -> float:
        return float(self.rows[frame - self.start_frame, state])

    # -- Viterbi::reset and the start of viterbi_align -------------------------------------------
    def _reset(self):
        self.fresh = False
        self.res.attempt_moves = 0
        self.cells = [dict() for _ in range(self.swins)]     # per frame: position -> [from, float32 log prob]
        self.ranges = [None] * self.swins                    # per frame: [start, end) or None (unused)
        self.cur = 0                                         # m_current_frame
        self.ffr = self.start_frame                          # m_feature_frame
        self.last_frame = self.swins
        self.last_position = self.swins
        self.tr = []                                         # m_transcription: states, re-based by every move
        self.base = 0                                        # positions erased so far (to report absolute ones)
        self.line = 0
        self.tr_eof = False
        self.best = -INF
        self.bestpos = -1
        self.acc = 0.0
        self.fin = 0.0
        self.wstart = self.start_frame
        self.path = [0] * self.swins
        self.out = []

    def _fill_transcription(self):
        if not self.tr:
            self.tr_eof = self.line >= len(self.line_states)
        while not self.tr_eof and len(self.tr) < self.last_position:
            n = self.line_states[self.line]
            at = self.base + len(self.tr)
            self.tr.extend(self.states[at:at + n])
            self.line += 1
            self.tr_eof = self.line >= len(self.line_states)
        if self.last_position > len(self.tr):
            self.last_position = len(self.tr)

    # -- Viterbi::fill_transition_probs --------------------------------------------------------
    def _transitions(self):
        f = self.cur - 1
        prev, rng = self.cells[f], self.ranges[f]
        beam = F32(self.beam)
        while True:                                          # prune at the beginning
            p = rng[0]
            if p >= rng[1]:
                raise _Abort("the whole range was pruned")
            c = prev[p]
            self._margin(c[1] + beam, self.best)
            if (c[0] < 0 and c[1] == -INF) or c[1] + beam < self.best or p + self.sbeam < self.bestpos:
                del prev[p]
                rng[0] = p + 1
                self.res.pruned_front += 1
            else:
                break
        while True:                                          # prune at the end
            p = rng[1] - 1
            if p < rng[0]:
                raise _Abort("the whole range was pruned")
            c = prev[p]
            self._margin(c[1] + beam, self.best)
            if (c[0] < 0 and c[1] == -INF) or c[1] + beam < self.best or p - self.sbeam > self.bestpos:
                del prev[p]
                rng[1] = p
                self.res.pruned_back += 1
            else:
                break
        new = self.cells[self.cur]
        assert not new and self.ranges[self.cur] is None     # frames from m_current_frame on are clear
        lo, hi = -1, -1
        for p in range(rng[0], rng[1]):
            src = prev[p]
            for off, lp in self.trans[self.tr[p]]:
                t = p + off
                if t < 0 or t >= self.last_position:
                    continue
                if hi <= t:
                    hi = t + 1
                if lo == -1 or lo > t:
                    lo = t
                v = src[1] + lp
                tc = new.get(t)
                if tc is None:                               # an unused cell: from < 0 and log_prob == -INF
                    new[t] = [p, v]
                else:
                    self._margin(v, tc[1])
                    if v == tc[1]:
                        self.res.exact_ties += 1
                    if v > tc[1]:
                        tc[0], tc[1] = p, v
        if lo < 0:
            raise _Abort("no transition leads into the lattice")
        self.ranges[self.cur] = [lo, hi]
        self.res.max_span = max(self.res.max_span, hi - rng[0])

    # -- Viterbi::fill_observation_probs -------------------------------------------------------
    def _observations(self):
        f = self.cur
        cells, (lo, hi) = self.cells[f], self.ranges[f]
        lik = {}
        best_prob = F32(-1)
        for p in range(lo, hi):
            lik[p] = F32(math.exp(self._ll(self.ffr, self.tr[p])))
            if lik[p] > best_prob:
                best_prob = lik[p]
        best_log = F32(safe_log(float(best_prob)))
        self.acc += float(best_log)
        self._term(best_log)
        self.bestpos = -1
        self.best = -INF
        prev_rng = self.ranges[f - 1]
        for p in range(lo, hi):
            c = cells.get(p)
            if c is None:
                raise _Abort("a hole in the new range at position %d" % p)
            if not (prev_rng[0] <= c[0] < prev_rng[1]):
                self.res.froms_ok = False
            sp = F32(safe_log(float(lik[p])) - float(best_log))
            c[1] = c[1] + sp
            if self.bestpos >= 0:
                self._margin(c[1], self.best)
                if c[1] == self.best:
                    self.res.exact_ties += 1
            if c[1] > self.best:
                self.best = c[1]
                self.bestpos = p
            if c[1] < -INF:
                c[1] = -INF
            self._cell_seen(c[1])
        if self.bestpos < 0:
            raise _Abort("no best position")
        self.res.frames += 1
        if self.wstart + f - self.start_frame >= self.swins:
            self.res.frames_past_first_ring += 1

    # -- Viterbi::compute_best_path ------------------------------------------------------------
    def _best_path(self):
        f = self.cur - 1
        rng = self.ranges[f]
        if not self.no_force_end and self.last_window:
            pos = self.last_position - 1
            if pos < len(self.tr) - 1:
                raise _Retry("transcription end out of window")
            if not (rng[0] <= pos < rng[1]):
                raise _Retry("transcription end out of range")
        else:
            pos = self.bestpos
        if not (rng[0] <= pos < rng[1]):
            pos = rng[1] - 1                                 # "last transcription states were lost"
        self.fin = float(self.cells[f][pos][1])
        self.path[f] = pos
        while f > 0:
            r = self.ranges[f]
            if not (r[0] <= pos < r[1]):
                raise _Abort("the traced path leaves the range at frame %d" % f)
            pos = self.cells[f][pos][0]
            self.path[f - 1] = pos
            f -= 1
        if pos < 0:
            raise _Abort("the traced path ends below the lattice")

    # -- Viterbi::fill -------------------------------------------------------------------------
    def _fill(self) -> bool:
        self._fill_transcription()
        if not self.tr:
            raise _Empty()
        if self.cur == 0:
            self.cells[0] = {0: [-1, F32(0)]}
            self.ranges[0] = [0, 1]
            self.acc = safe_log(math.exp(self._ll(self.ffr, self.tr[0])))
            self._term(self.acc)
            self.ffr += 1
            self.cur += 1
        eof = False
        while self.cur < self.last_frame:
            if self.ffr >= self.eof_frame:
                self.last_frame = self.cur
                self.last_window = True
                eof = True
                break
            self._transitions()
            self._observations()
            self.ffr += 1
            self.cur += 1
        self._best_path()
        return eof

    # -- Viterbi::move with Lattice::move ------------------------------------------------------
    def _move(self, frame, position):
        del self.tr[:position]
        self.base += position
        for f in range(frame):
            self.cells[f], self.ranges[f] = {}, None
        for src in range(frame, self.swins):
            if self.ranges[src] is None:
                break
            dst = src - frame
            self.cells[src], self.cells[dst] = self.cells[dst], self.cells[src]
            self.ranges[src], self.ranges[dst] = self.ranges[dst], self.ranges[src]
            cells, rng = self.cells[dst], self.ranges[dst]
            if rng[0] < position:
                for p in range(rng[0], min(position, rng[1])):
                    cells.pop(p, None)
                rng[0] = position
            moved = {}
            for p in range(rng[0], rng[1]):
                c = cells[p]
                c[0] -= position
                if dst == 0:
                    c[0] = -1
                elif p - position == 0:
                    c[0] = 0
                moved[p - position] = c
            self.cells[dst] = moved
            rng[0] -= position
            rng[1] -= position
        self.cur -= frame
        self.bestpos -= position
        for f in range(frame, self.last_frame):
            self.path[f - frame] = self.path[f] - position
        f = self.cur - 1
        rng = self.ranges[f]
        if not (rng[0] <= self.path[f] < rng[1]):
            raise _Abort("the path's cell of the last kept frame is gone")
        lp = self.cells[f][self.path[f]][1]
        self.acc += float(lp)
        self._term(lp)
        self.fin = 0.0
        for p in range(rng[0], rng[1]):
            c = self.cells[f][p]
            c[1] = c[1] - lp
            self._cell_seen(c[1])
        self.res.moves += 1
        self.res.attempt_moves += 1
        if self.cur == 1:
            self.res.kept_one += 1

    # -- one pass of viterbi_align's loop, with main's retry -------------------------------------
    def _window(self):
        res = self.res
        if self.fresh:
            self._reset()
        wend = self.wstart + self.swins
        last_window = False
        if self.end_frame > 0:
            if self.wstart >= self.end_frame:
                res.status = ALIGN_OK
                return
            if wend >= self.end_frame:
                wend = self.end_frame
                last_window = True
        self.last_window = last_window
        self.last_frame = wend - self.wstart
        try:
            if self._fill():
                last_window = True
                wend = self.wstart + self.last_frame
        except _Retry:
            res.n_fail += 1
            self.beam *= 2
            self.sbeam *= 2
            if self.beam <= self.maxbeam:
                self.fresh = True
            else:
                res.status = ALIGN_GAVE_UP
            return
        self._term(self.fin)
        target = self.target
        if last_window:
            target = wend - self.wstart
        if self.wstart + target > wend:
            target = wend - self.wstart
        if target > self.cur:
            raise _Abort("a committed frame was never filled")
        self.out.extend(self.base + self.path[f] for f in range(target))
        self.wstart += target
        if last_window and self.wstart >= self.end_frame:
            res.status = ALIGN_OK
            return
        if target < 1 or target >= self.cur:
            raise _Abort("move to frame %d of %d" % (target, self.cur))
        self._move(target, self.path[target])

    def step(self, windows: int) -> bool:
        """Run up to `windows` window steps.  -> True while the search is not finished."""
        res = self.res
        for _ in range(windows):
            if res.status != ALIGN_ACTIVE:
                break
            try:
                self._window()
            except _Empty:
                res.status = ALIGN_ERROR                     # the empty transcription: the kernel's search error 1
            except _Abort as e:
                res.status = ALIGN_ERROR
                res.aborts += 1
                res.abort_reason = str(e)
        res.positions = np.array(self.out, np.int64)
        res.loglik = self.acc + self.fin
        return res.status == ALIGN_ACTIVE


def align(states, line_states, trans, rows, start_frame, end_frame, eof_frame, *, swins, beam, sbeam, maxbeam,
          overlap=0.4, no_force_end=False, windows=1 << 20) -> Result:
    """The whole search of one utterance, `windows` window steps at a time."""
    s = Search(list(states), list(line_states), trans, np.asarray(rows), int(start_frame), int(end_frame),
               int(eof_frame), int(swins), float(beam), int(sbeam), float(maxbeam), float(overlap), bool(no_force_end))
    while s.step(windows):
        pass
    return s.res

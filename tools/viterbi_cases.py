"""viterbi_cases.py -- the inputs of the forced aligner's window tests (tests/test_viterbi_restate_host.py on the
CPU, tests/test_align_windows_gpu.py on the device): a topology written as a .ph text together with its tables, and
named cases, each the smallest shape that reaches one path of csrc/align_viterbi.hip.  A case is seeded; its seed was
chosen on the CPU so that viterbi_restate.align shows the counter the case is named for (`reached`) and decides
nothing within 64 float32 ulps (`fair`).  Both are asserted by the tests, on the restatement alone.

Nothing here touches the device or the library.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import viterbi_restate as VR  # noqa: E402

N_HMM, PER = 12, 3
WIDE = dict(beam=1e6, sbeam=100000, maxbeam=1e6)


def skip_topology(n_hmm: int = N_HMM, equal: bool = False):
    """3-state HMMs, pdf = 3 h + j; every third HMM has a skip from state 0 to state 2 and one from state 1 straight
    into the next HMM.  Unequal probabilities printed with four decimals (the text of tests/test_align_gpu.py's
    write_ph), or with equal=True the same shape with 1/2, 1/2 and 1/3, 1/3, 1/3.
    -> (.ph text, pdfs per HMM, per pdf [(target offset, probability as the text holds it)])"""
    rng = np.random.default_rng(5)
    lines = ["PHONE", "%d" % n_hmm]
    hmm_states, trans = [], []

    def row(state, targets, probs):
        text = [("%r" % p) if equal else ("%.4f" % p) for p in probs]
        lines.append("%d %d %s" % (state + 2, len(targets), " ".join("%d %s" % (t, s) for t, s in zip(targets, text))))
        offs = [(PER - state) if t == 1 else (t - 2 - state) for t in targets]
        trans.append([(o, float(s)) for o, s in zip(offs, text)])

    for h in range(n_hmm):
        lines.append("%d 5 h%d" % (h + 1, h))
        lines.append("-1 -2 %d %d %d" % (3 * h, 3 * h + 1, 3 * h + 2))
        lines.append("0 1 2 1.0")
        lines.append("1 0")
        hmm_states.append([3 * h, 3 * h + 1, 3 * h + 2])
        a = rng.uniform(0.3, 0.8)
        if h % 3 == 0:
            row(0, [2, 3, 4], [1 / 3] * 3 if equal else [a, (1 - a) * 0.7, (1 - a) * 0.3])
            b = rng.uniform(0.3, 0.8)
            row(1, [3, 4, 1], [1 / 3] * 3 if equal else [b, (1 - b) * 0.8, (1 - b) * 0.2])
        else:
            row(0, [2, 3], [0.5, 0.5] if equal else [a, 1 - a])
            b = rng.uniform(0.3, 0.8)
            row(1, [3, 4], [0.5, 0.5] if equal else [b, 1 - b])
        c = rng.uniform(0.3, 0.8)
        row(2, [4, 1], [0.5, 0.5] if equal else [c, 1 - c])
    return "\n".join(lines) + "\n", hmm_states, trans


def log_tables(trans):
    """per pdf [(offset, float32(log p))]: what the search adds"""
    return [[(o, np.float32(np.log(p))) for o, p in v] for v in trans]


@dataclass
class Case:
    name: str
    n: int                      # HMMs in the transcript
    T: int                      # frames of audio from start_frame
    swins: int
    seed: int
    overlap: float = 0.4
    beam: float = 1e6
    sbeam: int = 100000
    maxbeam: float = 1e6
    equal: bool = False         # the equal-probability topology
    rows: str = "f32"           # "f32": N(-60, 6) as float32; "f64": the same in double, not float32 values;
                                # "const": every score -60; "f64-lean": see lean_rows
    start: int = 0
    end: int = 0                # end_frame (absolute), 0: none
    no_force_end: bool = False
    reached: object = None      # Result -> bool: the counter that proves the path was reached

    def options(self) -> dict:
        return dict(swins=self.swins, beam=self.beam, sbeam=self.sbeam, maxbeam=self.maxbeam, overlap=self.overlap,
                    no_force_end=self.no_force_end)


def lean_rows(rng, T, S):
    """float64 rows whose rounding to float32 leans one way per state: float32 values near -80 (one ulp there is
    2^-17, and exp(-80) is a normal float: no denormal likelihood decides anything) plus 0.45 ulp on even states and minus 0.45 ulp on odd ones.  Two paths that differ in the frames they
    spend on even and on odd states drift apart by 0.9 ulp a frame when the rows are read as floats."""
    base = rng.normal(-80.0, 0.25, (T, S)).astype(np.float32).astype(np.float64)
    lean = np.where(np.arange(S) % 2 == 0, 0.45, -0.45) * 2.0 ** -17
    return base + lean[None, :]


def inputs(case: Case, seed: int = None) -> dict:
    """transcript (HMM per line), states per position, states per line, score rows (row 0 = frame `start`) and the
    frame limits of a case"""
    rng = np.random.default_rng(case.seed if seed is None else seed)
    S = N_HMM * PER
    transcript = [int(x) for x in rng.integers(0, N_HMM, case.n)]
    if case.rows == "const":
        rows = np.full((case.T, S), -60.0, np.float32)
    elif case.rows == "f64-lean":
        rows = lean_rows(rng, case.T, S)
    else:
        rows = rng.normal(-60.0, 6.0, (case.T, S))
        if case.rows == "f32":
            rows = rows.astype(np.float32)
    states = [3 * h + j for h in transcript for j in range(PER)]
    return dict(transcript=transcript, states=states, line_states=[PER] * case.n, rows=rows, start=case.start,
                end=case.end, eof=case.start + case.T)


_TABLES = {}


def tables(equal: bool):
    if equal not in _TABLES:
        _TABLES[equal] = log_tables(skip_topology(N_HMM, equal)[2])
    return _TABLES[equal]


def restate(case: Case, seed: int = None, rows=None, windows: int = 1 << 20, **override) -> "VR.Result":
    x = inputs(case, seed)
    opt = case.options()
    opt.update(override)
    return VR.align(x["states"], x["line_states"], tables(case.equal), x["rows"] if rows is None else rows, x["start"],
                    x["end"], x["eof"], windows=windows, **opt)


def fair(r: "VR.Result") -> bool:
    """No decision within 64 float32 ulps of a cell: the device's double exp and log are within an ulp of the
    host's, so a (float) rounding can differ only at a rounding boundary and then by one ulp of a cell."""
    return r.aborts == 0 and r.min_margin >= 64 * VR.ulp32(r.max_abs_cell)


def doublings(beam: float, maxbeam: float) -> int:
    """misses of the forced end until the doubled beam passes maxbeam"""
    n = 1
    while beam * 2 ** n <= maxbeam:
        n += 1
    return n


MAX_OFF = 2
OK, GAVE_UP = VR.ALIGN_OK, VR.ALIGN_GAVE_UP

CASES = [
    # 1. the ring wraps several times, with moves
    Case("ring8", n=4, T=48, swins=8, seed=1, overlap=0.4,
         reached=lambda r: r.status == OK and r.frames_past_first_ring > 4 * 8 and r.moves >= 8),
    Case("ring5", n=3, T=40, swins=5, seed=1, overlap=0.4,
         reached=lambda r: r.status == OK and r.frames_past_first_ring > 4 * 5 and r.moves >= 8),
    Case("ring7", n=3, T=44, swins=7, seed=1, overlap=0.5,
         reached=lambda r: r.status == OK and r.frames_past_first_ring > 4 * 7 and r.moves >= 8),
    # 2. moves that keep one frame
    Case("keep1", n=2, T=30, swins=4, seed=1, overlap=0.25,
         reached=lambda r: r.status == OK and r.target == 3 and r.kept_one >= 5),
    Case("keep1-of-10", n=3, T=40, swins=10, seed=1, overlap=0.1,
         reached=lambda r: r.status == OK and r.target == 9 and r.kept_one >= 3),
    # 3. the lattice width at its bound: 2 sbeam + 1 + max_off, and swins
    Case("width7", n=12, T=120, swins=40, seed=1, sbeam=2,
         reached=lambda r: r.status == OK and r.n_fail == 0 and r.max_span == 2 * 2 + 1 + MAX_OFF
         and r.pruned_front > 0 and r.pruned_back > 0),
    Case("width-swins", n=3, T=40, swins=6, seed=1,
         reached=lambda r: r.status == OK and r.max_span == 6),
    # 4. the probability beam alone prunes (and changes the path: asserted by the tests against the wide run)
    Case("pbeam", n=6, T=40, swins=16, seed=1, beam=10.0, maxbeam=1000.0,
         reached=lambda r: r.status == OK and r.n_fail == 0 and r.pruned_front + r.pruned_back > 0),
    # 5. retries
    Case("retry-ok", n=8, T=32, swins=16, seed=2, beam=10.0, sbeam=2, maxbeam=200.0,
         reached=lambda r: r.status == OK and r.n_fail >= 2),
    Case("give-up", n=8, T=32, swins=40, seed=1, beam=5.0, sbeam=1, maxbeam=15.0,
         reached=lambda r: r.status == GAVE_UP and r.n_fail == doublings(5.0, 15.0) == 2 and len(r.positions) == 0),
    Case("give-up-windows", n=8, T=32, swins=16, seed=1, beam=5.0, sbeam=1, maxbeam=15.0,
         reached=lambda r: r.status == GAVE_UP and r.n_fail == 2 and r.moves >= 3 and len(r.positions) > 0),
    Case("too-long", n=10, T=14, swins=16, seed=1, beam=20.0, sbeam=3, maxbeam=200.0,
         reached=lambda r: r.status == GAVE_UP and r.n_fail == doublings(20.0, 200.0) == 4 and len(r.positions) == 0),
    # 6. exact ties: equal probabilities and constant rows
    Case("ties-wide", n=6, T=40, swins=16, seed=3, equal=True, rows="const",
         reached=lambda r: r.status == OK and r.exact_ties > 100),
    # the smallest position wins the best cell, so the state beam holds the search back: three misses of the forced
    # end, and with sbeam = 16 it finishes
    Case("ties-sbeam2", n=6, T=40, swins=16, seed=3, equal=True, rows="const", sbeam=2, beam=1e5, maxbeam=1e6,
         reached=lambda r: r.status == OK and r.n_fail == 3 and r.exact_ties > 100 and r.pruned_back > 0),
    # 7. float64 rows
    Case("ring8-f64", n=4, T=48, swins=8, seed=1, overlap=0.4, rows="f64",
         reached=lambda r: r.status == OK and r.frames_past_first_ring > 4 * 8 and r.moves >= 8),
    Case("retry-ok-f64", n=8, T=32, swins=16, seed=2, beam=10.0, sbeam=2, maxbeam=200.0, rows="f64",
         reached=lambda r: r.status == OK and r.n_fail >= 2),
    Case("f64-decides", n=4, T=48, swins=8, seed=20779, rows="f64-lean",
         reached=lambda r: r.status == OK and r.moves >= 8),
    # 8. start_frame, end_frame, no_force_end
    Case("start7", n=4, T=40, swins=8, seed=1, start=7,
         reached=lambda r: r.status == OK and r.moves >= 6),
    Case("end-inside", n=4, T=48, swins=8, seed=1, end=30,       # windows start at 0, 4, ..., 24: 30 is inside one
         reached=lambda r: r.status == OK and len(r.positions) == 30),
    Case("end-on-border", n=4, T=48, swins=8, seed=1, end=32,    # the window from 24 ends at 32
         reached=lambda r: r.status == OK and len(r.positions) == 32),
    Case("no-force-end", n=8, T=32, swins=16, seed=1, beam=1e6, sbeam=2, maxbeam=1e6, no_force_end=True,
         reached=lambda r: r.status == OK and r.n_fail == 0 and r.positions[-1] != 3 * 8 - 1
         and r.pruned_front + r.pruned_back > 0),
]
BY_NAME = {c.name: c for c in CASES}

# one batch, one set of options: the utterances of four cases above and one with an empty transcription
BATCH_OPTIONS = dict(swins=16, overlap=0.4, beam=10.0, sbeam=2, maxbeam=200.0, no_force_end=False)
BATCH_MEMBERS = ["ring8", "width7", "retry-ok", "ties-wide"]


def restate_member(name: str, windows: int = 1 << 20) -> "VR.Result":
    """a batch member under the batch's options and the equal-probability topology (a batch has one of each)"""
    x = inputs(BY_NAME[name])
    return VR.align(x["states"], x["line_states"], tables(True), x["rows"], x["start"], x["end"], x["eof"],
                    windows=windows, **BATCH_OPTIONS)

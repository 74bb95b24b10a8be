"""tools/viterbi_restate.py, the plain restatement of the forced aligner's windowed beam search, checked without a
GPU: against an independent reference (with one window, wide beams and a forced end it gives exactly the path of a
plain dynamic programme in double), on its internal invariants over windowed runs, as a pure function of its inputs
however the run is cut into window steps, and on the inputs of tests/test_align_windows_gpu.py: every case there is
fair and reaches the path it is named for, which that module asserts again before it touches the device."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import viterbi_cases as VC  # noqa: E402
import viterbi_restate as VR  # noqa: E402

TRANS = VC.tables(False)


def _utterance(seed, n, T):
    rng = np.random.default_rng(seed)
    transcript = [int(x) for x in rng.integers(0, VC.N_HMM, n)]
    states = [3 * h + j for h in transcript for j in range(VC.PER)]
    rows = rng.normal(-60.0, 6.0, (T, VC.N_HMM * VC.PER)).astype(np.float32)
    return states, [VC.PER] * n, rows


def test_topology_text_and_tables_agree():
    """the tables the restatement gets are the transitions of the .ph text the device tests load"""
    text, hmm_states, trans = VC.skip_topology()
    assert hmm_states[4] == [12, 13, 14]
    assert [o for o, _ in trans[0]] == [0, 1, 2] and [o for o, _ in trans[1]] == [0, 1, 2]      # h0 skips
    assert [o for o, _ in trans[3]] == [0, 1] and [o for o, _ in trans[2]] == [0, 1]
    assert "2 3 2 " in text and text.startswith("PHONE\n12\n1 5 h0\n-1 -2 0 1 2\n0 1 2 1.0\n1 0\n")
    for v in trans:
        assert abs(sum(p for _, p in v) - 1) < 2e-4                      # four printed decimals
    _, _, eq = VC.skip_topology(equal=True)
    assert [p for _, p in eq[0]] == [1 / 3] * 3 and [p for _, p in eq[2]] == [0.5, 0.5]
    assert max(o for v in trans for o, _ in v) == VC.MAX_OFF


def test_tables_are_the_librarys(tmp_path):
    """capi.Topology reads the .ph text back as the tables the restatement uses (host only)"""
    from aaltoasr_amd import build, capi as A
    build.build()
    for equal in (False, True):
        text, hmm_states, trans = VC.skip_topology(VC.N_HMM, equal)
        p = tmp_path / ("t%d.ph" % equal)
        p.write_text(text)
        t = A.Topology(str(p))
        assert [t.hmm_states(h) for h in range(VC.N_HMM)] == hmm_states
        assert [t.transitions(s) for s in range(VC.N_HMM * VC.PER)] == trans
        assert t.max_offset() == VC.MAX_OFF


def test_window_target_is_computed_in_float():
    assert VR.window_target(10, 0.1) == 9            # float32(10) * (1 - float32(0.1)) rounds up to 9.0
    assert VR.window_target(4, 0.25) == 3
    assert VR.window_target(8, 0.4) == 4 and VR.window_target(5, 0.4) == 3 and VR.window_target(7, 0.5) == 3
    assert VR.window_target(1000, 0.4) == 600
    assert VR.window_target(16, 0.0) == 16           # what aasr_align_batch_create refuses: the whole window


@pytest.mark.parametrize("variant", ["plain", "end_frame", "start_frame"])
def test_one_window_is_the_global_viterbi(variant):
    """20 seeds, the skip topology: swins >= T, wide beams, the end forced -> exactly the path of the double DP.
    A seed counts when no decision is closer than T * 2^-23 * max |cell|: what float32 cells can lose over T frames."""
    done = 0
    for seed in range(100, 160):
        n, T = 3 + seed % 6, 40 + seed % 17
        states, lines, rows = _utterance(seed, n, T)
        start = 7 if variant == "start_frame" else 0
        end = start + T - 9 if variant == "end_frame" else 0
        r = VR.align(states, lines, TRANS, rows, start, end, start + T, swins=T + 8, **VC.WIDE)
        used = (end - start) if end else T
        if not (r.aborts == 0 and r.min_margin > used * 2.0 ** -23 * r.max_abs_cell):
            continue
        want = VR.global_viterbi(rows[:used].astype(np.float64), states, TRANS)
        assert r.status == VR.ALIGN_OK and r.n_fail == 0 and r.moves == 0
        assert np.array_equal(r.positions, want), (variant, seed)
        # the log-likelihood is the path's score under the same DP, the first frame's observation included
        ll = rows[:used].astype(np.float64)
        score = ll[0, states[0]]
        for t in range(1, used):
            lp = [l for o, l in TRANS[states[want[t - 1]]] if o == want[t] - want[t - 1]][0]
            score += float(lp) + ll[t, states[want[t]]]
        assert abs(r.loglik - score) <= 2 * used * VR.ulp32(max(r.max_abs_cell, r.max_abs_term)), (variant, seed)
        done += 1
        if done == 20:
            break
    assert done == 20


WINDOWED = [dict(swins=8, overlap=0.4), dict(swins=5, overlap=0.4), dict(swins=7, overlap=0.5),
            dict(swins=4, overlap=0.25), dict(swins=10, overlap=0.1), dict(swins=16, overlap=0.4, beam=20.0, sbeam=3,
                                                                           maxbeam=200.0)]


@pytest.mark.parametrize("k", range(len(WINDOWED)))
def test_windowed_runs_keep_their_invariants(k):
    opt = dict(VC.WIDE)
    opt.update(WINDOWED[k])
    finished = 0
    for seed in range(200, 230):
        n, T = 2 + seed % 3, 30 + seed % 13
        states, lines, rows = _utterance(seed, n, T)
        start = seed % 2 * 5
        end = start + T - 4 if seed % 3 == 0 else 0
        r = VR.align(states, lines, TRANS, rows, start, end, start + T, **opt)
        if r.aborts or r.status != VR.ALIGN_OK:
            continue
        finished += 1
        assert r.froms_ok                                            # from-pointers lie in the previous final range
        assert len(r.positions) == min(start + T, end or start + T) - start
        assert r.positions[0] == 0
        step = np.diff(r.positions)
        assert step.min() >= 0, seed
        # inside a window a step is a transition of the topology; the first frame of the next window starts from the
        # cells that survived the move, which the reference reports as a discontinuous path when it differs
        inside = [s for i, s in enumerate(step) if (i + 1) % r.target]
        assert max(inside) <= VC.MAX_OFF, seed
        assert math.isfinite(r.loglik)
        assert r.max_span <= opt["swins"]
    assert finished >= 10


@pytest.mark.parametrize("name", ["ring8", "keep1", "retry-ok", "give-up-windows", "ties-sbeam2", "end-inside"])
def test_cutting_a_run_into_window_steps_changes_nothing(name):
    case = VC.BY_NAME[name]
    whole = VC.restate(case)
    for windows in (1, 3):
        assert VC.restate(case, windows=windows).same(whole), windows
    assert VC.restate(case).same(whole)                              # and a second run finds no state left behind


@pytest.mark.parametrize("name", [c.name for c in VC.CASES])
def test_device_cases_are_fair_and_reach_their_path(name):
    case = VC.BY_NAME[name]
    r = VC.restate(case)
    assert r.aborts == 0, r.abort_reason
    assert VC.fair(r), (r.min_margin, r.max_abs_cell)
    assert case.reached(r), r
    assert r.max_abs_cell < 256
    if name == "pbeam":                                              # the probability beam changes the result
        assert not np.array_equal(VC.restate(case, **VC.WIDE).positions, r.positions)
    if name == "f64-decides":                                        # ... and so does reading the rows as floats
        rows32 = VC.inputs(case)["rows"].astype(np.float32)
        assert not np.array_equal(VC.restate(case, rows=rows32).positions, r.positions)
    if case.rows.startswith("f64"):
        rows = VC.inputs(case)["rows"]
        assert rows.dtype == np.float64 and (rows.astype(np.float32).astype(np.float64) != rows).all()


def test_empty_transcription_is_an_error_status():
    rows = np.full((5, 36), -60.0, np.float32)
    r = VR.align([], [0, 0], TRANS, rows, 0, 0, 5, swins=8, **VC.WIDE)
    assert r.status == VR.ALIGN_ERROR and r.aborts == 0 and len(r.positions) == 0


def test_what_the_reference_would_assert_on_is_counted():
    """overlap 0 moves to frame swins of swins: the read past the path that aasr_align_batch_create now refuses"""
    states, lines, rows = _utterance(1, 4, 40)
    r = VR.align(states, lines, TRANS, rows, 0, 0, 40, swins=8, overlap=0.0, **VC.WIDE)
    assert r.aborts == 1 and r.status == VR.ALIGN_ERROR

"""The forced aligner's kernel (csrc/align_viterbi.hip) against tools/viterbi_restate.py at the kernel's own
interface, capi.align_batch over synthetic score rows: ring wraps and moves, moves that keep one frame, the lattice
width at its bound, pruning by either beam, retries with doubled beams, exact ties, float64 rows, start and end
frames, and one bad utterance in a batch.  The inputs are the named cases of tools/viterbi_cases.py.

Every case is first judged on the restatement alone: the reference would not assert on it (aborts == 0), no decision
is closer than 64 float32 ulps of the largest cell (the device's double exp and log are within an ulp of the host's,
so a (float) rounding can differ only at a rounding boundary and then by one ulp of a cell: such decisions cannot
flip), and the counter the case is named for shows that its path was reached.  Then status, n_fail and positions are
compared with ==, and the log-likelihood within (frames + moves) * ulp32(largest term): one possible last-bit
difference per float term that enters the double sum.  Each case prints its counters and the observed difference.

Which single-line change of align_viterbi.hip which case catches (each was built and run once, not committed):
  `v >= cand` for `v > cand` in the pull           ties-wide, ties-sbeam2, both batch tests (the last source wins)
  `op > bpos` in the best-cell reduce              ties-wide, ties-sbeam2, both batch tests (the largest position wins)
  `W - 1` in the width check                       width7, width-swins and every case whose max_span equals the width
  reading `(float)` of a float64 row               f64-decides (the restatement on rounded rows takes another path)
Two changes no input can show.  `op <= bpos` in the reduce differs from `op < bpos` only where both lanes hold the same
position, and then assigns what is there.  Dropping `prev0` from the unused test differs only where a cell of a later
frame is exactly -1e24, the floor: every term added to a cell is at least log(1e-50), so no search of a few hundred
frames gets there."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import viterbi_cases as VC  # noqa: E402
import viterbi_restate as VR  # noqa: E402

from aaltoasr_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 3          # rows of a constant between utterances: a wrong row0 reads a likelihood no state has
PAD_VALUE = 7.0


@pytest.fixture(scope="module")
def world(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("align_windows")
    S = VC.N_HMM * VC.PER
    topo = {}
    for equal in (False, True):
        text, hmm_states, trans = VC.skip_topology(VC.N_HMM, equal)
        path = str(d / ("equal.ph" if equal else "skip.ph"))
        open(path, "w").write(text)
        t = capi.Topology(path)
        for h in range(VC.N_HMM):
            assert t.hmm_states(h) == hmm_states[h]
        for s in range(S):
            assert t.transitions(s) == trans[s], s               # the restatement's tables are the library's
        assert t.max_offset() == VC.MAX_OFF
        topo[equal] = t
    gmm = capi.Gmm.from_arrays(*synth.make_model(D=39, G=2 * S, S=S, comps=2, seed=7))   # only its state count matters
    return dict(topo=topo, gmm=gmm, want={})


def _restated(world, case):
    if case.name not in world["want"]:
        world["want"][case.name] = VC.restate(case)
    return world["want"][case.name]


def _device(capi, world, utts, equal, options, windows=1 << 20):
    """one batch: the utterances' rows stacked with pad rows between them -> align_batch's results"""
    import torch
    dtype = utts[0]["rows"].dtype
    rows, row0, at = [], [], 0
    for x in utts:
        assert x["rows"].dtype == dtype
        rows.append(np.full((PAD, x["rows"].shape[1]), PAD_VALUE, dtype))
        at += PAD
        row0.append(at)
        rows.append(x["rows"])
        at += len(x["rows"])
    rows.append(np.full((PAD, rows[0].shape[1]), PAD_VALUE, dtype))
    dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows))).cuda()
    o = dict(options)
    o["no_force_end"] = int(o.get("no_force_end", False))
    opts = capi.AlignOptions.defaults(**o)
    out = capi.align_batch(world["gmm"], world["topo"][equal], [x["transcript"] for x in utts], dev, row0,
                           [x["start"] for x in utts], [x["end"] for x in utts], [x["eof"] for x in utts], opts,
                           windows=windows)
    torch.cuda.synchronize()
    return out


def _compare(name, got, want, frames):
    bound = (frames + want.attempt_moves) * VR.ulp32(want.max_abs_term)
    diff = abs(got["loglik"] - want.loglik)
    print("%s: status %d n_fail %d moves %d kept_one %d max_span %d pruned %d+%d exact_ties %d past_ring %d "
          "min_margin %.3g max|cell| %.4g | loglik %.9g, |device - restatement| = %.3g (bound %.3g)"
          % (name, want.status, want.n_fail, want.moves, want.kept_one, want.max_span, want.pruned_front,
             want.pruned_back, want.exact_ties, want.frames_past_first_ring, want.min_margin, want.max_abs_cell,
             want.loglik, diff, bound))
    assert got["status"] == want.status, name
    assert got["n_fail"] == want.n_fail, name
    assert np.array_equal(got["positions"], want.positions), (name, got["positions"], want.positions)
    assert diff <= bound, (name, got["loglik"], want.loglik)


@pytest.mark.parametrize("name", [c.name for c in VC.CASES])
def test_kernel_equals_the_restatement(capi, world, name):
    case = VC.BY_NAME[name]
    x = VC.inputs(case)
    want = _restated(world, case)
    # the conditions, on the restatement alone, before the device is touched
    assert want.aborts == 0, want.abort_reason
    assert want.min_margin >= 64 * VR.ulp32(want.max_abs_cell), (want.min_margin, want.max_abs_cell)
    assert case.reached(want), want
    if name == "keep1-of-10":
        assert want.target == 9
    if name == "pbeam":
        assert not np.array_equal(VC.restate(case, **VC.WIDE).positions, want.positions)
    if name == "f64-decides":
        as_floats = VC.restate(case, rows=x["rows"].astype(np.float32))
        assert not np.array_equal(as_floats.positions, want.positions)
    got = _device(capi, world, [x], case.equal, case.options())[0]
    _compare(name, got, want, case.T)
    if name == "give-up":
        assert len(got["positions"]) == 0 and got["n_fail"] == VC.doublings(case.beam, case.maxbeam)
    if name == "too-long":
        assert len(got["positions"]) == 0 and got["status"] == capi.ALIGN_GAVE_UP


@pytest.mark.parametrize("windows", [1, 1 << 20])
def test_a_bad_utterance_leaves_its_neighbours_alone(capi, world, windows):
    """the utterances of ring8, width7, retry-ok and ties-wide and, in their middle, one whose transcript lines add
    no HMM (search error 1), under one set of options and the equal-probability topology: the bad one ends with
    ALIGN_ERROR, every other one equals its solo run bit for bit and the restatement"""
    names = VC.BATCH_MEMBERS
    utts = [VC.inputs(VC.BY_NAME[n]) for n in names]
    want = [VC.restate_member(n) for n in names]
    for n, w in zip(names, want):
        assert VC.fair(w) and w.status == VR.ALIGN_OK, n
    assert want[2].n_fail >= 2 and want[3].exact_ties > 100 and want[0].moves >= 3
    bad = dict(utts[0], transcript=[-1, -1, -1])
    batch = _device(capi, world, utts[:2] + [bad] + utts[2:], True, VC.BATCH_OPTIONS, windows=windows)
    assert batch[2]["status"] == capi.ALIGN_ERROR and len(batch[2]["positions"]) == 0
    if windows == 1:
        assert batch[0]["calls"] >= 4
    for k, (n, x, w) in enumerate(zip(names, utts, want)):
        b = batch[k if k < 2 else k + 1]
        _compare("batch/" + n, b, w, len(x["rows"]))
        solo = _device(capi, world, [x], True, VC.BATCH_OPTIONS)[0]
        assert solo["status"] == b["status"] and solo["n_fail"] == b["n_fail"], n
        assert np.array_equal(solo["positions"], b["positions"]), n
        assert solo["loglik"] == b["loglik"], n

"""The schedule of the chunked score + LNA step as data (csrc/gmm_score_lna.cc: plan_score_lna), read through
aasr_debug_score_lna_plan -- no handle, no device.  Whatever the knobs:

  - every frame is in exactly one scoring launch and in exactly one LNA segment;
  - every frame of a segment lies in a scoring launch with an index <= the one the segment waits for;
  - every scoring range begins on a multiple of 512 frames (the frame operand formed ahead serves only such ranges);
  - the segments come in the order of the launches they wait for (the executor issues them in one pass).

and per rule: the remainder is first in time and alone, no release behind a launch that another one follows exceeds
`share` of a chunk, what is left goes behind the last launch."""
import ctypes

import numpy as np
import pytest

SHARES = [0.6, 0.7, 0.8, 0.9, 1.0]
CAP = 4096


@pytest.fixture(scope="module")
def plan():
    from aaltoasr_amd import capi
    L = capi.lib()
    i64, p64 = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.aasr_debug_score_lna_plan.argtypes = [i64, ctypes.c_int, i64, ctypes.c_int, ctypes.c_double, ctypes.c_int, p64, p64, i64,
                                            p64, p64]
    L.aasr_debug_score_lna_plan.restype = i64

    def call(F, cus, chunk_frames, remainder_first=-1, share=-1.0, chunk_div=-1):
        score = np.zeros((CAP, 2), dtype=np.int64)
        lna = np.zeros((CAP, 3), dtype=np.int64)
        ns, nl = i64(0), i64(0)
        chunk = L.aasr_debug_score_lna_plan(F, cus, chunk_frames, remainder_first, share, chunk_div,
                                            score.ctypes.data_as(p64), lna.ctypes.data_as(p64), CAP,
                                            ctypes.byref(ns), ctypes.byref(nl))
        assert 0 <= ns.value <= CAP and 0 <= nl.value <= CAP
        return chunk, score[:ns.value], lna[:nl.value]

    return call


def _check_invariants(F, chunk, score, lna):
    launch_of = np.full(F, -1, dtype=np.int32)
    for i, (f0, n) in enumerate(score):
        assert n > 0 and 0 <= f0 and f0 + n <= F
        assert f0 % 512 == 0, (i, f0)
        assert (launch_of[f0:f0 + n] == -1).all(), "frames scored twice"
        launch_of[f0:f0 + n] = i
    assert (launch_of >= 0).all(), "frames never scored"
    encoded = np.zeros(F, dtype=np.int8)
    for f0, n, wait in lna:
        assert n > 0 and 0 <= f0 and f0 + n <= F and 0 <= wait < len(score)
        encoded[f0:f0 + n] += 1
        assert int(launch_of[f0:f0 + n].max()) <= wait, (f0, n, wait)
    assert (encoded == 1).all(), "frames encoded %s times" % sorted(set(encoded.tolist()))
    assert (np.diff(lna[:, 2]) >= 0).all(), "segments out of the order of their launches"
    assert chunk % 512 == 0


def _check_rules(F, chunk, score, lna, remainder_first, share):
    whole, rem = divmod(F, chunk)
    assert len(score) == whole + (1 if rem else 0)
    if rem:
        at = 0 if remainder_first else len(score) - 1
        assert tuple(score[at]) == (whole * chunk, rem)
    wholes = score[1:] if rem and remainder_first else score[:whole]
    assert [tuple(s) for s in wholes] == [(c * chunk, chunk) for c in range(whole)]
    last = len(score) - 1
    budget = max(1, int(share * chunk))
    released = np.zeros(len(score), dtype=np.int64)
    for _f0, n, wait in lna:
        released[wait] += n
    assert (released[:last] <= budget).all(), (released, budget)
    # nothing is held back that the budget allows: behind launch i the frames scored so far, less what went before, up to the budget
    scored = np.cumsum(score[:, 1])
    before = 0
    for i in range(last):
        assert released[i] == min(budget, scored[i] - before), (i, released, budget)
        before += released[i]
    assert released[last] == F - before


def _rounds(cus):
    return cus * 512


@pytest.mark.parametrize("chunk_div", [1, 2], ids=["chunk256", "chunk128"])
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("cus", [256, 64])
@pytest.mark.parametrize("which", ["headline", "two_rounds", "two_rounds_plus_1", "three_rounds_plus_517", "seven_rounds_plus_511"])
def test_automatic_plan(plan, which, cus, share, chunk_div):
    r = _rounds(cus)
    F = {"headline": 449280, "two_rounds": 2 * r, "two_rounds_plus_1": 2 * r + 1, "three_rounds_plus_517": 3 * r + 517,
         "seven_rounds_plus_511": 7 * r + 511}[which]
    chunk, score, lna = plan(F, cus, 0, 1, share, chunk_div)
    assert F >= 2 * r and chunk == r // chunk_div      # (the headline is 3.4 rounds of 256 CUs)
    _check_invariants(F, chunk, score, lna)
    _check_rules(F, chunk, score, lna, True, share)
    # remainder last as well: the parent's order with this share
    chunk2, score2, lna2 = plan(F, cus, 0, 0, share, chunk_div)
    assert chunk2 == chunk
    _check_invariants(F, chunk, score2, lna2)
    _check_rules(F, chunk, score2, lna2, False, share)


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("remainder_first", [1, 0])
@pytest.mark.parametrize("extra", [0, 3, 511])
def test_explicit_chunk_of_512_with_20_chunks(plan, extra, remainder_first, share):
    F = 20 * 512 + extra
    chunk, score, lna = plan(F, 256, 512, remainder_first, share)
    assert chunk == 512 and len(score) == 20 + (1 if extra else 0)
    _check_invariants(F, chunk, score, lna)
    _check_rules(F, chunk, score, lna, bool(remainder_first), share)


def test_headline_plan_as_compiled_in(plan):
    """The default knobs on the bench.py step: the 110 fine-cut blocks [393 216, 449 280) first, then whole chunks from
    frame 0; the first segment is the remainder's, beside the first whole chunk."""
    F = 449280
    chunk, score, lna = plan(F, 256, 0)
    assert chunk in (131072, 65536)
    _check_invariants(F, chunk, score, lna)
    assert tuple(score[0]) == (393216, 56064) and tuple(score[1]) == (0, chunk)
    assert tuple(lna[0]) == (393216, 56064, 0)
    assert int(lna[-1][2]) == len(score) - 1


def test_share_one_remainder_last_is_the_parent_schedule(plan):
    F, chunk = 3 * 8192 + 517, 8192
    got, score, lna = plan(F, 256, chunk, 0, 1.0)
    assert got == chunk
    want = [(0, chunk), (chunk, chunk), (2 * chunk, chunk), (3 * chunk, 517)]
    assert [tuple(s) for s in score] == want
    assert [tuple(l) for l in lna] == [(f0, n, i) for i, (f0, n) in enumerate(want)]


def test_plain_sequence_and_refusals(plan):
    assert plan(8191, 256, 0)[0] == 0
    assert plan(8192, 256, 8192)[0] == 0            # one chunk exactly: nothing to overlap
    chunk, score, lna = plan(1000, 256, 8192)
    assert chunk == 0 and [tuple(s) for s in score] == [(0, 1000)] and [tuple(l) for l in lna] == [(0, 1000, 0)]
    assert plan(0, 256, 0)[0] == 0 and len(plan(0, 256, 0)[1]) == 0
    for bad in (100, 513, -512):
        assert plan(20000, 256, bad)[0] == -1
    assert plan(20000, 256, 512, 1, 1.5)[0] == -1    # knobs out of range
    assert plan(20000, 256, 512, 1, 0.7, 0)[0] == -1

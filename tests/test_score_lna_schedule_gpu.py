"""The schedule of aasr_gmm_score_lna_pitched_dev (csrc/gmm_score_lna.cc: plan_score_lna and its executor) on the device:
the remainder scored first, LNA releases held to a share of a chunk, the rest behind the last scoring launch, other LNA
grids.  The rule is that of tests/test_score_lna_chunked_gpu.py -- d_scores (padding included) and d_bytes equal the bit
patterns the two-call sequence aasr_gmm_score_dev_pitched + aasr_lna_encode_dev_pitched leaves, no tolerance anywhere --
and so is the model: 77 states of 4 components in 39 dimensions, rows padded to 96 floats.

The knobs are set through aasr_debug_score_lna_knobs (process-wide, restored after every test); what a setting makes of a
call is read back through aasr_debug_score_lna_plan, so that every case is seen to exercise what it is named for."""
import ctypes
import faulthandler

import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu

S, COMPS, PITCH = 77, 4, 96
CHUNK = 8192
FILL = -7.0
SHARE70 = int(0.7 * CHUNK)     # 5734: where the first release of a whole chunk ends at share 0.7 -- no scoring boundary
F_RAGGED = 2 * CHUNK + 517
F_LONG = 3 * CHUNK + 517
TIME_LIMIT_S = 120             # per test: a step that hangs ends the run with a traceback instead of waiting for ever

# name -> (frames, chunk_frames, remainder_first, share in percent, LNA workgroups per CU)
CASES = {
    "remainder_first_ragged": (F_RAGGED, CHUNK, 1, 70, -1),     # remainder of 517 frames: 4-wave form, a partial block
    "exact_multiple_no_remainder": (2 * CHUNK, CHUNK, 1, 70, -1),
    "share_60_final_pass_spans_launches": (F_LONG, CHUNK, 1, 60, -1),
    "small_chunks_more_launches_than_events": (9 * 512 + 3, 512, 1, 70, -1),
    "remainder_last_share_90_grid_128": (F_RAGGED, CHUNK, 0, 90, 128),
    "share_100_grid_64": (F_LONG, CHUNK, 1, 100, 64),
}


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def dbg(capi):
    L = capi.lib()
    i64, p64 = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.aasr_debug_score_lna_plan.argtypes = [i64, ctypes.c_int, i64, ctypes.c_int, ctypes.c_double, ctypes.c_int, p64, p64, i64,
                                            p64, p64]
    L.aasr_debug_score_lna_plan.restype = i64
    L.aasr_debug_score_lna_knobs.argtypes = [ctypes.c_int] * 4
    L.aasr_debug_score_lna_knobs.restype = None

    def plan(F, cus, chunk_frames):
        """the plan under the knobs in force"""
        cap = 256
        score = np.zeros((cap, 2), dtype=np.int64)
        lna = np.zeros((cap, 3), dtype=np.int64)
        ns, nl = i64(0), i64(0)
        chunk = L.aasr_debug_score_lna_plan(F, cus, chunk_frames, -1, -1.0, -1, score.ctypes.data_as(p64),
                                            lna.ctypes.data_as(p64), cap, ctypes.byref(ns), ctypes.byref(nl))
        assert ns.value <= cap and nl.value <= cap
        return chunk, score[:ns.value], lna[:nl.value]

    return L.aasr_debug_score_lna_knobs, plan


@pytest.fixture
def knobs(dbg):
    setter, _plan = dbg
    yield setter
    setter(-1, -1, -1, -1)


@pytest.fixture(scope="module")
def world(capi):
    import torch
    model = synth.make_model(D=39, G=S * COMPS, S=S, comps=COMPS, seed=21)
    g = capi.Gmm.from_arrays(*model)
    assert g.effective_precision() == 4 and g.score_pitch_ok()
    frames = synth.make_frames(F_LONG, seed=77)
    # frames of the exact path of lna_row_from_registers, as tests/test_score_lna_chunked_gpu.py finds them: every state at
    # the 1e-50 floor, and one whose best state lies between the floor and e^-51
    scale = np.concatenate([np.linspace(1.0, 3.0, 48), np.full(16, 40.0)]).astype(np.float32)
    cand = synth.make_frames(64, seed=5) * scale[:, None]
    ll = g.score(cand)
    floor = float(np.float32(np.log(1e-50)))
    at_floor = np.flatnonzero((ll <= np.float32(floor)).all(axis=1))
    low = np.flatnonzero((ll.max(axis=1) < -51.0) & (ll.max(axis=1) > np.float32(floor)))
    assert len(at_floor) >= 4 and len(low) >= 1, (len(at_floor), len(low))
    # ... on both sides of the segment boundary at SHARE70, and of the one between the remainder and the last whole chunk
    floor_at = (SHARE70 - 1, SHARE70, 2 * CHUNK - 1, 2 * CHUNK)
    low_at = (SHARE70 - 2, SHARE70 + 1)
    for k, pos in enumerate(floor_at):
        frames[pos] = cand[at_floor[k]]
    for pos in low_at:
        frames[pos] = cand[low[0]]
    d_frames = torch.from_numpy(frames).cuda()
    refs = {}

    def reference(F, normalize, lnabytes, gmm=g, fr=d_frames, tag="default"):
        """the two-call sequence, once per (model tag, F, normalize, lnabytes); never written to afterwards"""
        key = (tag, F, normalize, lnabytes)
        if key not in refs:
            sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
            by = torch.full((F, S * lnabytes), 0xA5, dtype=torch.uint8, device="cuda")
            gmm.score_dev_pitched(fr[:F], sc, PITCH)
            capi.lna_encode_dev(sc, bool(normalize), lnabytes, None, by, num_states=S)
            torch.cuda.synchronize()
            refs[key] = (sc, by)
        return refs[key]

    yield {"g": g, "model": model, "frames": d_frames, "reference": reference, "floor_at": floor_at, "low_at": low_at,
           "low_ll": float(ll[low[0]].max()), "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    g.close()


def _run(g, d_frames, F, chunk, normalize, lnabytes):
    import torch
    sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
    by = torch.full((F, S * lnabytes), 0xA5, dtype=torch.uint8, device="cuda")
    g.score_lna_dev_pitched(d_frames[:F], sc, PITCH, by, bool(normalize), lnabytes, chunk)
    torch.cuda.synchronize()
    return sc, by


def _same(a, b):
    import torch
    # bit patterns, not values: no float comparison rule (NaN, -0) enters
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check_named_property(name, F, chunk, score, lna):
    """the plan in force does what the case is named for"""
    if name == "remainder_first_ragged":
        assert [tuple(s) for s in score] == [(2 * CHUNK, 517), (0, CHUNK), (CHUNK, CHUNK)]
        assert [tuple(l) for l in lna] == [(2 * CHUNK, 517, 0), (0, SHARE70, 1), (SHARE70, 2 * CHUNK - SHARE70, 2)]
    elif name == "exact_multiple_no_remainder":
        assert [tuple(s) for s in score] == [(0, CHUNK), (CHUNK, CHUNK)]
        assert [tuple(l) for l in lna] == [(0, SHARE70, 0), (SHARE70, 2 * CHUNK - SHARE70, 1)]
    elif name == "share_60_final_pass_spans_launches":
        last = [l for l in lna if l[2] == len(score) - 1]
        assert len(last) == 1
        f0, n, _w = last[0]
        assert CHUNK < f0 < 2 * CHUNK < f0 + n == 3 * CHUNK      # frames of the second and of the third whole chunk
    elif name == "small_chunks_more_launches_than_events":
        assert len(score) == 10 > 8 and tuple(score[0]) == (9 * 512, 3)
    elif name == "remainder_last_share_90_grid_128":
        assert tuple(score[-1]) == (2 * CHUNK, 517)
        assert tuple(lna[-1])[1:] == (2 * CHUNK + 517 - 2 * int(0.9 * CHUNK), 2)
    elif name == "share_100_grid_64":
        assert [tuple(l)[:2] for l in lna] == [tuple(s) for s in score]


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("lnabytes", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_scheduled_call_equals_the_two_call_sequence(dbg, knobs, world, name, lnabytes, normalize):
    F, chunk, rem_first, share, grid = CASES[name]
    knobs(rem_first, share, -1, grid)
    got_chunk, score, lna = dbg[1](F, world["cus"], chunk)
    assert got_chunk == chunk
    _check_named_property(name, F, chunk, score, lna)
    g = world["g"]
    assert g.score_lna_overlap_active(F, PITCH, chunk)
    ref_sc, ref_by = world["reference"](F, normalize, lnabytes)
    sc, by = _run(g, world["frames"], F, chunk, normalize, lnabytes)
    assert _same(sc, ref_sc)          # padding columns included: still FILL
    assert _same(by, ref_by)


def test_planted_frames_straddle_a_segment_boundary_that_is_no_scoring_boundary(dbg, knobs, world):
    """What the fixture planted is what it says, and where: at share 0.7 the release behind the first whole chunk ends at
    frame SHARE70, inside a scoring launch, with floor frames on either side and the low-maximum frame next to each."""
    knobs(1, 70, -1, -1)
    _chunk, score, lna = dbg[1](F_RAGGED, world["cus"], CHUNK)
    ends = {int(f0 + n) for f0, n, _w in lna}
    assert SHARE70 in ends and all(SHARE70 != f0 and SHARE70 != f0 + n for f0, n in score)
    assert world["low_ll"] < -51.0
    _sc, by = world["reference"](F_RAGGED, 0, 2)
    for pos in world["floor_at"]:
        assert bool((by[pos] == 0xFF).all()), pos
    _sc, by_n = world["reference"](F_RAGGED, 1, 2)
    for pos in world["low_at"]:
        assert not bool((by_n[pos] == 0xFF).all()), pos      # normalised, the low frame's best state has a real code


@pytest.mark.parametrize("precision", [0, 3], ids=["f32", "bf16x3"])
def test_other_arithmetics(capi, dbg, knobs, world, precision):
    """No frame operand formed ahead (f32 rows) and the three-term operand layout: remainder first, share 0.7."""
    g = capi.Gmm.from_arrays(*world["model"])
    try:
        g.set_precision(precision)
        assert g.score_pitch_ok()
        knobs(1, 70, -1, -1)
        assert g.score_lna_overlap_active(F_RAGGED, PITCH, CHUNK)
        ref_sc, ref_by = world["reference"](F_RAGGED, 1, 2, gmm=g, tag="precision %d" % precision)
        sc, by = _run(g, world["frames"], F_RAGGED, CHUNK, 1, 2)
        assert _same(sc, ref_sc) and _same(by, ref_by)
    finally:
        g.close()


@pytest.mark.parametrize("chunk_div", [1, 2], ids=["chunk_of_a_round", "chunk_of_half_a_round"])
def test_automatic_chunk(capi, dbg, knobs, world, chunk_div):
    """chunk_frames = 0 on two rounds of this device and a ragged remainder, the other knobs as compiled in: the path
    FullChainBench.step takes."""
    import torch
    cus = world["cus"]
    F = 2 * cus * 512 + 517
    knobs(-1, -1, chunk_div, -1)
    chunk, score, lna = dbg[1](F, cus, 0)
    assert chunk == cus * 512 // chunk_div // 512 * 512 and len(score) == 2 * chunk_div + 1
    g = world["g"]
    assert g.score_lna_overlap_active(F, PITCH, 0)
    reps = (F + F_LONG - 1) // F_LONG
    fr = world["frames"].repeat(reps, 1)[:F].contiguous()
    ref_sc, ref_by = world["reference"](F, 1, 2, fr=fr, tag="automatic")
    sc, by = _run(g, fr, F, 0, 1, 2)
    assert _same(sc, ref_sc) and _same(by, ref_by)


def test_back_to_back_calls_under_a_held_back_share(knobs, world):
    """Three calls with no host synchronisation between them into the same buffers (inputs A, B, A): the final pass of a
    call, which encodes frames of several launches, is ordered before the next call's scoring of the same rows."""
    import torch
    knobs(1, 60, -1, -1)
    g = world["g"]
    a = world["frames"][:F_LONG]
    b = torch.flip(a, dims=[0]).contiguous()
    sc = torch.full((F_LONG, PITCH), FILL, dtype=torch.float32, device="cuda")
    by = torch.full((F_LONG, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
    for fr in (a, b, a):
        g.score_lna_dev_pitched(fr, sc, PITCH, by, True, 2, CHUNK)
    got_sc, got_by = sc.clone(), by.clone()      # on the caller's stream: ordered behind the last LNA pass
    torch.cuda.synchronize()
    ref_sc, ref_by = world["reference"](F_LONG, 1, 2)
    assert _same(got_sc, ref_sc) and _same(got_by, ref_by)

"""aasr_gmm_score_lna_pitched_dev: scoring in frame chunks with the LNA pass of a chunk on the handle's side stream beside
the scoring of the next chunk.  The contract is the two-call sequence's result, byte for byte: d_scores (padding included)
and d_bytes after the call equal what aasr_gmm_score_dev_pitched + aasr_lna_encode_dev_pitched leave there.  No tolerance
anywhere in this file.

The model has 77 states -- an odd number, so the 2-byte rows start on odd halfwords every other frame -- of 4 components
in 39 dimensions; rows are padded to 96 floats."""
import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu

S, COMPS, PITCH = 77, 4, 96
CHUNK = 8192          # the smallest chunk the 8-wave form of the scoring kernel takes
FILL = -7.0

# (name, frames, chunk_frames, two-stream form expected)
CASES = [
    ("three_chunks_and_ragged_tail", 3 * CHUNK + 517, CHUNK, True),   # tail of 517 frames: 4-wave form, a partial block
    ("exact_chunk_multiple", 2 * CHUNK, CHUNK, True),
    ("auto_below_two_rounds", 8191, 0, False),                         # automatic choice: sequential fallback
    ("one_chunk_exactly", CHUNK, CHUNK, False),
    ("one_chunk_short", 1000, CHUNK, False),
    ("small_chunks", 9 * 512 + 3, 512, True),                         # every chunk on the 4-wave form, more chunks than events
]


@pytest.fixture(scope="module")
def world(capi):
    import torch
    model = synth.make_model(D=39, G=S * COMPS, S=S, comps=COMPS, seed=21)
    g = capi.Gmm.from_arrays(*model)
    assert g.effective_precision() == 4 and g.score_pitch_ok()
    fmax = max(c[1] for c in CASES)
    frames = synth.make_frames(fmax, seed=77)
    # frames of the exact path of lna_row_from_registers: far from every Gaussian (all states at the 1e-50 floor), and one
    # whose best state lies between the floor and e^-51; found by scoring candidates at growing distance
    scale = np.concatenate([np.linspace(1.0, 3.0, 48), np.full(16, 40.0)]).astype(np.float32)
    cand = synth.make_frames(64, seed=5) * scale[:, None]
    ll = g.score(cand)
    floor = float(np.float32(np.log(1e-50)))
    at_floor = np.flatnonzero((ll <= np.float32(floor)).all(axis=1))
    low = np.flatnonzero((ll.max(axis=1) < -51.0) & (ll.max(axis=1) > np.float32(floor)))
    assert len(at_floor) >= 5 and len(low) >= 1, (len(at_floor), len(low), ll.max(axis=1))
    # ... placed at the start, around a chunk boundary and in the ragged tail
    for k, pos in enumerate((0, 1, CHUNK - 1, CHUNK, 3 * CHUNK + 516)):
        frames[pos] = cand[at_floor[k]]
    frames[CHUNK + 1] = cand[low[0]]
    frames[700] = cand[low[0]]
    d_frames = torch.from_numpy(frames).cuda()
    refs = {}

    def reference(F, normalize, lnabytes, gmm=g, fr=d_frames, tag="default"):
        """the two-call sequence, once per (model tag, F, normalize, lnabytes)"""
        key = (tag, F, normalize, lnabytes)
        if key not in refs:
            sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
            by = torch.full((F, S * lnabytes), 0xA5, dtype=torch.uint8, device="cuda")
            gmm.score_dev_pitched(fr[:F], sc, PITCH)
            capi.lna_encode_dev(sc, bool(normalize), lnabytes, None, by, num_states=S)
            torch.cuda.synchronize()
            refs[key] = (sc, by)
        return refs[key]

    yield {"g": g, "model": model, "frames": d_frames, "reference": reference, "special": (at_floor, low, cand, ll)}
    g.close()


def _run(capi, g, d_frames, F, chunk, normalize, lnabytes):
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


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("lnabytes", [2, 4])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chunked_call_equals_the_two_call_sequence(capi, world, case, lnabytes, normalize):
    _name, F, chunk, overlapped = case
    g = world["g"]
    assert g.score_lna_overlap_active(F, PITCH, chunk) == overlapped
    ref_sc, ref_by = world["reference"](F, normalize, lnabytes)
    sc, by = _run(capi, g, world["frames"], F, chunk, normalize, lnabytes)
    assert _same(sc, ref_sc)          # padding columns included: still FILL
    assert _same(by, ref_by)


@pytest.mark.parametrize("precision", [0, 3], ids=["f32", "bf16x3"])
def test_other_arithmetics_overlap_and_match(capi, world, precision):
    """The f32 track kernel (no frame operand: its chunks' LNA passes wait for the scores alone) and the three-term kernel
    (its own operand layout) take the two-stream form too."""
    import torch
    g = capi.Gmm.from_arrays(*world["model"])
    try:
        g.set_precision(precision)
        assert g.score_pitch_ok()
        F = 3 * CHUNK + 517
        assert g.score_lna_overlap_active(F, PITCH, CHUNK)
        ref_sc, ref_by = world["reference"](F, 1, 2, gmm=g, tag="precision %d" % precision)
        sc, by = _run(capi, g, world["frames"], F, CHUNK, 1, 2)
        assert _same(sc, ref_sc) and _same(by, ref_by)
    finally:
        g.close()


@pytest.mark.parametrize("precision", [3, 4], ids=["bf16x3", "f16x2"])
def test_more_than_five_slabs(capi, precision):
    """44 dimensions are six K slabs: three terms then run on the wave-group kernel, which forms its operand itself (one
    launch per chunk, nothing formed in front), two terms on the pipelined kernel with the operand of all chunks formed in
    front.  Both take the two-stream form, say so, and give the two-call sequence's bytes."""
    import torch
    D = 44
    g = capi.Gmm.from_arrays(*synth.make_model(D=D, G=S * COMPS, S=S, comps=COMPS, seed=23))
    try:
        g.set_precision(precision)
        assert g.score_pitch_ok()
        F = 2 * CHUNK + 517
        fr = torch.from_numpy(synth.make_frames(F, D=D, seed=78)).cuda()
        assert g.score_lna_overlap_active(F, PITCH, CHUNK)
        ref_sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
        ref_by = torch.full((F, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
        g.score_dev_pitched(fr, ref_sc, PITCH)
        capi.lna_encode_dev(ref_sc, True, 2, None, ref_by, num_states=S)
        torch.cuda.synchronize()
        sc, by = _run(capi, g, fr, F, CHUNK, 1, 2)
        assert _same(sc, ref_sc) and _same(by, ref_by)
    finally:
        g.close()


def test_special_frames_take_the_exact_path(world):
    """What the fixture planted is what it says: frames with every state at the floor encode FF FF in every state without
    normalisation, and the low frame's best state is under e^-51 but over the floor."""
    import torch
    at_floor, low, _cand, ll = world["special"]
    assert float(ll[low[0]].max()) < -51.0
    _sc, by = world["reference"](3 * CHUNK + 517, 0, 2)
    for pos in (0, 1, CHUNK - 1, CHUNK, 3 * CHUNK + 516):
        assert bool((by[pos] == 0xFF).all()), pos
    _sc, by_n = world["reference"](3 * CHUNK + 517, 1, 2)
    assert not bool((by_n[CHUNK + 1] == 0xFF).all())      # normalised, the low frame's best state has a real code


def test_empty_input_is_a_no_op(capi, world):
    import torch
    g = world["g"]
    sc = torch.full((4, PITCH), FILL, dtype=torch.float32, device="cuda")
    by = torch.full((4, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
    for chunk in (0, CHUNK):
        g.score_lna_dev_pitched(world["frames"][:0], sc[:0], PITCH, by[:0], True, 2, chunk)
        assert not g.score_lna_overlap_active(0, PITCH, chunk)
    torch.cuda.synchronize()
    assert bool((sc == FILL).all()) and bool((by == 0xA5).all())


def test_back_to_back_calls_reuse_the_side_stream(capi, world):
    """Three calls with no host synchronisation between them into the same buffers (inputs A, B, A: a pass that ran early
    or late would leave B's bytes or scores behind), then a call with another frame count."""
    import torch
    g = world["g"]
    F = 3 * CHUNK + 517
    a = world["frames"][:F]
    b = torch.flip(a, dims=[0]).contiguous()
    sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
    by = torch.full((F, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
    for fr in (a, b, a):
        g.score_lna_dev_pitched(fr, sc, PITCH, by, True, 2, CHUNK)
    got_sc, got_by = sc.clone(), by.clone()      # on the caller's stream: ordered behind the last LNA pass
    torch.cuda.synchronize()
    ref_sc, ref_by = world["reference"](F, 1, 2)
    assert _same(got_sc, ref_sc) and _same(got_by, ref_by)
    F2 = 2 * CHUNK + 1
    ref_sc, ref_by = world["reference"](F2, 1, 2)
    g.score_lna_dev_pitched(a[:F2], sc[:F2], PITCH, by[:F2], True, 2, CHUNK)
    got_sc, got_by = sc[:F2].clone(), by[:F2].clone()
    torch.cuda.synchronize()
    assert _same(got_sc, ref_sc) and _same(got_by, ref_by)


def test_routed_model_runs_the_plain_sequence(capi, world):
    """States over the fp16 form's limits: engine parts and a column map, so no overlap -- and the same bytes."""
    import torch
    routed = synth.push_states_over_the_f16_limits(world["model"], [3, 17, 18])
    gr = capi.Gmm.from_arrays(*routed)
    try:
        assert gr.effective_precision() == 4 and gr.precision_states()[0] == S - 3
        F = 2 * CHUNK + 100
        assert not gr.score_lna_overlap_active(F, PITCH, CHUNK)
        assert not gr.score_lna_overlap_active(F, PITCH, 0)
        ref_sc, ref_by = world["reference"](F, 1, 2, gmm=gr, tag="routed")
        sc, by = _run(capi, gr, world["frames"], F, CHUNK, 1, 2)
        assert _same(sc, ref_sc) and _same(by, ref_by)
    finally:
        gr.close()


@pytest.mark.parametrize("bad", [100, 513, -512, 8191])
def test_bad_chunk_frames_is_invalid(capi, world, bad):
    import torch
    g = world["g"]
    F = 2 * CHUNK
    sc = torch.full((F, PITCH), FILL, dtype=torch.float32, device="cuda")
    by = torch.full((F, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(capi.AasrError) as e:
        g.score_lna_dev_pitched(world["frames"][:F], sc, PITCH, by, True, 2, bad)
    assert e.value.code == capi.AASR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((sc == FILL).all()) and bool((by == 0xA5).all())      # nothing was launched

"""The multi-frame LNA kernel (csrc/lna_encode.hip: k_state_norm_lna_multi, Q frame rows per workgroup pass) against the
one-frame kernel k_state_norm_lna_reg on the same inputs, byte for byte.  Which of them a production call (2-byte codes, no
float output, no column map, S in the <13> range) runs is set through aasr_debug_lna_frames_per_pass: 1 the old kernel,
2 and 4 the two instances of the new one.  No tolerance anywhere: the new kernel keeps every rounding step of the old one.

Rows come from tools/lna_cases.py and are laid out so that passes made of fast-path frames only, passes that mix fast
frames with frames the fast path's test refuses (a best state below -51, a row at the floor, a row of -inf, a row inside
the float-denormal band), and a pass of refused frames only all occur for Q = 2 and Q = 4.  Every output buffer lies
between guard bytes that are checked after each call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lna_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256
SEED = 23
SIZES = [2561, 3125, 3328]            # both ends of the <13> instance, and the headline's state count
PADDED = 3136                         # the headline's row pitch (3328 rows: the next multiple of 64)
BASE_FRAMES = 37
# frame -> kind of row.  F: fast path; the others fail its test.  Groups of four: 0-3 fast, 4-7 fast, 8-11 mixed (one
# refused frame), 12-15 fast, 16-19 mixed (two), 20-23 fast, 24-27 all refused, 28-31 fast, 32-35 mixed, 36 the short group
LAYOUT = (["plain", "band_fast", "gt1", "edge_hi", "one_hot", "flat", "plain", "band_fast"] +
          ["edge_lo", "gt1", "edge_hi", "one_hot"] +
          ["flat", "plain", "band_fast", "gt1"] +
          ["all_floor", "band_mid", "edge_hi", "one_hot"] +
          ["flat", "plain", "band_fast", "gt1"] +
          ["band_max", "all_ninf", "edge_lo", "all_floor"] +
          ["edge_hi", "one_hot", "flat", "plain"] +
          ["band_fast", "all_ninf", "gt1", "edge_hi"] +
          ["band_mid"])
assert len(LAYOUT) == BASE_FRAMES
FRAME_COUNTS = [1, 2, 3, 4, 5, 9, 37]   # 1, Q - 1, Q, Q + 1, 2 Q + 1 for Q = 2 and Q = 4, and 37
OFFSETS = [0, 7]                        # from frame 7 on even the shortest calls hold a refused frame beside a fast one

_BASE = {}


def _base(S):
    """[37 x S] rows in LAYOUT's order, read-only"""
    if S not in _BASE:
        pool, labels = LC.rows(S, SEED, frames=8 * len(LC.KINDS))
        by_kind = {}
        for row, kind in zip(pool, labels):
            by_kind.setdefault(kind, []).append(row)
        used = dict.fromkeys(by_kind, 0)
        ll = np.empty((BASE_FRAMES, S), np.float32)
        for r, kind in enumerate(LAYOUT):
            ll[r] = by_kind[kind][used[kind]]
            used[kind] += 1
        isfast = np.array([LC.fast(r) for r in ll])
        for g in range(0, 36, 4):       # what the layout's comment says of the groups of four
            want = {0: 4, 4: 4, 8: 3, 12: 4, 16: 2, 20: 4, 24: 0, 28: 4, 32: 3}[g]
            assert isfast[g:g + 4].sum() == want, (g, isfast[g:g + 4])
        assert not isfast[36]
        ll.setflags(write=False)
        _BASE[S] = ll
    return _BASE[S]


def _encode(capi, ll, S, normalize, q, wgs=None):
    """aasr_lna_encode_dev on rows ll [F x pitch] (S <= pitch) with Q = q; the bytes [F x 2 S], guards checked"""
    import torch
    F, pitch = ll.shape
    nbytes = F * S * 2
    d_in = torch.from_numpy(np.array(ll, dtype=np.float32, order="C", copy=True)).cuda()
    raw = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    body = raw[GUARD:GUARD + nbytes]
    capi.debug_lna_frames_per_pass(q)
    try:
        capi.lna_encode_dev(d_in, bool(normalize), 2, None, body, num_states=S, wgs_per_cu=wgs)
        torch.cuda.synchronize()
    finally:
        capi.debug_lna_frames_per_pass(-1)
    got = raw.cpu().numpy()
    what = "F=%d S=%d pitch=%d normalize=%d Q=%d wgs=%s" % (F, S, pitch, normalize, q, wgs)
    assert (got[:GUARD] == 0xA5).all(), what + ": bytes in front of the output were written"
    assert (got[GUARD + nbytes:] == 0xA5).all(), what + ": bytes behind the output were written"
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), ll.view(np.uint32)), what + ": the input was written"
    return got[GUARD:GUARD + nbytes].reshape(F, 2 * S)


def _pitched(ll, pitch):
    F, S = ll.shape
    if pitch == S:
        return np.ascontiguousarray(ll)
    out = np.full((F, pitch), 50.0, np.float32)      # one read of a padding column wrecks Z
    out[:, :S] = ll
    return out


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "pitch3136"])
@pytest.mark.parametrize("S", SIZES)
def test_bytes_equal_the_one_frame_kernel(capi, S, padded, normalize):
    if padded and S > PADDED:
        pitch = S + 64                 # 3328 does not fit a pitch of 3136: the same distance past its own end
    else:
        pitch = PADDED if padded else S
    base = _base(S)
    seen_ffff = seen_code = False
    for off in OFFSETS:
        for F in FRAME_COUNTS:
            if off + F > BASE_FRAMES:
                continue
            ll = _pitched(base[off:off + F], pitch)
            one = _encode(capi, ll, S, normalize, 1)
            assert not (one == 0xA5).all(axis=1).any()          # every row was written
            for q in (2, 4):
                got = _encode(capi, ll, S, normalize, q)
                bad = np.flatnonzero((got != one).any(axis=1))
                assert bad.size == 0, (S, pitch, normalize, off, F, q, bad[:8], [LAYOUT[off + b] for b in bad[:8]])
            codes = LC.codes(one, S)
            seen_ffff |= bool((codes == 0xFFFF).any())
            seen_code |= bool((codes != 0xFFFF).any())
            if F == BASE_FRAMES and normalize:
                # codes on either side of FF FF inside one fast-path row, next to one another
                row = codes[LAYOUT.index("plain")]
                assert (row == 0xFFFF).sum() > 100 and (row < 0xFFFF).sum() > 100
                edge = (-36.008 * -1820.0)
                assert ((row > edge - 2000) & (row < 0xFFFF)).any()      # visible codes within a nat of the switch
    assert seen_ffff and seen_code


@pytest.mark.parametrize("S", SIZES)
def test_several_passes_per_workgroup_and_a_short_last_group(capi, S):
    """One workgroup per CU and a little over two groups per workgroup: every workgroup walks two or three passes with its
    rows requested a pass ahead, passes of both kinds follow one another, and the last group holds one frame."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    base = _base(S)
    F = 2 * 4 * cus + 5                 # Q = 4: 2 cus + 2 groups, the last of one frame; Q = 2: 4 cus + 3, likewise
    reps = (F + BASE_FRAMES - 1) // BASE_FRAMES
    ll = np.tile(base, (reps, 1))[:F]   # period 37 against groups of 2 and 4: every alignment of the layout occurs
    ll = _pitched(ll, PADDED if S <= PADDED else S)
    one = _encode(capi, ll, S, 1, 1, wgs=1)
    for q in (2, 4):
        got = _encode(capi, ll, S, 1, q, wgs=1)
        bad = np.flatnonzero((got != one).any(axis=1))
        assert bad.size == 0, (S, q, bad[:8])
    # ... and the default grid gives the same bytes
    assert np.array_equal(_encode(capi, ll, S, 1, 4), one)


def test_chunked_score_lna_call(capi):
    """The route of tests/test_score_lna_schedule_gpu.py -- aasr_gmm_score_lna_pitched_dev with an explicit small
    chunk_frames -- on a model of the headline's state count: the LNA segments beside the scoring launches and the last
    pass give the same bytes with Q = 1, 2 and 4."""
    import torch
    from aaltoasr_amd import synth
    S, comps, pitch, chunk = 3125, 2, 3136, 512
    F = 3 * chunk + 37
    model = synth.make_model(D=39, G=S * comps, S=S, comps=comps, seed=21)
    g = capi.Gmm.from_arrays(*model)
    try:
        assert g.score_pitch_ok()
        assert g.score_lna_overlap_active(F, pitch, chunk)
        frames = synth.make_frames(F, seed=77)
        frames[5] *= 40.0               # far from every Gaussian: a frame off the fast path
        frames[chunk + 3] *= 40.0
        d_frames = torch.from_numpy(frames).cuda()
        out = {}
        for q in (1, 2, 4):
            sc = torch.full((F, pitch), -7.0, dtype=torch.float32, device="cuda")
            by = torch.full((F, S * 2), 0xA5, dtype=torch.uint8, device="cuda")
            capi.debug_lna_frames_per_pass(q)
            try:
                g.score_lna_dev_pitched(d_frames, sc, pitch, by, True, 2, chunk)
                torch.cuda.synchronize()
            finally:
                capi.debug_lna_frames_per_pass(-1)
            out[q] = (sc.cpu().numpy(), by.cpu().numpy())
        ll = out[1][0][:, :S]
        assert (ll.max(axis=1) < -51.0).any() and (ll.max(axis=1) >= -51.0).sum() > F // 2
        for q in (2, 4):
            assert np.array_equal(out[q][0].view(np.uint32), out[1][0].view(np.uint32)), q
            assert np.array_equal(out[q][1], out[1][1]), q
    finally:
        g.close()

"""aasr_fb_batch_frame_entries_dev (csrc/fb_frame_entries.hip): the forward-backward pass's occupancies as weighted
entries grouped by frame, against the pdf-major entries of aasr_fb_batch_entries_dev on the same batch and against
tools/mllr_bw_restate.py.

The fixture is the `world` of tests/test_stats_bw_gpu.py: a chain, a fan and a chain over windows of 40, 60 and 45 frames
of one 2 s utterance.  The state rows are the oracle's double log-likelihoods of the whole utterance, so the frame buffer
has the utterance's rows and the windows lie in it with gaps between them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmmnet_cases as HC  # noqa: E402
import mllr_bw_restate as MB  # noqa: E402
import test_stats_bw_gpu as SB  # noqa: E402

pytestmark = pytest.mark.gpu
world = SB.world
BW, RS, S = MB.BW, MB.RS, SB.S


def wide(capi):
    o = capi.FbOptions.defaults()
    o.fw_beam = o.bw_beam = 1e9
    return o


@pytest.fixture(scope="module")
def batch(capi, world):
    import torch
    w = world
    nets = [capi.HmmNet(w.topo, p) for p in w.nets]
    scores = torch.tensor(w.ll, device="cuda")
    T = [b - a for a, b in w.windows]
    row0 = [a for a, _ in w.windows]
    got = capi.fb_batch_frame_entries(nets, T, scores, row0, S, wide(capi), pdf_major=True)
    utts = [BW.entries(HC.parse(t, w.sp), w.ll[a:b], 1e9, 1e9) for (a, b), t in zip(w.windows, w.texts)]
    return dict(nets=nets, scores=scores, T=T, row0=row0, got=got, utts=utts)


def test_offsets(world, batch):
    w, got = world, batch["got"]
    off = got["off"]
    assert got["status"] == [capi_ok()] * 3
    assert len(off) == w.T + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == got["n_entries"] == len(got["pdf"])
    inside = np.zeros(w.T, bool)
    for a, b in w.windows:
        inside[a:b] = True
    n = np.diff(off)
    assert (n[~inside] == 0).all() and (n[inside] >= 1).all()        # every frame of a window has some pdf
    sh = got["shape"]
    assert sh["entries"] == got["n_entries"] and sh["utterances"] == 3
    assert sh["count_groups"] == 3 and sh["fill_groups"] == 3 and sh["scan_groups"] == 1


def capi_ok():
    return 1                                                         # AASR_FB_OK


def test_the_same_entries_as_the_pdf_major_call_bit_for_bit(world, batch):
    got = batch["got"]
    frame_of = np.repeat(np.arange(len(got["off"]) - 1), np.diff(got["off"]))
    pdf_of = np.repeat(np.arange(S), np.diff(got["cnt"]))
    assert got["cnt"][-1] == got["n_entries"]
    a = sorted(zip(got["pdf"].tolist(), frame_of.tolist(), got["weight"].view(np.int64).tolist()))
    b = sorted(zip(pdf_of.tolist(), got["rows"].tolist(), got["weights"].view(np.int64).tolist()))
    assert a == b


def test_a_frames_entries_follow_the_networks_pdf_list(world, batch):
    w, got = world, batch["got"]
    lists = MB.frame_lists(batch["utts"], batch["row0"], w.T)
    for e in batch["utts"]:
        assert e["status"] == RS.OK and e["min_positive_occ"] > 1e-200
    mine = MB.unflatten(got["off"], got["pdf"], got["weight"])
    worst = 0.0
    for (a, b), e in zip(w.windows, batch["utts"]):
        for r in range(a, b):
            slots = [e["pdfs"].index(p) for p, _ in mine[r]]
            assert slots == sorted(slots) and len(set(slots)) == len(slots), r
            assert [p for p, _ in mine[r]] == [p for p, _ in lists[r]], r
            worst = max(worst, max(abs(x[1] - y[1]) for x, y in zip(mine[r], lists[r])))
            assert abs(sum(x[1] for x in mine[r]) - 1.0) <= 1e-12
    print("largest weight difference from the restatement %.3g" % worst)
    assert worst <= 1e-9
    for u, s in enumerate(got["sums"]):                              # s_t: aasr_fb_batch_frame_sums works after this call
        assert np.abs(s - batch["utts"][u]["s"]).max() <= 1e-9


def test_a_failed_backward_pass_contributes_nothing_and_two_runs_agree(capi, world, batch, tmp_path):
    w = world
    long_net = str(tmp_path / "long.hmmnet")
    open(long_net, "w").write(HC.chain([s % S for s in range(25)]))  # 25 states over 20 frames never initialise
    nets = batch["nets"] + [capi.HmmNet(w.topo, long_net)]
    T, row0 = batch["T"] + [20], batch["row0"] + [220]
    assert 240 <= w.T
    runs = [capi.fb_batch_frame_entries(nets, T, batch["scores"], row0, S, wide(capi)) for _ in range(2)]
    got = runs[0]
    assert got["status"][:3] == [1, 1, 1] and got["status"][3] == capi.FB_FAILED_BACKWARD and got["attempts"][3] == 5
    assert got["sums"][3] is None and got["shape"]["utterances"] == 3
    assert (np.diff(got["off"])[220:240] == 0).all()
    for k in ("off", "pdf", "weight"):
        assert got[k].tobytes() == runs[1][k].tobytes() == batch["got"][k].tobytes(), k


def test_overlapping_rows_and_rows_outside_the_buffer_are_refused(capi, world, batch):
    with pytest.raises(capi.AasrError) as ei:
        capi.fb_batch_frame_entries(batch["nets"][:2], batch["T"][:2], batch["scores"], batch["row0"][:2], S, wide(capi),
                                    frame_row0=[10, 30])
    assert ei.value.code == capi.AASR_ERR_INVALID and "share frame row" in ei.value.msg
    with pytest.raises(capi.AasrError) as ei:
        capi.fb_batch_frame_entries(batch["nets"][:1], batch["T"][:1], batch["scores"], batch["row0"][:1], S, wide(capi),
                                    frame_row0=[0], n_rows=39)
    assert ei.value.code == capi.AASR_ERR_INVALID

"""Occupancies into weighted entries on the device (aasr_fb_batch_entries_dev, csrc/fb_entries.hip) against
tools/stats_bw_restate.py, both fed the same synthetic double state rows (tools/hmmnet_cases.py).

A batch of three utterances -- a chain of five states, a fan of three branches of four states over 12 states and the
network with deep epsilon chains over 8 states, at 12 ... 40 frames; the fan and the epsilon network share pdfs with the
chain -- gives cnt, the row list and so the grouping by pdf, then utterance, then frame exactly as the restatement
does; the weights within 1e-9 (the occupancy bound of tests/test_hmmnet_fb_gpu.py: a weight is an occupancy over a sum
of occupancies that is 1, or exp(tail) of the trailing epsilon arcs, to 1e-9); a frame's weights sum to 1 within 4 ulp
(summed here with math.fsum, so that the test adds no rounding of its own).  The restatement reports the smallest
positive occupancy of every input: all far above 1e-200, so no entry hangs on an underflow.  An utterance that fails (a
chain longer than its frames) contributes nothing and leaves the others' entries as they were; Viterbi gives one entry
per frame of weight exactly 1.0; with device_occ the occupancies are not handed out; the global-memory form gives the
same bytes."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402
import stats_bw_restate as BW  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
S = 40
WIDE = 1e9
TEXTS = [HC.chain([3, 0, 7, 2, 5]), HC.fan(12, 3, 4, seed=7), HC.deep_eps(8, seed=8)]
FRAMES = [40, 12, 23]


@pytest.fixture(scope="module")
def model(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("fb_entries")
    sp = HC.self_probs(S)
    HC.write_ph(str(d / "m.ph"), sp)
    return {"dir": d, "sp": sp, "topo": capi.Topology(str(d / "m.ph")), "n": [0]}


def _net(capi, model, text):
    model["n"][0] += 1
    p = str(model["dir"] / ("n%d.hmmnet" % model["n"][0]))
    open(p, "w").write(text)
    return capi.HmmNet(model["topo"], p), HC.parse(text, model["sp"])


def _run(capi, nets, lls, frame_row0, viterbi=False, force_global=False, max_attempts=1, fw=WIDE, bw=WIDE):
    """one batch on score rows stacked with pad rows between the utterances; the entries' rows count from frame_row0"""
    import torch
    o = capi.FbOptions.defaults()
    o.fw_beam, o.bw_beam = fw, bw
    o.mode = capi.FB_VITERBI if viterbi else capi.FB_BAUM_WELCH
    o.force_global = 1 if force_global else 0
    o.max_attempts = max_attempts
    rows, row0 = [], []
    for ll in lls:
        rows.append(np.full((2, ll.shape[1]), 7.0))
        row0.append(sum(len(r) for r in rows))
        rows.append(ll)
    dev = torch.from_numpy(np.concatenate(rows)).to("cuda")
    out = capi.fb_batch_entries(nets, [len(ll) for ll in lls], dev, row0, S, o, frame_row0=frame_row0)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def three(capi, model):
    pairs = [_net(capi, model, t) for t in TEXTS]
    lls = [HC.scores(T, S, 90 + i) for i, T in enumerate(FRAMES)]
    frame_row0 = [0, FRAMES[0], FRAMES[0] + FRAMES[1]]
    want = [BW.entries(p[1], ll, WIDE, WIDE) for p, ll in zip(pairs, lls)]
    return dict(pairs=pairs, lls=lls, frame_row0=frame_row0, want=want,
                got=_run(capi, [p[0] for p in pairs], lls, frame_row0))


def check_entries(got, want_utts, frame_row0, what):
    cnt, rows, weights = BW.group(want_utts, frame_row0, S)
    assert got["cnt"].tolist() == cnt.tolist(), what
    assert got["rows"].tolist() == rows.tolist(), what
    err = float(np.abs(got["weights"] - weights).max()) if len(rows) else 0.0
    worst = 0.0
    for r in np.unique(rows):
        worst = max(worst, abs(math.fsum(got["weights"][got["rows"] == r]) - 1.0))
    print(what, "entries", len(rows), "max |weight error| %.3g" % err, "max |frame sum - 1| %.3g ulp" % (worst / np.finfo(float).eps))
    assert err <= 1e-9, (what, err)
    assert worst <= 4 * np.finfo(float).eps, (what, worst)
    return cnt, rows, weights


def test_three_utterances_one_batch(three):
    got, want = three["got"], three["want"]
    for e in want:
        assert e["status"] == RS.OK and e["min_positive_occ"] > 1e-200, e["min_positive_occ"]
        print("smallest positive occupancy %.3g, max |1 - s_t| %.3g" % (e["min_positive_occ"], e["max_dev"]))
    assert got["status"] == [RS.OK] * 3
    shared = set(want[0]["pdfs"]) & (set(want[1]["pdfs"]) | set(want[2]["pdfs"]))
    assert shared, "the utterances share no pdf"
    cnt, rows, _ = check_entries(got, want, three["frame_row0"], "three")
    p = sorted(shared)[0]                                   # under a shared pdf: the first utterance's rows, then the others'
    r = rows[cnt[p]:cnt[p + 1]]
    assert (np.diff((r >= FRAMES[0]).astype(int)) >= 0).all() and (r < FRAMES[0]).any() and (r >= FRAMES[0]).any()
    for u in range(3):
        assert np.abs(got["sums"][u] - want[u]["s"]).max() <= 1e-9
    tail = float(np.float32(-0.15)) + float(np.float32(-0.7))
    assert np.abs(got["sums"][0] - 1.0).max() <= 1e-9 and np.abs(got["sums"][2] - np.exp(tail)).max() <= 1e-9
    sh = got["shape"]
    assert sh == {"entries": len(rows), "utterances": 3, "sum_groups": 3, "count_groups": 1, "fill_groups": 1}, sh
    code, msg = got["pdf_occ_refused"]                      # the occupancies stay on the device
    assert code != 0 and "device_occ" in msg, (code, msg)


def test_two_runs_and_the_global_form_give_the_same_bytes(capi, three):
    nets = [p[0] for p in three["pairs"]]
    for kw in ({}, {"force_global": True}):
        again = _run(capi, nets, three["lls"], three["frame_row0"], **kw)
        for k in ("cnt", "rows", "weights"):
            assert again[k].tobytes() == three["got"][k].tobytes(), (kw, k)


def test_a_failed_utterance_contributes_nothing(capi, model, three):
    long_net, long_rn = _net(capi, model, HC.chain(list(range(20, 35))))
    nets = [three["pairs"][0][0], long_net, three["pairs"][1][0], three["pairs"][2][0]]
    lls = [three["lls"][0], HC.scores(10, S, 55), three["lls"][1], three["lls"][2]]
    assert RS.forward_backward(long_rn, lls[1], WIDE, WIDE).status == RS.FAILED_BACKWARD
    fr0 = [three["frame_row0"][0], 1000, three["frame_row0"][1], three["frame_row0"][2]]
    got = _run(capi, nets, lls, fr0, max_attempts=2)
    assert got["status"] == [RS.OK, RS.FAILED_BACKWARD, RS.OK, RS.OK] and got["attempts"] == [1, 2, 1, 1]
    assert got["sums"][1] is None and got["shape"]["utterances"] == 3
    for k in ("cnt", "rows", "weights"):
        assert got[k].tobytes() == three["got"][k].tobytes(), k


def test_viterbi_gives_one_entry_of_weight_one_per_frame(capi, three):
    nets = [p[0] for p in three["pairs"]]
    got = _run(capi, nets, three["lls"], three["frame_row0"], viterbi=True)
    want = [BW.entries(p[1], ll, WIDE, WIDE, viterbi=True) for p, ll in zip(three["pairs"], three["lls"])]
    cnt, rows, weights = BW.group(want, three["frame_row0"], S)
    assert got["cnt"].tolist() == cnt.tolist() and got["rows"].tolist() == rows.tolist()
    assert sorted(got["rows"].tolist()) == list(range(sum(FRAMES)))
    assert (got["weights"] == 1.0).all()


def test_narrow_beams(capi, model):
    """beams that prune: the frame sums leave 1, the weights still sum to 1"""
    text = HC.fan(S, 70, 2, seed=20)
    net, rn = _net(capi, model, text)
    ll = HC.scores(8, S, 120)
    want = BW.entries(rn, ll, 4.0, 6.0)
    assert want["status"] == RS.OK and want["result"].pruned >= 1 and want["result"].min_margin >= 0.05
    got = _run(capi, [net], [ll], [0], fw=4.0, bw=6.0)
    check_entries(got, [want], [0], "narrow")
    print("max |1 - s_t|", want["max_dev"])
    assert np.abs(got["sums"][0] - want["s"]).max() <= 1e-9

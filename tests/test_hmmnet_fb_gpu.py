"""The forward-backward handle over HMM networks (aasr_fb_batch_*, csrc/hmmnet_fb.hip) against its NumPy
restatement (tools/hmmnet_restate.py), both fed the SAME synthetic double state rows: the kernel is isolated from
the scoring, and the only difference left is the order of sums in double.

Bounds (from that: a total is a sum of at most a few hundred terms of magnitude |total| or less, each rounded to
2^-53 relative): totals within 1e-9 * max(1, |total|), occupancies within 1e-9, with wide beams every frame's
occupancies sum to 1 within 1e-9 (to exp(s) where epsilon arcs of total score s trail the last frame: the forward
total leaves them out, aku/HmmNetBaumWelch.cc:1389-1416), and two runs give identical bytes.

Shapes, the smallest that reach each path of the kernel: (a) a left-to-right chain of 24 states over 40 frames;
(b) 300 emitting nodes, more than the workgroup's 256 lanes; (c) 70 epsilon arcs out of the initial node, more than
a wave; (d) epsilon chains three deep with a scored arc into the final node; (e) static scores and ac_scale 0.5;
(f) three utterances, three networks, one batch; (g) T = 2; (h) a network longer than its frames; (i) Viterbi;
(j) narrow beams on seeds the restatement clears of near-threshold decisions; (k) the global-memory form forced."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
S = 40
WIDE = 1e9


@pytest.fixture(scope="module")
def model(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("hmmnet_fb")
    sp = HC.self_probs(S)
    HC.write_ph(str(d / "m.ph"), sp)
    return {"dir": d, "sp": sp, "topo": capi.Topology(str(d / "m.ph")), "n": [0]}


def _net(capi, model, text):
    model["n"][0] += 1
    p = str(model["dir"] / ("n%d.hmmnet" % model["n"][0]))
    open(p, "w").write(text)
    return capi.HmmNet(model["topo"], p), HC.parse(text, model["sp"])


def _run(capi, nets, lls, fw=WIDE, bw=WIDE, ac=1.0, viterbi=False, force_global=False, pad_rows=3, max_attempts=1):
    """one batch: the utterances' rows stacked (pad rows between them, so a wrong row0 shows) -> results"""
    import torch
    o = capi.FbOptions.defaults()
    o.fw_beam, o.bw_beam, o.ac_scale = fw, bw, ac
    o.mode = capi.FB_VITERBI if viterbi else capi.FB_BAUM_WELCH
    o.want_pdf_occ = o.want_tr_occ = 1
    o.force_global = 1 if force_global else 0
    o.max_attempts = max_attempts
    rows, row0 = [], []
    for ll in lls:
        rows.append(np.full((pad_rows, ll.shape[1]), 7.0))
        row0.append(sum(len(r) for r in rows))
        rows.append(ll)
    dev = torch.from_numpy(np.concatenate(rows)).to("cuda")
    out = capi.fb_batch(nets, [len(ll) for ll in lls], dev, row0, o)
    torch.cuda.synchronize()
    return out


def _check(got, want, what, occ_sum=1.0):
    print(what, "status", got["status"], want.status, "backward", got["backward_total"], want.backward_total,
          "forward", got["forward_total"], want.forward_total)
    assert got["status"] == want.status, what
    if want.status != RS.OK:
        return
    for k, w in (("backward_total", want.backward_total), ("forward_total", want.forward_total)):
        assert abs(got[k] - w) <= 1e-9 * max(1.0, abs(w)), (what, k, got[k], w)
    e_occ = float(np.abs(got["pdf_occ"] - want.pdf_occ).max())
    e_tr = float(np.abs(got["tr_occ"] - want.tr_occ).max())
    print(what, "max |occupancy error|", e_occ, e_tr)
    assert e_occ <= 1e-9 and e_tr <= 1e-9, (what, e_occ, e_tr)
    if occ_sum is not None:
        s = got["pdf_occ"].sum(axis=1)
        assert np.abs(s - occ_sum).max() <= 1e-9, (what, s)


def _single(capi, model, text, T, seed, **kw):
    net, rn = _net(capi, model, text)
    ll = HC.scores(T, S, seed)
    got = _run(capi, [net], [ll], **kw)[0]
    rkw = {"fw_beam": kw.get("fw", WIDE), "bw_beam": kw.get("bw", WIDE), "ac_scale": kw.get("ac", 1.0),
           "viterbi": kw.get("viterbi", False)}
    return got, RS.forward_backward(rn, ll, **rkw), net, rn, ll


CHAIN24 = [h * 3 + j for h in (3, 0, 7, 2, 5, 1, 9, 6) for j in range(3)]


def test_a_chain_of_24_states_over_40_frames(capi, model):
    got, want, *_ = _single(capi, model, HC.chain(CHAIN24), 40, 1)
    assert got["shape"]["lds_form"] == 1 and got["attempts"] == 1
    _check(got, want, "a")


def test_b_300_emitting_nodes(capi, model):
    text = HC.fan(S, 30, 10, seed=2)
    got, want, net, *_ = _single(capi, model, text, 16, 2)
    assert net.counts()["emitting"] == 600 and net.counts()["nodes"] == 303
    _check(got, want, "b")


def test_c_fan_out_of_70_epsilon_arcs(capi, model):
    got, want, net, *_ = _single(capi, model, HC.fan(S, 70, 2, seed=3, eps_scores=True), 8, 3)
    assert net.counts()["epsilon"] == 71
    _check(got, want, "c")


def test_d_epsilon_chains_three_deep_and_a_scored_arc_into_the_final_node(capi, model):
    """the forward total leaves out the epsilon arcs behind the last frame (here -0.15, 0 and -0.7, stored as floats),
    the backward total has them"""
    got, want, net, rn, ll = _single(capi, model, HC.deep_eps(S, seed=4), 9, 4)
    assert net.counts()["backward_levels"] == 4 and net.counts()["forward_levels"] == 4
    tail = float(np.float32(-0.15)) + float(np.float32(-0.7))
    _check(got, want, "d", occ_sum=np.exp(tail))
    assert abs(got["backward_total"] - got["forward_total"] - tail) <= 1e-9 * abs(got["backward_total"])
    assert abs(got["backward_total"] - RS.brute_force(rn, ll)) <= 1e-9 * abs(got["backward_total"])


def test_e_static_scores_and_acoustic_scale(capi, model):
    got, want, *_ = _single(capi, model, HC.fan(S, 6, 3, seed=5, static=1.5, eps_scores=True), 10, 5, ac=0.5)
    _check(got, want, "e")
    got, want, *_ = _single(capi, model, HC.chain(CHAIN24[:9], static=2.0, seed=6), 14, 6, ac=0.5)
    _check(got, want, "e chain")


def test_f_three_utterances_three_networks_one_batch(capi, model):
    texts = [HC.chain(CHAIN24[:6]), HC.fan(S, 9, 3, seed=7), HC.deep_eps(S, seed=8)]
    Ts = [17, 9, 12]
    pairs = [_net(capi, model, t) for t in texts]
    lls = [HC.scores(T, S, 70 + i) for i, T in enumerate(Ts)]
    batch = _run(capi, [p[0] for p in pairs], lls)
    for i in range(3):
        one = _run(capi, [pairs[i][0]], [lls[i]], pad_rows=1)[0]
        for k in ("status", "backward_total", "forward_total"):
            assert batch[i][k] == one[k], (i, k)
        assert batch[i]["pdf_occ"].tobytes() == one["pdf_occ"].tobytes()
        assert batch[i]["tr_occ"].tobytes() == one["tr_occ"].tobytes()
        _check(batch[i], RS.forward_backward(pairs[i][1], lls[i], WIDE, WIDE), "f%d" % i, occ_sum=None)
    again = _run(capi, [p[0] for p in pairs], lls)
    for i in range(3):   # two runs: identical bytes
        assert again[i]["pdf_occ"].tobytes() == batch[i]["pdf_occ"].tobytes()
        assert (again[i]["backward_total"], again[i]["forward_total"]) == (batch[i]["backward_total"], batch[i]["forward_total"])


def test_g_two_frames(capi, model):
    got, want, *_ = _single(capi, model, HC.fan(S, 5, 2, seed=9), 2, 9)
    _check(got, want, "g")
    got, want, *_ = _single(capi, model, HC.chain([4]), 2, 10)
    _check(got, want, "g chain")


def test_h_a_network_longer_than_its_frames_fails_alone(capi, model):
    long_net, long_rn = _net(capi, model, HC.chain(CHAIN24))
    ok_net, ok_rn = _net(capi, model, HC.chain(CHAIN24[:5]))
    lls = [HC.scores(11, S, 20), HC.scores(10, S, 21), HC.scores(12, S, 22)]
    out = _run(capi, [ok_net, long_net, ok_net], lls, max_attempts=3)
    assert out[1]["status"] == capi.FB_FAILED_BACKWARD and out[1]["attempts"] == 3
    assert RS.forward_backward(long_rn, lls[1], WIDE, WIDE).status == RS.FAILED_BACKWARD
    for i in (0, 2):
        assert out[i]["attempts"] == 1
        _check(out[i], RS.forward_backward(ok_rn, lls[i], WIDE, WIDE), "h%d" % i)


@pytest.mark.parametrize("shape", ["a", "c"])
def test_i_viterbi(capi, model, shape):
    text, T = (HC.chain(CHAIN24), 40) if shape == "a" else (HC.fan(S, 70, 2, seed=3), 8)
    got, want, net, rn, ll = _single(capi, model, text, T, 30, viterbi=True)
    _check(got, want, "i " + shape)
    assert abs(got["forward_total"] - got["backward_total"]) <= 1e-9 * abs(got["backward_total"])
    assert set(np.unique(got["pdf_occ"])) <= {0.0, 1.0}
    if shape == "c":   # small enough to enumerate
        assert abs(got["forward_total"] - RS.brute_force(rn, ll, viterbi=True)) <= 1e-9 * abs(got["forward_total"])


@pytest.mark.parametrize("seed", [20, 26, 37])
def test_j_narrow_beams(capi, model, seed):
    """backward beam 6, forward beam 4 on (c).  The restatement first: it prunes at least one arc and no pruning
    comparison is closer than 0.05 to its threshold, so rounding cannot flip a decision on the device."""
    text = HC.fan(S, 70, 2, seed=seed)
    net, rn = _net(capi, model, text)
    ll = HC.scores(8, S, seed + 100)
    want = RS.forward_backward(rn, ll, fw_beam=4.0, bw_beam=6.0)
    assert want.status == RS.OK and want.pruned >= 1 and want.min_margin >= 0.05, (want.pruned, want.min_margin)
    wide = RS.forward_backward(rn, ll, WIDE, WIDE)
    assert abs(wide.forward_total - want.forward_total) > 1e-3      # the beams changed the result
    got = _run(capi, [net], [ll], fw=4.0, bw=6.0)[0]
    _check(got, want, "j %d" % seed, occ_sum=None)


def test_k_global_memory_form(capi, model):
    text = HC.fan(S, 30, 10, seed=2)
    got, want, net, rn, ll = _single(capi, model, text, 16, 2, force_global=True)
    assert got["shape"]["lds_form"] == 0 and got["shape"]["lds_bytes"] <= 2048 + 8
    _check(got, want, "k")
    lds = _run(capi, [net], [ll])[0]
    assert lds["shape"]["lds_form"] == 1
    assert lds["pdf_occ"].tobytes() == got["pdf_occ"].tobytes() and lds["forward_total"] == got["forward_total"]


def test_float_rows_and_bad_rows(capi, model):
    """float rows are read as the aligner reads them; rows the buffer does not have are refused before the launch"""
    import torch
    net, rn = _net(capi, model, HC.chain(CHAIN24[:4]))
    ll = HC.scores(9, S, 40).astype(np.float32)
    dev = torch.from_numpy(ll).to("cuda")
    o = capi.FbOptions.defaults()
    o.fw_beam = o.bw_beam = WIDE
    got = capi.fb_batch([net], [9], dev, [0], o)[0]
    want = RS.forward_backward(rn, ll.astype(np.float64), WIDE, WIDE)
    assert got["status"] == capi.FB_OK and abs(got["forward_total"] - want.forward_total) <= 1e-9 * abs(want.forward_total)
    with pytest.raises(capi.AasrError, match="reads rows"):
        capi.fb_batch([net], [9], dev, [1], o)

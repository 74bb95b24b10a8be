"""The three network drivers see the same groups through the shared network step (csrc/network_pass.cc): one recipe of
three utterances under one speaker through logl -H, stats --networks and mllr --networks (model mode: the statistics are
collected on the unadapted model, so all three score the same frames with the same model).

The world is that of tests/test_logl_gpu.py: the production feature chain, 30 states in HMMs of three, a model whose
Gaussians lie among the frames.  The lines, each a whole recording:

* `retry` (1 s): tests/test_logl_gpu.py's decoy -- next to the real path of three states a branch longer than the
  utterance that holds every frame's best state and sets each frame's best backward score.  Its backward pass fails at
  the backward beam W and succeeds at 2 W: one beam increase.
* `long` (1.2 s): a chain of more states than the utterance has frames.  It never initialises: four wider beams, then
  the tool gives up.
* `plain` (2 s): the chain of tests/test_logl_gpu.py, which runs at the first attempt.

W comes from the restatement (tools/hmmnet_restate.py) on the oracle's double state likelihoods: a candidate at which
`retry` fails at W and runs at 2 W, `plain` runs at W, and every pruning comparison of those three runs stays
10 x frames x 1e-4 away from its threshold -- ten times what the parity contract on state log-likelihoods
(conftest.TOL_LL) lets a path of that many frames differ by, the rule of tests/test_logl_gpu.py's retry test -- so the
device's float scores cannot flip a decision.

Asserted, from each tool's own messages: the same retries in the same order (one increase and it ran; four and it was
given up) in all three; logl's file lines name `retry` and `plain`, logl and mllr name `long` as given up, stats reports
two utterances; aasr_run_stats.frames of stats and mllr are the frames of `retry` and `plain`; stats and mllr print the
same "Weighted entries: N over M frames" line; the forward totals agree: logl's and mllr's %f are the same digits, and
stats' .lls figure rounds to them.  Measured on the commit before the shared step existed, where each driver still had
its own copy of it: logl -1609.667811, mllr -1609.667811, .lls -1609.66781137 -- no disagreement at the printed digit, so
equality is asserted.  The restatement's total is held to the bound of tests/test_logl_gpu.py, once per utterance that
ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmmnet_cases as HC  # noqa: E402
from test_logl_gpu import PER, Q, S, write_wav  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
SECONDS = {"retry": 1.0, "long": 1.2, "plain": 2.0}
ORDER = ("retry", "long", "plain")
TOL_LL = 1e-4                                                         # conftest.TOL_LL
MODEL_SPKC = "speaker default\n{\n  model cmllr\n  {\n  }\n}\n"


class World:
    pass


def decoy_network(ll):
    """tests/test_logl_gpu.py::test_the_backward_beam_is_widened_once's network for the frames of ll"""
    n = len(ll)
    order = np.argsort(ll.sum(axis=0))
    real = [int(order[0]), int(order[1]), int(order[2])]                 # the three worst states
    decoy = [int(ll[max(0, min(n - 1, n - 1 - k))].argmax()) for k in range(n + 4, -1, -1)]
    bld = HC.Builder()
    init, fin = bld.node(), bld.node()
    for states in (real, decoy):
        nodes = [bld.node() for _ in states]
        bld.eps(init, nodes[0])
        for i, s in enumerate(states):
            bld.emit(nodes[i], nodes[i], 2 * s)
            bld.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else fin, 2 * s + 1)
    return bld.text(init, fin)


def choose_beam(w):
    """-> W, the forward total of `retry` at 2 W and of `plain` at W"""
    cands = [round(10 * 1.12 ** k, 1) for k in range(70)]
    rnet, pnet = HC.parse(w.text["retry"], w.sp), HC.parse(w.text["plain"], w.sp)
    run = lambda net, name, bw: RS.forward_backward(net, w.ll[name], 1e9, float(bw))
    assert run(rnet, "retry", cands[0]).status == RS.FAILED_BACKWARD and run(rnet, "retry", cands[-1]).status == RS.OK
    lo, hi = 0, len(cands) - 1                                           # the first candidate at which `retry` runs
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if run(rnet, "retry", cands[mid]).status == RS.OK else (mid, hi)
    for W in reversed(cands[max(0, hi - 7):hi]):                         # 1.12^7 > 2: below these 2 W does not reach it
        r1, r2, p = run(rnet, "retry", W), run(rnet, "retry", 2 * W), run(pnet, "plain", W)
        margins = (r1.min_margin / w.T["retry"], r2.min_margin / w.T["retry"], p.min_margin / w.T["plain"])
        print("W %.1f: retry %d then %d, plain %d, margins a frame %.3g %.3g %.3g" % ((W, r1.status, r2.status, p.status) + margins))
        if r1.status == RS.FAILED_BACKWARD and r2.status == RS.OK and p.status == RS.OK and min(margins) >= 10 * TOL_LL:
            return W, r2.forward_total, p.forward_total
    raise AssertionError("no backward beam separates the runs on this fixture")


def run_tool(w, exe, *flags, env=None):
    cmd = [os.path.join(BIN, exe), "-b", w.base, "-c", w.cfg, "-r", w.recipe, "-i", "1", "-F", "1e9", "-W", str(w.W)] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def retries(w, stderr, increase, give_up):
    """the utterances that were run again, in the order of the messages: [beam increases, given up]"""
    runs = []
    for line in stderr.splitlines():
        if line.startswith(increase):
            if line == increase + "%.1f" % (2.0 * w.W):
                runs.append([0, False])
            runs[-1][0] += 1
        elif line.startswith(give_up):
            runs[-1][1] = True
    return runs


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = World()
    w.dir = d = tmp_path_factory.mktemp("network_pass")
    rng = np.random.default_rng(41)
    cfg_text = synth.make_feature_config()
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(cfg_text)
    ft = capi.Feat(cfg_text)
    w.wav, w.T, fea = {}, {}, {}
    for i, name in enumerate(ORDER):
        pcm = synth.make_audio(int(16000 * SECONDS[name]), seed=73 + i)
        w.wav[name] = str(d / (name + ".wav"))
        write_wav(w.wav[name], pcm)
        w.T[name] = ft.eof_frame(len(pcm))
        fea[name] = ft.run(pcm, 0, w.T[name], dtype=np.float64)
    allf = np.concatenate([fea[name] for name in ORDER])
    mean, var, off, idx, mw = synth.make_model(D=39, G=90, S=S, comps=3, seed=27)
    mean[:] = allf[rng.integers(0, len(allf), 90)] + 0.3 * rng.standard_normal((90, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    dm = oracle.DiagModel(mean, var, off, idx, mw)
    w.ll = {name: dm.score(fea[name]) for name in ORDER}
    w.sp = np.full(S, 0.5)
    w.text = {"retry": decoy_network(w.ll["retry"]), "long": HC.chain([s % S for s in range(w.T["long"] + 5)]),
              "plain": HC.chain(Q)}
    w.net = {}
    for name in ORDER:
        w.net[name] = str(d / (name + ".hmmnet"))
        open(w.net[name], "w").write(w.text[name])
    w.recipe = str(d / "three.recipe")
    open(w.recipe, "w").write("".join("audio=%s hmmnet=%s speaker=s1\n" % (w.wav[n], w.net[n]) for n in ORDER))
    w.spkc = str(d / "model.spkc")
    open(w.spkc, "w").write(MODEL_SPKC)
    w.W, w.want_retry, w.want_plain = choose_beam(w)
    assert RS.forward_backward(HC.parse(w.text["long"], w.sp), w.ll["long"], 1e9, 5.0 * w.W).status == RS.FAILED_BACKWARD
    w.frames = w.T["retry"] + w.T["plain"]
    # the three tools, once
    w.logl = run_tool(w, "logl", "-H")
    w.stats_out = str(d / "st")
    w.stats = run_tool(w, "stats", "-o", w.stats_out, "--ml", "--networks")
    w.mllr = run_tool(w, "mllr", "-S", w.spkc, "-o", str(d / "out.spkc"), "--networks")
    # and the two that report frames, through the library
    topo = capi.Topology(w.base + ".ph")
    gmm = lambda: capi.Gmm.from_files(w.base + ".gk", w.base + ".mc", w.base + ".ph")
    w.res_stats = capi.run_stats_recipe(capi.Feat(cfg_text), gmm(), topo, w.recipe, str(d / "lib_st"),
                                        networks=capi.StatsNetworkOptions.defaults(fw_beam=1e9, bw_beam=w.W))
    ft2, g = capi.Feat(cfg_text), gmm()
    sc = capi.SpeakerConfig(ft2, g)
    sc.read_text(MODEL_SPKC)
    w.res_mllr = capi.run_mllr_recipe(ft2, g, topo, w.recipe, sc,
                                      networks=capi.MllrNetworkOptions.defaults(networks=1, fw_beam=1e9, bw_beam=w.W))
    return w


def test_the_same_utterances_are_run_again_and_given_up(world):
    w = world
    bw = "Warning: Backward phase failed, increasing beam to "
    got = {"logl": retries(w, w.logl.stderr, bw, "Could not run Baum-Welch for file "),
           "stats": retries(w, w.stats.stderr, "Increasing beam to ", "Giving up for this file"),
           "mllr": retries(w, w.mllr.stderr, bw, "Could not run Baum-Welch for file ")}
    print(got)
    assert got["logl"] == got["stats"] == got["mllr"] == [[1, False], [4, True]]
    # which they were: logl names the files that ran, logl and mllr the one given up; stats counts
    ran = [l.split(" ")[4].rstrip(":") for l in w.logl.stdout.splitlines() if l.startswith("Log likelihood for file ")]
    assert ran == [w.wav["retry"], w.wav["plain"]]
    for r in (w.logl, w.mllr):
        assert [l for l in r.stderr.splitlines() if l.startswith("Could not run Baum-Welch")] == \
            ["Could not run Baum-Welch for file " + w.wav["long"]]
    assert w.stats.stderr.count("Could not initialize the utterance segmentation.\n") == 2
    assert len([l for l in w.stats.stderr.splitlines() if l.startswith("  ")]) == 2
    assert w.mllr.stderr.count("Processing file: ") == w.stats.stderr.count("Processing file: ") == 3


def test_the_same_frames_and_entries(world):
    w = world
    print("frames: want %d, stats %d, mllr %d" % (w.frames, w.res_stats["frames"], w.res_mllr["frames"]))
    assert w.res_stats["frames"] == w.res_mllr["frames"] == w.frames
    assert w.res_stats["utterances"] == w.res_mllr["utterances"] == 3
    lines = [[l for l in r.stderr.splitlines() if l.startswith("Weighted entries: ")] for r in (w.stats, w.mllr)]
    print(lines)
    assert len(lines[0]) == 1 and lines[0] == lines[1] and lines[0][0].endswith(" over %d frames" % w.frames)
    assert open(w.stats_out + ".lls").read().split("\n")[1] == "Number of frames: %d" % w.frames


def test_the_same_forward_totals(world):
    w = world
    logl = w.logl.stdout.strip().splitlines()[-1]
    assert logl.startswith("Total log likelihood (0/0): "), logl
    logl = logl.split(": ")[1]
    mllr = [l for l in w.mllr.stderr.splitlines() if l.startswith("Total log likelihood: ")]
    lls = open(w.stats_out + ".lls").read().split("\n")[0]
    assert len(mllr) == 1 and lls.startswith("Numerator loglikelihood: ")
    mllr, lls = mllr[0].split(": ")[1], lls.split(": ")[1]
    want = w.want_retry + w.want_plain
    print("forward totals: logl %s, mllr %s, stats .lls %s; restatement %.6f" % (logl, mllr, lls, want))
    assert logl == mllr == "%f" % float(lls)
    assert abs(float(logl) - want) <= 2 * 5e-3 + 1e-6 * (abs(w.want_retry) + abs(w.want_plain))

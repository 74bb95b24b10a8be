"""HMM networks, the host side (no GPU): the reader's flat arrays on written-out networks, every refusal with the
reference's message (aku/HmmNetBaumWelch.cc:65-289, 536-617), the logl tool's option list and its refusals -- each
comes before the device is opened -- and the restatement (tools/hmmnet_restate.py) against a brute-force
enumeration of paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402

RS = HC.RS
S = 12


@pytest.fixture(scope="module")
def model(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("hmmnet")
    sp = HC.self_probs(S)
    HC.write_ph(str(d / "m.ph"), sp)
    return {"dir": d, "sp": sp, "topo": capi.Topology(str(d / "m.ph"))}


def read(capi, model, text, name="n.hmmnet"):
    p = str(model["dir"] / name)
    open(p, "w").write(text)
    return capi.HmmNet(model["topo"], p)


def test_arrays_of_a_small_chain(capi, model):
    """I 0, F 3: 0 -eps-> 1, node 1 emits state 4 (transitions 8, 9), node 2 state 7 (14, 15) with a label and a score"""
    text = ("#FSTBasic MaxPlus\nI 0\nF 3\nT 0 1\nT 1 1 8\nT 1 2 9\nT 2 3 15;7;a-b+c , -1.5\nT 2 2 14;7;a-b+c\n")
    net = read(capi, model, text)
    assert net.counts() == {"nodes": 4, "emitting": 4, "epsilon": 1, "backward_levels": 1, "forward_levels": 1, "pdfs": 2,
                            "transitions": 4, "initial": 0, "final": 3}
    want = {"em_begin": [0, 0, 2, 4, 4], "em_src": [1, 1, 2, 2], "em_tgt": [1, 2, 3, 2], "em_pdf": [4, 4, 7, 7],
            "em_tr": [8, 9, 15, 14], "em_self": [1, 0, 0, 1], "in_begin": [0, 0, 1, 3, 4], "in_arcs": [0, 1, 3, 2],
            "pdfs": [4, 7], "pdf_begin": [0, 2, 4], "pdf_arcs": [0, 1, 2, 3], "trs": [8, 9, 14, 15],
            "tr_begin": [0, 1, 2, 3, 4], "tr_arcs": [0, 1, 3, 2], "eo_begin": [0, 1, 1, 1, 1], "ep_src": [0], "ep_tgt": [1],
            "ei_begin": [0, 0, 1, 1, 1], "ei_arcs": [0], "bl_begin": [0, 1], "bl_nodes": [0], "fl_begin": [0, 1],
            "fl_nodes": [1]}
    for k, v in want.items():
        assert net.array(k).tolist() == v, k
    sp = model["sp"]
    p = lambda x: float("%.3f" % x)
    np.testing.assert_allclose(net.array("em_logp"), np.log([p(sp[4]), p(1 - sp[4]), p(1 - sp[7]), p(sp[7])]), rtol=0, atol=1e-15)
    assert net.array("em_static").tolist() == [0.0, 0.0, -1.5, 0.0]
    assert net.array("ep_score").tolist() == [0.0]
    assert [net.arc_label(a) for a in range(4)] == ["", "", ";7;a-b+c", ";7;a-b+c"] and net.arc_label(4) is None


def test_epsilon_levels_and_labels(capi, model):
    """the network of case (d): epsilon chains three deep, two routes of different depth into one node, a "#" label"""
    net = read(capi, model, HC.deep_eps(S, seed=2))
    c = net.counts()
    assert (c["nodes"], c["emitting"], c["epsilon"], c["backward_levels"], c["forward_levels"]) == (17, 8, 14, 4, 4)
    assert net.array("bl_begin").tolist() == [0, 4, 7, 10, 12]
    assert net.array("bl_nodes").tolist() == [3, 6, 10, 15, 2, 8, 14, 1, 7, 12, 0, 5]
    assert net.array("fl_nodes").tolist() == [1, 7, 13, 14, 2, 8, 15, 3, 6, 16, 4, 9, 11]
    src, tgt = net.array("ep_src"), net.array("ep_tgt")
    height = {int(n): l for l in range(4) for n in net.array("bl_nodes")[net.array("bl_begin")[l]:net.array("bl_begin")[l + 1]]}
    for s, t in zip(src, tgt):       # a level reads only finished levels
        assert height[int(s)] > height.get(int(t), -1)
    np.testing.assert_array_equal(net.array("ep_score"), np.float32([-0.25, 0, -0.5, 0, -0.3, -0.1, 0, -0.6, -0.2, -0.4, 0, -0.15,
                                                                   0, -0.7]).astype(np.float64))


HEAD = "I 0\nF 2\n"
REFUSALS = [
    ("#FSTBinary\n", "FSTBinary format not supported"),
    (HEAD + "T 0 1\nT 1 1\nT 1 2 3\n", "HmmNetBaumWelch: Epsilon self loops are not allowed"),
    (HEAD + "T 0 1\nT 1 1 2\nT 1 2 3\nT 1 3 3\nT 3 2 5\n",
     "HmmNetBaumWelch: Self transitions and multiple out transitions can not be combined"),
    (HEAD + "T 0 1\nT 1 0 3\nT 1 2 3\n", "HmmNetBaumWelch: Initial node may not have in arcs!"),
    (HEAD + "T 0 1\nT 1 2 3\nT 2 1 5\n", "HmmNetBaumWelch: Final node may not have out arcs!"),
    (HEAD + "T 0 1\nT 1 3 3\nT 3 1 5\nT 3 2 5\n", "Failed to create a topological order of the nodes"),
    (HEAD + "T 0 1\nT 1 x 3\n", "HmmNetBaumWelch: Invalid transition specification: T 1 x 3"),
    (HEAD + "T 0 1\nT 1 2 3 , 0.5 extra\n", "HmmNetBaumWelch: Invalid transition specification: T 1 2 3 , 0.5 extra"),
    (HEAD + "I 1\n", "Initial node redefined: I 1"),
    (HEAD + "F 1\n", "Final node redefined: F 1"),
    ("I x\n", "Invalid initial node specification: I x"),
    ("I 0\nF\n", "Invalid final node specification: F"),
    ("F 2\nT 0 2 1\n", "initial node not specified"),
    ("I 0\nT 0 2 1\n", "final node not specified"),
    (HEAD + "T 0 1\nT 1 2 3x\n", "Invalid arc label 3x"),
    (HEAD + "T 0 1\nT 1 2 %d\n" % (2 * S), "transition index %d" % (2 * S)),
]


@pytest.mark.parametrize("text,message", REFUSALS)
def test_refusals(capi, model, text, message):
    with pytest.raises(capi.AasrError) as ei:
        read(capi, model, text, "bad.hmmnet")
    assert message in str(ei.value), str(ei.value)


def test_a_missing_file(capi, model):
    with pytest.raises(capi.AasrError, match="HmmNetBaumWelch::open: Could not open file `/nonexistent/x.hmmnet'."):
        capi.HmmNet(model["topo"], "/nonexistent/x.hmmnet")


SIX = ("I 0\nF 5\nT 0 1 , , -0.2\nT 0 2 #b , -0.9\nT 1 1 2\nT 1 3 3 , 0.4\nT 2 2 8\nT 2 3 9\nT 3 4 10 , -0.3\n"
       "T 3 5 11\nT 4 4 4\nT 4 5 5\n")


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("T,ac", [(2, 1.0), (5, 1.0), (6, 0.5)])
def test_restatement_against_path_enumeration(model, viterbi, T, ac):
    """six nodes: two scored epsilon arcs out of the initial node, two self-loop states that merge in a node without a
    self loop, from which one arc reaches the final node directly and one through a third state"""
    net = HC.parse(SIX, model["sp"])
    assert net.n_nodes == 6
    ll = HC.scores(T, S, 11 * T)
    want = RS.brute_force(net, ll, ac, viterbi)
    r = RS.forward_backward(net, ll, 1e9, 1e9, ac, viterbi)
    assert r.status == RS.OK and r.pruned == 0
    assert abs(r.backward_total - want) <= 1e-12 * abs(want) and abs(r.forward_total - want) <= 1e-12 * abs(want)
    np.testing.assert_allclose(r.pdf_occ.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert abs(r.tr_occ.sum() - T) <= 1e-12 * T
    if viterbi:
        assert len(r.path) == T


def test_restatement_failure_flag_and_pruning_report(model):
    net = HC.parse(HC.chain([1, 2, 3, 4]), model["sp"])
    r = RS.forward_backward(net, HC.scores(3, S, 1), 1e9, 1e9)
    assert r.status == RS.FAILED_BACKWARD and r.backward_total == RS.ZERO
    ll = HC.scores(8, 40, 120)
    fan = HC.parse(HC.fan(40, 70, 2, seed=20), HC.self_probs(40))
    r = RS.forward_backward(fan, ll, fw_beam=4.0, bw_beam=6.0)
    assert r.status == RS.OK and r.pruned >= 1 and r.min_margin >= 0.05


def test_the_library_refuses_without_a_device(capi, model):
    """the reader is host only; the batch needs the device and says so"""
    net = read(capi, model, HC.chain([1, 2]))
    if capi.lib().aasr_device_count() > 0:
        return
    with pytest.raises(capi.AasrError) as ei:
        capi.fb_batch([net], [4], np.zeros((4, S)), [0])
    assert ei.value.code == capi.AASR_ERR_NO_DEVICE


# ---- the logl tool: what it says before the device is opened ----------------------------------------------------------

LOGL = os.path.join(BIN, "logl")


@pytest.fixture(scope="module")
def files(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("logl_host")
    open(d / "f.cfg", "w").write("module\n{\n  name audiofile\n  type audiofile\n  sample_rate 16000\n}\n")
    open(d / "m.gk", "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(d / "full.gk", "w").write("1 2 full_cov\n0 0 1 0 1\n")
    open(d / "sub.gk", "w").write("1 2 variable\npcgmm 0 0 1 1\n")
    for name in ("m", "full", "sub"):
        open(d / (name + ".mc"), "w").write("1\n1 0 1.0\n")
        HC.write_ph(str(d / (name + ".ph")), [0.5])
    open(d / "r.recipe", "w").write("audio=%s hmmnet=%s\n" % (d / "a.wav", d / "a.hmmnet"))
    open(d / "lines.recipe", "w").write("audio=%s transcript=%s start-line=2 end-line=5\n" % (d / "a.wav", d / "a.phn"))
    open(d / "model.spkc", "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    return d


def run_logl(files, *extra, base="m", recipe="r.recipe"):
    return subprocess.run([LOGL, "-b", str(files / base), "-c", str(files / "f.cfg"), "-r", str(files / recipe)] + list(extra),
                          capture_output=True, text=True, timeout=60)


def test_logl_help_lists_the_reference_options(capi):
    """the option list of aku/logl.cc (tests/golden/logl_options.txt: short name, long name, help text), plus --device"""
    r = subprocess.run([LOGL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: logl [OPTION...]\n")
    rows = [l.split("\t") for l in open(os.path.join(GOLDEN, "logl_options.txt")).read().splitlines()]
    assert len(rows) == 20
    for short, long, text in rows:
        want = ("-%s, --%s" % (short, long)) if short else ("    --%s" % long)
        line = [l for l in r.stdout.splitlines() if want in l]
        assert len(line) == 1 and line[0].rstrip().endswith(text), (want, line)
    assert "--device=INT" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.lstrip().startswith("-")]) == 21


def test_logl_refusals_come_before_the_device(capi, files):
    r = run_logl(files, "-H", "--mpv")
    assert r.returncode == 1 and "exception: logl: --mpv" in r.stderr, r.stderr
    r = run_logl(files, "-H", base="full")
    assert r.returncode == 1 and "logl: only diagonal Gaussians are supported" in r.stderr and "full_cov" in r.stderr, r.stderr
    r = run_logl(files, "-H", base="sub")
    assert r.returncode == 1 and "logl: only diagonal Gaussians are supported" in r.stderr and "pcgmm" in r.stderr, r.stderr
    r = run_logl(files, "-H", "-S", str(files / "model.spkc"))
    assert r.returncode == 1 and "logl: speaker files with model transforms" in r.stderr, r.stderr
    r = run_logl(files, recipe="lines.recipe")
    assert r.returncode == 1 and "logl: recipe line limits (start-line / end-line) are not supported" in r.stderr, r.stderr
    r = run_logl(files, "-H", "-B", "2")
    assert r.returncode == 1 and "exception: Must give both --batch and --bindex" in r.stderr, r.stderr
    r = run_logl(files, "-H", "-I", "1")
    assert r.returncode == 1 and "exception: Must give both --batch and --bindex" in r.stderr, r.stderr
    r = subprocess.run([LOGL, "-c", str(files / "f.cfg"), "-r", str(files / "r.recipe"), "-g", str(files / "m.gk")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Must give either --base or all --gk, --mc and --ph" in r.stderr, r.stderr
    for res in (r,):
        assert "Aborted" not in res.stderr


def test_logl_reaches_the_device_and_fails_there_without_one(capi, files):
    """the counterpart of the refusals: an accepted command line goes on to open the device and says so when there is none"""
    if capi.lib().aasr_device_count() > 0:
        return
    r = run_logl(files, "-H")
    assert r.returncode == 1 and "logl:" not in r.stderr and "no HIP device available" in r.stderr, r.stderr

"""Viterbi alignments over HMM networks, the host side (no GPU): the restatement (tools/align_restate.py) against its own
enumeration of paths, the condition on the inputs of the GPU tests, and what the library and the stats tool refuse
before the device is opened.

The enumeration walks every path of a network one by one; the restatement's Viterbi pass takes the backward scores and a
single token.  On inputs whose best path leads the runner-up by 1e-6 or more -- seven orders above the rounding of a sum
of at most 40 scores of magnitude 10 to 100 in double -- both must name the same arcs, and so must the device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import align_restate as AR  # noqa: E402
import hmmnet_cases as HC  # noqa: E402

RS = HC.RS
S = 40
CASES = AR.path_cases()
IDS = ["%s-%d" % (c[0], c[2]) for c in CASES]


def test_the_new_symbols_are_declared_and_exported(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for name in ("aasr_fb_batch_path", "aasr_run_dur_est", "aasr_dur_est_default_options", "aasr_dur_est_fit_gamma"):
        assert name in declared and hasattr(L, name), name
    fo = capi.FbOptions.defaults()
    assert fo.want_path == 0 and type(fo)._fields_[-1][0] == "want_path" and type(fo).want_path.offset == 48
    no = capi.StatsNetworkOptions.defaults()
    assert no.alignment == 0 and capi.StatsNetworkOptions._fields_[-1][0] == "alignment"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restated_path_is_the_enumerated_best_path_and_leads_by_1e_6(case):
    """every fixed seed of tests/test_fb_path_gpu.py: a condition on the inputs, checked here"""
    name, text, T, seed = case
    net = HC.parse(text, HC.self_probs(S))
    ll = HC.scores(T, S, seed)
    r = RS.forward_backward(net, ll, 1e9, 1e9, viterbi=True)
    best, gap = AR.best_two_paths(net, ll)
    print(name, T, "nodes", net.n_nodes, "gap to the runner-up %.6g" % gap)
    assert r.status == RS.OK and r.path == best and len(best) == T
    assert gap >= 1e-6
    if name == "six":
        assert net.n_nodes == 6 and abs(r.forward_total - RS.brute_force(net, ll, viterbi=True)) <= 1e-12 * abs(r.forward_total)


def test_alignment_text_of_a_known_path():
    labels = ["4;0;h2", "5;0;h2#", "7", "8;1;g3;w", "9;x"]
    assert [AR.frame_label(l) for l in labels] == ["h2.0", "h2.0", "7", "g3.1", "9;x"]
    text = AR.alignment_text([0, 0, 1, 2, 3, 3, 4], labels, 50, 125.0)
    assert text == "6400 6784 h2.0\n6784 6912 7\n6912 7168 g3.1\n7168 7424 9;x\n"        # the last line: one frame past the range
    assert AR.alignment_text([], labels, 50, 125.0) == ""
    assert AR.arc_labels("I 0\nF 1\nT 0 0 4;0;h2 , 0.0\nT 0 1 #e\nT 0 1\nT 0 1 5 w#\n") == ["4;0;h2", "5;w#"]


def test_engine_arc_numbering(capi, tmp_path):
    """csrc/hmmnet.h numbers the emitting arcs by source node; AR.engine_arcs says where each arc of the file went"""
    sp = HC.self_probs(S)
    HC.write_ph(str(tmp_path / "m.ph"), sp)
    topo = capi.Topology(str(tmp_path / "m.ph"))
    for name, text, _, _ in CASES[::2]:
        p = str(tmp_path / (name + ".hmmnet"))
        open(p, "w").write(text)
        h = capi.HmmNet(topo, p)
        net = HC.parse(text, sp)
        where = AR.engine_arcs(net)
        src, tgt, tr = h.array("em_src"), h.array("em_tgt"), h.array("em_tr")
        labels = AR.arc_labels(text)
        for a, e in enumerate(net.emitting):
            k = where[a]
            assert (src[k], tgt[k], tr[k]) == (e[0], e[1], e[5])
            assert str(tr[k]) + h.arc_label(k) == labels[a]


def test_want_path_is_refused_under_baum_welch_before_the_device(capi, tmp_path):
    HC.write_ph(str(tmp_path / "m.ph"), HC.self_probs(S))
    p = str(tmp_path / "n.hmmnet")
    open(p, "w").write(AR.SIX)
    net = capi.HmmNet(capi.Topology(str(tmp_path / "m.ph")), p)
    o = capi.FbOptions.defaults()
    o.want_path = 1
    with pytest.raises(capi.AasrError, match="want_path needs the Viterbi mode") as e:
        capi.fb_batch([net], [7], None, [0], o)
    assert e.value.code == -2                                    # AASR_ERR_UNSUPPORTED, with or without a device


# ---- the stats tool: -a before the device is opened ------------------------------------------------------------------

@pytest.fixture
def files(capi, tmp_path):
    d = tmp_path
    open(d / "f.cfg", "w").write("module\n{\n  name audiofile\n  type audiofile\n  sample_rate 16000\n}\n")
    open(d / "m.gk", "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(d / "m.mc", "w").write("1\n1 0 1.0\n")
    HC.write_ph(str(d / "m.ph"), [0.5])
    open(d / "net.recipe", "w").write("audio=%s hmmnet=%s alignment=%s\n" % (d / "a.wav", d / "a.hmmnet", d / "a.phn"))
    return d


def run_stats(files, *extra):
    return subprocess.run([os.path.join(BIN, "stats"), "-b", str(files / "m"), "-c", str(files / "f.cfg"), "-r",
                           str(files / "net.recipe"), "-o", str(files / "o"), "--ml"] + list(extra),
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["--networks", "-a"], ["--networks", "-a", "-M", "bw"]], ids=["default", "bw"])
def test_minus_a_under_baum_welch_names_minus_m_vit(files, extra):
    r = run_stats(files, *extra)
    assert r.returncode == 1 and r.stderr.startswith("exception: stats: -a") and "-M vit" in r.stderr, r.stderr
    assert not os.path.exists(str(files / "o.lls")) and not os.path.exists(str(files / "a.phn"))


@pytest.mark.parametrize("extra", [["-a", "-O"], ["--networks", "-M", "vit", "-a", "-O"]], ids=["phn", "networks"])
def test_minus_a_with_minus_o_is_the_reference_message(files, extra):
    r = run_stats(files, *extra)
    assert r.returncode == 1 and r.stderr == "exception: Can not read and write to output PHNs\n", r.stderr


def test_an_accepted_minus_a_goes_on_to_the_device(capi, files):
    if capi.lib().aasr_device_count() > 0:
        return
    r = run_stats(files, "--networks", "-M", "vit", "-a", "-n")
    assert r.returncode == 1 and "stats:" not in r.stderr and "no HIP device available" in r.stderr, r.stderr

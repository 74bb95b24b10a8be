"""Baum-Welch statistics over HMM networks, the host side (no GPU): the new symbols and option defaults, what the stats
tool says about --networks before the device is opened, and the restatement (tools/stats_bw_restate.py) against an
enumeration of paths.

The enumeration: on the six-node network of tests/test_hmmnet_host.py every path from the initial to the final node is
walked; the expected statistics are the sum over the paths of (path probability) x (the statistics of the path's state
sequence with gamma 1, tools/fuzz_stats.py's restate).  The restatement takes the other route -- occupancies, the
per-frame sum and division, weighted accumulation.  Both are NumPy double sums of fewer than 100 terms, so they agree
within 1e-12 relative to the largest entry of each quantity."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402
import stats_bw_restate as BW  # noqa: E402

RS, FS = HC.RS, BW.FS
S = 12
SIX = ("I 0\nF 5\nT 0 1 , , -0.2\nT 0 2 #b , -0.9\nT 1 1 2\nT 1 3 3 , 0.4\nT 2 2 8\nT 2 3 9\nT 3 4 10 , -0.3\n"
       "T 3 5 11\nT 4 4 4\nT 4 5 5\n")
NEW_SYMBOLS = ["aasr_fb_batch_entries_dev", "aasr_fb_batch_entries_host", "aasr_fb_batch_frame_sums",
               "aasr_debug_fb_entries_shape", "aasr_stats_accumulate_weighted_dev", "aasr_stats_network_default_options",
               "aasr_run_stats_networks_recipe"]


def test_the_new_symbols_are_declared_and_exported(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name


def test_option_defaults(capi):
    fo = capi.FbOptions.defaults()
    assert fo.device_occ == 0 and (fo.fw_beam, fo.bw_beam, fo.max_attempts) == (15.0, 200.0, 5)
    # the network options travel in a struct of their own: aasr_stats_options ends with full_stats, as its callers know it
    assert [f[0] for f in capi.StatsOptions._fields_][-1] == "full_stats"
    no = capi.StatsNetworkOptions.defaults()
    assert (no.viterbi, no.fw_beam, no.bw_beam, no.ac_scale, no.ac_scale_given) == (0, 0.0, 0.0, 1.0, 0)
    assert [f[0] for f in capi.FbOptions._fields_][-2:] == ["force_global", "device_occ"]


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("T,ac", [(2, 1.0), (5, 1.0), (6, 0.5)])
def test_restatement_against_path_enumeration(viterbi, T, ac):
    sp = HC.self_probs(S)
    net = HC.parse(SIX, sp)
    assert net.n_nodes == 6
    rng = np.random.default_rng(100 * T + viterbi)
    model = FS.make_model(rng, 3, [2, 1, 3, 2, 2, 2, 1, 1, 2, 2, 1, 1], spare=1)
    off, w = model[2], model[4]
    mix_w = np.concatenate([w[off[s]:off[s + 1]] / w[off[s]:off[s + 1]].sum() for s in range(S)])
    x = rng.standard_normal((T, 3))
    ll = HC.scores(T, S, 11 * T)
    e = BW.entries(net, ll, 1e9, 1e9, ac, viterbi)
    assert e["status"] == RS.OK and e["result"].pruned == 0
    paths = BW.enumerate_paths(net, ll, ac)
    assert len(paths) < 100
    want_total = RS.brute_force(net, ll, ac, viterbi)
    m = max(p[0] for p in paths)
    got_total = m if viterbi else m + np.log(sum(np.exp(p[0] - m) for p in paths))
    assert abs(got_total - want_total) <= 1e-12 * abs(want_total)
    assert e["max_dev"] <= 1e-12 and e["min_positive_occ"] > 1e-200
    cnt, rows, weights = BW.group([e], [0], S)
    for t in range(T):                                   # a frame's weights sum to 1
        assert abs(weights[rows == t].sum() - 1.0) <= 4 * np.finfo(float).eps
    if viterbi:
        assert len(rows) == T and (weights == 1.0).all()
    got = BW.accumulate(model, mix_w, x, cnt, rows, weights)
    want = BW.path_weighted(net, ll, model, mix_w, x, ac, viterbi)
    for q, w_ in want.items():
        scale = np.abs(w_).max()
        err = np.abs(got[q] - w_).max()
        print(q, "largest entry %.3g, largest difference %.3g" % (scale, err))
        assert err <= 1e-12 * scale, (q, err, scale)
    # the counts: an entry counts once, however many paths share it
    assert got["count"].sum() == len(rows) and (got["count"] == np.diff(cnt)).all()


def test_group_order_is_pdf_then_utterance_then_frame():
    sp = HC.self_probs(S)
    a = BW.entries(HC.parse(HC.chain([3, 1]), sp), HC.scores(4, S, 1), 1e9, 1e9)
    b = BW.entries(HC.parse(HC.chain([1, 5]), sp), HC.scores(3, S, 2), 1e9, 1e9)
    bad = BW.entries(HC.parse(HC.chain([1, 2, 3, 4, 5]), sp), HC.scores(3, S, 3), 1e9, 1e9)
    assert bad["status"] == RS.FAILED_BACKWARD
    cnt, rows, weights = BW.group([a, bad, b], [0, 4, 7], S)
    assert cnt[0] == 0 and cnt[-1] == len(rows) == len(weights)
    assert set(np.nonzero(np.diff(cnt))[0]) == {1, 3, 5}
    r1 = rows[cnt[1]:cnt[2]]
    assert (r1 < 4).sum() > 0 and (r1 >= 7).sum() > 0 and not ((r1 >= 4) & (r1 < 7)).any()
    k = int((r1 < 4).sum())
    assert (np.diff(r1[:k]) > 0).all() and (np.diff(r1[k:]) > 0).all() and (r1[:k] < 4).all()   # utterance a, then b


# ---- the stats tool: what it says before the device is opened -------------------------------------------------------

@pytest.fixture
def files(capi, tmp_path):
    d = tmp_path
    open(d / "f.cfg", "w").write("module\n{\n  name audiofile\n  type audiofile\n  sample_rate 16000\n}\n")
    open(d / "m.gk", "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(d / "m.mc", "w").write("1\n1 0 1.0\n")
    HC.write_ph(str(d / "m.ph"), [0.5])
    open(d / "net.recipe", "w").write("audio=%s hmmnet=%s\n" % (d / "a.wav", d / "a.hmmnet"))
    open(d / "phn.recipe", "w").write("audio=%s transcript=%s\n" % (d / "a.wav", d / "a.phn"))
    return d


def run_stats(files, *extra, recipe="net.recipe"):
    return subprocess.run([os.path.join(BIN, "stats"), "-b", str(files / "m"), "-c", str(files / "f.cfg"), "-r",
                           str(files / recipe), "-o", str(files / "o"), "--ml"] + list(extra),
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,words", [
    (["--networks", "-M", "mpv"], ["-M mpv", "--networks"]),
    (["--networks", "--full-stats"], ["--full-stats", "--networks"]),
    (["--networks", "-O"], ["-O", "--networks"]),
])
def test_tool_refusals_with_networks(files, extra, words):
    r = run_stats(files, *extra)
    assert r.returncode == 1 and r.stderr.startswith("exception: stats: ") and "not supported" in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert "Aborted" not in r.stderr and not os.path.exists(str(files / "o.lls"))


def test_a_line_without_hmmnet_is_the_reference_message(files):
    r = run_stats(files, "--networks", recipe="phn.recipe")
    assert r.returncode == 1 and "exception: Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe." in r.stderr, r.stderr


def test_help_lists_networks_and_minus_h_points_to_it(files):
    r = subprocess.run([os.path.join(BIN, "stats"), "--help"], capture_output=True, text=True, timeout=60)
    line = [l for l in r.stdout.splitlines() if "--networks" in l and not l.startswith("usage")]
    assert r.returncode == 0 and len(line) == 1 and "hmmnet= networks" in line[0] and "-H" in line[0], r.stdout
    assert r.stdout.startswith("usage: stats [OPTION...] --ml [--full-stats | --networks]\n")
    r = run_stats(files, "-H")
    assert r.returncode == 1 and "-H" in r.stderr and "not supported" in r.stderr and r.stderr.rstrip().endswith("--networks"), r.stderr


def test_an_accepted_command_line_goes_on_to_the_device(capi, files):
    """the counterpart of the refusals: --networks with -M vit, beams and a scale is accepted, and without a device the
    run fails where the device is opened"""
    if capi.lib().aasr_device_count() > 0:
        return
    r = run_stats(files, "--networks", "-M", "vit", "-F", "20", "-W", "300", "-A", "0.5", "-t")
    assert r.returncode == 1 and "stats:" not in r.stderr and "no HIP device available" in r.stderr, r.stderr

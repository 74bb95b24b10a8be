"""CMLLR statistics over HMM networks, the host side (no GPU): the restatement (tools/mllr_bw_restate.py) against an
enumeration of paths and against its extended variant, what the mllr tool says about --networks before the device is
opened, and the new symbols.

The enumeration: on the six-node network of tests/test_stats_bw_host.py every path from the initial to the final node is
walked; the expected G, k and beta are the sum over the paths of (path probability) x (mllr_restate.collect along the
path's state sequence).  The restatement takes the other route -- occupancies, the per-frame sum and division, the
frame-major lists, collect_data once per (pdf, probability).  Both are NumPy double sums of fewer than 100 terms per
frame, so they agree within 1e-12 of the largest entry of each quantity: the bound of that file's enumeration."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402
import mllr_bw_restate as MB  # noqa: E402

MR, BW, RS, FS = MB.MR, MB.BW, MB.RS, MB.FS
S = 12
SIX = ("I 0\nF 5\nT 0 1 , , -0.2\nT 0 2 #b , -0.9\nT 1 1 2\nT 1 3 3 , 0.4\nT 2 2 8\nT 2 3 9\nT 3 4 10 , -0.3\n"
       "T 3 5 11\nT 4 4 4\nT 4 5 5\n")
TOL = {"G": 4 * 2.9e-14, "k": 4 * 5.0e-14, "beta": 4 * 9.7e-15}     # tests/test_mllr_gpu.py
NEW_SYMBOLS = ["aasr_fb_batch_frame_entries_dev", "aasr_fb_batch_frame_entries_host", "aasr_debug_fb_frame_entries_shape",
               "aasr_mllr_accumulate_weighted_dev", "aasr_mllr_network_default_options", "aasr_run_mllr_networks_recipe"]


def errs(got, want):
    return {"G": MR.rel_err(got[0], want[0]), "k": MR.rel_err(got[1], want[1]),
            "beta": abs(float(got[2]) - float(want[2])) / max(float(want[2]), 1e-300)}


def six_case(T, viterbi):
    sp = HC.self_probs(S)
    net = HC.parse(SIX, sp)
    assert net.n_nodes == 6
    rng = np.random.default_rng(100 * T + viterbi)
    model = FS.make_model(rng, 3, [2, 1, 3, 2, 2, 2, 1, 1, 2, 2, 1, 1], spare=1)
    x = rng.standard_normal((T, 3))
    ll = HC.scores(T, S, 11 * T)
    return net, model, x, ll


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("T,ac", [(2, 1.0), (5, 1.0), (6, 0.5)])
def test_restatement_against_path_enumeration(viterbi, T, ac):
    net, model, x, ll = six_case(T, viterbi)
    e = BW.entries(net, ll, 1e9, 1e9, ac, viterbi)
    assert e["status"] == RS.OK and e["result"].pruned == 0
    assert len(BW.enumerate_paths(net, ll, ac)) < 100
    assert e["max_dev"] <= 1e-12 and e["min_positive_occ"] > 1e-200
    lists = MB.frame_lists([e], [0], T)
    for l in lists:                                      # a frame's weights sum to 1, its pdfs in pdf-list order
        assert abs(sum(w for _, w in l) - 1.0) <= 4 * np.finfo(float).eps
        slots = [e["pdfs"].index(p) for p, _ in l]
        assert slots == sorted(slots) and len(set(slots)) == len(slots)
    if viterbi:
        assert all(len(l) == 1 and l[0][1] == 1.0 for l in lists)
    got = MB.collect(model, x, lists)
    want = MB.path_weighted(net, ll, model, x, ac, viterbi)
    for q, g_, w_ in zip(("G", "k", "beta"), got, want):
        scale = np.abs(w_).max()
        err = np.abs(np.asarray(g_) - w_).max()
        print(q, "largest entry %.3g, largest difference %.3g" % (scale, err))
        assert err <= 1e-12 * scale, (q, err, scale)
    # the flat arrays are the lists again, and the same entries as the pdf-major grouping
    off, pdf, weight = MB.flatten(lists)
    assert MB.unflatten(off, pdf, weight) == lists
    cnt, rows, weights = BW.group([e], [0], S)
    frame_of = np.repeat(np.arange(T), np.diff(off))
    a = sorted(zip(pdf.tolist(), frame_of.tolist(), weight.tolist()))
    b = sorted(zip(np.repeat(np.arange(S), np.diff(cnt)).tolist(), rows.tolist(), weights.tolist()))
    assert a == b


def test_one_entry_of_weight_one_is_the_phn_restatement():
    rng = np.random.default_rng(7)
    model, x, pdf = MR.make_case(rng, 5, [3, 1, 2], [40, 30, 20], skipped=6)
    lists = [[(int(p), 1.0)] if p >= 0 else [] for p in pdf]
    for a, b in zip(MB.collect(model, x, lists), MR.collect(model, x, pdf)):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def random_lists(rng, n, S_, most=6, long_at=None, long_len=40):
    lists = []
    for f in range(n):
        m = long_len if f == long_at else int(rng.integers(0, most + 1))
        w = rng.uniform(0.05, 1.0, m)
        w = w / w.sum() if m else w
        lists.append([(int(rng.integers(0, S_)), float(w[j])) for j in range(m)])
    return lists


@pytest.mark.parametrize("D,n", [(1, 150), (15, 200), (39, 300)])
def test_restatement_against_its_extended_variant(D, n):
    rng = np.random.default_rng(500 + D)
    model, x, _ = MR.make_case(rng, D, [4, 1, 3, 2], [n // 4] * 4)
    lists = random_lists(rng, len(x), 4, long_at=len(x) // 2)
    lists[3].append((-1, 0.5))                           # an entry the model does not have: skipped by both
    lists[4].append((4, 0.5))
    e = errs(MB.collect(model, x, lists), MB.collect(model, x, lists, extended=True))
    print("restatement against extended sums", {q: "%.3g" % v for q, v in e.items()})
    assert all(e[q] <= TOL[q] for q in TOL), e


# ---- the mllr tool: what it says before the device is opened --------------------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mllr_bw_host")
    open(str(d / "m.gk"), "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(str(d / "m.mc"), "w").write("1\n1 0 1.0\n")
    HC.write_ph(str(d / "m.ph"), [0.5])
    open(str(d / "f.cfg"), "w").write("module\n{\n  name a\n  type audiofile\n}\n")
    open(str(d / "net.rcp"), "w").write("audio=%s hmmnet=%s speaker=s1\n" % (d / "a.wav", d / "a.hmmnet"))
    open(str(d / "phn.rcp"), "w").write("audio=%s transcript=%s speaker=s1\n" % (d / "a.wav", d / "a.phn"))
    open(str(d / "s.spkc"), "w").write("speaker default\n{\n}\n")
    return d


def run_tool(files, *extra, recipe="net.rcp"):
    cmd = [os.path.join(BIN, "mllr"), "-b", str(files / "m"), "-c", str(files / "f.cfg"), "-r", str(files / recipe),
           "-S", str(files / "s.spkc")] + list(extra)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("extra,words", [
    (["--networks", "--segmode", "mpv"], ["--segmode mpv", "--networks"]),
    (["--networks", "-O"], ["-O", "--networks"]),
])
def test_tool_refusals_with_networks(capi, files, extra, words):
    r = run_tool(files, *extra)
    assert r.returncode == 1 and r.stderr.startswith("exception: mllr: ") and "not supported" in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert "hip" not in r.stderr.lower() and "Aborted" not in r.stderr


def test_a_line_without_hmmnet_is_the_reference_message(capi, files):
    r = run_tool(files, "--networks", recipe="phn.rcp")
    assert r.returncode == 1 and "exception: Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe." in r.stderr, r.stderr
    assert "hip" not in r.stderr.lower()


def test_minus_h_stays_refused_and_points_to_networks(capi, files):
    r = run_tool(files, "-H")
    assert r.returncode == 1 and "exception: mllr: -H" in r.stderr and "not supported" in r.stderr and "--networks" in r.stderr
    r = run_tool(files, "--segmode", "vit")              # without --networks: refused as before
    assert r.returncode == 1 and "exception: mllr: --segmode" in r.stderr and "not supported" in r.stderr
    r = subprocess.run([os.path.join(BIN, "mllr"), "--help"], capture_output=True, text=True, timeout=60)
    line = [l for l in r.stdout.splitlines() if "--networks" in l]
    assert r.returncode == 0 and len(line) == 1 and "hmmnet= networks" in line[0] and "-H" in line[0], r.stdout


def test_an_accepted_command_line_reaches_the_device_and_fails_there(capi, files):
    """the counterpart of the refusals: --networks with --segmode vit and beams is accepted and goes on to open the
    device, which the run does not have"""
    r = run_tool(files, "--networks", "--segmode", "vit", "-F", "20", "-W", "300")
    assert r.returncode == 1 and "mllr:" not in r.stderr and "unknown option" not in r.stderr.lower(), r.stderr
    assert "networks" not in r.stderr, r.stderr


# ---- the library ----------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_declared_and_exported(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
    # the network options travel in a struct of their own: aasr_mllr_options ends with out, as its callers know it
    assert [f[0] for f in capi.MllrOptions._fields_][-1] == "out"
    no = capi.MllrNetworkOptions.defaults()
    assert (no.networks, no.viterbi, no.fw_beam, no.bw_beam) == (0, 0, 0.0, 0.0)


def test_without_handles_the_calls_name_themselves(capi):
    L = capi.lib()
    n = ctypes.c_int64(7)
    p = [ctypes.c_void_p(1) for _ in range(3)]
    assert L.aasr_fb_batch_frame_entries_dev(None, 1, None, 0, None, ctypes.byref(n), ctypes.byref(p[0]), ctypes.byref(p[1]),
                                             ctypes.byref(p[2])) == capi.AASR_ERR_INVALID
    assert b"aasr_fb_batch_frame_entries_dev" in L.aasr_last_error()
    assert L.aasr_fb_batch_frame_entries_host(None, None, None, None) == capi.AASR_ERR_INVALID
    assert b"aasr_fb_batch_frame_entries_host" in L.aasr_last_error()
    assert L.aasr_mllr_accumulate_weighted_dev(None, None, 0, None, None, None, 0, None) == capi.AASR_ERR_INVALID
    assert b"aasr_mllr_accumulate_weighted_dev" in L.aasr_last_error()
    assert L.aasr_run_mllr_networks_recipe(None, None, None, None, None, None, None) == capi.AASR_ERR_INVALID
    assert b"aasr_run_mllr_networks_recipe" not in L.aasr_last_error()          # no network options: the .phn call's name
    sh = (ctypes.c_int32 * 5)(*[9] * 5)
    L.aasr_debug_fb_frame_entries_shape(None, sh)
    assert list(sh) == [9] * 5


def test_the_new_entry_points_need_the_device(capi, tmp_path):
    """without a device the frame entries and the weighted accumulation are AASR_ERR_NO_DEVICE where their handles are
    made: the batch and the model (no fallback)"""
    if capi.lib().aasr_device_count() > 0:
        return
    HC.write_ph(str(tmp_path / "m.ph"), HC.self_probs(S))
    open(str(tmp_path / "a.hmmnet"), "w").write(HC.chain([1, 2]))
    net = capi.HmmNet(capi.Topology(str(tmp_path / "m.ph")), str(tmp_path / "a.hmmnet"))
    with pytest.raises(capi.AasrError) as ei:
        capi.fb_batch_frame_entries([net], [4], np.zeros((4, S)), [0], S)
    assert ei.value.code == capi.AASR_ERR_NO_DEVICE
    rng = np.random.default_rng(1)
    with pytest.raises(capi.AasrError) as ei:
        capi.Gmm.from_arrays(rng.normal(size=(2, 3)), np.ones((2, 3)), np.arange(7, dtype=np.int32), np.zeros(6, np.int32),
                             np.ones(6))
    assert ei.value.code == capi.AASR_ERR_NO_DEVICE

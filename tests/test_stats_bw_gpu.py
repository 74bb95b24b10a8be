"""stats --networks (csrc/stats.cc, csrc/aku/main_stats.cc): Baum-Welch statistics over the recipe's HMM networks on the
device, against tools/stats_bw_restate.py.

The fixture is that of tests/test_logl_gpu.py: 2 s of audio, the production feature chain, 30 states in HMMs of three;
three utterances (windows of 40, 60 and 45 frames) over a chain, a fan and another chain.  The restatement runs on the
oracle's double state likelihoods and the engine's own f64 features; the tool runs under AASR_PREC=1 unless a test says
otherwise.

Bounds.  .gks / .mcs: those that tests/test_stats_gpu.py::check_against holds the .phn mode to, written out in
tools/stats_bw_restate.py::compare_dumps (feacount and the accumulated sets exact; gamma, aux gamma 1e-12 relative; sum
x / sum x^2 one float ulp; component gammas 1e-9 relative + 1e-12; mixture_ll 1e-9 relative).  .phs: within 1e-9 x
frames of the restatement's count as the file can hold it -- HmmSet::dump_ph_statistics prints six significant digits,
so the restatement's count is rounded to them first.  .lls: the total of logl -H on the same files to the six decimals
that logl prints, the frame count the sum of the frame ranges.  In the default precision the total is held to the bound
tests/test_logl_gpu.py uses for it (5e-3 + 1e-6 |want|)."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hmmnet_cases as HC  # noqa: E402
import stats_bw_restate as BW  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
S, PER = 30, 3
Q = [h * PER + j for h in (3, 0, 7, 2, 5, 1, 9, 6) for j in range(PER)]
SPANS = ((0.4, 0.72), (0.8, 1.28), (1.36, 1.72))
PREC64 = {"AASR_PREC": "1"}
WIDE = ("-F", "1e9", "-W", "1e9")


class World:
    pass


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = World()
    w.dir = d = tmp_path_factory.mktemp("stats_bw")
    rng = np.random.default_rng(41)
    cfg_text = synth.make_feature_config()
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(cfg_text)
    pcm = synth.make_audio(16000 * 2, seed=73)
    w.wav = str(d / "a.wav")
    with wave.open(w.wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.astype("<i2").tobytes())
    ft = capi.Feat(cfg_text)
    w.fr = ft.frame_rate
    w.T = T = ft.eof_frame(len(pcm))
    w.fea = ft.run(pcm, 0, T, dtype=np.float64)
    mean, var, off, idx, mw = synth.make_model(D=39, G=90, S=S, comps=3, seed=27)
    mean[:] = w.fea[rng.integers(0, T, 90)] + 0.3 * rng.standard_normal((90, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    w.model = (mean, var, off, idx, mw)
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    dm = oracle.DiagModel(mean, var, off, idx, mw)
    w.mix_w = dm.mix_w
    w.ll = dm.score(w.fea)
    w.sp = np.full(S, 0.5)
    w.topo = capi.Topology(w.base + ".ph")
    w.windows = [tuple(capi.recipe_frame_limits(a, b, w.fr)) for a, b in SPANS]
    assert [b - a for a, b in w.windows] == [40, 60, 45], w.windows
    w.texts = [HC.chain(Q[:9]), HC.fan(S, 3, 4, seed=1), HC.chain(Q[9:18])]
    w.nets = []
    for i, t in enumerate(w.texts):
        w.nets.append(str(d / ("n%d.hmmnet" % i)))
        open(w.nets[-1], "w").write(t)
    w.recipe = write_recipe(w, "three.recipe", list(zip(SPANS, w.nets)))
    return w


def write_recipe(w, name, lines):
    path = str(w.dir / name)
    open(path, "w").write("".join("audio=%s hmmnet=%s start-time=%s end-time=%s\n" % (w.wav, net, a, b) for (a, b), net in lines))
    return path


def run(w, exe, recipe, *flags, out=None, env=None):
    cmd = [os.path.join(BIN, exe), "-b", w.base, "-c", w.cfg, "-r", recipe, "-i", "1"] + list(flags)
    if out:
        cmd += ["-o", out, "--ml", "--networks"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def restate(w, windows, texts, **kw):
    """the statistics of stats --networks -t over the lines, in double"""
    utts = [BW.entries(HC.parse(t, w.sp), w.ll[a:b], **kw) for (a, b), t in zip(windows, texts)]
    row0 = np.concatenate([[0], np.cumsum([b - a for a, b in windows])])[:-1]
    x = np.concatenate([w.fea[a:b] for a, b in windows])
    cnt, rows, weights = BW.group(utts, row0, S)
    want = BW.accumulate(w.model, w.mix_w, x, cnt, rows, weights)
    want["tr"] = np.zeros(2 * S)
    want["lls"], want["frames"] = 0.0, 0
    for e, (a, b), t in zip(utts, windows, texts):
        if e["status"] != RS.OK:
            continue
        net = HC.parse(t, w.sp)
        for k, tr in enumerate(net.transitions):
            want["tr"][tr] += e["result"].tr_occ[k]
        want["lls"] += e["result"].forward_total
        want["frames"] += b - a
    want["utts"] = utts
    return want


def read_lls(out):
    lines = open(out + ".lls").read().split("\n")
    assert lines[0].startswith("Numerator loglikelihood: ") and lines[1].startswith("Number of frames: ")
    return float(lines[0].split(": ")[1]), int(lines[1].split(": ")[1])


def check_phs(out, want):
    rows = open(out + ".phs").read().splitlines()
    assert int(rows[0]) == 2 * S
    got = [(int(a), int(b), float(c)) for a, b, c in (r.split() for r in rows[1:])]
    expect = [(t, want["tr"][t]) for t in range(2 * S) if want["tr"][t] > 0]
    assert [g[0] for g in got] == [t // 2 for t, _ in expect]
    worst = 0.0
    for (_, _, c), (t, v) in zip(got, expect):
        worst = max(worst, abs(c - float("%g" % v)))
    print("phs: largest difference from the restatement's printed count %.3g" % worst)
    assert worst <= 1e-9 * want["frames"]
    assert abs(sum(c for _, _, c in got) - want["frames"]) <= 1e-4 * want["frames"]   # one transition a frame


def check_dumps(w, out, want, what):
    worst = {}
    fails = BW.compare_dumps(out, want, w.model, worst)
    print(what, "worst difference in units of the bound", {k: "%.3g" % v for k, v in worst.items()})
    assert not fails, "\n".join(fails[:12])


def test_the_tool_against_the_restatement(world, tmp_path):
    w = world
    want = restate(w, w.windows, w.texts, fw_beam=1e9, bw_beam=1e9)
    for e in want["utts"]:
        assert e["status"] == RS.OK and e["min_positive_occ"] > 1e-200
    out = str(tmp_path / "o")
    r = run(w, "stats", w.recipe, "-t", *WIDE, out=out, env=PREC64)
    check_dumps(w, out, want, "wide")
    check_phs(out, want)
    total, frames = read_lls(out)
    assert frames == sum(b - a for a, b in w.windows) == want["frames"]
    assert abs(total - want["lls"]) <= 2e-6 + 1e-12 * abs(want["lls"])
    lg = run(w, "logl", w.recipe, "-H", *WIDE, env=PREC64)
    logl_total = float(lg.stdout.strip().splitlines()[-1].split(":")[-1])
    print("lls %.12g logl %f" % (total, logl_total))
    assert abs(total - logl_total) <= 1e-6                      # logl prints six decimals
    per = [l for l in r.stderr.splitlines() if l.startswith("  ")]
    assert len(per) == 3 and "Could not" not in r.stderr and "Warning" not in r.stderr, r.stderr
    assert r.stderr.count("Processing file: ") == 3 and "Finished collecting statistics (0/0)\n" in r.stderr
    out2 = str(tmp_path / "p")                                   # a second run writes the same bytes
    run(w, "stats", w.recipe, "-t", *WIDE, out=out2, env=PREC64)
    for ext in (".gks", ".mcs", ".phs", ".lls"):
        assert open(out + ext, "rb").read() == open(out2 + ext, "rb").read(), ext


def test_default_precision_and_default_beams(world, tmp_path):
    w = world
    want = restate(w, w.windows, w.texts, fw_beam=15.0, bw_beam=200.0)
    out = str(tmp_path / "o")
    r = run(w, "stats", w.recipe, "-t", out=out)
    total, frames = read_lls(out)
    print("default precision: lls %.9f want %.9f" % (total, want["lls"]))
    assert frames == want["frames"] and abs(total - want["lls"]) <= 5e-3 + 1e-6 * abs(want["lls"])
    line = [l for l in r.stderr.splitlines() if l.startswith("Largest |1 - sum of PDF probabilities| of a frame: ")]
    assert len(line) == 1, r.stderr
    dev = max(e["max_dev"] for e in want["utts"])
    print("max |1 - s_t|: tool %s restatement %.3g" % (line[0].split(": ")[1], dev))
    # no frame drew the reference's warning (|1 - s_t| > 0.02), on either side
    assert "Warning: Sum of PDF probabilities" not in r.stderr and dev <= 0.02 and 0.0 <= float(line[0].split(": ")[1]) <= 0.02
    for ext in (".gks", ".mcs", ".phs"):
        assert os.path.exists(out + ext)


@pytest.mark.parametrize("flags,kw", [(("-M", "vit"), dict(viterbi=True)), (("-A", "0.5"), dict(ac_scale=0.5))],
                         ids=["viterbi", "ac-scale"])
def test_viterbi_and_acoustic_scale(world, tmp_path, flags, kw):
    w = world
    want = restate(w, w.windows, w.texts, fw_beam=1e9, bw_beam=1e9, **kw)
    out = str(tmp_path / "o")
    run(w, "stats", w.recipe, "-t", *WIDE, *flags, out=out, env=PREC64)
    check_dumps(w, out, want, " ".join(flags))
    check_phs(out, want)
    total, frames = read_lls(out)
    assert frames == want["frames"] and abs(total - want["lls"]) <= 2e-6 + 1e-12 * abs(want["lls"])
    if "viterbi" in kw:
        assert want["count"].sum() == want["frames"]            # one entry a frame


def test_no_train_writes_only_lls(world, tmp_path):
    w = world
    out = str(tmp_path / "n")
    run(w, "stats", w.recipe, "-t", "-n", *WIDE, out=out, env=PREC64)
    assert os.path.exists(out + ".lls") and not any(os.path.exists(out + e) for e in (".gks", ".mcs", ".phs"))
    want = restate(w, w.windows, w.texts, fw_beam=1e9, bw_beam=1e9)
    total, frames = read_lls(out)
    assert frames == want["frames"] and abs(total - want["lls"]) <= 2e-6 + 1e-12 * abs(want["lls"])


def test_batches_add_up(world, tmp_path):
    """-B 2 -I 1 plus -I 2 against the single run, under the bounds of tests/test_stats_gpu.py's batches test: counts
    exactly, gamma 1e-12 relative, the floats within the ulps of the values added, mixture values 1e-9"""
    w = world
    whole = str(tmp_path / "all")
    run(w, "stats", w.recipe, "-t", *WIDE, out=whole, env=PREC64)
    parts = []
    for k in (1, 2):
        parts.append(str(tmp_path / ("b%d" % k)))
        r = run(w, "stats", w.recipe, "-t", *WIDE, "-B", "2", "-I", str(k), out=parts[-1], env=PREC64)
        assert "Finished collecting statistics (%d/2)\n" % k in r.stderr
    g_whole = BW.read_gks(whole + ".gks")[1]
    g_parts = [BW.read_gks(p + ".gks")[1] for p in parts]
    assert set(g_whole) == set(g_parts[0]) | set(g_parts[1])
    ulp = lambda v: np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)
    for g, (fc, gam, aux, sx, sxx) in g_whole.items():
        got = [p[g] for p in g_parts if g in p]
        assert sum(x[0] for x in got) == fc
        assert sum(x[1] for x in got) == pytest.approx(gam, rel=1e-12)
        assert sum(x[2] for x in got) == pytest.approx(aux, rel=1e-12)
        for j, whole_v in ((3, sx), (4, sxx)):
            lim = ulp(whole_v) + sum(ulp(x[j]) for x in got)
            assert (np.abs(sum(x[j] for x in got) - whole_v) <= lim).all(), g
    m_whole = BW.read_mcs(whole + ".mcs")[1]
    m_parts = [BW.read_mcs(p + ".mcs")[1] for p in parts]
    assert set(m_whole) == set(m_parts[0]) | set(m_parts[1])
    for p, f in m_whole.items():
        got = [m[p] for m in m_parts if p in m]
        for i in range(3, len(f) - 2, 2):
            assert sum(float(x[i]) for x in got) == pytest.approx(float(f[i]), rel=1e-9, abs=1e-12)
        assert sum(float(x[-1]) for x in got) == pytest.approx(float(f[-1]), rel=1e-9)
    lls = [read_lls(p) for p in parts]
    tw, fw = read_lls(whole)
    assert sum(x[1] for x in lls) == fw and sum(x[0] for x in lls) == pytest.approx(tw, rel=1e-9)


def test_a_single_path_network_is_the_phn_mode_byte_for_byte(world, capi, tmp_path):
    """12 states left to right without self loops over 12 frames: every frame has one pdf and occ / s_t is exactly 1.0,
    so the entries are the .phn path's row list and .gks / .mcs come out as identical bytes (.phs is not compared: the
    .phn reader counts no transition on the last frame)"""
    w = world
    states = Q[:12]
    text = "#FSTBasic MaxPlus\nI 0\nF 12\n" + "".join("T %d %d %d\n" % (i, i + 1, 2 * s + 1) for i, s in enumerate(states))
    net = str(tmp_path / "line.hmmnet")
    open(net, "w").write(text)
    first, last = capi.recipe_frame_limits(0.4, 0.496, w.fr)
    assert (first, last) == (50, 62)
    phn = str(tmp_path / "line.phn")
    with open(phn, "w") as f:
        for i, s in enumerate(states):
            f.write("%d %d h%d.%d\n" % ((first + i) * 128, (first + i + 1) * 128, s // PER, s % PER))
    seg = capi.stats_read_segmentation(w.topo, phn, w.fr, first, last, w.T, False)
    assert seg[0] == first and seg[1].tolist() == states
    rn = str(tmp_path / "net.recipe")
    open(rn, "w").write("audio=%s hmmnet=%s start-time=0.4 end-time=0.496\n" % (w.wav, net))
    rp = str(tmp_path / "phn.recipe")
    open(rp, "w").write("audio=%s transcript=%s start-time=0.4 end-time=0.496\n" % (w.wav, phn))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run(w, "stats", rn, *WIDE, out=a, env=PREC64)
    cmd = [os.path.join(BIN, "stats"), "-b", w.base, "-c", w.cfg, "-r", rp, "-o", b, "--ml"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **PREC64))
    assert r.returncode == 0, r.stderr
    assert len(BW.read_gks(a + ".gks")[1]) > 0 and read_lls(a)[1] == 12 == read_lls(b)[1]
    for ext in (".gks", ".mcs"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext


def test_retries_and_giving_up(world, tmp_path):
    """The fixture of tests/test_logl_gpu.py's retry test: next to the real path of three states runs a branch of 45 states
    -- the best state of every frame -- that is longer than the 40 frames, so it sets each frame's best backward score
    and never reaches the initial node.  W is taken from the restatement's pruning-margin report: the first candidate at
    which it fails at W, succeeds at 2 W and keeps every pruning comparison of both runs 0.05 from its threshold."""
    w = world
    a, b_ = w.windows[0]
    ll = w.ll[a:b_]
    order = np.argsort(ll.sum(axis=0))
    real = [int(order[0]), int(order[1]), int(order[2])]
    decoy = [int(ll[max(0, min(39, 39 - k))].argmax()) for k in range(44, -1, -1)]
    bld = HC.Builder()
    init, fin = bld.node(), bld.node()
    for states in (real, decoy):
        nodes = [bld.node() for _ in states]
        bld.eps(init, nodes[0])
        for i, s in enumerate(states):
            bld.emit(nodes[i], nodes[i], 2 * s)
            bld.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else fin, 2 * s + 1)
    text = bld.text(init, fin)
    net = str(tmp_path / "retry.hmmnet")
    open(net, "w").write(text)
    rnet = HC.parse(text, w.sp)
    chosen = None
    for W in [round(10 * 1.12 ** k, 1) for k in range(40)]:
        r1 = RS.forward_backward(rnet, ll, 1e9, float(W))
        r2 = RS.forward_backward(rnet, ll, 1e9, 2.0 * W)
        if r1.status == RS.FAILED_BACKWARD and r2.status == RS.OK and min(r1.min_margin, r2.min_margin) >= 0.05:
            chosen = (W, r2.forward_total)
            break
    assert chosen, "no backward beam separates the two runs on this fixture"
    W, want = chosen
    recipe = write_recipe(w, "retry.recipe", [(SPANS[0], net)])
    out = str(tmp_path / "r")
    r = run(w, "stats", recipe, "-F", "1e9", "-W", str(W), out=out)
    assert r.stderr.count("Could not initialize the utterance segmentation.\n") == 1
    assert [l for l in r.stderr.splitlines() if l.startswith("Increasing beam to")] == ["Increasing beam to %.1f" % (2.0 * W)]
    assert "Giving up" not in r.stderr
    total, frames = read_lls(out)
    assert frames == 40 and abs(total - want) <= 5e-3 + 1e-6 * abs(want)
    # a chain longer than its frames never initialises: four wider beams, then the reference gives up; status 0
    long_net = str(tmp_path / "long.hmmnet")
    open(long_net, "w").write(HC.chain([s % S for s in range(45)]))
    recipe = write_recipe(w, "long.recipe", [(SPANS[0], long_net), (SPANS[2], w.nets[2])])
    out = str(tmp_path / "g")
    r = run(w, "stats", recipe, *WIDE, out=out)
    assert r.stderr.count("Could not initialize the utterance segmentation.\n") == 1
    assert r.stderr.count("Increasing beam to") == 4 and r.stderr.count("Giving up for this file\n") == 1
    total, frames = read_lls(out)
    one = restate(w, [w.windows[2]], [w.texts[2]], fw_beam=1e9, bw_beam=1e9)
    assert frames == 45 and abs(total - one["lls"]) <= 5e-3 + 1e-6 * abs(one["lls"])   # the given-up utterance adds nothing
    mcs = BW.read_mcs(out + ".mcs")[1]
    assert set(mcs) == set(np.nonzero(one["count"])[0].tolist())

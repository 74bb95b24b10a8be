"""stats --networks -M vit -a (csrc/stats.cc, csrc/aku/main_stats.cc): the alignment files of the best paths, written by the
tool on the device, against tools/align_restate.py; and dur_est over the written files.

The fixture is that of tests/test_stats_bw_gpu.py (2 s of audio, the production feature chain, 30 states in HMMs of three,
windows of 40, 60 and 45 frames) with networks small enough to enumerate: a chain of one HMM's three states (741 paths), two
labelled branches of two states that share their first pdf (118 paths), a chain of four states over two HMMs (13 244 paths).
Every arc carries the label ";state;hmm", so a frame is called "hmm.state" and dur_est can read the files.  The restatement
runs on the oracle's double state likelihoods, the tool under AASR_PREC=1 with wide beams; the fixture asserts that each
best path leads its runner-up by 1e-6 or more, seven orders above what the two sides' scores differ by, so the texts are
compared as bytes."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import align_restate as AR  # noqa: E402
import dur_est_restate as DR  # noqa: E402
import hmmnet_cases as HC  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
S, PER = 30, 3
SPANS = ((0.4, 0.72), (0.8, 1.28), (1.36, 1.72))
PREC64 = {"AASR_PREC": "1"}
WIDE = ("-F", "1e9", "-W", "1e9")
HMM_STATES = {"h%d" % h: [h * PER + j for j in range(PER)] for h in range(S // PER)}


class World:
    pass


def labelled(b, nodes, states, last):
    for i, s in enumerate(states):
        lab = ";%d;h%d" % (s % PER, s // PER)
        b.emit(nodes[i], nodes[i], 2 * s, 0.0, lab)
        b.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else last, 2 * s + 1, 0.0, lab + "#")


def chain(states):
    b = HC.Builder()
    init = b.node()
    nodes = [b.node() for _ in states]
    fin = b.node()
    b.eps(init, nodes[0])
    labelled(b, nodes, states, fin)
    return b.text(init, fin)


def branches(first, second):
    b = HC.Builder()
    init, merge, fin = b.node(), b.node(), b.node()
    for states, score in ((first, -0.3), (second, -0.1)):
        nodes = [b.node() for _ in states]
        b.eps(init, nodes[0], score)
        labelled(b, nodes, states, merge)
    b.eps(merge, fin)
    return b.text(init, fin)


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = World()
    w.dir = d = tmp_path_factory.mktemp("stats_align")
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
    T = ft.eof_frame(len(pcm))
    fea = ft.run(pcm, 0, T, dtype=np.float64)
    mean, var, off, idx, mw = synth.make_model(D=39, G=90, S=S, comps=3, seed=27)
    mean[:] = fea[rng.integers(0, T, 90)] + 0.3 * rng.standard_normal((90, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    w.ll = oracle.DiagModel(mean, var, off, idx, mw).score(fea)
    w.sp = np.full(S, 0.5)
    w.windows = [tuple(capi.recipe_frame_limits(a, b, w.fr)) for a, b in SPANS]
    assert [b - a for a, b in w.windows] == [40, 60, 45], w.windows
    w.texts = [chain([9, 10, 11]), branches([3, 4], [3, 17]), chain([21, 22, 6, 7])]
    w.nets, w.paths, w.want = [], [], []
    for i, (t, (a, b)) in enumerate(zip(w.texts, w.windows)):
        w.nets.append(str(d / ("n%d.hmmnet" % i)))
        open(w.nets[-1], "w").write(t)
        net = HC.parse(t, w.sp)
        r = RS.forward_backward(net, w.ll[a:b], 1e9, 1e9, viterbi=True)
        best, gap = AR.best_two_paths(net, w.ll[a:b])
        print("utterance", i, "gap to the runner-up %.6g" % gap)
        assert r.status == RS.OK and r.path == best and gap >= 1e-6        # a condition on the fixture, never a skip
        w.paths.append(r)
        w.want.append(AR.alignment_text(r.path, AR.arc_labels(t), a, w.fr))
    return w


def write_recipe(w, path, lines):
    """lines: (span, network, alignment file)"""
    open(path, "w").write("".join("audio=%s hmmnet=%s alignment=%s start-time=%s end-time=%s\n" % (w.wav, net, al, a, b)
                                  for (a, b), net, al in lines))
    return path


def run_stats(w, recipe, out, *flags):
    cmd = [os.path.join(BIN, "stats"), "-b", w.base, "-c", w.cfg, "-r", recipe, "-i", "1", "-o", out, "--ml", "--networks",
           "-M", "vit", *WIDE] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **PREC64))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def read_lls(out):
    lines = open(out + ".lls").read().split("\n")
    return float(lines[0].split(": ")[1]), int(lines[1].split(": ")[1])


def test_a_with_no_train_writes_the_restated_text_and_lls_and_no_dumps(world, tmp_path):
    w = world
    als = [str(tmp_path / ("u%d.phn" % i)) for i in range(3)]
    recipe = write_recipe(w, str(tmp_path / "r.recipe"), list(zip(SPANS, w.nets, als)))
    out = str(tmp_path / "o")
    r = run_stats(w, recipe, out, "-a", "-n")
    for i in range(3):
        got = open(als[i]).read()
        print("utterance", i, "lines", got.count("\n"))
        assert got == w.want[i], (i, got, w.want[i])
    # what the text must show: absolute sample numbers, "hmm.state" labels, the "+1" on the last line
    a, b = w.windows[0]
    rows = [l.split() for l in w.want[0].splitlines()]
    assert int(rows[0][0]) == a * 128 and int(rows[-1][1]) == (b + 1) * 128 and [x[2] for x in rows] == ["h3.0", "h3.1", "h3.2"]
    assert {l.split()[2] for l in w.want[1].splitlines()} in ({"h1.0", "h1.1"}, {"h1.0", "h5.2"})
    assert not any(os.path.exists(out + e) for e in (".gks", ".mcs", ".phs"))
    total, frames = read_lls(out)
    want = sum(p.forward_total for p in w.paths)
    assert frames == 145 and abs(total - want) <= 2e-6 + 1e-12 * abs(want)         # the bound of tests/test_stats_bw_gpu.py
    assert "Could not" not in r.stderr


def test_dumps_are_the_bytes_of_a_run_without_a(world, tmp_path):
    w = world
    als = [str(tmp_path / ("u%d.phn" % i)) for i in range(3)]
    recipe = write_recipe(w, str(tmp_path / "r.recipe"), list(zip(SPANS, w.nets, als)))
    with_a, without = str(tmp_path / "a"), str(tmp_path / "b")
    run_stats(w, recipe, with_a, "-a", "-t")
    assert [open(p).read() for p in als] == w.want
    for p in als:
        os.remove(p)
    run_stats(w, recipe, without, "-t")
    assert not any(os.path.exists(p) for p in als)                                  # no -a: no alignment files
    for ext in (".gks", ".mcs", ".phs", ".lls"):
        x, y = open(with_a + ext, "rb").read(), open(without + ext, "rb").read()
        assert len(x) > 0 and x == y, ext


def test_a_given_up_utterance_leaves_an_empty_file_and_an_unwritable_one_is_reported(world, tmp_path):
    w = world
    long_net = str(tmp_path / "long.hmmnet")
    open(long_net, "w").write(chain([s % S for s in range(45)]))                      # 45 states, 40 frames: never initialises
    als = [str(tmp_path / "gone.phn"), str(tmp_path / "nowhere" / "x.phn"), str(tmp_path / "ok.phn")]
    recipe = write_recipe(w, str(tmp_path / "r.recipe"),
                          [(SPANS[0], long_net, als[0]), (SPANS[1], w.nets[1], als[1]), (SPANS[2], w.nets[2], als[2])])
    out = str(tmp_path / "o")
    r = run_stats(w, recipe, out, "-a", "-n")
    assert r.stderr.count("Giving up for this file\n") == 1
    assert os.path.exists(als[0]) and open(als[0]).read() == ""
    assert "Could not open alignment file %s\n" % als[1] in r.stderr and not os.path.exists(als[1])
    assert open(als[2]).read() == w.want[2]
    total, frames = read_lls(out)
    want = w.paths[1].forward_total + w.paths[2].forward_total                        # the unwritable utterance still counts
    assert frames == 105 and abs(total - want) <= 2e-6 + 1e-12 * abs(want)


def test_dur_est_over_the_written_files(world, tmp_path):
    """--hist equals the run lengths of the restated paths: per file every segment after the first (the reader's
    init_utterance_segmentation takes that one), the last one a frame longer"""
    w = world
    als = [str(tmp_path / ("u%d.phn" % i)) for i in range(3)]
    recipe = write_recipe(w, str(tmp_path / "r.recipe"), list(zip(SPANS, w.nets, als)))
    run_stats(w, recipe, str(tmp_path / "o"), "-a", "-n")
    table = np.zeros((S, 100), np.int64)
    for i, (a, b) in enumerate(w.windows):
        segs = AR.segments(w.paths[i].path, AR.arc_labels(w.texts[i]), a)
        assert segs[-1][1] == b + 1 and len(segs) >= 2
        for start, end, name in segs[1:]:
            hmm, state = name.split(".")
            table[HMM_STATES[hmm][int(state)], min(end - start, 100) - 1] += 1
    hist = str(tmp_path / "d.hist")
    # the recipe's start and end times hold for the .phn reader too, at its own 125 frames a second: the feature rate here
    assert w.fr == 125.0
    r = subprocess.run([os.path.join(BIN, "dur_est"), "-p", w.base + ".ph", "-r", recipe, "-O", "--hist", hist],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    # the reader cuts a line at the recipe line's end time, so the last segment's +1 is cut away again there ...
    cut = table.copy()
    for i, (a, b) in enumerate(w.windows):
        start, end, name = AR.segments(w.paths[i].path, AR.arc_labels(w.texts[i]), a)[-1]
        hmm, state = name.split(".")
        s = HMM_STATES[hmm][int(state)]
        cut[s, end - start - 1] -= 1
        cut[s, end - start - 2] += 1
    assert open(hist).read() == DR.hist_text(cut)
    # ... and is there without time limits in the recipe
    free = str(tmp_path / "free.recipe")
    open(free, "w").write("".join("audio=%s alignment=%s\n" % (w.wav, p) for p in als))
    r = subprocess.run([os.path.join(BIN, "dur_est"), "-p", w.base + ".ph", "-r", free, "-O", "--hist", hist],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert open(hist).read() == DR.hist_text(table)
    assert table.sum() == sum(len(AR.segments(p.path, AR.arc_labels(t), 0)) - 1 for p, t in zip(w.paths, w.texts))

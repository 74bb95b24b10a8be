"""The native logl tool (csrc/aku/main_logl.cc, csrc/logl.cc): aku/logl.cc with the likelihood of a .phn segmentation
(seg_loglik.hip) or, with -H / -D, the forward-backward total over HMM networks (hmmnet_fb.hip) on the device.

The fixture is that of tests/test_reference_callers.py::test_reference_logl_with_both_segmentators_on_the_engine, built
here: 2 s of audio, the production feature chain, 30 states in HMMs of three, a left-to-right network over 24 states.
The references: the oracle's sum along the segmentation within 2e-3 + 1e-6 |ll| (the bound of that test and of
tests/test_vtln_gpu.py for the same quantity), and tools/hmmnet_restate.py over the oracle's double state likelihoods
within 5e-3 + 1e-6 |want| in the default precision and 2e-6 + 1e-12 |want| under AASR_PREC=1 (both from that test).
Where oracle/_ref/logl_refmain was built, the same command lines go through it under the same bounds."""
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

RS = HC.RS
pytestmark = pytest.mark.gpu
TOOL = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "logl")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "logl_refmain")
S, PER = 30, 3
Q = [h * PER + j for h in (3, 0, 7, 2, 5, 1, 9, 6) for j in range(PER)]


def write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


class World:
    pass


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = World()
    w.dir = d = tmp_path_factory.mktemp("logl")
    rng = np.random.default_rng(41)
    cfg_text = synth.make_feature_config()
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(cfg_text)
    pcm = synth.make_audio(16000 * 2, seed=73)
    w.wav = str(d / "a.wav")
    write_wav(w.wav, pcm)
    ft = capi.Feat(cfg_text)
    w.T = T = ft.eof_frame(len(pcm))
    fea = ft.run(pcm, 0, T, dtype=np.float64)
    mean, var, off, idx, mw = synth.make_model(D=39, G=90, S=S, comps=3, seed=27)
    mean[:] = fea[rng.integers(0, T, 90)] + 0.3 * rng.standard_normal((90, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    w.ll = oracle.DiagModel(mean, var, off, idx, mw).score(fea)          # [T x S], floored at log 1e-50
    w.sp = np.full(S, 0.5)                                                # every state: self 2 s and next 2 s + 1, both 0.5
    w.net_text = HC.chain(Q)
    w.net = str(d / "net.hmmnet")
    open(w.net, "w").write(w.net_text)
    w.rnet = HC.parse(w.net_text, w.sp)
    w.recipe = str(d / "b.recipe")
    open(w.recipe, "w").write("audio=%s hmmnet=%s\n" % (w.wav, w.net))
    return w


def run(exe, w, recipe, *flags, env=None, ok=True):
    r = subprocess.run([exe, "-b", w.base, "-c", w.cfg, "-r", recipe, "-i", "1"] + list(flags), capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def total_of(r):
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("Total log likelihood ("), last
    return float(last.split(":")[-1])


def file_lines(r):
    return [l for l in r.stdout.splitlines() if l.startswith("Log likelihood for file ")]


def close(got, want, prec64=False):
    print("got %.9f want %.9f" % (got, want))
    return abs(got - want) <= ((2e-6 + 1e-12 * abs(want)) if prec64 else (5e-3 + 1e-6 * abs(want)))


def with_refmain(w, recipe, flags, want, ran):
    """the same command line through the reference's main() where it was built, both precisions"""
    if not os.access(REFMAIN, os.X_OK):
        return
    ran.append(1)
    assert close(total_of(run(REFMAIN, w, recipe, *flags)), want)
    assert close(total_of(run(REFMAIN, w, recipe, *flags, env={"AASR_PREC": "1"})), want, True)


def skip_note(ran):
    if not ran:
        pytest.skip("oracle/_ref/logl_refmain was not built: the tool was checked against the oracle and the restatement alone")


def test_phn_mode_against_the_oracle(world):
    w = world
    seg = [int(w.ll[a:a + 12].sum(axis=0).argmax()) for a in range(0, w.T, 12)]
    with open(w.dir / "seg.phn", "w") as f:
        for k, s in enumerate(seg):
            f.write("%d %d %d\n" % (k * 12 * 128, min((k + 1) * 12, w.T) * 128, s))
    recipe = str(w.dir / "a.recipe")
    open(recipe, "w").write("audio=%s transcript=%s\n" % (w.wav, w.dir / "seg.phn"))
    want = sum(float(w.ll[t, seg[t // 12]]) for t in range(w.T))
    r = run(TOOL, w, recipe, "--snl")
    got = total_of(r)
    print("phn", got, want)
    assert abs(got - want) <= 2e-3 + 1e-6 * abs(want)
    assert r.stdout.splitlines() == ["Log likelihood for file %s: %f" % (w.wav, got), "Total log likelihood (0/0): %f" % got]
    if not os.access(REFMAIN, os.X_OK):
        pytest.skip("oracle/_ref/logl_refmain was not built: the tool was checked against the oracle alone")
    ref = total_of(run(REFMAIN, w, recipe, "--snl"))
    assert abs(ref - want) <= 2e-3 + 1e-6 * abs(want) and abs(ref - got) <= 2e-3 + 1e-6 * abs(want)


@pytest.mark.parametrize("flags,kw", [
    (("-F", "1e9", "-W", "1e9"), dict(fw_beam=1e9, bw_beam=1e9)),
    (("-F", "1e9", "-W", "1e9", "-V"), dict(fw_beam=1e9, bw_beam=1e9, viterbi=True)),
    ((), dict(fw_beam=15.0, bw_beam=200.0)),
    (("-F", "0", "-W", "0"), dict(fw_beam=15.0, bw_beam=200.0)),          # 0 keeps the defaults
], ids=["wide", "viterbi", "default-beams", "zero-beams"])
def test_hmmnet_against_the_restatement(world, flags, kw):
    w = world
    want = RS.forward_backward(w.rnet, w.ll, **kw)
    assert want.status == RS.OK
    r = run(TOOL, w, w.recipe, "-H", *flags)
    assert close(total_of(r), want.forward_total)
    assert len(file_lines(r)) == 1 and "Warning" not in r.stderr and "Could not" not in r.stderr, r.stderr
    assert close(total_of(run(TOOL, w, w.recipe, "-H", *flags, env={"AASR_PREC": "1"})), want.forward_total, True)
    ran = []
    with_refmain(w, w.recipe, ("-H",) + flags, want.forward_total, ran)
    skip_note(ran)


def test_acoustic_scale_applies_only_when_given(world):
    w = world
    want = RS.forward_backward(w.rnet, w.ll, 1e9, 1e9, ac_scale=0.5)
    r = run(TOOL, w, w.recipe, "-H", "-F", "1e9", "-W", "1e9", "-A", "0.5", env={"AASR_PREC": "1"})
    assert close(total_of(r), want.forward_total, True)


def test_two_lines_with_time_windows(world):
    """start-time / end-time as frame limits (aku/Recipe.cc:223-228): frames 50 .. 150 and 125 .. 200 at 125 frames a second"""
    w = world
    recipe = str(w.dir / "win.recipe")
    open(recipe, "w").write("audio=%s hmmnet=%s start-time=0.4 end-time=1.2\naudio=%s hmmnet=%s start-time=1.0 end-time=1.6\n"
                            % (w.wav, w.net, w.wav, w.net))
    wants = [RS.forward_backward(w.rnet, w.ll[a:b], 1e9, 1e9).forward_total for a, b in ((50, 150), (125, 200))]
    r = run(TOOL, w, recipe, "-H", "-F", "1e9", "-W", "1e9", env={"AASR_PREC": "1"})
    lines = file_lines(r)
    assert len(lines) == 2 and " (0.40-1.20): " in lines[0] and " (1.00-1.60): " in lines[1], lines
    for line, want in zip(lines, wants):
        assert close(float(line.split(":")[-1]), want, True)
    assert close(total_of(r), sum(wants), True)
    assert close(total_of(run(TOOL, w, recipe, "-H", "-F", "1e9", "-W", "1e9")), sum(wants))
    ran = []
    with_refmain(w, recipe, ("-H", "-F", "1e9", "-W", "1e9"), sum(wants), ran)


def test_batches_add_up(world):
    w = world
    recipe = str(w.dir / "three.recipe")
    spans = ((0.0, 0.8), (0.4, 1.2), (1.0, 1.6))
    open(recipe, "w").write("".join("audio=%s hmmnet=%s start-time=%.1f end-time=%.1f speaker=s%d\n" % (w.wav, w.net, a, b, i)
                                    for i, (a, b) in enumerate(spans)))
    flags = ("-H", "-F", "1e9", "-W", "1e9")
    env = {"AASR_PREC": "1"}
    whole = run(TOOL, w, recipe, *flags, env=env)
    b1 = run(TOOL, w, recipe, *flags, "-B", "2", "-I", "1", env=env)
    b2 = run(TOOL, w, recipe, *flags, "-B", "2", "-I", "2", env=env)
    assert b1.stdout.strip().splitlines()[-1].startswith("Total log likelihood (1/2): ")
    assert b2.stdout.strip().splitlines()[-1].startswith("Total log likelihood (2/2): ")
    assert len(file_lines(b1)) + len(file_lines(b2)) == 3 and file_lines(b1) + file_lines(b2) == file_lines(whole)
    assert abs(total_of(b1) + total_of(b2) - total_of(whole)) <= 3e-6        # three printed values of six decimals


def test_denominator_networks(world):
    w = world
    den_text = HC.chain(Q[:12])
    den = str(w.dir / "den.hmmnet")
    open(den, "w").write(den_text)
    recipe = str(w.dir / "den.recipe")
    open(recipe, "w").write("audio=%s hmmnet=%s den-hmmnet=%s\n" % (w.wav, w.net, den))
    want = RS.forward_backward(HC.parse(den_text, w.sp), w.ll, 1e9, 1e9).forward_total
    assert close(total_of(run(TOOL, w, recipe, "-D", "-F", "1e9", "-W", "1e9", env={"AASR_PREC": "1"})), want, True)
    ran = []
    with_refmain(w, recipe, ("-D", "-F", "1e9", "-W", "1e9"), want, ran)


def test_the_backward_beam_is_widened_once(world):
    """40 frames; the network's real path is three states, next to it runs a branch of 45 states -- the best state of
    every frame -- that is longer than the utterance, so it never reaches the initial node but sets each frame's best
    backward score.  With a backward beam W between half of and the whole lead that branch builds up, the real path is
    pruned at W and survives at 2 W: one warning, then the total of the restatement at 2 W.  W is taken from the
    restatement: the first candidate at which it fails at W, succeeds at 2 W, and keeps every pruning comparison of both
    runs 0.05 away from its threshold -- ten times the 40 x 1e-4 that the parity contract on state log-likelihoods
    (conftest.TOL_LL) lets a path of 40 frames differ by, so the device's float scores cannot flip a decision."""
    w = world
    a, b_ = 50, 90
    ll = w.ll[a:b_]
    order = np.argsort(ll.sum(axis=0))
    real = [int(order[0]), int(order[1]), int(order[2])]                 # the three worst states
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
    net = str(w.dir / "retry.hmmnet")
    open(net, "w").write(text)
    rnet = HC.parse(text, w.sp)
    chosen = None
    for W in [round(10 * 1.12 ** k, 1) for k in range(40)]:
        r1 = RS.forward_backward(rnet, ll, 1e9, float(W))
        r2 = RS.forward_backward(rnet, ll, 1e9, 2.0 * W)
        if r1.status == RS.FAILED_BACKWARD and r2.status == RS.OK and min(r1.min_margin, r2.min_margin) >= 0.05:
            chosen = (W, r2.forward_total)
            print("W", W, "margins", r1.min_margin, r2.min_margin)
            break
    assert chosen, "no backward beam separates the two runs on this fixture"
    W, want = chosen
    recipe = str(w.dir / "retry.recipe")
    open(recipe, "w").write("audio=%s hmmnet=%s start-time=0.4 end-time=0.72\n" % (w.wav, net))
    r = run(TOOL, w, recipe, "-H", "-F", "1e9", "-W", str(W))
    warnings = [l for l in r.stderr.splitlines() if l.startswith("Warning: Backward phase failed")]
    assert warnings == ["Warning: Backward phase failed, increasing beam to %.1f" % (2.0 * W)], r.stderr
    assert "Could not run Baum-Welch" not in r.stderr
    assert close(total_of(r), want)
    # the beam never suffices at 5 x 1: the reference's message, the utterance skipped, status 0
    r = run(TOOL, w, recipe, "-H", "-F", "1e9", "-W", "1")
    assert r.stderr.count("Warning: Backward phase failed, increasing beam to") == 4
    assert "Could not run Baum-Welch for file %s\nThe HMM network may be incorrect or initial beam too low.\n" % w.wav in r.stderr
    assert file_lines(r) == [] and total_of(r) == 0.0


def test_the_wrong_feature_dimension_is_the_reference_message(world):
    w = world
    bad = str(w.dir / "short.cfg")
    open(bad, "w").write(synth.make_feature_config(dim_cep=11))
    r = subprocess.run([TOOL, "-b", w.base, "-c", bad, "-r", w.recipe, "-H"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "exception: gaussian dimension is 39 but feature dimension is 36" in r.stderr, r.stderr

"""The native vtln tool (csrc/aku/main_vtln.cc, csrc/vtln.cc): aku/vtln.cc's warp-factor estimation with the features of
every grid point and the log-likelihood of the segmentations on the device (seg_loglik.hip).

The fixture is that of tests/test_reference_callers.py::test_reference_vtln_estimation_on_the_engine, built here: two
speakers, 2 s of audio each, a fft - vtln - mel - dct - delta chain of 24 dimensions, 72 Gaussians drawn from the
speakers' features at their true warp factors (1.04 and 0.96), state-number labels, --grid-size 5 --grid-rad 0.04.
The references are the oracle's feature chain and DiagModel with that test's own bounds -- warp factors within 5e-4,
log-likelihoods within 2e-3 + 1e-6 |ll| -- and, where oracle/_ref/vtln_refmain was built, the reference's main() on
the adapter classes with the same command lines: the same speakers, warp texts and best warps, a byte-identical speaker
file, log-likelihoods within the same bound (the refmain reads state rows that may be float; the tool computes in
double, so the "%.3f" texts need not be equal)."""
import os
import subprocess
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "vtln")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "vtln_refmain")

CFG = """module
{
  name audiofile
  type audiofile
  sample_rate 16000
}
module
{
  name fft
  type fft
  magnitude 0
  sources audiofile
}
module
{
  name vtln
  type vtln
  sources fft
}
module
{
  name mel
  type mel
  sources vtln
}
module
{
  name mfcc
  type dct
  dim 12
  sources mel
}
module
{
  name d1
  type delta
  sources mfcc
}
module
{
  name merged
  type merge
  sources mfcc d1
}
"""
SPEAKERS = {"spkA": np.float32(1.04), "spkB": np.float32(0.96)}
SPKC_IN = "speaker default\n{\n  feature vtln\n  {\n  }\n}\n"
STRETCH = 10         # frames per state of the segmentations


def write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def write_phn(path, states, n_frames, first_sample=0):
    with open(path, "w") as f:
        for k, s in enumerate(states):
            f.write("%d %d %d\n" % (first_sample + k * STRETCH * 128, first_sample + min((k + 1) * STRETCH, n_frames) * 128, s))


class World:
    pass


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = World()
    w.dir = d = tmp_path_factory.mktemp("vtln")
    rng = np.random.default_rng(29)
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(CFG)
    w.chain = chain = oracle.FeatureChain(CFG)
    D = 24
    w.pcm, feats = {}, {}
    for i, (spk, wf) in enumerate(SPEAKERS.items()):
        w.pcm[spk] = synth.make_audio(16000 * 2, seed=90 + i)
        write_wav(str(d / (spk + ".wav")), w.pcm[spk])
        T = chain.last_frame(len(w.pcm[spk])) + 1
        chain.set_parameters("vtln", {"warp_factor": "%.9g" % wf})
        feats[spk] = chain.generate(w.pcm[spk], 0, T)
    # a model drawn from the speakers' features AT their true warp: the grid must find it back
    S, G = 24, 72
    mean, var, off, idx, mw = synth.make_model(D=D, G=G, S=S, comps=3, seed=31)
    allf = np.vstack(list(feats.values()))
    scale = allf.std(axis=0)
    mean[:] = allf[rng.integers(0, len(allf), G)] + 0.2 * scale * rng.standard_normal((G, D))
    var[:] = (scale * rng.uniform(0.7, 1.3, (G, D))) ** 2
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=3)
    w.om = om = oracle.DiagModel(mean, var, off, idx, mw)
    # per speaker a state segmentation (state-number labels): the best state of each 10-frame stretch
    w.seg = {}
    for spk in SPEAKERS:
        T = len(feats[spk]) - 2
        ll = om.score(feats[spk])
        st = [int(ll[a:a + STRETCH].sum(axis=0).argmax()) for a in range(0, T, STRETCH)]
        w.seg[spk] = (T, st)
        write_phn(str(d / (spk + ".phn")), st, T)
    w.recipe = str(d / "r.recipe")
    open(w.recipe, "w").write("".join("audio=%s transcript=%s speaker=%s\n" % (d / (s + ".wav"), d / (s + ".phn"), s)
                                       for s in SPEAKERS))
    w.spkc = str(d / "in.spkc")
    open(w.spkc, "w").write(SPKC_IN)
    return w


def grid(centre, n, rad):
    """aku/vtln.cc:72-73, 214-225 in float"""
    start = np.float32(rad)
    step = np.float32(2) * start / np.float32(max(n - 1, 1))
    start = -start
    return [np.float32(np.float32(centre) + start + np.float32(i) * step) for i in range(n)]


def loglik(w, pcm, states, first, n_frames, wf):
    """the oracle's total along a segmentation: frames first ... first + n_frames - 1 under warp factor wf"""
    w.chain.set_parameters("vtln", {"warp_factor": "%.9g" % wf})
    ll = w.om.score(w.chain.generate(pcm, first, n_frames))
    return sum(float(ll[t, states[t // STRETCH]]) for t in range(n_frames))


def run(exe, w, tag, recipe=None, spkc=None, extra=("--snl", "--grid-size", "5", "--grid-rad", "0.04")):
    out, summ = str(w.dir / (tag + ".spkc")), str(w.dir / (tag + ".sum"))
    r = subprocess.run([exe, "-b", w.base, "-c", w.cfg, "-r", recipe or w.recipe, "-v", "vtln", "-S", spkc or w.spkc,
                        "-o", out, "-s", summ] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(out).read(), open(summ).read()


def parse_summary(text):
    got, cur = {}, None
    for line in text.splitlines():
        if line.startswith("["):
            cur = line.strip("[]")
            got[cur] = []
        elif line.strip():
            a, b = line.split(":")
            got[cur].append((a.strip(), float(b)))
    return got


def close_ll(a, b):
    return abs(a - b) <= 2e-3 + 1e-6 * abs(b)


def check_summary(got, want):
    """got: a parsed summary; want: {speaker: [(warp, loglik)]}"""
    assert list(got) == sorted(want), (list(got), sorted(want))
    for spk in want:
        assert len(got[spk]) == len(want[spk]), (spk, got[spk], want[spk])
        for (gw, gl), (ww, wl) in zip(got[spk], want[spk]):
            print("%s warp %s loglik %.3f, expected %.9g %.6f" % (spk, gw, gl, ww, wl))
            assert abs(float(gw) - float(ww)) < 5e-4 and close_ll(gl, wl), (spk, gw, ww, gl, wl)


def check_refmain(w, tag, out, summ, **kw):
    """the same command line through the reference's main(), where it was built"""
    if not os.access(REFMAIN, os.X_OK):
        return False
    rout, rsumm = run(REFMAIN, w, tag + "_ref", **kw)
    g, r = parse_summary(summ), parse_summary(rsumm)
    assert list(g) == list(r)
    for spk in g:
        assert [a for a, _ in g[spk]] == [a for a, _ in r[spk]], (spk, g[spk], r[spk])       # the warp texts
        assert all(close_ll(x[1], y[1]) for x, y in zip(g[spk], r[spk])), (spk, g[spk], r[spk])
        assert max(g[spk], key=lambda x: x[1])[0] == max(r[spk], key=lambda x: x[1])[0]
    assert out == rout, (out, rout)
    return True


def block_of(text, spk):
    return text.split("speaker %s\n" % spk)[1].split("}\n\n}")[0]


def test_against_the_oracle_and_the_reference_binary(world):
    w = world
    out, summ = run(TOOL, w, "plain")
    want = {}
    for spk, true_wf in SPEAKERS.items():
        T, st = w.seg[spk]
        want[spk] = [(wf, loglik(w, w.pcm[spk], st, 0, T, wf)) for wf in grid(1, 5, 0.04)]
        best = max(want[spk], key=lambda x: x[1])[0]
        assert abs(float(best) - float(true_wf)) < 1e-6, (spk, want[spk])
    got = parse_summary(summ)
    check_summary(got, want)
    for spk, true_wf in SPEAKERS.items():      # the best warp is the true one, in the summary and in the speaker file
        assert abs(float(max(got[spk], key=lambda x: x[1])[0]) - float(true_wf)) < 5e-4
        block = block_of(out, spk)
        assert "feature vtln" in block and ("warp_factor %g" % float(true_wf)) in block, block
    assert "speaker default" in out
    if not check_refmain(w, "plain", out, summ):
        pytest.skip("oracle/_ref/vtln_refmain was not built: the tool was checked against the oracle alone")


def test_relative_grid_around_each_speakers_own_warp(world):
    """--relative with the defaults 5 / 0.03: the centre is the warp factor the speaker file gives the speaker"""
    w = world
    centres = {"spkA": np.float32(1.03), "spkB": np.float32(0.97)}
    spkc = str(w.dir / "rel_in.spkc")
    open(spkc, "w").write(SPKC_IN + "".join("speaker %s\n{\n  feature vtln\n  {\n    warp_factor %g\n  }\n}\n" % (s, float(c))
                                            for s, c in centres.items()))
    out, summ = run(TOOL, w, "rel", spkc=spkc, extra=("--snl", "--relative"))
    want = {}
    for spk, c in centres.items():
        T, st = w.seg[spk]
        want[spk] = [(wf, loglik(w, w.pcm[spk], st, 0, T, wf)) for wf in grid(c, 5, 0.03)]
    got = parse_summary(summ)
    check_summary(got, want)
    assert [a for a, _ in got["spkA"]] == ["1.000", "1.015", "1.030", "1.045", "1.060"]
    for spk in centres:
        best = max(want[spk], key=lambda x: x[1])[0]
        assert ("warp_factor %g" % float(best)) in block_of(out, spk)
    check_refmain(w, "rel", out, summ, spkc=spkc, extra=("--snl", "--relative"))


@pytest.fixture(scope="module")
def pieces(world):
    """three utterances of each speaker (thirds of its audio, segmentations of their own), interleaved in the recipe,
    with utterance ids"""
    w = world
    lines, utts = [], []
    third = 16000 * 2 // 3
    for k in range(3):
        for spk in SPEAKERS:
            name = "%s_%d" % (spk, k)
            pcm = w.pcm[spk][k * third:(k + 1) * third]
            write_wav(str(w.dir / (name + ".wav")), pcm)
            T = w.chain.last_frame(len(pcm)) + 1 - 2
            st = [w.seg[spk][1][(k * 7 + a) % len(w.seg[spk][1])] for a in range(-(-T // STRETCH))]
            write_phn(str(w.dir / (name + ".phn")), st, T)
            utts.append((spk, pcm, st, T))
            lines.append("audio=%s transcript=%s speaker=%s utterance=%s\n" % (w.dir / (name + ".wav"), w.dir / (name + ".phn"), spk, name))
    recipe = str(w.dir / "pieces.recipe")
    open(recipe, "w").write("".join(lines))
    spkc = str(w.dir / "pieces_in.spkc")
    open(spkc, "w").write(SPKC_IN + "utterance default\n{\n}\n")
    return recipe, spkc, utts


def test_several_utterances_per_speaker_interleaved(world, pieces):
    w = world
    recipe, spkc, utts = pieces
    out, summ = run(TOOL, w, "pieces", recipe=recipe, spkc=spkc)
    want = {}
    for spk in SPEAKERS:
        want[spk] = []
        for wf in grid(1, 5, 0.04):
            total = 0.0
            for s, pcm, st, T in utts:      # recipe order, then frame order
                if s == spk:
                    total += loglik(w, pcm, st, 0, T, wf)
            want[spk].append((wf, total))
    check_summary(parse_summary(summ), want)
    check_refmain(w, "pieces", out, summ, recipe=recipe, spkc=spkc)


def test_a_time_window_over_relative_sample_numbers(world):
    """start-time / end-time on the recipe line, the .phn file counting from the window's start (--rsamp)"""
    w = world
    first, last = 50, 150              # 0.4 s and 1.2 s at 125 frames a second
    lines = []
    for spk in SPEAKERS:
        st = w.seg[spk][1][5:15]
        write_phn(str(w.dir / (spk + "_win.phn")), st, last - first)
        lines.append("audio=%s transcript=%s speaker=%s start-time=0.4 end-time=1.2\n" % (w.dir / (spk + ".wav"), w.dir / (spk + "_win.phn"), spk))
    recipe = str(w.dir / "win.recipe")
    open(recipe, "w").write("".join(lines))
    extra = ("--snl", "--rsamp", "--grid-size", "5", "--grid-rad", "0.04")
    out, summ = run(TOOL, w, "win", recipe=recipe, extra=extra)
    want = {spk: [(wf, loglik(w, w.pcm[spk], w.seg[spk][1][5:15], first, last - first, wf)) for wf in grid(1, 5, 0.04)]
            for spk in SPEAKERS}
    check_summary(parse_summary(summ), want)
    check_refmain(w, "win", out, summ, recipe=recipe, extra=extra)


def test_batches_write_their_own_speakers(world):
    """-B 2: the recipe's two speakers fall into one batch each; "default" goes out with batch 1 only, no utterances"""
    w = world
    extra = ("--snl", "--grid-size", "5", "--grid-rad", "0.04", "-B", "2")
    out1, summ1 = run(TOOL, w, "b1", extra=extra + ("-I", "1"))
    out2, summ2 = run(TOOL, w, "b2", extra=extra + ("-I", "2"))
    assert list(parse_summary(summ1)) == ["spkA"] and list(parse_summary(summ2)) == ["spkB"]
    assert "speaker default" in out1 and "speaker spkA" in out1 and "speaker spkB" not in out1
    assert "speaker default" not in out2 and "speaker spkB" in out2 and "speaker spkA" not in out2
    assert "utterance" not in out1 and "utterance" not in out2
    assert ("warp_factor %g" % 1.04) in block_of(out1, "spkA") and ("warp_factor %g" % 0.96) in block_of(out2, "spkB")
    check_refmain(w, "b1", out1, summ1, extra=extra + ("-I", "1"))


def test_the_wrong_feature_dimension_is_the_reference_message(world):
    w = world
    bad = str(w.dir / "short.cfg")
    open(bad, "w").write(CFG.replace("dim 12", "dim 11"))
    r = subprocess.run([TOOL, "-b", w.base, "-c", bad, "-r", w.recipe, "-v", "vtln", "-S", w.spkc, "--snl"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "exception: gaussian dimension is 24 but feature dimension is 22" in r.stderr, r.stderr


def test_group_cuts_do_not_change_the_files(capi, world, pieces):
    """the recipe of six interleaved utterances in one group and, with the debug bound at 100 frames, in several
    (each speaker spans more than one): the summary and the speaker file are the same bytes"""
    w = world
    recipe, spkc, _ = pieces
    texts = []
    try:
        for tag, bound in (("one", 0), ("cut", 100)):
            capi.vtln_set_group_frames(bound)
            feat = capi.Feat(CFG)
            gmm = capi.Gmm.from_files(w.base + ".gk", w.base + ".mc", w.base + ".ph")
            topo = capi.Topology(w.base + ".ph")
            spk = capi.SpeakerConfig(feat, gmm)
            spk.read_file(spkc)
            out, summ = str(w.dir / (tag + ".spkc")), str(w.dir / (tag + ".sum"))
            opts = capi.VtlnOptions.defaults(snl=1, grid_size=5, grid_size_given=1, grid_rad=0.04, grid_rad_given=1)
            st = capi.run_vtln_recipe(feat, gmm, topo, recipe, spk, "vtln", out=out, savesum=summ, opts=opts)
            assert st["utterances"] == 6 and st["frames"] > 400
            texts.append((open(out).read(), open(summ).read()))
            del spk
            gmm.close()
            feat.close()
    finally:
        capi.vtln_set_group_frames(0)
    assert texts[0] == texts[1]
    assert sorted(parse_summary(texts[0][1])) == sorted(SPEAKERS) and "utterance spkB_2" in texts[0][0]

"""The confidence classes of the FstDecoder module and fst_decode --confidence on the device: against the reference's
recorded answers (tests/golden/fst_conf), and the tool's engine mode against --lna-files on the LNA file that phone_probs
writes for the same audio, byte for byte."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402
import fst_conf_restate as CR  # noqa: E402

FST = os.path.join(ROOT, "tests", "golden", "fst")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst_conf")
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
CASES = ["durhi", "rand1", "rand2", "rand4", "toy"]


def tool(*args, name="fst_decode"):
    return subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, timeout=300)


def expected(case):
    return [l.split(b"\t") for l in open(os.path.join(GOLDEN, "expected_conf_%s.txt" % case), "rb").read().split(b"\n") if l]


def g9(x) -> bytes:
    return ("%.9g" % x).encode()


@pytest.mark.gpu
def test_module_on_the_golden_cases(capi):
    from aaltoasr_amd import FstDecoder
    for case in CASES:
        paths = [os.path.join(FST, case + ".fst"), os.path.join(GOLDEN, case + ".ploop.fst"), None, os.path.join(FST, case + ".dur")]
        for f in expected(case)[:3]:
            s = FstDecoder.FstConfidenceWithPhoneLoop(*paths)
            plain = FstDecoder.FstConfidence(paths[0], None, paths[3])
            for o in (s, plain):
                o.set_beam(float(f[0]))
                o.set_token_limit(int(f[1]))
                o.set_duration_scale(float(f[2]))
                o.set_transition_scale(float(f[3]))
            s.set_phone_beam(float(f[4]))
            s.set_phone_token_limit(int(f[5]))
            s.set_phone_duration_scale(float(f[6]))
            for o in (s, plain):
                o.lna_open(os.path.join(FST, case + ".lna"), 1024)
                o.init_search()
                o.run()
                o.lna_close()
            text, conf = s.result_and_confidence()
            assert isinstance(text, bytes) and isinstance(conf, float)
            assert [text, g9(s.get_token_conf()), g9(s.get_ploop_conf()), g9(s.get_edit_conf()), g9(s.get_best_acu_conf()), g9(conf)] == \
                [f[7], f[9], f[10], f[11], f[12], f[19]], (case, f[:7])
            assert s.get_result() == text and g9(s.get_result_and_logprob()[1]) == f[13] and g9(s.get_best_final_token_logprob()) == f[15]
            ptext, pconf = plain.result_and_confidence()
            assert (ptext, g9(pconf)) == (f[7], f[20]), (case, f[:7])
            s.init_search()      # both searches back at their start: no confidence before the next run
            with pytest.raises(RuntimeError):
                s.result_and_confidence()


@pytest.mark.gpu
def test_tool_on_the_golden_lna_files(capi, tmp_path):
    """a recipe of two lines per case, both in one launch; the first two recorded settings; then the plain confidence"""
    rec = str(tmp_path / "g.recipe")
    for case in CASES:
        lna = os.path.join(FST, case + ".lna")
        open(rec, "w").write("lna=%s\n" % lna * 2)
        for f in expected(case)[:2]:
            out = str(tmp_path / "out.txt")
            common = ["--fst", os.path.join(FST, case + ".fst"), "--dur", os.path.join(FST, case + ".dur"), "-r", rec, "-o", out,
                      "--lna-files", "--beam", f[0].decode(), "--token-limit", f[1].decode(), "--duration-scale", f[2].decode(),
                      "--transition-scale", f[3].decode(), "--confidence"]
            r = tool(*common, "--phone-loop", os.path.join(GOLDEN, case + ".ploop.fst"), "--phone-beam", f[4].decode(),
                     "--phone-token-limit", f[5].decode(), "--phone-duration-scale", f[6].decode())
            assert r.returncode == 0 and r.stderr == b"", r.stderr
            line = lna.encode() + b" " + f[13] + b" " + f[19] + (b" " + f[7] if f[7] else b"") + b"\n"
            assert open(out, "rb").read() == line * 2, (case, f)
            r = tool(*common)
            assert r.returncode == 0, r.stderr
            line = lna.encode() + b" " + f[13] + b" " + f[20] + (b" " + f[7] if f[7] else b"") + b"\n"
            assert open(out, "rb").read() == line * 2, (case, f, "plain")
    # -i 1: the reference's verbose block per utterance on stderr
    r = tool(*common, "--phone-loop", os.path.join(GOLDEN, case + ".ploop.fst"), "-i", "1")
    assert r.returncode == 0 and r.stderr.count(b"\tToken: ") == 2 and r.stderr.count(b"\tTotal: ") == 2, r.stderr


@pytest.mark.gpu
def test_engine_mode_equals_lna_files_on_what_phone_probs_writes(capi, oracle, tmp_path):
    from aaltoasr_amd import synth
    rng = np.random.default_rng(5)
    S = 12
    cfg_text = synth.make_feature_config()
    cfg = str(tmp_path / "f.cfg")
    open(cfg, "w").write(cfg_text)
    wavs = []
    for i, seconds in enumerate((1.0, 0.6)):
        pcm = synth.make_audio(int(16000 * seconds), seed=90 + i)
        wavs.append(str(tmp_path / ("a%d.wav" % i)))
        with wave.open(wavs[-1], "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.astype("<i2").tobytes())
    ft = capi.Feat(cfg_text)
    fea = ft.run(pcm, 0, ft.eof_frame(len(pcm)), dtype=np.float64)
    mean, var, off, idx, mw = synth.make_model(D=39, G=36, S=S, comps=3, seed=3)
    mean[:] = fea[rng.integers(0, len(fea), 36)] + 0.3 * rng.standard_normal((36, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    base = str(tmp_path / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, mw)
    oracle.write_ph(base + ".ph", S, states_per_hmm=3)
    fst, ploop = str(tmp_path / "n.fst"), str(tmp_path / "p.fst")
    open(fst, "wb").write(R.random_net(np.random.default_rng(11), 40, S, max_deg=5, p_word=0.2))
    open(ploop, "wb").write(CR.random_phone_loop(np.random.default_rng(12), S, n_phones=5, letters=b"w0123456"))
    rec = str(tmp_path / "a.recipe")
    open(rec, "w").write("".join("audio=%s lna=%s\n" % (w, w[:-4] + ".lna") for w in wavs))
    r = tool("-b", base, "-c", cfg, "-r", rec, "--lnabytes", "2", name="phone_probs")
    assert r.returncode == 0, r.stderr
    outs = []
    for mode in (["-b", base, "-c", cfg, "--lnabytes", "2"], ["--lna-files"]):
        out = str(tmp_path / ("out%d.txt" % len(outs)))
        for w in wavs:      # engine mode writes no LNA file: those of phone_probs are moved away while it runs
            if mode[0] == "-b":
                os.rename(w[:-4] + ".lna", w[:-4] + ".kept")
        r = tool("--fst", fst, "-r", rec, "-o", out, "--beam", "60", "--confidence", "--phone-loop", ploop, "--phone-beam", "80", *mode)
        assert r.returncode == 0, r.stderr
        for w in wavs:
            if mode[0] == "-b":
                assert not os.path.exists(w[:-4] + ".lna")
                os.rename(w[:-4] + ".kept", w[:-4] + ".lna")
        outs.append([l.split(b" ", 1) for l in open(out, "rb").read().split(b"\n") if l])
    assert [l[0] for l in outs[0]] == [w.encode() for w in wavs] and [l[0] for l in outs[1]] == [(w[:-4] + ".lna").encode() for w in wavs]
    assert [l[1] for l in outs[0]] == [l[1] for l in outs[1]] and len(outs[0]) == 2
    # the grammar search's part of the lines against the restatement on the file's values (the phone loop's random acoustics
    # tie at its token limit, so the confidence itself is held by the golden cases above, not here)
    net = R.read_fst(open(fst, "rb").read())
    for w, l in zip(wavs, outs[1]):
        ac, nb = R.read_lna(w[:-4] + ".lna")
        want = R.search(net, ac, beam=60.0)
        assert nb == 2 and want.ties == []
        f = l[1].split(b" ")
        assert f[0] == g9(float(want.logprob)) and float(f[1]) <= 1.0
        assert f[2:2 + len(want.words)] == [net.symbols[x] for x in want.words]

"""The fst_decode tool (csrc/aku/main_fst_decode.cc) and the FstDecoder module (aaltoasr_amd/FstDecoder.py): refusals before the
device is opened and the module's surface on the host; on the device the tool and the module against the reference
decoder's recorded answers (tests/golden/fst) and the tool's engine mode against --lna-files on the LNA file that
phone_probs writes for the same audio, byte for byte."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
CASES = ["durhi", "rand1", "rand2", "rand4", "toy", "wide"]


def tool(*args, name="fst_decode"):
    return subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, timeout=300)


def expected(case):
    return [l.split(b"\t") for l in open(os.path.join(GOLDEN, "expected_%s.txt" % case), "rb").read().split(b"\n") if l]


@pytest.fixture(scope="module")
def recipe(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("fst_tool")
    path = str(d / "lna.recipe")
    open(path, "w").write("lna=%s\n" % os.path.join(GOLDEN, "toy.lna"))
    return path


REFUSALS = [(["--lna-files", "--lnabytes", "4"], "--lnabytes belongs to engine mode"),
            (["--lna-files", "-c", "x.cfg"], "--lna-files takes no model and no feature configuration"),
            ([], "engine mode needs --config"),
            (["-c", "x.cfg"], "Must give either --base or all --gk, --mc and --ph"),
            (["--lna-files", "--beam", "-3"], "the beam must not be negative"),
            (["--lna-files", "--token-limit", "-1"], "the token limit must not be negative"),
            (["--lna-files", "--dur-by-state"], "--dur-by-state without --dur"),
            (["--lna-files", "-S", "x.spkc"], "-S belongs to engine mode"),
            (["--lna-files", "--cap-recomb", "12"], "--cap-recomb and --cap-history are powers of two"),
            (["--lna-files", "--cap-candidates", "-1"], "a capacity must not be negative"),
            (["--lna-files", "-B", "2"], "Must give both --batch and --bindex"),
            (["--lna-files", "--group", "0"], "--group must be at least 1")]


@pytest.mark.parametrize("flags,message", REFUSALS)
def test_tool_refuses_before_the_device_is_opened(recipe, tmp_path, flags, message):
    out = str(tmp_path / "out.txt")
    r = tool("--fst", os.path.join(GOLDEN, "toy.fst"), "-r", recipe, "-o", out, *flags)
    assert r.returncode == 1 and r.stderr.startswith(b"exception: ") and message.encode() in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_tool_reports_the_reader_message(recipe, tmp_path):
    bad = str(tmp_path / "bad.fst")
    open(bad, "w").write("#FSTBasic MaxPlus\nI 0\nX 0 1\n")
    r = tool("--fst", bad, "-r", recipe, "-o", str(tmp_path / "o"), "--lna-files")
    assert r.returncode == 1 and r.stderr == b"exception: fst_decode: Weird type indicator: 'X'.\n"
    audio = str(tmp_path / "a.recipe")
    open(audio, "w").write("audio=a.wav\n")
    r = tool("--fst", os.path.join(GOLDEN, "toy.fst"), "-r", audio, "-o", str(tmp_path / "o"), "--lna-files")
    assert r.returncode == 1 and b"a recipe line without lna=" in r.stderr


def test_module_surface(capi, tmp_path):
    from aaltoasr_amd import FstDecoder
    s = FstDecoder.FstSearch(os.path.join(GOLDEN, "toy.fst"), None, os.path.join(GOLDEN, "toy.dur"))
    assert (s.get_beam(), s.get_token_limit(), s.get_duration_scale(), s.get_transition_scale()) == (2600.0, 5000, 3.0, 1.0)
    s.set_beam(30)
    s.set_token_limit(7)
    s.set_duration_scale(1.5)
    s.set_transition_scale(0.5)
    assert (s.get_beam(), s.get_token_limit(), s.get_duration_scale(), s.get_transition_scale()) == (30.0, 7, 1.5, 0.5)
    for name in ("lna_open", "lna_close", "init_search", "run", "get_result", "get_result_and_logprob", "get_best_token_logprob",
                 "get_best_final_token_logprob", "best_tokens", "tokens_at_final_states"):
        assert callable(getattr(s, name))
    s.init_search()      # the start: one token at the initial node, which is no end node in the toy
    assert s.get_result() == b"" and s.get_result_and_logprob() == (b"", -1.0) and s.get_best_token_logprob() == 0.0
    assert s.best_tokens(3) == b"Best tokens:\n  Token 0 0 dur 0 ' '\n" and s.tokens_at_final_states() == b"Tokens at final nodes:\n"
    with pytest.raises(RuntimeError, match="open error"):
        FstDecoder.FstSearch(os.path.join(GOLDEN, "toy.fst"), str(tmp_path / "none.ph"), None)
    with pytest.raises(RuntimeError, match="Unknown header"):
        FstDecoder.FstSearch(os.path.join(GOLDEN, "toy.dur"), None, None)
    with pytest.raises(RuntimeError, match="invalid LNA byte number"):
        open(str(tmp_path / "bad.lna"), "wb").write(b"\0\0\0\3\7")
        s.lna_open(str(tmp_path / "bad.lna"), 1024)
    assert "never consults the HMM file" in FstDecoder.__doc__


@pytest.mark.gpu
def test_tool_on_the_golden_lna_files(capi, tmp_path):
    """a recipe of two lines per case, both in one launch; the settings are the first two of the recorded ones"""
    rec = str(tmp_path / "g.recipe")
    for case in CASES:
        open(rec, "w").write("lna=%s\n" % os.path.join(GOLDEN, case + ".lna") * 2)
        for f in expected(case)[:2]:
            out = str(tmp_path / "out.txt")
            r = tool("--fst", os.path.join(GOLDEN, case + ".fst"), "--dur", os.path.join(GOLDEN, case + ".dur"), "-r", rec, "-o", out,
                     "--lna-files", "--beam", f[0].decode(), "--token-limit", f[1].decode(), "--duration-scale", f[2].decode(),
                     "--transition-scale", f[3].decode())
            assert r.returncode == 0, r.stderr
            name = os.path.join(GOLDEN, case + ".lna").encode()
            line = name + b" " + f[4] + (b" " + f[7] if f[7] else b"") + b"\n"
            assert open(out, "rb").read() == line * 2, (case, f)


@pytest.mark.gpu
def test_module_on_the_golden_cases(capi):
    from aaltoasr_amd import FstDecoder
    for case in CASES:
        net = R.read_fst(open(os.path.join(GOLDEN, case + ".fst"), "rb").read())
        for f in expected(case)[:3]:
            s = FstDecoder.FstSearch(os.path.join(GOLDEN, case + ".fst"), None, os.path.join(GOLDEN, case + ".dur"))
            s.set_beam(float(f[0]))
            s.set_token_limit(int(f[1]))
            s.set_duration_scale(float(f[2]))
            s.set_transition_scale(float(f[3]))
            s.lna_open(os.path.join(GOLDEN, case + ".lna"), 1024)
            s.init_search()
            s.run()
            s.lna_close()
            text, lp = s.get_result_and_logprob()
            g9 = lambda x: ("%.9g" % x).encode()
            assert [g9(lp), g9(s.get_best_token_logprob()), g9(s.get_best_final_token_logprob()), text] == f[4:] and s.get_result() == text
            ac, _ = R.read_lna(os.path.join(GOLDEN, case + ".lna"))
            want = R.search(net, ac, float(f[0]), int(f[1]), float(f[2]), float(f[3]), R.read_durations(open(os.path.join(GOLDEN, case + ".dur")).read()))
            lines = s.tokens_at_final_states().split(b"\n")
            assert lines[0] == b"Tokens at final nodes:" and len(lines) == 2 + sum(bool(net.node_end[t[0]]) for t in want.tokens)
            first = want.tokens[0]
            assert s.best_tokens(0).split(b"\n")[1] == b"  Token %d %s dur %d '%s '" % (
                first[0], b"%g" % float(first[1]), first[2], b"".join(b" " + net.symbols[w] for w in first[3]))


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
    fst = str(tmp_path / "n.fst")
    open(fst, "wb").write(R.random_net(np.random.default_rng(11), 40, S, max_deg=5, p_word=0.2))
    rec = str(tmp_path / "a.recipe")
    open(rec, "w").write("".join("audio=%s lna=%s speaker=s%d\n" % (w, w[:-4] + ".lna", i) for i, w in enumerate(wavs)))
    spk = str(tmp_path / "s.spkc")      # -S: each utterance its own speaker, each speaker its own normalisation
    open(spk, "w").write("".join("speaker s%d\n{\n  feature normalization\n  {\n    scale %s\n  }\n}\n" % (
        i, " ".join("%.3f" % x for x in rng.uniform(0.8, 1.2, 39))) for i in range(len(wavs))))
    seen = []
    for lnabytes, speakers in (("2", []), ("4", []), ("2", ["-S", spk])):
        r = tool("-b", base, "-c", cfg, "-r", rec, "--lnabytes", lnabytes, *speakers, name="phone_probs")
        assert r.returncode == 0, r.stderr
        seen.append(open(wavs[0][:-4] + ".lna", "rb").read())
        outs = []
        for mode in (["-b", base, "-c", cfg, "--lnabytes", lnabytes] + speakers, ["--lna-files"]):
            out = str(tmp_path / ("out%d.txt" % len(outs)))
            for w in wavs:      # engine mode writes no LNA file: those of phone_probs are moved away while it runs
                if mode[0] == "-b":
                    os.rename(w[:-4] + ".lna", w[:-4] + ".kept")
            r = tool("--fst", fst, "-r", rec, "-o", out, "--beam", "60", *mode)
            assert r.returncode == 0, r.stderr
            for w in wavs:
                if mode[0] == "-b":
                    assert not os.path.exists(w[:-4] + ".lna")
                    os.rename(w[:-4] + ".kept", w[:-4] + ".lna")
            outs.append([l.split(b" ", 1) for l in open(out, "rb").read().split(b"\n") if l])
        assert [l[0] for l in outs[0]] == [w.encode() for w in wavs] and [l[0] for l in outs[1]] == [(w[:-4] + ".lna").encode() for w in wavs]
        assert [l[1] for l in outs[0]] == [l[1] for l in outs[1]] and len(outs[0]) == 2
        # and the restatement on the file's values
        net = R.read_fst(open(fst, "rb").read())
        for w, l in zip(wavs, outs[1]):
            ac, nb = R.read_lna(w[:-4] + ".lna")
            want = R.search(net, ac, beam=60.0)
            assert nb == int(lnabytes) and want.ties == []
            tail = (b" " + want.text(net.symbols) if want.words else b"") + (b" NO_TOKENS" if want.status else b"")
            assert l[1] == ("%.9g" % float(want.logprob)).encode() + tail
    assert seen[0] != seen[2] and len(seen[0]) == len(seen[2])      # the speaker file changed the acoustics


@pytest.mark.gpu
def test_tool_reruns_utterances_that_overflow(capi, tmp_path):
    """--cap-candidates too small for `wide` by less than a factor of two: the tool's own rerun gives the recorded answer; too
    small by more: the line carries the status"""
    case, f = "wide", expected("wide")[0]
    net = R.read_fst(open(os.path.join(GOLDEN, case + ".fst"), "rb").read())
    ac, _ = R.read_lna(os.path.join(GOLDEN, case + ".lna"))
    most = R.search(net, ac, float(f[0]), int(f[1]), float(f[2]), float(f[3]),
                    R.read_durations(open(os.path.join(GOLDEN, case + ".dur")).read())).max_candidates
    assert most > 64
    rec, out = str(tmp_path / "w.recipe"), str(tmp_path / "out.txt")
    lna = os.path.join(GOLDEN, case + ".lna")
    open(rec, "w").write("lna=%s\n" % lna)
    common = ["--fst", os.path.join(GOLDEN, case + ".fst"), "--dur", os.path.join(GOLDEN, case + ".dur"), "-r", rec, "-o", out, "--lna-files"]
    r = tool(*common, "--cap-candidates", str(most - 1))
    assert r.returncode == 0 and b"1 utterances overflowed a capacity" in r.stderr, r.stderr
    assert open(out, "rb").read() == lna.encode() + b" " + f[4] + b" " + f[7] + b"\n"
    r = tool(*common, "--cap-candidates", str(most // 2 - 1))
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == lna.encode() + b" -1 OVERFLOW_CANDIDATES\n"

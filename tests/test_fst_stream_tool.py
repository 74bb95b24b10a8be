"""The fst_stream tool (csrc/aku/main_fst_stream.cc, csrc/fst_live.cc) on the device: its final line is fst_decode's
engine-mode line for the same samples whatever the chunk size, and it writes partial hypotheses while its input is still
open -- the same ones a capi.FstStream gives on the LNA codes phone_probs writes for the same audio."""
import os
import queue
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402

BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
S = 12


def word_loop(rng, words=5) -> bytes:
    """a hub and words of three states with costly self-loops, every node final: the paths keep moving through words (on
    stationary audio they move in step, so a final hub alone would be empty at three frame counts of four), and the
    hypotheses are not empty"""
    lines, node = [b"I 0"], 1
    for w in range(words):
        states = [int(x) for x in rng.integers(0, S, 3)]
        lines.append(b"T 0 %d %d , %.4f" % (node, states[0], -float(np.log(words))))
        for k in range(3):
            lines.append(b"T %d %d %d , -2.5" % (node, node, states[k]))
            if k < 2:
                lines.append(b"T %d %d %d , -0.1" % (node, node + 1, states[k + 1]))
            else:
                lines.append(b"T %d 0 -1 w%d -0.1" % (node, w))
            node += 1
    return R.write_fst(lines + [b"F %d" % n for n in range(node)])


def tool(name, *args, **kw):
    return subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def setup(capi, oracle, tmp_path_factory):
    """a model of a handful of states, the production feature graph, a second of audio as a headerless PCM16 file"""
    from aaltoasr_amd import synth
    d = tmp_path_factory.mktemp("fst_stream_tool")
    rng = np.random.default_rng(7)
    cfg_text = synth.make_feature_config()
    cfg = str(d / "f.cfg")
    open(cfg, "w").write(cfg_text)
    pcm = synth.make_audio(16000, seed=91)
    raw = str(d / "a.raw")
    open(raw, "wb").write(pcm.astype("<i2").tobytes())
    ft = capi.Feat(cfg_text)
    fea = ft.run(pcm, 0, ft.eof_frame(len(pcm)), dtype=np.float64)
    mean, var, off, idx, mw = synth.make_model(D=39, G=36, S=S, comps=3, seed=3)
    mean[:] = fea[rng.integers(0, len(fea), 36)] + 0.3 * rng.standard_normal((36, 39))
    var[:] = rng.uniform(20.0, 40.0, var.shape)      # broad Gaussians: no state outruns the beam, the paths keep moving
    base = str(d / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, mw)
    oracle.write_ph(base + ".ph", S, states_per_hmm=3)
    fst = str(d / "n.fst")
    open(fst, "wb").write(word_loop(np.random.default_rng(11)))
    dur = str(d / "n.dur")
    open(dur, "w").write("4\n%d\n" % S + "".join("%d %.4f %.4f\n" % (i, 1.2 + i / 50.0, 1.0 + i / 40.0) for i in range(S)))      # short stays are the likely ones
    rec = str(d / "a.recipe")
    open(rec, "w").write("audio=%s lna=%s\n" % (raw, str(d / "a.lna")))
    return {"dir": d, "cfg": cfg, "raw": raw, "pcm": pcm.astype("<i2").tobytes(), "base": base, "fst": fst, "dur": dur, "rec": rec,
            "frames": ft.eof_frame(len(pcm))}


@pytest.mark.gpu
@pytest.mark.parametrize("with_dur", [False, True], ids=["plain", "dur"])
@pytest.mark.parametrize("lnabytes", ["2", "4"])
def test_final_line_is_fst_decodes_whatever_the_chunk_size(setup, tmp_path, lnabytes, with_dur):
    common = ["--fst", setup["fst"], "-b", setup["base"], "-c", setup["cfg"], "--lnabytes", lnabytes, "--beam", "200"]
    if with_dur:
        common += ["--dur", setup["dur"], "--dur-by-state"]
    out = str(tmp_path / "out.txt")
    r = tool("fst_decode", *common, "-r", setup["rec"], "-o", out)
    assert r.returncode == 0, r.stderr
    line = open(out, "rb").read()
    assert line.startswith(setup["raw"].encode() + b" ") and line.count(b"\n") == 1
    want = b"-" + line[len(setup["raw"]):]
    assert len(want.split()) > 2, want      # words, not only a number
    for chunk in ("1", "16", "10000"):
        r = tool("fst_stream", *common, "--chunk-frames", chunk, input=setup["pcm"])
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (chunk, r.stdout, want)


@pytest.mark.gpu
def test_partial_lines_arrive_while_the_input_is_open(capi, setup, tmp_path):
    import torch
    chunk = 8
    # what a stream over phone_probs' codes gives, fed the same chunks: a line whenever the partial words change
    r = tool("phone_probs", "-b", setup["base"], "-c", setup["cfg"], "-r", setup["rec"], "--lnabytes", "2")
    assert r.returncode == 0, r.stderr
    lna = open(str(setup["dir"] / "a.lna"), "rb").read()[5:]
    T = len(lna) // (2 * S)
    assert T == setup["frames"]
    capi.check(capi.lib().aasr_set_device(0))
    net = capi.FstNet(setup["fst"])
    s = capi.FstStream(net, 1, T, capi.FstOptions.defaults(beam=200.0))
    want, last = [], ()
    for t in range(0, T, chunk):
        n = min(chunk, T - t)
        d_lna = torch.frombuffer(bytearray(lna[t * 2 * S:(t + n) * 2 * S] + bytes(16)), dtype=torch.uint8).cuda()
        s.feed_dev(d_lna, 2, S, [0], [n])
        s.sync()
        got = s.result(0, want_tokens=False)
        if got["status"] == capi.AASR_FST_OK and got["partial_words"] != last:
            want.append(b" ".join([b"%d" % got["frames_done"], ("%.9g" % float(got["best_logprob"])).encode()] +
                                  [net.symbols[w] for w in got["partial_words"]]))
            last = got["partial_words"]
    final = s.result(0, want_tokens=False)
    s.close()
    half = [w for w in want if int(w.split()[0]) <= T // 2 - 16]
    assert half, want      # a partial hypothesis well inside the first half of the audio

    p = subprocess.Popen([os.path.join(BIN, "fst_stream"), "--fst", setup["fst"], "-b", setup["base"], "-c", setup["cfg"], "--beam", "200",
                          "--chunk-frames", str(chunk), "--partial"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    lines = queue.Queue()

    def reader():
        for l in p.stdout:
            lines.put(l)
        lines.put(None)

    th = threading.Thread(target=reader)
    th.start()
    try:
        pcm = setup["pcm"]
        p.stdin.write(pcm[:len(pcm) // 2])
        p.stdin.flush()
        first = lines.get(timeout=120)      # arrives while the tool's input is still open: it cannot have seen the rest
        assert first is not None and p.poll() is None, p.stderr.read()
        p.stdin.write(pcm[len(pcm) // 2:])
        p.stdin.close()
        got = [first]
        while True:
            l = lines.get(timeout=120)
            if l is None:
                break
            got.append(l)
        assert p.wait(timeout=120) == 0, p.stderr.read()
    finally:
        if p.poll() is None:
            p.kill()
        th.join()
    partial, last_line = [l.rstrip(b"\n") for l in got[:-1]], got[-1]
    frames = [int(l.split()[0]) for l in partial]
    assert frames == sorted(frames) and frames[0] <= T // 2
    assert partial == want
    assert last_line == b"- %s%s\n" % (("%.9g" % float(final["logprob"])).encode(), b" " + final["text"] if final["words"] else b"")

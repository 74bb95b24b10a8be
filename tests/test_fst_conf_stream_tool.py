"""Confidence on a stream at the public surface, on the device: the confidence classes of the FstDecoder module reading a
pipe (lna_open_fd) against the same classes reading the file and against the reference's recorded answers
(tests/golden/fst_conf), and fst_stream --confidence against fst_decode --confidence on the same audio."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fst_conf_restate as CR  # noqa: E402
from test_fst_conf_tool import CASES, FST, GOLDEN, expected, g9  # noqa: E402
from test_fst_stream_tool import S, setup, tool  # noqa: E402,F401  (setup: the module fixture of the fst_stream tool's tests)


def through_a_pipe(obj, data, piece):
    """lna_open_fd + run() on a pipe that a thread fills in pieces (the header in two)"""
    rd, wr = os.pipe()

    def writer():
        for p in [data[:3]] + [data[3 + i:3 + i + piece] for i in range(0, len(data) - 3, piece)]:
            os.write(wr, p)
        os.close(wr)

    th = threading.Thread(target=writer)
    th.start()
    try:
        obj.lna_open_fd(rd, 1024)
        obj.init_search()
        obj.run()
    finally:
        th.join()
        os.close(rd)


def answers(o, loop):
    a = [o.result_and_confidence(), o.get_result_and_logprob(), o.best_tokens(5), o.tokens_at_final_states(), o.get_best_token_logprob(),
         o.get_best_final_token_logprob(), o.status]
    if loop:
        a += [o.get_token_conf(), o.get_ploop_conf(), o.get_edit_conf(), o.get_best_acu_conf()]
    return [np.float32(x).tobytes() if isinstance(x, float) else x for x in a]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_module_on_a_pipe_is_the_module_on_the_file(capi, case, tmp_path):
    from aaltoasr_amd import FstDecoder
    paths = [os.path.join(FST, case + ".fst"), os.path.join(GOLDEN, case + ".ploop.fst"), None, os.path.join(FST, case + ".dur")]
    lna = os.path.join(FST, case + ".lna")
    data = open(lna, "rb").read()
    for f in expected(case)[:2]:
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
        for o, loop in ((s, True), (plain, False)):
            o.lna_open(lna, 1024)
            o.init_search()
            o.run()
            want = answers(o, loop)
            o.lna_close()
            through_a_pipe(o, data, 37)
            assert answers(o, loop) == want, (case, f[:7], loop)
        # the reference's recorded values, from the pipe
        text, conf = s.result_and_confidence()
        assert [text, g9(s.get_token_conf()), g9(s.get_ploop_conf()), g9(s.get_edit_conf()), g9(s.get_best_acu_conf()), g9(conf)] == \
            [f[7], f[9], f[10], f[11], f[12], f[19]], (case, f[:7])
        assert g9(s.get_result_and_logprob()[1]) == f[13] and g9(s.get_best_final_token_logprob()) == f[15]
        assert (plain.result_and_confidence()[0], g9(plain.result_and_confidence()[1])) == (f[7], f[20]), (case, f[:7])
        # lna_open after lna_open_fd selects the file
        rd, wr = os.pipe()
        os.write(wr, data[:5])
        try:
            s.lna_open_fd(rd, 1024)
            s.lna_open(lna, 1024)
            s.init_search()
            s.run()      # (the pipe is still open and empty: reading it would block)
        finally:
            os.close(wr)
            os.close(rd)
        assert g9(s.result_and_confidence()[1]) == f[19]


@pytest.fixture(scope="module")
def ploop(setup):
    path = str(setup["dir"] / "p.fst")
    open(path, "wb").write(CR.random_phone_loop(np.random.default_rng(12), S, n_phones=5, letters=b"w0123456"))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [False, True], ids=["plain", "ploop"])
def test_final_line_is_fst_decode_confidence_whatever_the_chunk_size(setup, ploop, tmp_path, loop):
    common = ["--fst", setup["fst"], "-b", setup["base"], "-c", setup["cfg"], "--beam", "200", "--dur", setup["dur"], "--dur-by-state",
              "--confidence"]
    if loop:
        common += ["--phone-loop", ploop, "--phone-beam", "150", "--phone-token-limit", "400", "--phone-duration-scale", "2"]
    out = str(tmp_path / "out.txt")
    r = tool("fst_decode", *common, "-r", setup["rec"], "-o", out)
    assert r.returncode == 0, r.stderr
    line = open(out, "rb").read()
    assert line.startswith(setup["raw"].encode() + b" ") and line.count(b"\n") == 1
    want = b"-" + line[len(setup["raw"]):]
    f = want.split()
    assert len(f) > 3 and 0.0 <= float(f[2]) <= 1.0, want      # a log-probability, a confidence, words
    for chunk in ("1", "16", "10000"):
        r = tool("fst_stream", *common, "--chunk-frames", chunk, input=setup["pcm"])
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (chunk, r.stdout, want)


@pytest.mark.gpu
def test_without_the_option_the_output_is_the_searchs_and_partial_lines_carry_the_confidence(setup, ploop):
    common = ["--fst", setup["fst"], "-b", setup["base"], "-c", setup["cfg"], "--beam", "200", "--chunk-frames", "8", "--partial"]
    r = tool("fst_stream", *common, input=setup["pcm"])
    assert r.returncode == 0, r.stderr
    plain = r.stdout.split(b"\n")[:-1]
    r = tool("fst_stream", *common, "--confidence", "--phone-loop", ploop, input=setup["pcm"])
    assert r.returncode == 0, r.stderr
    conf = r.stdout.split(b"\n")[:-1]
    # the same lines with one more field: `frames logprob confidence words...`, and `- logprob confidence words...`
    assert len(conf) == len(plain) > 2
    for a, b in zip(plain, conf):
        fa, fb = a.split(b" "), b.split(b" ")
        assert fb[:2] + fb[3:] == fa and float(fb[2]) <= 1.0, (a, b)
    partial, final = conf[:-1], conf[-1].split(b" ")
    assert final[0] == b"-" and all(l.split(b" ")[0].isdigit() for l in partial)
    # the confidence of the last partial line is the final one when it was written at the last chunk
    r16 = tool("fst_stream", *common[:-3], "--chunk-frames", "10000", "--partial", "--confidence", "--phone-loop", ploop, input=setup["pcm"])
    assert r16.returncode == 0, r16.stderr
    one = r16.stdout.split(b"\n")[:-1]
    assert len(one) == 2 and one[0].split(b" ")[2] == one[1].split(b" ")[2] == final[2], one

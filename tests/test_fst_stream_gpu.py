"""Streaming sessions of the FST decoder (aasr_fst_stream_*, csrc/fst_stream.h) against the restatement
tools/fst_restate.py: whatever the chunking, a session after t frames is the batch search of those t frames, bit for
bit -- after every feed, for every session.  frames_done counts the frames consumed, the one that ended the search
included; R.search of that many frames is the yardstick.  No input has a tie (asserted, never skipped)."""
import os
import struct
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fst_restate as R  # noqa: E402
from test_fst_gpu import LIMITS, MODELS, RANDOM, bits, make_inputs, token_set  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
BY_NAME = {c[0]: c for c in RANDOM}


@pytest.fixture(scope="module")
def dev(capi):
    import torch
    capi.check(capi.lib().aasr_set_device(0))
    return torch


class Want:
    """R.search of every prefix that is asked for, computed once per (utterance, frames)"""

    def __init__(self, net, acs, **kw):
        self.net, self.acs, self.kw, self.memo = net, acs, kw, {}

    def at(self, u, t):
        if (u, t) not in self.memo:
            self.memo[(u, t)] = R.search(self.net, self.acs[u][:t], **self.kw)
        return self.memo[(u, t)]

    def frames_done(self, u, fed):
        """the frames a session consumes of `fed`: all of them, or up to and including the one that ends the search"""
        w = self.at(u, fed)
        return fed if w.status == R.OK else w.frames_done + 1


WANTS = {}


def want_of(cfg):
    key = (cfg[0], cfg[6])      # the restatement's answers are shared by every test of a configuration
    if key not in WANTS:
        fst, raws, acs = make_inputs(cfg)
        WANTS[key] = (fst, raws, Want(R.read_fst(fst), acs, beam=cfg[5], token_limit=cfg[6]))
    return WANTS[key]


def open_stream(capi, tmp_path, fst, n_sessions, max_frames, dur_text=None, **opts):
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    net = capi.FstNet(path)
    dur = None
    if dur_text is not None:
        open(path + ".dur", "w").write(dur_text)
        dur = capi.FstDurations(path + ".dur")
    return capi.FstStream(net, n_sessions, max_frames, capi.FstOptions.defaults(**opts), dur=dur)


def feed(torch, s, chunks, lnabytes, n_models=MODELS, pad=True):
    """one feed: session u gets the rows chunks[u] (bytes, maybe none); a row of 0xff between the sessions' rows"""
    w = n_models * lnabytes
    row, row0, n_new, blob = 0, [], [], b""
    for c in chunks:
        row0.append(row)
        n_new.append(len(c) // w)
        blob += c + (b"\xff" * w if pad else b"")
        row += len(c) // w + (1 if pad else 0)
    d_lna = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()
    s.feed_dev(d_lna, lnabytes, n_models, row0, n_new)
    s.sync()


def assert_session(got, want, net, frames_done, what):
    assert want.ties == [], (what, want.ties)
    assert got["frames_done"] == frames_done, (what, got["frames_done"], frames_done)
    assert got["status"] == want.status, (what, got["status"], want.status)
    assert got["n_tokens"] == len(want.tokens), what
    assert token_set(got["tokens"]) == token_set(want.tokens), what
    assert [bits(t[1]) for t in got["tokens"]] == [bits(t[1]) for t in want.tokens], what
    assert (got["words"], got["text"]) == (want.words, want.text(net.symbols)), what
    assert (bits(got["logprob"]), bits(got["best_logprob"]), bits(got["best_final_logprob"])) == \
        (bits(want.logprob), bits(want.best_logprob), bits(want.best_final_logprob)), what
    first = want.tokens[0][3] if want.tokens else ()
    assert got["partial_words"] == first == (got["tokens"][0][3] if got["tokens"] else ()), what
    assert got["partial_text"] == b" ".join(net.symbols[w] for w in first), what


def plan(pattern, frames):
    """per feed, per session: how many frames it gets"""
    n = len(frames)
    if pattern == "whole":
        return [list(frames)]
    if pattern == "single":
        return [[1 if t < frames[u] else 0 for u in range(n)] for t in range(max(frames + [1]))]
    left, out, k = list(frames), [], 0
    while any(left) or not out:      # ragged: 1, 2, 5, 3, 0 in turn, session u starting at phase u
        step = [min(left[u], (1, 2, 5, 3, 0)[(k + u) % 5]) for u in range(n)]
        left = [a - b for a, b in zip(left, step)]
        out.append(step)
        k += 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["whole", "single", "ragged"])
@pytest.mark.parametrize("cfg", RANDOM + LIMITS, ids=lambda c: "%s-%d" % (c[0], c[6]))
def test_every_chunking_is_the_batch_search_at_every_boundary(capi, dev, tmp_path, cfg, pattern):
    fst, raws, want = want_of(cfg)
    frames, w = cfg[4], MODELS * cfg[3]
    s = open_stream(capi, tmp_path, fst, len(frames), max(frames + [1]), beam=cfg[5], token_limit=cfg[6])
    fed = [0] * len(frames)
    steps = plan(pattern, frames)
    if pattern == "ragged" and len(frames) > 2:      # in one launch: nothing for some, more for some, some at their end
        assert any(0 in st and max(st) > 0 for st in steps)
    for k, step in enumerate(steps):
        feed(dev, s, [raws[u][fed[u] * w:(fed[u] + step[u]) * w] for u in range(len(frames))], cfg[3])
        fed = [a + b for a, b in zip(fed, step)]
        for u in range(len(frames)):
            done = want.frames_done(u, fed[u])
            assert_session(s.result(u), want.at(u, done), want.net, done, (cfg[0], pattern, k, u))
    assert fed == list(frames)
    s.close()


def read_golden(case):
    lna = open(os.path.join(GOLDEN, case + ".lna"), "rb").read()
    n_models, lnabytes = struct.unpack(">iB", lna[:5])
    rows = [l.split(b"\t") for l in open(os.path.join(GOLDEN, "expected_%s.txt" % case), "rb").read().split(b"\n") if l]
    return open(os.path.join(GOLDEN, case + ".fst"), "rb").read(), lna[5:], n_models, lnabytes, \
        open(os.path.join(GOLDEN, case + ".dur")).read(), rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["durhi", "rand1", "rand2", "rand4", "toy", "wide"])
def test_golden_cases_in_chunks_of_seven_frames(capi, dev, tmp_path, case):
    fst, raw, n_models, lnabytes, dur, rows = read_golden(case)
    w = n_models * lnabytes
    T = len(raw) // w
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    net = capi.FstNet(path)
    d_all = dev.frombuffer(bytearray(raw + bytes(16)), dtype=dev.uint8).cuda()
    g9 = lambda x: ("%.9g" % float(x)).encode()
    for f in rows:
        opts = dict(beam=float(f[0]), token_limit=int(f[1]), duration_scale=float(f[2]), transition_scale=float(f[3]))
        s = open_stream(capi, tmp_path, fst, 1, max(T, 1), dur_text=dur, **opts)
        for t in range(0, max(T, 1), 7):
            feed(dev, s, [raw[t * w:min(T, t + 7) * w]], lnabytes, n_models)
        got = s.result(0)
        assert [g9(got["logprob"]), g9(got["best_logprob"]), g9(got["best_final_logprob"]), got["text"]] == f[4:], (case, f[:4])
        ref = capi.fst_batch(net, [T], d_all, lnabytes, n_models, [0], capi.FstOptions.defaults(**opts), dur=capi.FstDurations(path + ".dur"))[0]
        assert got["frames_done"] == T and got["status"] == ref["status"] and got["n_tokens"] == ref["n_tokens"]
        assert [(n, bits(lp), d, ws) for n, lp, d, ws in got["tokens"]] == [(n, bits(lp), d, ws) for n, lp, d, ws in ref["tokens"]]
        assert (got["words"], got["text"], bits(got["logprob"]), bits(got["best_logprob"]), bits(got["best_final_logprob"])) == \
            (ref["words"], ref["text"], bits(ref["logprob"]), bits(ref["best_logprob"]), bits(ref["best_final_logprob"]))
        assert got["partial_words"] == (ref["tokens"][0][3] if ref["tokens"] else ())
        s.close()


DUR1 = "4\n1\n0 2.5000 1.2500\n"


@pytest.mark.gpu
def test_durations_carry_over_feed_boundaries(capi, dev, tmp_path):
    # one emitting self-loop node: the token's dur counts the frames, one feed each
    loop = R.write_fst([b"I 0", b"T 0 0 0 , -0.5", b"F 0"])
    ac = (-np.arange(1, 13, dtype=np.float32) / 8).reshape(12, 1)
    s = open_stream(capi, tmp_path, loop, 1, 12, dur_text=DUR1, dur_by_state=1)
    for t in range(12):
        feed(dev, s, [ac[t:t + 1].tobytes()], 4, 1)
        r = s.result(0)
        assert r["frames_done"] == t + 1 and r["tokens"][0][2] == t + 1 and len(r["tokens"]) == 1
    s.close()
    # an arc out of the loop: the term duration_scale * dur_lp[d] with d grown over three feeds
    out = R.write_fst([b"I 0", b"T 0 1 0 , -0.25", b"T 1 1 0 , -0.5", b"T 1 2 0 w -1", b"T 2 2 0 , -0.125", b"F 2"])
    net = R.read_fst(out)
    durations = R.read_durations(DUR1, by_state=True)
    s = open_stream(capi, tmp_path, out, 1, 12, dur_text=DUR1, dur_by_state=1, duration_scale=2.0)
    plain = R.search(net, ac, duration_scale=2.0)
    fed = 0
    for n in (1, 1, 1, 2, 2, 5):
        feed(dev, s, [ac[fed:fed + n].tobytes()], 4, 1)
        fed += n
        want = R.search(net, ac[:fed], duration_scale=2.0, durations=durations)
        assert_session(s.result(0), want, net, fed, fed)
    # the best end-node token spent frames 0 and 1 in node 1 (feeds one and two) and left it with d = 2 in feed three
    assert [t[2] for t in want.tokens if t[0] == 2] == [9] and fed == 12
    assert bits(want.logprob) != bits(plain.logprob)      # and the term is not zero
    s.close()


def start_state(r):
    return (r["status"], r["frames_done"], r["n_tokens"], [(t[0], bits(t[1]), t[2], t[3]) for t in r["tokens"]], r["text"],
            bits(r["logprob"]), bits(r["best_logprob"]), r["partial_words"])


@pytest.mark.gpu
def test_reset_and_independence(capi, dev, tmp_path):
    cfg = BY_NAME["batch8"]
    fst, raws, want = want_of(cfg)
    w = MODELS * cfg[3]
    s = open_stream(capi, tmp_path, fst, 3, 64, beam=cfg[5], token_limit=cfg[6])
    # sessions 0 and 1 on utterances 0 and 5; session 0 is reset after 20 frames and given utterance 7; session 2 gets
    # utterance 7 from the start and was never used before
    feed(dev, s, [raws[0][:20 * w], raws[5][:20 * w], b""], cfg[3])
    assert_session(s.result(0), want.at(0, 20), want.net, 20, "before the reset")
    s.reset(0)
    fed7, fed5 = 0, 20
    for n7, n5 in ((10, 5), (0, 8), (40, 0)):
        feed(dev, s, [raws[7][fed7 * w:(fed7 + n7) * w], raws[5][fed5 * w:(fed5 + n5) * w], raws[7][fed7 * w:(fed7 + n7) * w]], cfg[3])
        fed7, fed5 = fed7 + n7, fed5 + n5
        assert_session(s.result(0), want.at(7, fed7), want.net, fed7, ("reset", fed7))
        assert_session(s.result(2), want.at(7, fed7), want.net, fed7, ("never used", fed7))
        assert_session(s.result(1), want.at(5, fed5), want.net, fed5, ("uninterrupted", fed5))
    assert (fed7, fed5) == (50, 33)
    s.reset(-1)
    end = bool(want.net.node_end[want.net.initial])
    for u in range(3):
        r = s.result(u)
        assert start_state(r) == (capi.AASR_FST_OK, 0, 1, [(want.net.initial, bits(0.0), 0, ())], b"",
                                  bits(0.0 if end else -1.0), bits(0.0), ())
    feed(dev, s, [b"", raws[1], b""], cfg[3])      # a feed of nothing starts a fresh session: still the start state
    assert start_state(s.result(0)) == start_state(s.result(2)) and s.result(0)["frames_done"] == 0
    assert_session(s.result(0), want.at(0, 0), want.net, 0, "fresh, fed nothing")
    assert_session(s.result(1), want.at(1, 3), want.net, 3, "after reset(-1)")
    s.close()


@pytest.mark.gpu
def test_sticky_statuses(capi, dev, tmp_path):
    # the dead end: node 1 has no arc out
    dead = R.write_fst([b"I 0", b"T 0 1 0", b"F 1"])
    net = R.read_fst(dead)
    ac = np.zeros((6, 1), np.float32)
    full = R.search(net, ac)
    assert full.status == R.NO_TOKENS and full.frames_done == 1
    s = open_stream(capi, tmp_path, dead, 1, 6)
    feed(dev, s, [ac[:1].tobytes()], 4, 1)
    assert_session(s.result(0), R.search(net, ac[:1]), net, 1, "one frame")
    feed(dev, s, [ac[1:3].tobytes()], 4, 1)      # frame 1 (the restatement's frames_done) finds no candidate
    r = s.result(0)
    assert_session(r, R.search(net, ac[:2]), net, 2, "the dead end")
    assert r["status"] == capi.AASR_FST_NO_TOKENS and r["tokens"] == []
    for _ in range(2):
        feed(dev, s, [ac[3:4].tobytes()], 4, 1)
        assert start_state(s.result(0)) == start_state(r) and s.result(0)["status"] == capi.AASR_FST_NO_TOKENS
    s.reset(0)
    feed(dev, s, [ac[:1].tobytes()], 4, 1)
    assert_session(s.result(0), R.search(net, ac[:1]), net, 1, "after the reset")
    s.close()

    # too few candidates on `large`, beside a session on `tiny`'s input and capacities that suffice for it
    big, small = BY_NAME["large"], BY_NAME["tiny"]
    fst, raws, want = want_of(big)
    _, raws_small, _ = make_inputs(small)
    acs_small = R.decode_lna(raws_small[2], MODELS, 4)
    most = want.at(1, 40).max_candidates
    at = next(t for t in range(1, 41) if want.at(1, t).max_candidates > most // 2)      # the frame that overflows
    assert most > 16 and at > 2
    assert R.search(want.net, acs_small, beam=big[5], token_limit=big[6]).max_candidates <= most // 2
    caps = dict(beam=big[5], token_limit=big[6], cap_candidates=most // 2)
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    d_all = dev.frombuffer(bytearray(raws[1] + bytes(16)), dtype=dev.uint8).cuda()
    ref = capi.fst_batch(capi.FstNet(path), [40], d_all, 4, MODELS, [0], capi.FstOptions.defaults(**caps), rerun=False)[0]
    assert ref["status"] == capi.AASR_FST_OVERFLOW_CANDIDATES
    s = open_stream(capi, tmp_path, fst, 2, 40, **caps)
    w = MODELS * 4
    net = want.net
    fed = 0
    for n in (1, 1, 38):
        feed(dev, s, [raws[1][fed * w:(fed + n) * w], raws_small[2][fed * w:(fed + n) * w]], 4)
        fed += n
    got = s.result(0)
    assert (got["status"], got["tokens"], got["text"], bits(got["logprob"]), bits(got["best_logprob"]), bits(got["best_final_logprob"])) == \
        (ref["status"], ref["tokens"], ref["text"], bits(ref["logprob"]), bits(ref["best_logprob"]), bits(ref["best_final_logprob"]))
    assert got["frames_done"] == at and got["partial_words"] == ()
    assert_session(s.result(1), R.search(net, acs_small, beam=big[5], token_limit=big[6]), net, 2, "the neighbour")
    s.reset(0)
    feed(dev, s, [raws[1][:(at - 1) * w], b""], 4)
    assert_session(s.result(0), want.at(1, at - 1), net, at - 1, "after the reset")
    s.close()


@pytest.mark.gpu
def test_refused_feeds_change_nothing(capi, dev, tmp_path):
    cfg = BY_NAME["mid2"]
    fst, raws, want = want_of(cfg)
    w = MODELS * 2
    s = open_stream(capi, tmp_path, fst, 1, 31, beam=cfg[5], token_limit=cfg[6])
    feed(dev, s, [raws[0][:20 * w]], 2)
    before = s.result(0)
    d = dev.frombuffer(bytearray(raws[0] + bytes(16)), dtype=dev.uint8).cuda()
    rows = d.numel() // w
    bad = [dict(lnabytes=2, n_models=MODELS, row0=[0], n_new=[12]),                  # past max_frames
           dict(lnabytes=2, n_models=MODELS, row0=[rows - 3], n_new=[4]),            # rows outside the buffer
           dict(lnabytes=2, n_models=MODELS, row0=[-1], n_new=[2]),
           dict(lnabytes=2, n_models=MODELS, row0=[0], n_new=[-1]),
           dict(lnabytes=2, n_models=want.net.node_pdf.max(), row0=[0], n_new=[1]),  # the network's largest pdf is no model
           dict(lnabytes=4, n_models=MODELS, row0=[0], n_new=[1])]                   # another width mid-utterance
    for kw in bad:
        with pytest.raises(capi.AasrError) as ei:
            s.feed_dev(d, kw["lnabytes"], int(kw["n_models"]), kw["row0"], kw["n_new"])
        assert ei.value.code == capi.AASR_ERR_INVALID and "aasr_fst_stream_feed_dev" in ei.value.msg, kw
        after = s.result(0)      # (no sync needed: nothing was queued)
        assert start_state(after) == start_state(before) and after["words"] == before["words"], kw
    feed(dev, s, [raws[0][20 * w:]], 2)
    assert_session(s.result(0), want.at(0, 31), want.net, 31, "the rest")
    s.close()


@pytest.mark.gpu
def test_lna_open_fd_reads_a_pipe_as_it_fills(capi, dev):
    from aaltoasr_amd import FstDecoder
    path = os.path.join(GOLDEN, "rand2.lna")
    data = open(path, "rb").read()
    s = FstDecoder.FstSearch(os.path.join(GOLDEN, "rand2.fst"), None, os.path.join(GOLDEN, "rand2.dur"))
    s.set_beam(60.0)
    s.lna_open(path, 1024)
    s.init_search()
    s.run()
    want = (s.get_result_and_logprob(), s.best_tokens(5), s.tokens_at_final_states(), s.get_best_token_logprob(),
            s.get_best_final_token_logprob())
    s.lna_close()
    rd, wr = os.pipe()

    def writer():
        pieces = [data[:3]] + [data[3 + i:3 + i + 1000] for i in range(0, len(data) - 3, 1000)]      # the header in two pieces
        for p in pieces:
            os.write(wr, p)
        os.close(wr)

    th = threading.Thread(target=writer)
    th.start()
    try:
        s.lna_open_fd(rd, 1024)
        s.init_search()
        s.run()
    finally:
        th.join()
        os.close(rd)
    got = (s.get_result_and_logprob(), s.best_tokens(5), s.tokens_at_final_states(), s.get_best_token_logprob(),
           s.get_best_final_token_logprob())
    assert got == want and want[0][0] != b""

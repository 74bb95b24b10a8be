"""FST decoder confidence on the device (csrc/fst_conf.hip, csrc/fst_conf.cc) against the restatement
tools/fst_conf_restate.py and the reference's recorded answers (tests/golden/fst_conf): the frame-best pass and its sums,
the token records, the handle's ten floats, batches, the overflow rerun, and the plain search beside it -- all for exact
equality of bits.  Every search input is one for which the restatement reports no tie (asserted, never skipped); the
seeds of RANDOM were chosen on the CPU with `python tests/test_fst_conf_gpu.py`."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402
import fst_conf_restate as CR  # noqa: E402

FST = os.path.join(ROOT, "tests", "golden", "fst")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst_conf")
CASES = ["durhi", "rand1", "rand2", "rand4", "toy"]
FIELDS = ("token_conf", "ploop_conf", "edit_conf", "best_acu_conf", "grammar_logprob", "ploop_logprob", "best_final_logprob",
          "best_different_logprob", "best_acu_score")
MODELS = 9


def bits(x) -> bytes:
    return np.float32(x).tobytes()


def g9(x) -> bytes:
    return ("%.9g" % float(x)).encode()


@pytest.fixture(scope="module")
def dev(capi):
    import torch
    capi.check(capi.lib().aasr_set_device(0))
    return torch


# ---- frame best --------------------------------------------------------------------------------------------------------

FRAMES = [0, 1, 2, 37]


def frame_best_rows(lnabytes, n_models):
    """40 rows (raw bytes [40, n_models * lnabytes]) with the maximum planted in the first column, the last column, twice,
    and (4-byte) rows of -inf and rows that mix -inf, +0 and -0"""
    rng = np.random.default_rng([lnabytes, n_models])
    n = sum(FRAMES)
    if lnabytes == 4:
        v = (-rng.random((n, n_models)) * 30 - 0.5).astype(np.float32)
        v[1, 0] = -0.25
        v[2, -1] = -0.125
        v[3, 0] = v[3, -1] = -0.375
        v[4, n_models // 2] = v[4, 0] = -0.0625
        v[5, :] = -np.inf
        v[6, ::2] = -np.inf
        v[7, -1] = 0.0
        v[8, 0] = -0.0
        v[8, -1] = 0.0          # the loop keeps the first of the two zeros
        v[9, 0] = 0.0
        v[9, -1] = -0.0
        return v.view(np.uint8).reshape(n, -1).copy(), v
    hi = 60000 if lnabytes == 2 else 256
    c = rng.integers(hi // 4, hi, (n, n_models))
    c[1, 0] = 7
    c[2, -1] = 3
    c[3, 0] = c[3, -1] = 5
    c[4, n_models // 2] = c[4, 0] = 0
    c[5, :] = hi - 1
    c[6, -1] = 256 if lnabytes == 2 else 1      # low byte zero: a byte-order slip would rank it first
    c[7, 0] = 255 if lnabytes == 2 else 2
    raw = c.astype(">u2").view(np.uint8).reshape(n, -1).copy() if lnabytes == 2 else c.astype(np.uint8)
    return raw, R.decode_lna(raw.tobytes(), n_models, lnabytes)


@pytest.mark.gpu
@pytest.mark.parametrize("n_models", [1, 3, 63, 64, 65, 257, 1031])
@pytest.mark.parametrize("lnabytes", [1, 2, 4])
def test_frame_best_and_its_sums(capi, dev, lnabytes, n_models):
    raw, ac = frame_best_rows(lnabytes, n_models)
    # the utterances' rows scattered over a larger buffer, out of order, with rows of 0xff between them, and the whole
    # buffer one element off the allocation's start: no row starts on a 16-byte boundary by luck
    order, at, row0, src = [3, 1, 0, 2], 2, [0] * 4, [0] * 4
    first = np.concatenate([[0], np.cumsum(FRAMES)])
    for u in order:
        row0[u] = at
        at += FRAMES[u] + 3
    buf = np.full((at, n_models * lnabytes), 0xff, np.uint8)
    if lnabytes == 4:
        buf.view(np.float32)[:] = 1e30      # (a row read by mistake would win)
    for u in range(4):
        buf[row0[u]:row0[u] + FRAMES[u]] = raw[first[u]:first[u + 1]]
    blob = bytes(lnabytes) + buf.tobytes() + bytes(16)
    d_all = dev.frombuffer(bytearray(blob), dtype=dev.uint8).cuda()
    d_lna = d_all[lnabytes:]
    assert d_lna.data_ptr() % 16 == lnabytes
    net = capi.FstNet(os.path.join(FST, "toy.fst"))
    runs = [capi.fst_frame_best(FRAMES, d_lna, lnabytes, n_models, row0, net) for _ in range(2)]
    for u in range(4):
        want = CR.frame_best(ac[first[u]:first[u + 1]])
        got, s = runs[0][u]
        assert got.tobytes() == want.tobytes(), (u, got, want)
        assert bits(s) == bits(CR.frame_best_sum(ac[first[u]:first[u + 1]])), u
        assert runs[1][u][0].tobytes() == got.tobytes() and bits(runs[1][u][1]) == bits(s)
    assert bits(runs[0][0][1]) == bits(0.0)
    if lnabytes == 4 and n_models > 1:
        b = runs[0][3][0]      # rows 3 ... 39: planted rows 5, 8, 9 are its frames 2, 5, 6
        assert bits(b[2]) == bits(-999999999.9) and bits(b[5]) == bits(-0.0) and bits(b[6]) == bits(0.0)


# ---- searches ------------------------------------------------------------------------------------------------------------

#          name     seed nodes lnabytes frames             beam  limit
RANDOM = [("mid",    12,  37, 2, [40, 3, 17, 1, 0, 33],     25.0, 300),
          ("big",     2, 300, 4, [20, 31],                  30.0, 257),
          ("one",    78,  37, 2, [30, 12, 5],               0.0,  5000),
          ("limit1",  0,  60, 1, [10, 25, 7],               2600.0, 1),
          ("open",    1,  23, 4, [12, 9],                   2600.0, 5000)]


def make_inputs(cfg):
    name, seed, nodes, lnabytes, frames, _, _ = cfg
    rng = np.random.default_rng([seed, nodes, lnabytes, 77])
    fst = R.random_net(rng, nodes, MODELS, max_deg=6, p_word=0.15)
    raws = []
    for T in frames:
        if lnabytes == 4:
            raws.append((-rng.random((T, MODELS)) * 9).astype("<f4").tobytes())
        elif lnabytes == 2:
            raws.append(rng.integers(0, 20000, (T, MODELS)).astype(">u2").tobytes())
        else:
            raws.append(rng.integers(0, 256, (T, MODELS)).astype(np.uint8).tobytes())
    return fst, raws, [R.decode_lna(r, MODELS, lnabytes) for r in raws]


def upload(torch, raws, n_models, lnabytes):
    row, row0 = 0, []
    for r in raws:      # a row of padding between the utterances
        row0.append(row)
        row += len(r) // (n_models * lnabytes) + 1
    blob = b"".join(r + b"\xff" * (n_models * lnabytes) for r in raws)
    return torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda(), row0, [len(r) // (n_models * lnabytes) for r in raws]


def device_conf(capi, torch, tmp_path, fst, raws, lnabytes, n_models=MODELS, ploop=None, dur_path=None, gopt=None, popt=None, **kw):
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    net, pnet = capi.FstNet(path), None
    if ploop is not None:
        open(path + ".ploop", "wb").write(ploop)
        pnet = capi.FstNet(path + ".ploop")
    o = capi.FstConfOptions.defaults(phone_loop=1 if ploop is not None else 0)
    for k, v in (gopt or {}).items():
        setattr(o.grammar, k, v)
    for k, v in (popt or {}).items():
        setattr(o.phone, k, v)
    d_lna, row0, T = upload(torch, raws, n_models, lnabytes)
    dur = capi.FstDurations(dur_path) if dur_path else None
    return capi.fst_conf_batch(net, pnet, T, d_lna, lnabytes, n_models, row0, o, dur=dur, want_tokens=True, **kw)


def assert_record(rec, result, end, what):
    """the device's token record against the restatement's scan of Result.tokens"""
    assert result.ties == [], (what, result.ties)
    has_final, words, bf, bd, has_diff = CR.best_different(result.tokens, end)
    assert (rec["has_final"], rec["n_words"] == 0, rec["has_different"]) == (int(has_final), len(words) == 0, int(has_diff)), (what, rec)
    assert rec["n_words"] == len(words), what
    assert bits(rec["best_final_logprob"]) == bits(bf) and bits(rec["best_different_logprob"]) == bits(bd), (what, rec, bf, bd)


def assert_conf(got, want, what):
    for k in CR.FLOATS:
        assert bits(got[k]) == bits(want.r[k]), (what, k, got[k], want.r[k])
    assert got["no_final"] == int(want.no_final) and got["valid"] == 1 and got["text"] == want.text, what


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", RANDOM, ids=lambda c: c[0])
def test_token_records_on_random_networks(capi, dev, tmp_path, cfg):
    fst, raws, acs = make_inputs(cfg)
    net = R.read_fst(fst)
    g = dict(beam=cfg[5], token_limit=cfg[6])
    got = device_conf(capi, dev, tmp_path, fst, raws, cfg[3], gopt=g)
    seen = set()
    for u, ac in enumerate(acs):
        want = CR.confidence(net, ac, g)
        assert_record(got[u]["grammar"]["record"], want.grammar, net.node_end, (cfg[0], u))
        assert_conf(got[u], want, (cfg[0], u))
        assert got[u]["phone"] is None and got[u]["best_acu_score"] == 0
        seen.add(("final" if not want.no_final else "nofinal", "diff" if want.has_different else "alone", "words" if want.n_words else "empty"))
    if cfg[0] in ("one", "limit1"):      # one hypothesis survives, or two tokens at the most
        assert all(len(CR.confidence(net, ac, g).grammar.tokens) <= (1 if cfg[0] == "one" else 2) for ac in acs)
    if cfg[0] == "mid":
        assert len(seen) >= 3, seen


def one_utt(capi, dev, tmp_path, lines, frames, **g):
    fst = R.write_fst(lines)
    ac = np.zeros((frames, 1), np.float32)
    got = device_conf(capi, dev, tmp_path, fst, [ac.tobytes()], 4, n_models=1, gopt=g)[0]
    net = R.read_fst(fst)
    want = CR.confidence(net, ac, g)
    assert_record(got["grammar"]["record"], want.grammar, net.node_end, lines)
    assert_conf(got, want, lines)
    return got


@pytest.mark.gpu
def test_token_records_on_hand_networks(capi, dev, tmp_path):
    none = np.float32(-9999999.9)
    # two hypotheses at end nodes, and a third with the winner's words elsewhere: the different one is "b", not the copy
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 -1 a -1", b"T 0 2 -1 b -3", b"T 0 3 -1 a -2", b"F 1", b"F 2"], 1)
    assert got["best_different_logprob"] == -3 and got["best_final_logprob"] == -1 and got["token_conf"] == 1
    # a better token outside the end nodes with other words: token_conf clamps at 0
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 -1 a -3", b"T 0 2 -1 b -1", b"F 1"], 1)
    assert got["best_different_logprob"] == -1 and got["token_conf"] == 0
    # only one hypothesis: the sentinel
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 -1 a -1", b"T 0 2 -1 a -3", b"F 1"], 1)
    assert bits(got["best_different_logprob"]) == bits(none) and got["grammar"]["record"]["has_different"] == 0 and got["token_conf"] == 1
    # token limit 1 keeps two tokens
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 -1 a -1", b"T 0 2 -1 b -2", b"T 0 3 -1 c -3", b"F 1", b"F 3"], 1, token_limit=1)
    assert got["grammar"]["n_tokens"] == 2 and got["best_different_logprob"] == -2
    # the best end-node token has no words: "Emptiness"
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 -1 , -1", b"T 0 2 -1 b -2", b"F 1", b"F 2"], 1)
    assert bits(got["token_conf"]) == bits(none) and got["no_final"] == 0 and got["grammar"]["record"]["n_words"] == 0
    assert got["grammar"]["record"]["has_different"] == 1
    # no token at an end node
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 0 0 w"], 2)
    assert got["no_final"] == 1 and bits(got["token_conf"]) == bits(none) and bits(got["best_final_logprob"]) == bits(none)
    assert got["grammar_logprob"] == -1
    # zero frames: the start token at an end node
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 0 0 w", b"F 0"], 0)
    assert got["frames"] == 0 and got["no_final"] == 0
    # no tokens at all
    got = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 0", b"F 1"], 3)
    assert got["grammar_status"] == capi.AASR_FST_NO_TOKENS and got["no_final"] == 1 and got["valid"] == 1


# ---- the handle on the golden cases --------------------------------------------------------------------------------------

def golden(case):
    fst = open(os.path.join(FST, case + ".fst"), "rb").read()
    ploop = open(os.path.join(GOLDEN, case + ".ploop.fst"), "rb").read()
    lna = open(os.path.join(FST, case + ".lna"), "rb").read()
    n_models, lnabytes = struct.unpack(">iB", lna[:5])
    rows = []
    for line in open(os.path.join(GOLDEN, "expected_conf_%s.txt" % case), "rb").read().split(b"\n"):
        if line:
            f = line.split(b"\t")
            g = dict(beam=float(f[0]), token_limit=int(f[1]), duration_scale=float(f[2]), transition_scale=float(f[3]))
            p = dict(beam=float(f[4]), token_limit=int(f[5]), duration_scale=float(f[6]), transition_scale=1.0)
            rows.append((g, p, f[7:]))
    return fst, ploop, lna[5:], n_models, lnabytes, os.path.join(FST, case + ".dur"), rows


@pytest.fixture(scope="module")
def restated():
    """the restatement of every golden row, computed once: case -> [(with phone loop, plain)]"""
    out = {}
    for case in CASES:
        fst, ploop, raw, n_models, lnabytes, dur, rows = golden(case)
        net, pnet = R.read_fst(fst), R.read_fst(ploop)
        ac, d = R.decode_lna(raw, n_models, lnabytes), R.read_durations(open(dur).read())
        out[case] = [(CR.confidence(net, ac, g, d, pnet, p), CR.confidence(net, ac, g, d)) for g, p, _ in rows]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_golden_rows_against_the_reference_and_the_restatement(capi, dev, tmp_path, restated, case):
    fst, ploop, raw, n_models, lnabytes, dur, rows = golden(case)
    net, pnet = R.read_fst(fst), R.read_fst(ploop)
    for (g, p, f), (want, plain) in zip(rows, restated[case]):
        got = device_conf(capi, dev, tmp_path, fst, [raw], lnabytes, n_models, ploop=ploop, dur_path=dur, gopt=g, popt=p)[0]
        assert [got["text"], got["phone"]["text"]] + [g9(got[k]) for k in FIELDS] + [b"%d" % got["frames"], g9(got["confidence"])] == f[:-1], (case, g, p)
        assert_conf(got, want, (case, g, p))
        assert_record(got["grammar"]["record"], want.grammar, net.node_end, (case, g))
        assert_record(got["phone"]["record"], want.phone, pnet.node_end, (case, p))
        assert (got["grammar_status"], got["phone_status"], got["reran"]) == (0, 0, False)
        one = device_conf(capi, dev, tmp_path, fst, [raw], lnabytes, n_models, dur_path=dur, gopt=g)[0]      # the plain FstConfidence
        assert g9(one["confidence"]) == f[-1], (case, g)
        assert_conf(one, plain, (case, g, "plain"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_a_batch_in_one_launch_equals_the_singles(capi, dev, tmp_path, case):
    fst, ploop, raw, n_models, lnabytes, dur, rows = golden(case)
    g, p, _ = rows[1]
    row = n_models * lnabytes
    T = len(raw) // row
    raws = [raw, raw[:(T // 2) * row], b"", raw[:row], raw]
    kw = dict(ploop=ploop, dur_path=dur, gopt=g, popt=p)
    batch = device_conf(capi, dev, tmp_path, fst, raws, lnabytes, n_models, **kw)
    for u, r in enumerate(raws[:4]):
        single = device_conf(capi, dev, tmp_path, fst, [r], lnabytes, n_models, **kw)[0]
        for k in CR.FLOATS:
            assert bits(batch[u][k]) == bits(single[k]) or (np.isnan(batch[u][k]) and np.isnan(single[k])), (case, u, k)
        assert (batch[u]["text"], batch[u]["phone"]["text"], batch[u]["no_final"]) == (single["text"], single["phone"]["text"], single["no_final"])
        assert batch[u]["grammar"]["record"] == single["grammar"]["record"] and batch[u]["phone"]["record"] == single["phone"]["record"]
    assert all(bits(batch[4][k]) == bits(batch[0][k]) for k in CR.FLOATS)
    # zero frames: against the restatement (the reference is not asked)
    net, pnet = R.read_fst(fst), R.read_fst(ploop)
    want = CR.confidence(net, np.zeros((0, n_models), np.float32), g, R.read_durations(open(dur).read()), pnet, p)
    for k in CR.FLOATS:
        assert bits(batch[2][k]) == bits(want.r[k]) or (np.isnan(batch[2][k]) and np.isnan(want.r[k])), (case, k, batch[2][k], want.r[k])


@pytest.mark.gpu
def test_overflow_is_reported_and_the_rerun_succeeds(capi, dev, tmp_path, restated):
    case = "rand4"
    fst, ploop, raw, n_models, lnabytes, dur, rows = golden(case)
    g, p, _ = rows[0]
    want = restated[case][0][0]
    hist = len(want.grammar.histories)
    assert hist > 4
    cap = 1
    while 2 * cap - 2 * cap // 4 < hist:      # the largest power of two whose three quarters do not hold the histories
        cap *= 2
    for which in ("grammar", "phone"):
        if which == "phone":
            hist = len(want.phone.histories)
            cap = 1
            while 2 * cap - 2 * cap // 4 < hist:
                cap *= 2
        kw = dict(ploop=ploop, dur_path=dur, gopt=dict(g, **({"cap_history": cap} if which == "grammar" else {})),
                  popt=dict(p, **({"cap_history": cap} if which == "phone" else {})))
        got = device_conf(capi, dev, tmp_path, fst, [raw], lnabytes, n_models, rerun=False, **kw)[0]
        assert got[which + "_status"] == capi.AASR_FST_OVERFLOW_HISTORY and got["valid"] == 0 and got["confidence"] is None, which
        got = device_conf(capi, dev, tmp_path, fst, [raw], lnabytes, n_models, **kw)[0]
        assert got["reran"], which
        assert_conf(got, want, which)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_plain_search_is_what_it_was(capi, dev, tmp_path, restated, case):
    """aasr_fst_batch_* for the same inputs against fst_restate, and the confidence batch's inner results equal to it"""
    fst, ploop, raw, n_models, lnabytes, dur, rows = golden(case)
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    net = capi.FstNet(path)
    d_lna, row0, T = upload(dev, [raw], n_models, lnabytes)
    rnet = R.read_fst(fst)
    for (g, p, _), (want, _) in list(zip(rows, restated[case]))[:3]:
        got = capi.fst_batch(net, T, d_lna, lnabytes, n_models, row0, capi.FstOptions.defaults(**g), dur=capi.FstDurations(dur))[0]
        w = want.grammar
        tok = lambda ts: sorted((int(n), bits(lp), int(d), tuple(ws)) for n, lp, d, ws in ts)
        assert got["status"] == w.status and tok(got["tokens"]) == tok(w.tokens)
        assert (got["words"], got["text"]) == (w.words, w.text(rnet.symbols))
        assert (bits(got["logprob"]), bits(got["best_logprob"]), bits(got["best_final_logprob"])) == (bits(w.logprob), bits(w.best_logprob), bits(w.best_final_logprob))
        inner = device_conf(capi, dev, tmp_path, fst, [raw], lnabytes, n_models, ploop=ploop, dur_path=dur, gopt=g, popt=p)[0]["grammar"]
        assert tok(inner["tokens"]) == tok(got["tokens"]) and inner["text"] == got["text"] and bits(inner["logprob"]) == bits(got["logprob"])


if __name__ == "__main__":      # seed search on the CPU: the first seed of every configuration without a tie
    for cfg in RANDOM:
        for seed in range(200):
            c = (cfg[0], seed) + cfg[2:]
            fst, raws, acs = make_inputs(c)
            net = R.read_fst(fst)
            out = [CR.confidence(net, ac, dict(beam=c[5], token_limit=c[6])) for ac in acs]
            ok = not any(o.ties for o in out)
            if cfg[0] in ("mid", "big", "open"):
                ok = ok and sum(not o.no_final and o.n_words > 0 for o in out) >= (len(out) + 1) // 2
            if cfg[0] == "mid":
                ok = ok and len({(o.no_final, o.has_different, o.n_words > 0) for o in out}) >= 3
            if ok:
                print(c, [(o.grammar.status, len(o.grammar.tokens), o.no_final, o.has_different, o.n_words) for o in out])
                break
        else:
            print("NO SEED", cfg)

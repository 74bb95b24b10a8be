"""FST decoder on the device against the restatement tools/fst_restate.py: every final token (node, log-probability bits,
dur, words), the three log-probabilities and the result string, for exact equality -- both sides perform the same IEEE
float operations in the same order.  Every input is one for which the restatement reports no tie (asserted, never
skipped): the seeds below were chosen on the CPU with `python tests/test_fst_gpu.py`, which prints the first tie-free
seed of every configuration."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
HEAD = b"#FSTBasic MaxPlus\n"
MODELS = 9

#          name      seed nodes lnabytes frames                          beam   limit
RANDOM = [("tiny",     0,   5, 4, [0, 1, 2],                             2600.0, 5000),
          ("batch8",  26,  37, 2, [64, 3, 17, 1, 0, 33, 2, 50],          25.0,   300),
          ("large",    2, 400, 4, [20, 40],                              30.0,   400),
          ("mid2",     3, 120, 2, [31],                                  40.0,   5000),
          ("bytes1",   0,  60, 1, [10, 25, 7],                           30.0,   200),
          ("open",     0,  23, 4, [12, 9],                               2600.0, 5000)]
#          the token limit at the workgroup's size and around it, on a network with more distinct (node, words) than that
LIMITS = [("limits", 0, 400, 4, [14], 2600.0, limit) for limit in (1, 3, 255, 256, 257)]


def make_inputs(cfg):
    """the network's text, per utterance the raw LNA rows (bytes) and the decoded float32 values"""
    name, seed, nodes, lnabytes, frames, _, _ = cfg
    rng = np.random.default_rng([seed, nodes, lnabytes])
    fst = R.random_net(rng, nodes, MODELS, max_deg=6, p_word=0.1)
    raws = []
    for T in frames:
        if lnabytes == 4:
            raws.append((-rng.random((T, MODELS)) * 9).astype("<f4").tobytes())
        elif lnabytes == 2:
            raws.append(rng.integers(0, 20000, (T, MODELS)).astype(">u2").tobytes())
        else:
            raws.append(rng.integers(0, 256, (T, MODELS)).astype(np.uint8).tobytes())
    return fst, raws, [R.decode_lna(r, MODELS, lnabytes) for r in raws]


def restate(cfg, fst, acs, durations=None, **kw):
    net = R.read_fst(fst)
    out = [R.search(net, ac, cfg[5], cfg[6], durations=durations, **kw) for ac in acs]
    return net, out


@pytest.fixture(scope="module")
def dev(capi):
    import torch
    capi.check(capi.lib().aasr_set_device(0))
    return torch


def device_run(capi, torch, tmp_path, fst, raws, lnabytes, n_models=MODELS, dur_text=None, **opts):
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(fst)
    net = capi.FstNet(path)
    dur = None
    if dur_text is not None:
        open(path + ".dur", "w").write(dur_text)
        dur = capi.FstDurations(path + ".dur")
    rerun = opts.pop("rerun", True)
    row, row0 = 0, []
    for r in raws:      # a row of padding between the utterances: row0 is honoured, not assumed
        row0.append(row)
        row += len(r) // (n_models * lnabytes) + 1
    blob = b"".join(r + b"\xff" * (n_models * lnabytes) for r in raws)
    d_lna = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    T = [len(r) // (n_models * lnabytes) for r in raws]
    return capi.fst_batch(net, T, d_lna, lnabytes, n_models, row0, capi.FstOptions.defaults(**opts), dur=dur, rerun=rerun)


def bits(x) -> bytes:
    return np.float32(x).tobytes()


def token_set(tokens):
    return sorted((int(n), bits(lp), int(d), tuple(w)) for n, lp, d, w in tokens)


def assert_same(got, want, net, what=""):
    assert want.ties == [], (what, want.ties)
    assert got["status"] == want.status, (what, got["status"], want.status)
    assert token_set(got["tokens"]) == token_set(want.tokens), what
    assert [bits(t[1]) for t in got["tokens"]] == [bits(t[1]) for t in want.tokens], what      # descending, as the reference's list
    assert (got["words"], got["text"]) == (want.words, want.text(net.symbols)), what
    assert (bits(got["logprob"]), bits(got["best_logprob"]), bits(got["best_final_logprob"])) == \
        (bits(want.logprob), bits(want.best_logprob), bits(want.best_final_logprob)), what


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", RANDOM + LIMITS, ids=lambda c: "%s-%d" % (c[0], c[6]))
def test_random_networks(capi, dev, tmp_path, cfg):
    fst, raws, acs = make_inputs(cfg)
    net, want = restate(cfg, fst, acs)
    got = device_run(capi, dev, tmp_path, fst, raws, cfg[3], beam=cfg[5], token_limit=cfg[6])
    for u in range(len(raws)):
        assert_same(got[u], want[u], net, (cfg[0], u))
        assert not got[u]["reran"]
    if cfg[0] == "limits":      # more distinct candidates than the limit keeps, and exactly limit + 1 kept
        assert want[0].max_keys > cfg[6] + 1 and len(want[0].tokens) == cfg[6] + 1 == got[0]["n_tokens"]
    if cfg[0] == "open":        # a beam that cuts nothing: every distinct (node, words) of the last frame survives
        assert all(len(w.tokens) == w.last_keys for w in want)


@pytest.mark.gpu
def test_beam_that_cuts_to_one_token(capi, dev, tmp_path):
    cfg = ("batch8", 42, 37, 2, [64, 3, 17, 1, 0, 33, 2, 50], 0.0, 5000)
    fst, raws, acs = make_inputs(cfg)
    net, want = restate(cfg, fst, acs)
    got = device_run(capi, dev, tmp_path, fst, raws, 2, beam=0.0)
    for u in range(len(raws)):
        assert_same(got[u], want[u], net, u)
        assert got[u]["n_tokens"] == (1 if want[u].status == R.OK else 0)
    assert sum(w.status == R.OK for w in want) >= 4


def one_utt(capi, dev, tmp_path, lines, frames, **opts):
    fst = R.write_fst(lines)
    ac = np.zeros((frames, 1), np.float32)
    got = device_run(capi, dev, tmp_path, fst, [ac.tobytes()], 4, n_models=1, **opts)[0]
    net = R.read_fst(fst)
    kw = {k: v for k, v in opts.items() if k in ("beam", "token_limit")}
    want = R.search(net, ac, **kw)
    return got, want, net


@pytest.mark.gpu
def test_recombination_is_on_node_and_word_sequence(capi, dev, tmp_path):
    # the same words on two paths into node 3: one token, the better; "a b" built through two different parent tokens
    same = [b"I 0", b"T 0 1 -1 a -1", b"T 0 2 -1 a -2", b"T 1 3 -1 b -1", b"T 2 3 -1 b -1.5", b"F 3"]
    got, want, net = one_utt(capi, dev, tmp_path, same, 2)
    assert_same(got, want, net)
    assert [(t[0], t[3]) for t in got["tokens"]] == [(3, (0, 1))] and got["text"] == b"a b" and got["logprob"] == -2
    # different words into one node: both stay
    differ = [b"I 0", b"T 0 1 -1 a -1", b"T 0 2 -1 c -2", b"T 1 3 -1 b -1", b"T 2 3 -1 b -1.5", b"F 3"]
    got, want, net = one_utt(capi, dev, tmp_path, differ, 2)
    assert_same(got, want, net)
    assert [(t[0], t[3]) for t in got["tokens"]] == [(3, (0, 2)), (3, (1, 2))]


@pytest.mark.gpu
def test_dead_end_and_no_end_node(capi, dev, tmp_path):
    got, want, net = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 1 0", b"F 1"], 3)
    assert_same(got, want, net)
    assert got["status"] == capi.AASR_FST_NO_TOKENS and got["tokens"] == [] and got["text"] == b""
    got, want, net = one_utt(capi, dev, tmp_path, [b"I 0", b"T 0 0 0 w"], 2)
    assert_same(got, want, net)
    assert got["status"] == capi.AASR_FST_OK and got["text"] == b"" and got["logprob"] == -1 and got["best_final_logprob"] == np.float32(-9999999.9)


@pytest.mark.gpu
def test_overflow_statuses_and_the_rerun(capi, dev, tmp_path):
    cfg = RANDOM[3]
    fst, raws, acs = make_inputs(cfg)
    net, want = restate(cfg, fst, acs)
    w = want[0]

    def pow2_below(v, f=lambda c: c):      # the largest power of two c with f(c) < v
        c = 1
        while f(2 * c) < v:
            c *= 2
        return c

    assert w.max_candidates > 8 and w.max_keys > 4 and len(w.histories) > 4
    tiny = {capi.AASR_FST_OVERFLOW_CANDIDATES: {"cap_candidates": w.max_candidates - 1},
            capi.AASR_FST_OVERFLOW_RECOMB: {"cap_recomb": pow2_below(w.max_keys)},
            capi.AASR_FST_OVERFLOW_HISTORY: {"cap_history": pow2_below(len(w.histories), lambda c: c - c // 4)}}
    for status, caps in tiny.items():
        got = device_run(capi, dev, tmp_path, fst, raws, 2, beam=40.0, rerun=False, **caps)[0]
        assert got["status"] == status and got["tokens"] == [] and got["text"] == b"", (status, caps)
        got = device_run(capi, dev, tmp_path, fst, raws, 2, beam=40.0, **caps)[0]
        assert got["reran"], caps
        assert_same(got, w, net, caps)


DUR = "4\n%d\n" % MODELS + "".join("%d %.4f %.4f\n" % (i, 0 if i % 3 == 0 else 1.5 + i / 4.0, 0.75 + i / 8.0) for i in range(MODELS))


@pytest.mark.gpu
def test_duration_term_by_state(capi, dev, tmp_path):
    cfg = ("dur", 12, 37, 2, [40, 11], 60.0, 5000)
    fst, raws, acs = make_inputs(cfg)
    net, want = restate(cfg, fst, acs, durations=R.read_durations(DUR, by_state=True))
    _, plain = restate(cfg, fst, acs)
    got = device_run(capi, dev, tmp_path, fst, raws, 2, dur_text=DUR, beam=60.0, dur_by_state=1)
    ref = device_run(capi, dev, tmp_path, fst, raws, 2, dur_text=DUR, beam=60.0)      # the reference's indexing: no term below n
    for u in range(2):
        assert_same(got[u], want[u], net, u)
        assert_same(ref[u], plain[u], net, u)
    assert bits(want[0].best_logprob) != bits(plain[0].best_logprob)


def read_golden(case):
    fst = open(os.path.join(GOLDEN, case + ".fst"), "rb").read()
    lna = open(os.path.join(GOLDEN, case + ".lna"), "rb").read()
    n_models, lnabytes = struct.unpack(">iB", lna[:5])
    rows = []
    for line in open(os.path.join(GOLDEN, "expected_%s.txt" % case), "rb").read().split(b"\n"):
        if line:
            rows.append(line.split(b"\t"))
    return fst, lna[5:], n_models, lnabytes, open(os.path.join(GOLDEN, case + ".dur")).read(), rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["durhi", "rand1", "rand2", "rand4", "toy", "wide"])
def test_golden_cases_against_the_reference_and_the_restatement(capi, dev, tmp_path, case):
    fst, raw, n_models, lnabytes, dur, rows = read_golden(case)
    net = R.read_fst(fst)
    ac = R.decode_lna(raw, n_models, lnabytes)
    for f in rows:
        beam, limit, ds, ts = float(f[0]), int(f[1]), float(f[2]), float(f[3])
        got = device_run(capi, dev, tmp_path, fst, [raw], lnabytes, n_models=n_models, dur_text=dur, beam=beam, token_limit=limit,
                         duration_scale=ds, transition_scale=ts)[0]
        assert_same(got, R.search(net, ac, beam, limit, ds, ts, R.read_durations(dur)), net, (case, f[:4]))
        g9 = lambda x: ("%.9g" % float(x)).encode()
        assert [g9(got["logprob"]), g9(got["best_logprob"]), g9(got["best_final_logprob"]), got["text"]] == f[4:], (case, f[:4])


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes(capi, dev, tmp_path):
    cfg = RANDOM[1]
    fst, raws, _ = make_inputs(cfg)
    runs = [device_run(capi, dev, tmp_path, fst, raws, cfg[3], beam=cfg[5], token_limit=cfg[6]) for _ in range(2)]
    for a, b in zip(*runs):
        assert [(n, bits(lp), d, w) for n, lp, d, w in a["tokens"]] == [(n, bits(lp), d, w) for n, lp, d, w in b["tokens"]]
        assert (a["status"], a["words"], bits(a["logprob"]), bits(a["best_logprob"])) == (b["status"], b["words"], bits(b["logprob"]), bits(b["best_logprob"]))


@pytest.mark.gpu
def test_network_pdf_beyond_the_models_is_refused(capi, dev, tmp_path):
    fst, raws, _ = make_inputs(RANDOM[0])
    with pytest.raises(capi.AasrError) as ei:
        device_run(capi, dev, tmp_path, fst, [r[:len(r) // MODELS * (MODELS - 1)] for r in raws], 4, n_models=MODELS - 1)
    assert ei.value.code == capi.AASR_ERR_INVALID and "models" in ei.value.msg


if __name__ == "__main__":      # seed search on the CPU: the first seed of every configuration without a tie
    extra = [("batch8", 0, 37, 2, [64, 3, 17, 1, 0, 33, 2, 50], 0.0, 5000), ("dur", 0, 37, 2, [40, 11], 60.0, 5000)]
    for cfg in RANDOM + LIMITS[:1] + extra:
        for seed in range(200):
            c = (cfg[0], seed) + cfg[2:]
            if cfg[0] == "limits" and any(o.ties or o.max_keys <= lim + 1 or len(o.tokens) != lim + 1 for lim in (1, 3, 255, 256, 257)
                                          for o in restate(c[:6] + (lim,), *make_inputs(c)[::2])[1]):
                continue
            fst, raws, acs = make_inputs(c)
            d = R.read_durations(DUR, by_state=True) if cfg[0] == "dur" else None
            _, out = restate(c, fst, acs, durations=d)
            ok = not any(o.ties for o in out)
            if cfg[0] == "dur":
                ok = ok and not any(o.ties for o in restate(c, fst, acs)[1])
            if cfg[0] in ("batch8", "large", "mid2", "bytes1", "dur"):
                ok = ok and sum(o.status == R.OK and len(o.words) > 0 for o in out) >= (len(out) + 1) // 2
            if ok:
                print(c, [(o.status, len(o.tokens), o.max_candidates, o.max_keys, len(o.histories)) for o in out])
                break
        else:
            print("NO SEED", cfg)

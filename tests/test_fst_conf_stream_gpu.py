"""Confidence scores on streaming sessions (aasr_fst_conf_stream_*, csrc/fst_conf_stream.h).  The yardstick is the
confidence batch (capi.fst_conf_batch, itself held to the reference's recorded rows by test_fst_conf_gpu.py): whatever
the chunking, a session after t frames answers what the batch answers for an utterance of those t rows -- every float by
its bits, every int, the words and both strings -- after every feed, for every session.  The batch's answers for every
prefix of a case come from ONE batch launch and are shared by the case's tests; so are the restatement's
(tools/fst_conf_restate.py), which is compared wherever it reports no tie.  The carried sum is held to
CR.frame_best_sum, bitwise, at every feed boundary."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fst_restate as R  # noqa: E402
import fst_conf_restate as CR  # noqa: E402
from test_fst_conf_gpu import CASES, FIELDS, MODELS, RANDOM, bits, g9, golden, make_inputs  # noqa: E402
from test_fst_stream_gpu import plan  # noqa: E402

BY_NAME = {c[0]: c for c in RANDOM}


@pytest.fixture(scope="module")
def dev(capi):
    import torch
    capi.check(capi.lib().aasr_set_device(0))
    return torch


# ---- the cases: networks, utterances, options, and which utterance (and how much of it) every session is fed -------------

class Case:
    """fst, ploop: the networks' text; raws: the utterances' native rows; sessions: (utterance, frames) per session"""


def random_case(name) -> Case:
    cfg = BY_NAME[name]
    c = Case()
    c.name, c.lnabytes, c.n_models, c.dur = name, cfg[3], MODELS, None
    c.fst, c.raws, c.acs = make_inputs(cfg)
    c.ploop = CR.random_phone_loop(np.random.default_rng([cfg[1], 5]), MODELS)
    c.gopt = c.popt = dict(beam=cfg[5], token_limit=cfg[6])
    order = list(range(len(c.raws))) + [0] * max(0, 3 - len(c.raws))      # at least three sessions
    c.sessions = [(u, len(c.acs[u])) for u in order]
    c.recorded = None
    return c


def golden_case(case, row) -> Case:
    c = Case()
    c.name = "%s-%d" % (case, row)
    c.fst, c.ploop, raw, c.n_models, c.lnabytes, c.dur, rows = golden(case)
    c.raws, c.acs = [raw], [R.decode_lna(raw, c.n_models, c.lnabytes)]
    c.gopt, c.popt, c.recorded = rows[row]
    T = len(c.acs[0])
    c.sessions = [(0, T), (0, T // 2), (0, 1), (0, T)]      # the whole utterance twice, at different phases of a ragged plan
    return c


CASE_IDS = [c[0] for c in RANDOM] + ["%s-%d" % (k, r) for k in CASES for r in (0, 1)]
_CASES = {}


def case_of(cid) -> Case:
    if cid not in _CASES:
        _CASES[cid] = random_case(cid) if cid in BY_NAME else golden_case(cid.rsplit("-", 1)[0], int(cid.rsplit("-", 1)[1]))
    return _CASES[cid]


def rows_of(c: Case, u: int, width: str):
    """(bytes of utterance u's rows, lnabytes): the native codes, or the floats they decode to"""
    if width == "f32":
        return np.ascontiguousarray(c.acs[u], "<f4").tobytes(), 4
    return c.raws[u], c.lnabytes


# ---- the restatement at every boundary, once per case -------------------------------------------------------------------

_RESTATED = {}


def restated(c: Case, u: int, t: int, phone: bool):
    """CR.confidence of the first t rows of utterance u.  With a phone loop both searches run; the plain variant reuses
    nothing (its formulas differ), but its grammar search is the same"""
    key = (c.name, u, t, phone)
    if key not in _RESTATED:
        net = R.read_fst(c.fst)
        d = R.read_durations(open(c.dur).read()) if c.dur else None
        _RESTATED[key] = CR.confidence(net, c.acs[u][:t], c.gopt, d, R.read_fst(c.ploop) if phone else None, c.popt if phone else None)
    return _RESTATED[key]


PAIRS = 455      # (row, boundary) pairs of CASE_IDS: every prefix 0 ... T of every utterance


def test_restatement_ties_stay_within_the_cap():
    """On the CPU, the restatement alone: at most one fifth of the (row, boundary) pairs may be skipped for a tie in either
    search.  The chosen rows have none."""
    total = skipped = 0
    for cid in CASE_IDS:
        c = case_of(cid)
        for u, ac in enumerate(c.acs):
            for t in range(len(ac) + 1):
                total += 1
                skipped += bool(restated(c, u, t, True).ties)
    assert total == PAIRS
    assert skipped == 0 and 5 * skipped <= total


# ---- the batch at every boundary, one launch per (case, phone loop, width) ------------------------------------------------

_BATCH = {}


def nets_of(capi, tmp_path, c: Case, phone: bool):
    path = os.path.join(str(tmp_path), "net.fst")
    open(path, "wb").write(c.fst)
    open(path + ".ploop", "wb").write(c.ploop)
    return capi.FstNet(path), capi.FstNet(path + ".ploop") if phone else None, capi.FstDurations(c.dur) if c.dur else None


def options_of(capi, c: Case, phone: bool, gopt=None, popt=None):
    o = capi.FstConfOptions.defaults(phone_loop=1 if phone else 0)
    for k, v in dict(c.gopt, **(gopt or {})).items():
        setattr(o.grammar, k, v)
    for k, v in dict(c.popt, **(popt or {})).items():
        setattr(o.phone, k, v)
    return o


def batch_prefixes(capi, torch, tmp_path, c: Case, phone: bool, width: str, gopt=None, popt=None) -> dict:
    """(utterance, t) -> capi.fst_conf_batch's entry for its first t rows; nothing is rerun"""
    key = (c.name, phone, width, str(gopt), str(popt))
    if key not in _BATCH:
        net, pnet, dur = nets_of(capi, tmp_path, c, phone)
        blob, row0, T, who, at = b"", [], [], [], 0
        for u in range(len(c.raws)):
            raw, lnabytes = rows_of(c, u, width)
            n = len(c.acs[u])
            for t in range(n + 1):
                row0.append(at)
                T.append(t)
                who.append((u, t))
            blob += raw + b"\xff" * (c.n_models * lnabytes)
            at += n + 1
        d_lna = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()
        out = capi.fst_conf_batch(net, pnet, T, d_lna, lnabytes, c.n_models, row0, options_of(capi, c, phone, gopt, popt), dur=dur,
                                  want_tokens=False, rerun=False)
        _BATCH[key] = dict(zip(who, out))
    return _BATCH[key]


def open_stream(capi, tmp_path, c: Case, phone: bool, n_sessions: int, max_frames: int, gopt=None, popt=None):
    net, pnet, dur = nets_of(capi, tmp_path, c, phone)
    return capi.FstConfStream(net, pnet, n_sessions, max_frames, options_of(capi, c, phone, gopt, popt), dur=dur)


def feed(torch, s, chunks, lnabytes, n_models):
    """one feed: session u gets the rows chunks[u] (bytes, maybe none); a row of 0xff between the sessions' rows"""
    w = n_models * lnabytes
    row, row0, n_new, blob = 0, [], [], b""
    for ch in chunks:
        row0.append(row)
        n_new.append(len(ch) // w)
        blob += ch + b"\xff" * w
        row += len(ch) // w + 1
    d_lna = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()
    s.feed_dev(d_lna, lnabytes, n_models, row0, n_new)
    s.sync()


def search_image(r):
    return (r["status"], bits(r["logprob"]), bits(r["best_logprob"]), bits(r["best_final_logprob"]), r["words"], r["text"], r["n_tokens"],
            {k: (bits(v) if isinstance(v, np.float32) else v) for k, v in r["record"].items()})


def image(capi, r):
    """everything the contract names: the ten floats by their bits, the ints, the words, both strings, both records"""
    return ([None if r[k] is None else bits(r[k]) for k in capi.FST_CONF_FLOATS],
            (r["frames"], r["grammar_status"], r["phone_status"], r["no_final"], r["valid"]), r["text"],
            search_image(r["grammar"]), search_image(r["phone"]) if r["phone"] is not None else None)


def assert_restated(got, want, what):
    """the restatement, where it reports no tie in either search (the caller looks)"""
    for k in CR.FLOATS:
        assert bits(got[k]) == bits(want.r[k]) or (np.isnan(got[k]) and np.isnan(want.r[k])), (what, k, got[k], want.r[k])
    assert got["no_final"] == int(want.no_final) and got["valid"] == 1 and got["text"] == want.text, what
    if want.phone is not None:
        assert got["phone"]["text"] == want.ploop_text, what


VARIANTS = [(cid, phone, "native") for cid in CASE_IDS for phone in (True, False) if phone or cid in BY_NAME or cid.endswith("-0")] + \
           [(cid, True, "f32") for cid in ("mid", "one", "limit1", "durhi-0", "rand1-0", "rand2-1")]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["whole", "single", "ragged"])
@pytest.mark.parametrize("cid,phone,width", VARIANTS, ids=["%s-%s-%s" % (c, "ploop" if p else "plain", w) for c, p, w in VARIANTS])
def test_every_chunking_is_the_batch_at_every_boundary(capi, dev, tmp_path, cid, phone, width, pattern):
    c = case_of(cid)
    want = batch_prefixes(capi, dev, tmp_path, c, phone, width)
    frames = [n for _, n in c.sessions]
    assert len(frames) >= 3
    s = open_stream(capi, tmp_path, c, phone, len(frames), max(frames + [1]))
    steps = plan(pattern, frames)
    if pattern == "ragged":      # in one launch: nothing for some, more for some
        assert any(0 in st and max(st) > 0 for st in steps)
    fed = [0] * len(frames)
    skipped = compared = 0
    for k, step in enumerate(steps):
        chunks = []
        for (u, _), a, n in zip(c.sessions, fed, step):
            raw, lnabytes = rows_of(c, u, width)
            w = c.n_models * lnabytes
            chunks.append(raw[a * w:(a + n) * w])
        feed(dev, s, chunks, lnabytes, c.n_models)
        fed = [a + b for a, b in zip(fed, step)]
        for i, (u, _) in enumerate(c.sessions):
            got = s.result(i)
            assert image(capi, got) == image(capi, want[(u, fed[i])]), (cid, pattern, k, i, fed[i])
            assert got["frames"] == fed[i]
            if phone:
                assert (bits(s.best_acu(i)[0]), s.best_acu(i)[1]) == (bits(got["best_acu_score"]), fed[i])
            rs = restated(c, u, fed[i], phone)
            if rs.ties:
                skipped += 1
                continue
            compared += 1
            assert_restated(got, rs, (cid, pattern, k, i, fed[i]))
    assert fed == frames
    assert 5 * skipped <= skipped + compared
    if c.recorded is not None:      # the reference's recorded values for the whole utterance, as test_fst_conf_gpu.py compares them
        got, f = s.result(0), c.recorded
        if phone:
            assert [got["text"], got["phone"]["text"]] + [g9(got[k]) for k in FIELDS] + [b"%d" % got["frames"], g9(got["confidence"])] == f[:-1]
        else:
            assert g9(got["confidence"]) == f[-1]
        assert image(capi, got) == image(capi, s.result(3))      # the same utterance at another phase of the plan
    s.close()


# ---- the carried sum -----------------------------------------------------------------------------------------------------

SUM_FRAMES = [1, 63, 64, 65, 130]
LOOP = R.write_fst([b"I 0", b"T 0 0 0 , -0.5", b"F 0"])                       # pdf 0 only: any model count will do
PLOOP = R.write_fst([b"I 0", b"T 0 1 0 a -0.25", b"T 1 1 0 , -0.5", b"T 1 0 -1 , -0.125", b"F 0", b"F 1"])


# the generator's third seed word per (lnabytes, n_models): the first for which, in every session of 63 frames or more, the
# chain's sum differs from NumPy's pairwise sum of the same values (searched on the CPU; asserted in the test)
SUM_SEEDS = {(1, 1): 1, (1, 3): 2, (1, 63): 1, (1, 65): 0, (1, 257): 8, (2, 1): 0, (2, 3): 5, (2, 63): 2, (2, 65): 0, (2, 257): 0,
             (4, 1): 1, (4, 3): 0, (4, 63): 1, (4, 65): 0, (4, 257): 0}


def sum_rows(lnabytes, n_models):
    """sum(SUM_FRAMES) rows whose best values have mixed magnitudes; 4-byte rows also hold +0 / -0 pairs and equal maxima"""
    rng = np.random.default_rng([lnabytes, n_models, SUM_SEEDS[(lnabytes, n_models)]])
    n = sum(SUM_FRAMES)
    if lnabytes == 4:
        v = (-rng.random((n, n_models)) * 30 - 40).astype(np.float32)
        v[:, 0] = -(10.0 ** rng.integers(-6, 2, n)) * (1 + rng.random(n))      # the row's best: eight decades of magnitudes
        v[::11, 0] = -0.0
        v[::11, -1] = 0.0            # (one model: the row is +0)
        v[5::13, -1] = v[5::13, 0]   # the maximum twice
        return v.view(np.uint8).reshape(n, -1).copy(), v
    hi = 65536 if lnabytes == 2 else 256
    c = rng.integers(hi // 2, hi, (n, n_models))
    c[:, n_models // 2] = rng.integers(0, hi, n) >> rng.integers(0, 12 if lnabytes == 2 else 6, n)      # best codes of every size
    raw = c.astype(">u2").view(np.uint8).reshape(n, -1).copy() if lnabytes == 2 else c.astype(np.uint8)
    return raw, R.decode_lna(raw.tobytes(), n_models, lnabytes)


def sequential_sums(best):
    pre = [np.float32(0)]
    with np.errstate(all="ignore"):
        for x in best:
            pre.append(np.float32(pre[-1] + x))
    return pre


@pytest.mark.gpu
@pytest.mark.parametrize("n_models", [1, 3, 63, 65, 257])
@pytest.mark.parametrize("lnabytes", [1, 2, 4])
def test_the_carried_sum_is_the_reference_chain_at_every_boundary(capi, dev, tmp_path, lnabytes, n_models):
    raw, ac = sum_rows(lnabytes, n_models)
    first = np.concatenate([[0], np.cumsum(SUM_FRAMES)])
    pre = []
    for u, T in enumerate(SUM_FRAMES):
        a = ac[first[u]:first[u + 1]]
        best = CR.frame_best(a)
        pre.append(sequential_sums(best))
        assert bits(pre[u][T]) == bits(CR.frame_best_sum(a))
        if T >= 63:      # a tree would not pass: NumPy's pairwise sum of the same values differs from the chain
            assert bits(np.sum(best, dtype=np.float32)) != bits(pre[u][T]), (u, T)
    c = Case()
    c.fst, c.ploop, c.dur, c.gopt, c.popt = LOOP, PLOOP, None, {}, {}
    w = n_models * lnabytes
    rows = [raw[first[u]:first[u + 1]].tobytes() for u in range(5)]
    for way in ("whole", "ones", "64+rest"):
        s = open_stream(capi, tmp_path, c, True, 5, 130)
        if way == "whole":
            steps = [list(SUM_FRAMES)]
        elif way == "ones":
            steps = [[1 if t < T else 0 for T in SUM_FRAMES] for t in range(130)]
        else:
            steps = [[min(64, T) for T in SUM_FRAMES], [T - min(64, T) for T in SUM_FRAMES]]
        fed = [0] * 5
        for step in steps:
            # the sessions' rows out of order, rows of 0xff between them, the buffer one element off the allocation's start:
            # no row starts on the 16-byte grid by luck
            order, at, row0 = [3, 1, 4, 0, 2], 1, [0] * 5
            for u in order:
                row0[u] = at
                at += step[u] + 2
            buf = np.full((at, w), 0xff, np.uint8)
            if lnabytes == 4:
                buf.view(np.float32)[:] = 1e30      # (a row read by mistake would win)
            for u in range(5):
                buf[row0[u]:row0[u] + step[u]] = np.frombuffer(rows[u][fed[u] * w:(fed[u] + step[u]) * w], np.uint8).reshape(step[u], w)
            d_all = dev.frombuffer(bytearray(bytes(lnabytes) + buf.tobytes() + bytes(16)), dtype=dev.uint8).cuda()
            d_lna = d_all[lnabytes:]
            assert d_lna.data_ptr() % 16 == lnabytes
            s.feed_dev(d_lna, lnabytes, n_models, row0, step)
            s.sync()
            fed = [a + b for a, b in zip(fed, step)]
            for u in range(5):      # (a session with n_new = 0 keeps its sum)
                got, n = s.best_acu(u)
                assert (bits(got), n) == (bits(pre[u][fed[u]]), fed[u]), (way, u, fed[u], got, pre[u][fed[u]])
                assert bits(s.result(u)["best_acu_score"]) == bits(got) and s.result(u)["frames"] == fed[u]
        assert fed == SUM_FRAMES
        s.close()


# ---- statuses, resets, refusals --------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_grammar_without_tokens_while_the_phone_loop_goes_on(capi, dev, tmp_path):
    c = Case()
    c.name, c.dur, c.gopt, c.popt, c.n_models, c.lnabytes = "dead", None, {}, {}, 3, 4
    c.fst = R.write_fst([b"I 0", b"T 0 1 0", b"F 1"])      # node 1 has no arc out
    c.ploop = CR.random_phone_loop(np.random.default_rng(11), 3, n_phones=3)
    ac = (-np.random.default_rng(12).random((6, 3)) * 7).astype(np.float32)
    c.acs, c.raws = [ac], [ac.tobytes()]
    want = batch_prefixes(capi, dev, tmp_path, c, True, "native")
    s = open_stream(capi, tmp_path, c, True, 1, 6)
    fed = 0
    for n in (1, 2, 3):
        feed(dev, s, [ac[fed:fed + n].tobytes()], 4, 3)
        fed += n
        got = s.result(0)
        assert image(capi, got) == image(capi, want[(0, fed)]), fed
        assert got["frames"] == fed and bits(got["best_acu_score"]) == bits(CR.frame_best_sum(ac[:fed])) and got["valid"] == 1
        assert got["grammar_status"] == (capi.AASR_FST_NO_TOKENS if fed >= 2 else capi.AASR_FST_OK) and got["phone_status"] == capi.AASR_FST_OK
        assert got["grammar"]["frames_done"] == min(fed, 2) and got["phone"]["frames_done"] == fed
    s.close()


@pytest.mark.gpu
def test_overflow_is_sticky_and_resets_start_anew_beside_continuing_sessions(capi, dev, tmp_path):
    c = case_of("mid")
    pnet = R.read_fst(c.ploop)
    hist = lambda u, t: len(R.search(pnet, c.acs[u][:t], **c.popt).histories)
    cap = 1
    while 2 * cap - 2 * cap // 4 < hist(0, 40):      # the largest power of two whose three quarters do not hold the histories
        cap *= 2
    assert max(hist(2, 8), hist(5, 6), hist(0, 3)) < cap // 2
    popt = dict(cap_history=cap)
    want = batch_prefixes(capi, dev, tmp_path, c, True, "native", popt=popt)
    assert want[(0, 40)]["phone_status"] == capi.AASR_FST_OVERFLOW_HISTORY and want[(0, 40)]["valid"] == 0
    s = open_stream(capi, tmp_path, c, True, 3, 48, popt=popt)
    w = MODELS * c.lnabytes
    rows = lambda u, a, b: c.raws[u][a * w:b * w]
    same = lambda i, u, t: image(capi, s.result(i)) == image(capi, want[(u, t)])
    feed(dev, s, [rows(0, 0, 20), rows(2, 0, 4), rows(5, 0, 3)], c.lnabytes, MODELS)
    assert same(0, 0, 20) and same(1, 2, 4) and same(2, 5, 3)
    feed(dev, s, [rows(0, 20, 40), rows(2, 4, 8), b""], c.lnabytes, MODELS)
    assert same(0, 0, 40) and same(1, 2, 8) and same(2, 5, 3)      # the neighbours are unaffected
    over = s.result(0)
    assert over["valid"] == 0 and over["confidence"] is None and over["phone_status"] == capi.AASR_FST_OVERFLOW_HISTORY
    feed(dev, s, [rows(0, 0, 3), b"", b""], c.lnabytes, MODELS)      # sticky: the frames are counted, the search does not move
    again = s.result(0)
    assert again["frames"] == 43 and again["valid"] == 0 and again["phone_status"] == capi.AASR_FST_OVERFLOW_HISTORY
    assert again["phone"]["frames_done"] == over["phone"]["frames_done"] <= 40 and search_image(again["phone"]) == search_image(over["phone"])
    assert same(1, 2, 8) and same(2, 5, 3)
    s.reset(0)
    assert same(0, 0, 0)                                            # before any feed: the zero-frame result of the batch
    feed(dev, s, [rows(0, 0, 3), b"", rows(5, 3, 6)], c.lnabytes, MODELS)      # the reset session beside a continuing one
    assert same(0, 0, 3) and same(1, 2, 8) and same(2, 5, 6)
    s.reset(1)
    assert same(1, 2, 0) and same(0, 0, 3)
    feed(dev, s, [b"", b"", b""], c.lnabytes, MODELS)                # a fresh session fed nothing
    assert same(1, 2, 0) and same(0, 0, 3) and same(2, 5, 6)
    assert np.isnan(s.result(1)["best_acu_conf"]) or np.isinf(s.result(1)["best_acu_conf"])      # the IEEE division is kept
    s.close()


@pytest.mark.gpu
def test_refused_feeds_change_nothing(capi, dev, tmp_path):
    c = case_of("mid")
    want = batch_prefixes(capi, dev, tmp_path, c, True, "native")
    s = open_stream(capi, tmp_path, c, True, 1, 40)
    w = MODELS * 2
    feed(dev, s, [c.raws[0][:20 * w]], 2, MODELS)
    before = image(capi, s.result(0))
    assert before == image(capi, want[(0, 20)])
    d = dev.frombuffer(bytearray(c.raws[0] + bytes(16)), dtype=dev.uint8).cuda()
    rows = d.numel() // w
    top = max(R.read_fst(c.fst).node_pdf.max(), R.read_fst(c.ploop).node_pdf.max())
    bad = [dict(d=d, lnabytes=2, n_models=MODELS, row0=[0], n_new=[-1]),
           dict(d=d, lnabytes=2, n_models=MODELS, row0=[0], n_new=[21]),                 # past max_frames
           dict(d=d, lnabytes=2, n_models=MODELS, row0=[rows - 3], n_new=[4]),           # rows outside the buffer
           dict(d=d, lnabytes=2, n_models=MODELS, row0=[-1], n_new=[2]),
           dict(d=d, lnabytes=2, n_models=int(top), row0=[0], n_new=[1]),                # a network's largest pdf is no model
           dict(d=d, lnabytes=2, n_models=int(R.read_fst(c.ploop).node_pdf.max()), row0=[0], n_new=[1]),
           dict(d=d, lnabytes=4, n_models=MODELS, row0=[0], n_new=[1]),                  # another width mid-utterance
           dict(d=d, lnabytes=2, n_models=MODELS + 1, row0=[0], n_new=[1]),              # another model count
           dict(d=d[1:], lnabytes=2, n_models=MODELS, row0=[0], n_new=[1])]              # not aligned to lnabytes
    for kw in bad:
        with pytest.raises(capi.AasrError) as ei:
            s.feed_dev(kw["d"], kw["lnabytes"], kw["n_models"], kw["row0"], kw["n_new"])
        assert ei.value.code == capi.AASR_ERR_INVALID and "aasr_fst_conf_stream_feed_dev" in ei.value.msg, kw
        assert image(capi, s.result(0)) == before, kw      # (no sync needed: nothing was queued)
    feed(dev, s, [c.raws[0][20 * w:]], 2, MODELS)
    assert image(capi, s.result(0)) == image(capi, want[(0, 40)])
    s.close()


@pytest.mark.gpu
def test_the_same_feeds_twice_give_identical_bytes(capi, dev, tmp_path):
    c = case_of("rand4-0")
    raw, T = c.raws[0], len(c.acs[0])
    w = c.n_models * c.lnabytes
    runs = []
    for _ in range(2):
        s = open_stream(capi, tmp_path, c, True, 2, T)
        out, fed = [], 0
        for n in (5, 1, 7, T - 13):
            feed(dev, s, [raw[fed * w:(fed + n) * w], raw[fed * w:(fed + n) * w]], c.lnabytes, c.n_models)
            fed += n
            for u in range(2):
                r = s.result(u, want_tokens=True)
                out.append((image(capi, r), [(n_, bits(lp), d, ws) for n_, lp, d, ws in r["grammar"]["tokens"]],
                            [(n_, bits(lp), d, ws) for n_, lp, d, ws in r["phone"]["tokens"]], bits(s.best_acu(u)[0])))
        runs.append(out)
        s.close()
    assert runs[0] == runs[1] and runs[0][0] == runs[0][1]

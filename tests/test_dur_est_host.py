"""The dur_est tool (csrc/dur_est.cc, csrc/aku/main_dur_est.cc), host only: its .dur and --hist files byte for byte
against tools/dur_est_restate.py and, for the one recipe the reference's own dur_est could be run on, against the
files that program wrote (tests/golden/dur_est/README.md).  The fit is compared as bytes because both sides run the
same IEEE double operations with the C library's log and lgamma (tools/dur_est_restate.py's header)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
GOLD = os.path.join(ROOT, "tests", "golden", "dur_est")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dur_est_restate as DR  # noqa: E402

NH, PER = 4, 3
HMM_STATES = {"h%d" % h: [h * PER + j for j in range(PER)] for h in range(NH)}
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


def run(tmp_path, lines, *args, ph=None, env=None):
    """lines: dicts of recipe fields -> (CompletedProcess, hist text or None, dur text or None)"""
    rec = str(tmp_path / "r.recipe")
    with open(rec, "w") as f:
        for l in lines:
            f.write("audio=none.wav " + " ".join("%s=%s" % kv for kv in l.items()) + "\n")
    hist, dur = str(tmp_path / "o.hist"), str(tmp_path / "o.dur")
    cmd = [os.path.join(BIN, "dur_est"), "-p", ph or os.path.join(GOLD, "m.ph"), "-r", rec, "--hist", hist, "--gamma", dur]
    r = subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
    read = lambda p: open(p).read() if os.path.exists(p) else None
    return r, read(hist), read(dur)


def restate(lines, ophn=False, maxdur=100, skip=0, mincount=10):
    files, seen = [], {}
    for fields in lines:
        seen.update(fields)     # Recipe::read keeps one key-value map over the lines (aku/Recipe.cc:80-91): a key holds until restated
        l = dict(seen)
        files.append({"path": l["alignment" if ophn else "transcript"], "start_time": float(l.get("start-time", 0)),
                      "end_time": float(l.get("end-time", 0)), "start_line": int(l.get("start-line", 0)),
                      "end_line": int(l.get("end-line", 0))})
    table = DR.histograms(HMM_STATES, NH * PER, files, maxdur, skip)
    return table, DR.hist_text(table, skip), DR.dur_text(table, skip, mincount)


def gold(name):
    return os.path.join(GOLD, name)


def test_the_recorded_run_of_the_reference(capi, tmp_path):
    case = json.load(open(gold("cases.json")))["plain"]
    lines = [{k: gold(v) for k, v in l.items()} for l in case["lines"]]
    r, hist, dur = run(tmp_path, lines, *case["args"], env=NO_DEVICE)            # runs with no device present
    assert r.returncode == 0, r.stderr
    assert hist == open(gold("plain.hist")).read() and dur == open(gold("plain.dur")).read()
    table, want_hist, want_dur = restate(lines)
    assert (hist, dur) == (want_hist, want_dur)
    sums = table.sum(axis=1)
    assert (sums[:9] >= 10).all() and (sums[9:] < 10).all() and (sums[9:] > 0).all()    # h3 is under --mincount
    assert dur.splitlines()[:2] == ["4", "12"] and all(l.endswith(" 0.0000 0.0000") for l in dur.splitlines()[11:])


def test_options_limits_and_ophn_against_the_restatement(capi, tmp_path):
    """-O, -M clamping, --skip, --mincount, a start and end time that cut lines, line limits, and a file without
    lines: the reference's two messages, and the run goes on"""
    lines = [{"alignment": gold("a.phn"), "transcript": gold("empty.phn"), "start-time": "0.6", "end-time": "2.4"},
             {"alignment": gold("b.phn"), "transcript": gold("empty.phn"), "start-line": "3", "end-line": "30"},
             {"alignment": gold("empty.phn"), "transcript": gold("a.phn")},
             {"alignment": gold("c.phn"), "transcript": gold("empty.phn")}]
    r, hist, dur = run(tmp_path, lines, "-O", "-M", "6", "--skip", "2", "--mincount", "4", "-i", "1")
    assert r.returncode == 0, r.stderr
    table, want_hist, want_dur = restate(lines, ophn=True, maxdur=6, skip=2, mincount=4)
    assert (hist, dur) == (want_hist, want_dur)
    assert table[:, 5].sum() > 0 and table[:2].sum() == 0 and hist.startswith("2 ")       # clamped durations; skipped states
    unlimited = restate([{"alignment": l["alignment"], "transcript": l["transcript"]} for l in lines], ophn=True, maxdur=6, skip=2)[0]
    assert table.sum() < unlimited.sum()                                                  # the limits dropped lines
    assert "Could not initialize the utterance for PhnReader.Current file was: %s\n" % gold("a.phn") in r.stderr
    assert r.stderr.count("Processing file: none.wav\n") == 4
    for s in (0, 1):
        assert "Warning: No duration model for state %d\n" % s in r.stderr


def test_one_point_and_a_short_histogram(capi, tmp_path):
    """state 0 once (init_utterance_segmentation takes the file's first line), state 1 once, state 2 twice with
    different durations, state 3 twice with the same one: the variance floor"""
    phn = str(tmp_path / "s.phn")
    rows = [("h0.0", 3), ("h0.0", 2), ("h0.1", 4), ("h0.2", 1), ("h0.2", 7), ("h1.0", 5), ("h1.0", 5)]
    t = 0
    with open(phn, "w") as f:
        for lab, d in rows:
            f.write("%d %d %s\n" % (t * 128, (t + d) * 128, lab))
            t += d
    lines = [{"transcript": phn}]
    r, hist, dur = run(tmp_path, lines, "--mincount", "1", "-i", "1")
    assert r.returncode == 0, r.stderr
    table, want_hist, want_dur = restate(lines, mincount=1)
    assert (hist, dur) == (want_hist, want_dur)
    assert table.sum(axis=1).tolist()[:4] == [1, 1, 2, 2] and table[0, 1] == 1               # the first line is not counted
    got = [l.split() for l in dur.splitlines()[2:]]
    assert got[0][1:] == got[1][1:] == ["0.0000", "0.0000"] and float(got[2][1]) > 0 and float(got[3][1]) > 0
    assert r.stderr.count("Warning: Needs at least 2 points for estimating gamma models\n") == 2
    assert abs(float(got[3][1]) * float(got[3][2]) - 5.0) < 1e-2                              # a * b is the mean


def test_fit_through_the_library_call(capi):
    rng = np.random.default_rng(3)
    for _ in range(20):
        hist = rng.poisson(rng.uniform(0.2, 6.0), int(rng.integers(2, 40)))
        got, want = capi.dur_est_fit_gamma(hist), DR.fit_gamma(hist)
        assert (got is None) == (want is None)
        if want:
            assert ("%.4f %.4f" % got) == ("%.4f %.4f" % want), (hist, got, want)
    assert capi.dur_est_fit_gamma([0, 1, 0]) is None


@pytest.mark.parametrize("text,message", [
    ("0 256 h0.0\n256 512 h1\n", "Collecting duration statistics requires phn files with state numbers!"),
    ("0 256 h0.0\n256 512 zz.1\n", "HmmSet::hmm_index(): unknown hmm 'zz'"),
    ("0 256 h0.0\n256 512 h1.7\n", "state 7 of hmm 'h1'"),
    ("0 256 h0.0\n256 256 h1.1\n", "a duration of 0 frames"),
])
def test_messages(capi, tmp_path, text, message):
    phn = str(tmp_path / "bad.phn")
    open(phn, "w").write(text)
    r, hist, dur = run(tmp_path, [{"transcript": phn}])
    assert r.returncode == 1 and r.stderr.startswith("exception: ") and message in r.stderr, r.stderr
    assert hist is None and dur is None and "Aborted" not in r.stderr


def test_missing_files(capi, tmp_path):
    r, _, _ = run(tmp_path, [{"transcript": str(tmp_path / "none.phn")}])
    assert r.returncode == 1 and "PhnReader::open(): could not open " + str(tmp_path / "none.phn") in r.stderr
    r, _, _ = run(tmp_path, [{"transcript": gold("a.phn")}], ph=str(tmp_path / "none.ph"))
    assert r.returncode == 1 and r.stderr.startswith("exception: ")

"""make_fst_conf_golden.py -- records the reference's own confidences for the cases of tests/golden/fst/.

    python tools/make_fst_conf_golden.py REFERENCE_ROOT [BUILD_DIR]

Run by hand on a CPU machine that has the reference's sources; never run by a test.  The grammar networks, LNA and .dur
files of tests/golden/fst/ are read in place.  It

  * writes per case a phone-loop network NAME.ploop.fst (a few KB) with tools/fst_conf_restate.py's generator, its
    single-letter symbols drawn from the bytes of the grammar's own symbols, from the first listed seed for which the
    restatement reports no tie for either search and every recorded row has an end-node token in both searches,
  * compiles the reference's FstConfidence.cc, Fst.cc, FstAcoustics.cc, LnaReaderCircular.cc, NowayHmmReader.cc, Hmm.cc,
    str.cc and io.cc with the small driver below (this project's own) into BUILD_DIR (default: oracle/_ref/fst_conf,
    git-ignored), and
  * records, per case and setting, into tests/golden/fst_conf/expected_conf_NAME.txt, tab-separated:
        beam limit duration_scale transition_scale   (grammar)     phone_beam phone_limit phone_duration_scale
        result  phone-loop result
        token_conf ploop_conf edit_conf best_acu_conf grammar_logprob ploop_logprob best_final_logprob
        best_different_logprob best_acu_score frames                (%.9g)
        confidence                                                   (FstConfidenceWithPhoneLoop)
        confidence of the plain FstConfidence on the same grammar setting
    best_final_logprob, best_acu_score and frames are the reference's members; best_different_logprob is a local of the
    reference that never leaves it: the driver scans the reference's token list for it (the first token, in the list's
    descending order, whose words differ from the best end-node token's) -- token_conf is the reference's own check of it.

Only those data files are committed.  Every seed and setting tried is printed, with what ruled it out.  A case none of
whose settings leaves token_conf strictly inside (0, 1) is not recorded (printed; of tests/golden/fst/ that is `wide`,
where a token outside the end nodes outranks the best end-node token whatever the setting).  Across the recorded rows
the script asserts: overall a row with token_conf clamped at 0 and one at 1; a row with edit_conf strictly inside (0, 1).
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fst_restate as R  # noqa: E402
import fst_conf_restate as CR  # noqa: E402

FST = os.path.join(ROOT, "tests", "golden", "fst")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst_conf")

DRIVER = r"""
// driver of the reference's FstConfidence classes for tools/make_fst_conf_golden.py:
//   GRAMMAR PLOOP LNA DUR beam:limit:dscale:tscale:pbeam:plimit:pdscale ...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <sstream>
#include <map>
#define private public      // m_phone_fst, for the phone loop's own result string
#include "FstConfidence.hh"
#undef private
struct Probe : public FstConfidenceWithPhoneLoop {
  using FstConfidenceWithPhoneLoop::FstConfidenceWithPhoneLoop;
  float acu() { return m_best_acu_score; }
  int frames() { return m_cur_frame; }
  float different() {      // the first token whose words differ from the best end-node token's
    const FstConfidenceToken *best = nullptr;
    for (const auto &t : m_new_tokens) if (m_fst.nodes[t.node_idx].end_node) { best = &t; break; }
    if (!best) return -9999999.9f;
    for (const auto &t : m_new_tokens) if (t.unemitted_words != best->unemitted_words) return t.logprob;
    return -9999999.9f;
  }
};
int main(int argc, char **argv) {
  for (int i = 5; i < argc; i++) {
    float beam, ds, ts, pbeam, pds; int limit, plimit;
    if (sscanf(argv[i], "%f:%d:%f:%f:%f:%d:%f", &beam, &limit, &ds, &ts, &pbeam, &plimit, &pds) != 7) return 2;
    Probe s(argv[1], argv[2], nullptr, argv[4]);     // a search per setting: FstAcoustics never rewinds its frame counter
    s.set_beam(beam); s.set_token_limit(limit); s.set_duration_scale(ds); s.set_transition_scale(ts);
    s.set_phone_beam(pbeam); s.set_phone_token_limit(plimit); s.set_phone_duration_scale(pds);
    s.lna_open(argv[3], 1024);
    s.init_search();
    s.run();
    float conf, glp, plp;
    std::string r = s.result_and_confidence(&conf);
    s.get_result_and_logprob(glp);
    std::string pr = s.m_phone_fst.get_result_and_logprob(plp);
    FstConfidence plain(argv[1], nullptr, argv[4]);
    plain.set_beam(beam); plain.set_token_limit(limit); plain.set_duration_scale(ds); plain.set_transition_scale(ts);
    plain.lna_open(argv[3], 1024);
    plain.init_search();
    plain.run();
    float pconf;
    std::string r2 = plain.result_and_confidence(&pconf);
    if (r2 != r) return 3;
    printf("%s\t%s\t%s\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\n", argv[i], r.c_str(), pr.c_str(),
           (double)s.get_token_conf(), (double)s.get_ploop_conf(), (double)s.get_edit_conf(), (double)s.get_best_acu_conf(),
           (double)glp, (double)plp, (double)s.get_best_final_token_logprob(), (double)s.different(), (double)s.acu(),
           (double)s.frames(), (double)conf, (double)pconf);
    s.lna_close();
    plain.lna_close();
  }
  return 0;
}
"""

#            grammar: beam:limit:dscale:tscale   phone: beam:limit:dscale
SETTINGS = ["2600:5000:3:1:2600:5000:3", "30:5000:3:1:40:50:2", "8:5000:1.5:0.7:2600:5000:3", "2600:3:3:1:15:8:1.5",
            "2600:1:3:1:2600:5000:3", "12:6:2:1.25:40:50:2", "0:5000:3:1:2600:2:3", "60:5000:1:1:25:5000:0.5",
            "2600:5000:0.5:2:2600:5000:1", "20:40:3:0.25:30:20:3"]
CASES = ["toy", "rand2", "rand1", "rand4", "durhi", "wide"]
SEEDS = range(40)
FIELDS = ("token_conf", "ploop_conf", "edit_conf", "best_acu_conf", "grammar_logprob", "ploop_logprob", "best_final_logprob",
          "best_different_logprob", "best_acu_score")


def parse(setting: str):
    f = setting.split(":")
    g = dict(beam=float(f[0]), token_limit=int(f[1]), duration_scale=float(f[2]), transition_scale=float(f[3]))
    p = dict(beam=float(f[4]), token_limit=int(f[5]), duration_scale=float(f[6]), transition_scale=1.0)
    return g, p


def load(case):
    net = R.read_fst(open(os.path.join(FST, case + ".fst"), "rb").read())
    ac, _ = R.read_lna(os.path.join(FST, case + ".lna"))
    dur = R.read_durations(open(os.path.join(FST, case + ".dur")).read())
    return net, ac, dur


def restate_rows(net, ac, dur, ploop: bytes, settings):
    """-> (rows, why not): the restatement's row per setting, or the first reason to drop the seed / setting"""
    pnet = R.read_fst(ploop)
    rows = []
    for s in settings:
        g, p = parse(s)
        c = CR.confidence(net, ac, g, dur, pnet, p)
        plain = CR.confidence(net, ac, g, dur)
        if c.ties or plain.ties:
            return None, "%s: ties %s" % (s, c.ties + plain.ties)
        if c.grammar.status != R.OK or c.phone.status != R.OK:
            return None, "%s: no tokens" % s
        if c.no_final:
            return None, "%s: no end-node token in the grammar search" % s
        if not any(pnet.node_end[t[0]] for t in c.phone.tokens):
            return None, "%s: no end-node token in the phone-loop search" % s
        rows.append((s, c, plain))
    return rows, None


def main():
    ref = sys.argv[1]
    build = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "oracle", "_ref", "fst_conf")
    os.makedirs(build, exist_ok=True)
    os.makedirs(GOLDEN, exist_ok=True)
    src = os.path.join(ref, "decoder", "src")
    open(os.path.join(build, "fst_conf_driver.cc"), "w").write(DRIVER)
    exe = os.path.join(build, "fst_conf_driver")
    subprocess.run(["g++", "-O2", "-std=c++11", "-w", "-I", src, "-I", os.path.join(src, "misc"), os.path.join(build, "fst_conf_driver.cc")] +
                   [os.path.join(src, f) for f in ("FstConfidence.cc", "Fst.cc", "FstAcoustics.cc", "LnaReaderCircular.cc",
                                                   "NowayHmmReader.cc", "Hmm.cc", "str.cc", "io.cc")] + ["-o", exe], check=True)
    seen = {"zero": 0, "one": 0, "edit": 0}
    for ci, case in enumerate(CASES):
        net, ac, dur = load(case)
        letters = bytes(sorted(set(b"".join(net.symbols)))) or b"ab"
        # the grammar settings that can be recorded at all (the phone loop does not change them)
        usable = []
        for s in SETTINGS:
            plain = CR.confidence(net, ac, parse(s)[0], dur)
            why = "ties %s" % plain.ties if plain.ties else "no tokens" if plain.grammar.status != R.OK else \
                  "no end-node token" if plain.no_final else None
            print(case, "setting", s, "dropped: " + why if why else "kept")
            if not why:
                usable.append(s)
        rows = None
        for seed in SEEDS:
            rng = np.random.default_rng([7, ci, seed])
            ploop = CR.random_phone_loop(rng, ac.shape[1], n_phones=min(len(letters), 8), letters=letters)
            rows, why = restate_rows(net, ac, dur, ploop, usable)
            print(case, "seed", seed, "dropped: " + why if why else "kept")
            if rows:
                break
        assert rows, case
        inside = [0 < float(c.r["token_conf"]) < 1 for _, c, _ in rows]
        if not any(inside):      # (wide: a token that is not at an end node outranks the best end-node token at every setting)
            print(case, "NOT RECORDED: no setting leaves token_conf strictly inside (0, 1):", [float(c.r["token_conf"]) for _, c, _ in rows])
            continue
        ppath = os.path.join(GOLDEN, case + ".ploop.fst")
        open(ppath, "wb").write(ploop)
        r = subprocess.run([exe, os.path.join(FST, case + ".fst"), ppath, os.path.join(FST, case + ".lna"),
                            os.path.join(FST, case + ".dur")] + [s for s, _, _ in rows], check=True, capture_output=True)
        lines = []
        for line, (s, c, plain) in zip([l for l in r.stdout.split(b"\n") if l], rows):
            f = line.split(b"\t")
            assert f[0].decode() == s
            lines.append(b"\t".join(f[0].split(b":") + f[1:]))
            tok, edit = float(f[3]), float(f[5])
            seen["zero"] += tok == 0
            seen["one"] += tok == 1
            seen["edit"] += 0 < edit < 1
            # the restatement against the reference, here already (tests/test_fst_conf_host.py holds it)
            want = [c.text, c.ploop_text] + [("%.9g" % float(c.r[k])).encode() for k in FIELDS] + \
                   [b"%d" % ac.shape[0], ("%.9g" % float(c.r["confidence"])).encode(), ("%.9g" % float(plain.r["confidence"])).encode()]
            if f[1:] != want:
                print("MISMATCH", case, s, f[1:], want)
        open(os.path.join(GOLDEN, "expected_conf_%s.txt" % case), "wb").write(b"\n".join(lines) + b"\n")
        print(case, "recorded", len(lines), "rows; token_conf inside (0, 1) in", sum(inside))
    print(seen)
    assert seen["zero"] and seen["one"] and seen["edit"], seen


if __name__ == "__main__":
    main()

"""make_fst_golden.py -- records the reference decoder's own answers for the tiny cases of tests/golden/fst/.

    python tools/make_fst_golden.py REFERENCE_ROOT [BUILD_DIR]

Run by hand on a CPU machine that has the reference's sources; never run by a test.  It

  * writes the cases' inputs (NAME.fst, NAME.lna, NAME.dur; a few KB each) from fixed seeds with tools/fst_restate.py's
    generators, keeping only seeds for which the restatement reports no tie,
  * compiles the reference's Fst.cc, FstAcoustics.cc, LnaReaderCircular.cc, NowayHmmReader.cc, Hmm.cc, str.cc and io.cc
    with the small driver below (this project's own) into BUILD_DIR (default: oracle/_ref/fst, git-ignored), and
  * records, per case and (beam, token limit, duration scale, transition scale) setting, the binary's result string and
    its three log-probabilities as %.9g into expected_NAME.txt: tab-separated
        beam  limit  duration_scale  transition_scale  logprob  best_token_logprob  best_final_token_logprob  result

Only those data files are committed.  Every case has a .dur file: without one the reference's duration tables are empty
and its duration_logprob reads through a null pointer.  The case `durhi` puts its pdf indices in [n, 2n) of an LNA with
2n models, where the reference's tables hold the file's values: its duration term is not zero.
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")

DRIVER = r"""
// driver of the reference's FstSearch for tools/make_fst_golden.py: FST LNA DUR beam:limit:dscale:tscale ...
#include <cstdio>
#include <cstdlib>
#include <string>
#include "FstSearch.hh"
int main(int argc, char **argv) {
  for (int i = 4; i < argc; i++) {
    float beam, ds, ts; int limit;
    if (sscanf(argv[i], "%f:%d:%f:%f", &beam, &limit, &ds, &ts) != 4) return 2;
    FstSearch s(argv[1], nullptr, argv[3]);     // a search per setting: FstAcoustics never rewinds its frame counter
    s.set_beam(beam); s.set_token_limit(limit); s.set_duration_scale(ds); s.set_transition_scale(ts);
    s.lna_open(argv[2], 1024);
    s.init_search();
    s.run();
    float lp;
    std::string r = s.get_result_and_logprob(lp);
    printf("%s\t%.9g\t%.9g\t%.9g\t%s\n", argv[i], (double)lp, (double)s.get_best_token_logprob(),
           (double)s.get_best_final_token_logprob(), r.c_str());
    s.lna_close();
  }
  return 0;
}
"""

SETTINGS = ["2600:5000:3:1", "30:5000:3:1", "8:5000:1.5:0.7", "2600:3:3:1", "2600:1:3:1", "12:6:2:1.25", "0:5000:3:1"]


def lna_bytes(rng, frames: int, n_models: int, lnabytes: int) -> bytes:
    head = struct.pack(">iB", n_models, lnabytes)
    if lnabytes == 4:
        return head + (-rng.random((frames, n_models)) * 12).astype("<f4").tobytes()
    if lnabytes == 2:
        return head + rng.integers(0, 30000, (frames, n_models, 1)).astype(">u2").tobytes()
    return head + rng.integers(0, 256, (frames, n_models)).astype(np.uint8).tobytes()


def dur_text(rng, n: int, zero_every: int = 4) -> str:
    lines = ["4", str(n)]
    for i in range(n):
        a, b = (0.0, 0.0) if i % zero_every == 0 else (1 + rng.integers(1, 60) / 8.0, 0.5 + rng.integers(1, 40) / 8.0)
        lines.append("%d %.4f %.4f" % (i, a, b))
    return "\n".join(lines) + "\n"


TOY = R.write_fst([b"I 0", b"T 0 1 0 hello -0.5", b"T 0 2 1 , -1.25", b"T 1 1 0 , -0.1", b"T 1 3 2 , -0.7",
                   b"T 2 2 1", b"T 2 3 2 world -0.3", b"T 3 3 2 , -0.2", b"T 3 4 -1 again -0.9", b"T 4 1 0 , -0.4",
                   b"T 3 5 -1", b"T 5 5 -1 , -0.05", b"F 3", b"F 5"])

#        name     nodes models lnabytes frames  pdf offset
CASES = [("toy", None, 3, 4, 9, 0),
         ("rand2", 30, 8, 2, 20, 0),
         ("rand1", 24, 6, 1, 16, 0),
         ("rand4", 60, 10, 4, 24, 0),
         ("durhi", 20, 5, 2, 18, 5),
         ("wide", 40, 6, 2, 12, 0)]


def make_case(name, nodes, models, lnabytes, frames, offset, seed):
    rng = np.random.default_rng(seed)
    if nodes is None:
        fst = TOY
    else:
        fst = R.random_net(rng, nodes, models, max_deg=8 if name == "wide" else 6, p_word=0.3 if name == "wide" else 0.1)
        if offset:       # pdf indices into [n, 2n)
            out = []
            for line in fst.split(b"\n"):
                f = line.split(b" ")
                if f[0] == b"T" and int(f[3]) >= 0:
                    f[3] = b"%d" % (int(f[3]) + offset)
                out.append(b" ".join(f))
            fst = b"\n".join(out)
    lna = lna_bytes(rng, frames, models + offset, lnabytes)
    dur = dur_text(rng, models if offset else models + 2)
    return fst, lna, dur


def ties_of(fst, lna, dur):
    net = R.read_fst(fst)
    n_models, lnabytes = struct.unpack(">iB", lna[:5])
    ac = R.decode_lna(lna[5:], n_models, lnabytes)
    ties, finals = [], 0
    for s in SETTINGS:
        beam, limit, ds, ts = s.split(":")
        r = R.search(net, ac, float(beam), int(limit), float(ds), float(ts), R.read_durations(dur))
        ties += r.ties
        if r.status != R.OK:      # (the reference indexes an empty vector there)
            ties.append(("no tokens",))
        finals += len(r.words) > 0 and bool(np.isfinite(r.logprob))
    return ties, finals


def main():
    ref = sys.argv[1]
    build = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "oracle", "_ref", "fst")
    os.makedirs(build, exist_ok=True)
    os.makedirs(GOLDEN, exist_ok=True)
    src = os.path.join(ref, "decoder", "src")
    open(os.path.join(build, "fst_driver.cc"), "w").write(DRIVER)
    exe = os.path.join(build, "fst_driver")
    subprocess.run(["g++", "-O2", "-std=c++11", "-w", "-I", src, "-I", os.path.join(src, "misc"), os.path.join(build, "fst_driver.cc")] +
                   [os.path.join(src, f) for f in ("Fst.cc", "FstAcoustics.cc", "LnaReaderCircular.cc", "NowayHmmReader.cc",
                                                   "Hmm.cc", "str.cc", "io.cc")] + ["-o", exe], check=True)
    for name, nodes, models, lnabytes, frames, offset in CASES:
        seed = 0
        while True:      # the first seed without a tie (and, past the toy, with a result at the widest setting)
            fst, lna, dur = make_case(name, nodes, models, lnabytes, frames, offset, 1000 * len(name) + seed)
            ties, finals = ties_of(fst, lna, dur)
            if not ties and (nodes is None or finals >= 3):
                break
            assert nodes is not None, ties
            seed += 1
        paths = {}
        for ext, data in (("fst", fst), ("lna", lna), ("dur", dur.encode())):
            paths[ext] = os.path.join(GOLDEN, "%s.%s" % (name, ext))
            open(paths[ext], "wb").write(data)
        r = subprocess.run([exe, paths["fst"], paths["lna"], paths["dur"]] + SETTINGS, check=True, capture_output=True)
        lines = []
        for line in r.stdout.split(b"\n"):
            if line:
                f = line.split(b"\t")
                lines.append(b"\t".join(f[0].split(b":") + f[1:]))
        open(os.path.join(GOLDEN, "expected_%s.txt" % name), "wb").write(b"\n".join(lines) + b"\n")
        print(name, "seed", seed, "settings", len(lines))


if __name__ == "__main__":
    main()

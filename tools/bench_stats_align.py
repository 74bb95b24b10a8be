"""What -a costs stats --networks -M vit -n: the wall time of the tool with and without alignment output on
tools/bench_stats_bw.py's workload, and, with --parent BINDIR, of another build's `stats` without it.

    python tools/bench_stats_align.py [--utts 200] [--seconds 2.4] [--runs 2] [--parent BINDIR] [--out FILE]

Data: bench_stats_bw.py's -- tools/bench_align.py's model (D = 39, 50 000 Gaussians, 3 125 states x 16 components),
speech-like audio of about --seconds each, per utterance a left-to-right network of 100 random states -- with an
alignment= file per line.  Default beams.  --runs alternating runs of each command, every run under its own time limit.
-a adds one 4-byte store per frame to the Viterbi walk, one copy of the group's paths and a file per utterance.
One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_logl as BL  # noqa: E402

BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=2.4)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per tool run")
    ap.add_argument("--parent", default="", help="bin directory of another build whose stats runs -M vit -n without -a")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_stats_align_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.seconds - 0.2, a.seconds + 0.2)
    plain = BL.write_recipes(d, lines, a.utts)["chain"][0]
    recipe = os.path.join(d, "align.recipe")
    with open(recipe, "w") as f:
        for i, row in enumerate(open(plain).read().splitlines()):
            f.write("%s alignment=%s\n" % (row, os.path.join(d, "a%04d.phn" % i)))
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "model": "D=39, G=50000, S=3125 x 16", "networks": "100 states, 200 emitting arcs, one per utterance"}
    args = ["-b", base, "-c", BA.CFG, "-i", "1", "-r", recipe, "--ml", "--networks", "-M", "vit", "-n", "-o"]
    cmds = {"vit_n": [os.path.join(BIN, "stats")] + args + [os.path.join(d, "v")],
            "vit_n_a": [os.path.join(BIN, "stats")] + args + [os.path.join(d, "va"), "-a"]}
    if a.parent:
        cmds["parent_vit_n"] = [os.path.join(a.parent, "stats")] + args + [os.path.join(d, "vp")]
    walls = {k: [] for k in cmds}
    for r in range(a.runs):
        order = list(cmds.items())
        for k, c in (order if r % 2 == 0 else order[::-1]):
            wall, _ = BL.run(c, a.timeout)
            walls[k].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, k, wall), file=sys.stderr, flush=True)
    res["wall_s"] = walls
    written = [os.path.join(d, "a%04d.phn" % i) for i in range(a.utts)]
    res["alignment_files"] = sum(os.path.exists(p) for p in written)
    res["alignment_lines"] = sum(open(p).read().count("\n") for p in written if os.path.exists(p))
    res["lls_equal"] = open(os.path.join(d, "v.lls")).read() == open(os.path.join(d, "va.lls")).read()
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Full-statistics throughput: `stats --ml -t -O --full-stats` (mode-3 dumps, csrc/stats_full_accum.hip) against the
plain `stats --ml -t -O` on the same recipe, on the same box, in the same session.

    python tools/bench_stats_full.py [--utts 200] [--min-s 5] [--max-s 20] [--runs 2] [--prof DIR] [--out FILE]

Data: tools/bench_stats.py's: speech-like audio, D = 39, 50 000 Gaussians, 3 125 states x 16 components,
random state segmentations read with -O.

Measured:
* --runs alternating wall-time runs of the plain and the full tool (model text parse and the dump writes included: the
  mode-3 .gks of 50 000 Gaussians is 164 MB of floats);
* --prof DIR: one run of the full tool under `rocprofv3 --kernel-trace --stats`, a run of its own; device ms per 10^6
  frames of the full pass (k_full_*: likelihoods, posteriors, units, slab add; the pack pass runs once per fetch) and
  of the mode-1 passes (k_stats_*) of that same run, and the FP64 matrix-pipe bound of the unit kernel as DESIGN 4.10
  works it out: M PB (PB + 1) / 2 tiles of 16 x 16 x 2 = 512 FLOP per frame (M = 16, PB = 3: 49 152) at 78.6 TFLOP/s.
Every run has its own time limit.  One JSON line on stdout (and in --out)."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_stats as BS  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6   # MI355X datasheet
M, PB = 16, 3


def kernel_families(stats_csv):
    fam = {"full_lik": 0.0, "full_norm": 0.0, "full_units": 0.0, "full_slab_add": 0.0, "full_pack": 0.0, "mode1": 0.0}
    calls = dict.fromkeys(fam, 0)
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        for key, pat in (("full_lik", "k_full_lik"), ("full_norm", "k_full_norm"), ("full_units", "k_full_units"),
                         ("full_slab_add", "k_full_slab_add"), ("full_pack", "k_full_pack"), ("mode1", "k_stats_")):
            if pat in name:
                fam[key] += ns
                calls[key] += int(r["Calls"])
    return fam, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of the full tool")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_stats_full_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5", "stats_options": "--ml -t -O [--full-stats]"}
    log = os.path.join(d, "progress.log")
    srec = BS.write_segmentations(d, lines)
    common = [BS.STATS, "-b", base, "-c", BA.CFG, "-i", "1", "-r", srec, "--ml", "-t", "-O"]
    cmds = {"plain": common + ["-o", os.path.join(d, "plain")], "full": common + ["--full-stats", "-o", os.path.join(d, "full")]}
    walls = {"plain": [], "full": []}
    for r in range(a.runs):
        for tag in (("plain", "full") if r % 2 == 0 else ("full", "plain")):
            wall = BA.run(cmds[tag], a.timeout, log)
            walls[tag].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, tag, wall), file=sys.stderr, flush=True)
    frames = BS.lls_frames(os.path.join(d, "full"))
    res["frames"] = frames
    res["wall_s"] = walls
    res["gks_bytes"] = {k: os.path.getsize(os.path.join(d, k + ".gks")) for k in walls}
    flop = M * PB * (PB + 1) // 2 * 512
    res["matrix_pipe_bound"] = {"flop_per_frame": flop, "ms_per_1e6_frames": round(flop * 1e6 / (FP64_MATRIX_TFLOPS * 1e12) * 1e3, 4)}
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + cmds["full"]
        wall = BA.run(cmd, a.timeout, log, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = kernel_families(stats[0])
        per = {k: round(v / 1e6 / frames * 1e6, 3) for k, v in fam.items() if k != "full_pack"}   # (the pack pass: per fetch)
        full_ms = sum(v for k, v in per.items() if k.startswith("full_"))
        units_s = fam["full_units"] / 1e9
        res["prof"] = {"wall_s_under_profiler": round(wall, 2), "launches": calls, "ms_per_1e6_frames": per,
                       "full_pass_ms_per_1e6_frames": round(full_ms, 3), "mode1_ms_per_1e6_frames": per["mode1"],
                       "pack_ms_per_fetch": round(fam["full_pack"] / 1e6, 3),
                       "units_TFLOPS": round(frames * flop / units_s / 1e12, 2) if units_s > 0 else None,
                       "units_share_of_fp64_matrix_peak": round(frames * flop / units_s / 1e12 / FP64_MATRIX_TFLOPS, 3) if units_s > 0 else None}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

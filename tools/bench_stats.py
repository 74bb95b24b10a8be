"""ML statistics throughput: the native stats tool (features, segmentation and the accumulation on the
device, aasr_run_stats_recipe) against the native align on the same recipe, the two steps of a Viterbi
training round that run on the engine.

    python tools/bench_stats.py [--utts 200] [--min-s 5] [--max-s 20] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_align.py's recipe (speech-like audio, D = 39, 50 000 Gaussians, 3 125 states x 16
components, 625 five-state HMMs, random transcripts) for align; for stats the same audio with random
state segmentations (whole HMMs, 1-6 frames per state) as the recipe's alignment= files, read with -O as
train.pl reads align's output.  (align's own output on this random model is not used: where a search
window cuts a path the .phn files can jump between states that no transition joins, and stats -- like
the reference's PhnReader -- stops there with "Correct transition was not found".)

Measured:
* --runs alternating wall-time runs of `align` and `stats --ml -t -O` (model text parse included in both);
* --prof DIR: one run of stats under `rocprofv3 --kernel-trace --stats`; device ms per 10^6 frames of the
  accumulation (item, pdf and Gaussian passes) and of the feature chain, and the accumulation's bytes
  roofline: 8 x 39 bytes of double frame per frame read once, against the HBM peak.
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

STATS = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "stats")
HBM_TBPS = 8.0   # MI355X HBM3E peak


def kernel_families(stats_csv):
    fam = {"accumulation": 0.0, "features": 0.0, "other": 0.0}
    calls = {"accumulation": 0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_stats_" in name:
            fam["accumulation"] += ns
            calls["accumulation"] += int(r["Calls"])
        elif any(k in name for k in ("fft", "spectral", "temporal", "mean_sub", "feat", "mel", "dct", "delta")):
            fam["features"] += ns
        else:
            fam["other"] += ns
    return fam, calls


def write_segmentations(d, lines, seed=9):
    """per utterance a state-segmented .phn over its frames: random HMMs, every state 1-6 frames"""
    import wave
    import numpy as np
    rng = np.random.default_rng(seed)
    p = os.path.join(d, "stats.recipe")
    with open(p, "w") as rf:
        for wav, _tr, i in lines:
            with wave.open(wav) as w:
                frames = w.getnframes() // 128
            seg = os.path.join(d, "seg_%04d.phn" % i)
            with open(seg, "w") as f:
                t = 0
                while t < frames:
                    h = int(rng.integers(0, 3125 // BA.PER))
                    for k in range(BA.PER):
                        n = int(rng.integers(1, 7))
                        f.write("%d %d h%d.%d\n" % (t * 128, (t + n) * 128, h, k))
                        t += n
            rf.write("audio=%s alignment=%s\n" % (wav, seg))
    return p


def lls_frames(out):
    rows = open(out + ".lls").read().splitlines()
    return int(rows[1].split(": ")[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of stats")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_stats_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1),
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5",
           "stats_options": "--ml -t -O"}
    log = os.path.join(d, "progress.log")
    rec = BA.write_recipe(d, lines, "al")
    srec = write_segmentations(d, lines)
    align_cmd = [BA.ALIGN, "-b", base, "-c", BA.CFG, "-i", "1", "-r", rec]
    stats_cmd = [STATS, "-b", base, "-c", BA.CFG, "-i", "1", "-r", srec, "--ml", "-t", "-O", "-F", "0", "-W", "0",
                 "-A", "1", "-o", os.path.join(d, "st")]
    walls = {"align": [], "stats": []}
    for r in range(a.runs):
        order = [("align", align_cmd), ("stats", stats_cmd)]
        for tag, cmd in (order if r % 2 == 0 else order[::-1]):
            wall = BA.run(cmd, a.timeout, log)
            walls[tag].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, tag, wall), file=sys.stderr, flush=True)
    frames = lls_frames(os.path.join(d, "st"))
    res["frames"] = frames
    res["wall_s"] = walls
    res["frames_per_s"] = {k: round(frames / min(v), 1) for k, v in walls.items()}
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof),
               "--"] + stats_cmd
        wall = BA.run(cmd, a.timeout, log, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = kernel_families(stats[0])
        acc_s = fam["accumulation"] / 1e9
        moved = frames * 39 * 8
        res["prof"] = {"wall_s_under_profiler": round(wall, 2), "accumulation_launches": calls["accumulation"],
                       "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 3) for k, v in fam.items()},
                       "accumulation_bytes_per_frame": 39 * 8,
                       "accumulation_GBps": round(moved / acc_s / 1e9, 1) if acc_s > 0 else None,
                       "roofline_ms_per_1e6_frames": round(1e6 * 39 * 8 / (HBM_TBPS * 1e12) * 1e3, 4),
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

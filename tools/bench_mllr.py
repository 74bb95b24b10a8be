"""CMLLR estimation throughput: the native mllr tool in -M mode (features under the speaker's configuration,
segmentations, the statistics on the FP64 matrix pipe, one host solve per speaker; aasr_run_mllr_recipe), with the
native stats on the same recipe for orientation.

    python tools/bench_mllr.py [--utts 200] [--speakers 20] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_stats.py's recipe (speech-like audio, D = 39, 50 000 Gaussians, 3 125 states x 16 components, random
state segmentations read with -O) with speaker ids dealt to the utterances in blocks, and a speaker file whose default
speaker lists the feature configuration's lin_transform module.

Measured:
* --runs alternating wall-time runs of `mllr -M` and `stats --ml -O` (model text parse included in both);
* the host solve (aasr_mllr_solve) on the statistics of well-conditioned drawn data at D = 39, per speaker;
* --prof DIR: one run of mllr under `rocprofv3 --kernel-trace --stats`; device ms per 10^6 frames of pass 1
  (k_mllr_weights), pass 2 (k_mllr_rank) and the slab pass (k_mllr_slab_add), and pass 2's share of the FP64 matrix
  peak: 39 x 6 tiles x 256 x 2 operations per frame against 78.6 TFLOP/s.
Every run has its own time limit.  One JSON line on stdout (and in --out)."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_stats as BS  # noqa: E402

MLLR = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "mllr")
F64_MATRIX_TFLOPS = 78.6
OPS_PER_FRAME = 39 * 6 * 256 * 2


def lin_transform_module(cfg_path):
    """the name of the configuration's (last) lin_transform module"""
    names = re.findall(r"name\s+(\S+)\s+type\s+lin_transform", open(cfg_path).read())
    if not names:
        raise SystemExit("%s has no lin_transform module" % cfg_path)
    return names[-1]


def kernel_families(stats_csv):
    fam = {"pass1_weights": 0.0, "pass2_rank": 0.0, "slab_add": 0.0, "features": 0.0, "other": 0.0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_mllr_weights" in name:
            fam["pass1_weights"] += ns
        elif "k_mllr_rank" in name:
            fam["pass2_rank"] += ns
        elif "k_mllr_slab_add" in name:
            fam["slab_add"] += ns
        elif any(k in name for k in ("fft", "spectral", "temporal", "mean_sub", "feat", "mel", "dct", "delta")):
            fam["features"] += ns
        else:
            fam["other"] += ns
    return fam


def solve_seconds():
    import numpy as np
    from aaltoasr_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mllr_restate as MR
    rng = np.random.default_rng(5)
    model, x, pdf = MR.make_case(rng, 39, [16, 8, 16], [2000, 1500, 1500])
    G, k, beta = (np.asarray(a, np.float64) for a in MR.collect(model, x, pdf, extended=True))
    capi.mllr_solve(G, k, float(beta))
    t = time.time()
    for _ in range(3):
        capi.mllr_solve(G, k, float(beta))
    return (time.time() - t) / 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--speakers", type=int, default=20)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of mllr")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_mllr_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    srec = BS.write_segmentations(d, lines)
    per = -(-a.utts // a.speakers)
    rows = open(srec).read().splitlines()
    mrec = os.path.join(d, "mllr.recipe")
    open(mrec, "w").write("".join("%s speaker=spk%03d\n" % (r, i // per) for i, r in enumerate(rows)))
    module = lin_transform_module(BA.CFG)
    spk = os.path.join(d, "in.spkc")
    open(spk, "w").write("speaker default\n{\n  feature %s\n  {\n  }\n}\n" % module)
    res = {"utterances": a.utts, "speakers": a.speakers, "audio_seconds": round(samples / 16000.0, 1),
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5",
           "mllr_options": "-M %s -O" % module}
    log = os.path.join(d, "progress.log")
    mllr_cmd = [MLLR, "-b", base, "-c", BA.CFG, "-i", "1", "-r", mrec, "-S", spk, "-M", module, "-O",
                "-o", os.path.join(d, "out.spkc")]
    stats_cmd = [BS.STATS, "-b", base, "-c", BA.CFG, "-i", "1", "-r", srec, "--ml", "-O", "-o", os.path.join(d, "st")]
    walls = {"mllr": [], "stats": []}
    for r in range(a.runs):
        order = [("mllr", mllr_cmd), ("stats", stats_cmd)]
        for tag, cmd in (order if r % 2 == 0 else order[::-1]):
            wall = BA.run(cmd, a.timeout, log)
            walls[tag].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, tag, wall), file=sys.stderr, flush=True)
    frames = BS.lls_frames(os.path.join(d, "st"))
    res["frames"] = frames
    res["wall_s"] = walls
    res["wall_s_per_1e6_frames"] = {k: round(min(v) / frames * 1e6, 2) for k, v in walls.items()}
    res["host_solve_s_per_speaker"] = round(solve_seconds(), 4)
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof),
               "--"] + mllr_cmd
        wall = BA.run(cmd, a.timeout, log, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam = kernel_families(stats[0])
        p2 = fam["pass2_rank"] / 1e9
        res["prof"] = {"wall_s_under_profiler": round(wall, 2),
                       "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 3) for k, v in fam.items()},
                       "pass2_fp64_ops_per_frame": OPS_PER_FRAME,
                       "pass2_TFLOPS": round(frames * OPS_PER_FRAME / p2 / 1e12, 2) if p2 > 0 else None,
                       "pass2_fraction_of_matrix_peak": round(frames * OPS_PER_FRAME / p2 / 1e12 / F64_MATRIX_TFLOPS, 3) if p2 > 0 else None,
                       "roofline_ms_per_1e6_frames": round(1e6 * OPS_PER_FRAME / (F64_MATRIX_TFLOPS * 1e12) * 1e3, 3),
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

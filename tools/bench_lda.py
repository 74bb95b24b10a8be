"""LDA estimation throughput: the native lda tool (per-state counts on the host, the features at the transform module's
source on the device, the states' scatter sums on the FP64 matrix pipe, one host solve; aasr_run_lda_recipe).

    python tools/bench_lda.py [--utts 200] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_stats.py's recipe (speech-like audio, 3 125 states in 625 HMMs, random state segmentations read with
-O) with the first two HMMs renamed _ and __, and tests/golden/mfcc_cms_norm.feaconf, whose lin_transform module follows
a 39-dimensional source.

Measured:
* --runs wall-time runs of `lda -O --mingamma 1`;
* one in-process run (aasr_run_lda_recipe): device seconds of the feature pass and of the scatter pass from the
  driver's events, per 10^6 frames;
* --prof DIR: one run of the tool under `rocprofv3 --kernel-trace --stats` (a run of its own); device ms per 10^6 frames
  of k_scatter_items and k_scatter_slab_add, and the scatter kernel's share of the FP64 matrix peak: at 39 dimensions
  PB (PB + 1) / 2 = 6 tiles x 256 x 2 operations per frame against 78.6 TFLOP/s.  For comparison: k_mllr_rank reaches
  0.105 of that peak.
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
from bench_mllr import lin_transform_module  # noqa: E402

LDA = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "lda")
F64_MATRIX_TFLOPS = 78.6
OPS_PER_FRAME = 6 * 256 * 2


def kernel_families(stats_csv):
    fam = {"scatter_items": 0.0, "slab_add": 0.0, "features": 0.0, "other": 0.0}
    calls = {"scatter_items": 0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_scatter_items" in name:
            fam["scatter_items"] += ns
            calls["scatter_items"] += int(r["Calls"])
        elif "k_scatter_slab_add" in name:
            fam["slab_add"] += ns
        elif any(k in name for k in ("fft", "spectral", "temporal", "mean_sub", "feat", "mel", "dct", "delta")):
            fam["features"] += ns
        else:
            fam["other"] += ns
    return fam, calls


def with_silence_hmms(d, base, recipe):
    """the model's first two HMMs renamed _ and __, in the .ph and in every segmentation; -> (ph, recipe)"""
    ph = os.path.join(d, "lda.ph")
    open(ph, "w").write(re.sub(r" h1\n", " __\n", re.sub(r" h0\n", " _\n", open(base + ".ph").read())))
    out = os.path.join(d, "lda.recipe")
    with open(out, "w") as rf:
        for line in open(recipe).read().splitlines():
            info = dict(kv.split("=", 1) for kv in line.split())
            seg = info["alignment"]
            new = seg[:-4] + "_lda.phn"
            text = re.sub(r" h1\.", " __.", re.sub(r" h0\.", " _.", open(seg).read()))
            open(new, "w").write(text)
            rf.write("audio=%s alignment=%s\n" % (info["audio"], new))
    return ph, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of lda")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_lda_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    ph, rec = with_silence_hmms(d, base, BS.write_segmentations(d, lines))
    module = lin_transform_module(BA.CFG)
    from aaltoasr_amd import capi
    cfg_text = open(BA.CFG).read()
    dim = capi.Feat(cfg_text).module_dim(module)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "model": "S=3125 in 625 HMMs x 5", "lda_options": "-M %s -d %d -O --mingamma 1" % (module, dim)}
    log = os.path.join(d, "progress.log")
    cmd = [LDA, "-p", ph, "-c", BA.CFG, "-r", rec, "-M", module, "-d", str(dim), "-O", "--mingamma", "1",
           "-w", os.path.join(d, "out.cfg")]
    walls = []
    for r in range(a.runs):
        walls.append(round(BA.run(cmd, a.timeout, log), 2))
        print("run %d lda: %.2f s" % (r, walls[-1]), file=sys.stderr, flush=True)
    # in process: the driver's own device times
    run = capi.run_lda_recipe(cfg_text, capi.Topology(ph), rec, module, dim,
                              opts=capi.LdaOptions.defaults(ophn=1, mingamma=1.0))
    frames = int(run["frames"])
    res["frames"] = frames
    res["states_with_frames"] = int((run["state_gamma"] > 0).sum())
    res["wall_s"] = walls
    res["wall_s_per_1e6_frames"] = round(min(walls) / frames * 1e6, 2) if walls else None
    res["device_ms_per_1e6_frames"] = {"features": round(run["seconds_features"] / frames * 1e9, 3),
                                       "scatter": round(run["seconds_scatter"] / frames * 1e9, 3)}
    res["in_process_wall_s"] = round(run["seconds_total"], 2)
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        pcmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + cmd
        wall = BA.run(pcmd, a.timeout, log, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = kernel_families(stats[0])
        sc = fam["scatter_items"] / 1e9
        res["prof"] = {"wall_s_under_profiler": round(wall, 2),
                       "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 3) for k, v in fam.items()},
                       "scatter_launches": calls["scatter_items"],
                       "scatter_fp64_ops_per_frame": OPS_PER_FRAME,
                       "scatter_TFLOPS": round(frames * OPS_PER_FRAME / sc / 1e12, 3) if sc > 0 else None,
                       "scatter_fraction_of_matrix_peak": round(frames * OPS_PER_FRAME / sc / 1e12 / F64_MATRIX_TFLOPS, 4) if sc > 0 else None,
                       "roofline_ms_per_1e6_frames": round(1e6 * OPS_PER_FRAME / (F64_MATRIX_TFLOPS * 1e12) * 1e3, 4),
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

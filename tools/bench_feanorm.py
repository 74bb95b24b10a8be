"""Normalization / PCA estimation throughput: the native feanorm tool (the features at the normalization module's source
on the device, their blocked moments there, the blocked sums and the solve on the host; aasr_run_feanorm_recipe).

    python tools/bench_feanorm.py [--utts 200] [--runs 3] [--prof DIR] [--out FILE]

Data: the audio of tools/bench_stats.py's recipe (speech-like, 200 utterances of 5-20 s) and
tests/golden/mfcc_cms_norm.feaconf, whose normalization module follows a 39-dimensional source and whose lin_transform
module follows the normalization.  Block size 1000 (the default).

Measured, for the diagonal mode (`-M normalization`) and the full mode (`-M normalization -P transform`):
* --runs wall-time runs of the tool;
* one in-process run (aasr_run_feanorm_recipe): device seconds of the feature pass and of the moments pass from the
  driver's events, per 10^6 frames;
* --prof DIR: one run of the tool per mode under `rocprofv3 --kernel-trace --stats` (runs of their own); device ms per
  10^6 frames of k_moments_diag / k_moments_full and k_moments_seg_add, against the bytes roofline (8 x 39 = 312 bytes of
  double frame per frame read once, against the HBM peak) and, for the full mode, the FP64 matrix peak: at 39 dimensions
  PB (PB + 1) / 2 = 6 tiles x 256 x 2 operations per frame against 78.6 TFLOP/s.  For comparison: k_scatter_items<3>
  took 0.27 ms per 10^6 frames on the same audio.
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

FEANORM = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "feanorm")
HBM_TBPS = 8.0   # MI355X HBM3E peak
F64_MATRIX_TFLOPS = 78.6
OPS_PER_FRAME = 6 * 256 * 2
BYTES_PER_FRAME = 39 * 8
SCATTER_ITEMS_MS_PER_1E6 = 0.27   # k_scatter_items<3>, DESIGN 4.10


def kernel_families(stats_csv):
    fam = {"moments_diag": 0.0, "moments_full": 0.0, "seg_add": 0.0, "features": 0.0, "other": 0.0}
    calls = {"moments_diag": 0, "moments_full": 0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_moments_diag" in name or "k_moments_full" in name:
            key = "moments_diag" if "k_moments_diag" in name else "moments_full"
            fam[key] += ns
            calls[key] += int(r["Calls"])
        elif "k_moments_seg_add" in name:
            fam["seg_add"] += ns
        elif any(k in name for k in ("fft", "spectral", "temporal", "mean_sub", "feat", "mel", "dct", "delta")):
            fam["features"] += ns
        else:
            fam["other"] += ns
    return fam, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for the rocprofv3 --kernel-trace --stats runs of feanorm")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_feanorm_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    _base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    rec = os.path.join(d, "feanorm.recipe")
    open(rec, "w").write("".join("audio=%s\n" % wav for wav, _tr, _i in lines))
    from aaltoasr_amd import capi
    cfg_text = open(BA.CFG).read()
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "block_size": 1000}
    log = os.path.join(d, "progress.log")
    modes = {"diagonal": ["-M", "normalization"], "full": ["-M", "normalization", "-P", "transform"]}
    for mode, extra in modes.items():
        cmd = [FEANORM, "-c", BA.CFG, "-r", rec, "-w", os.path.join(d, mode + ".cfg")] + extra
        walls = []
        for r in range(a.runs):
            walls.append(round(BA.run(cmd, a.timeout, log), 2))
            print("run %d feanorm %s: %.2f s" % (r, mode, walls[-1]), file=sys.stderr, flush=True)
        # in process: the driver's own device times
        run = capi.run_feanorm_recipe(cfg_text, rec, module="normalization", pca="transform" if mode == "full" else None)
        frames = int(run["frames"])
        m = {"options": " ".join(extra), "frames": frames, "blocks": round(run["blocks"], 3), "wall_s": walls,
             "wall_s_per_1e6_frames": round(min(walls) / frames * 1e6, 2) if walls else None,
             "device_ms_per_1e6_frames": {"features": round(run["seconds_features"] / frames * 1e9, 3),
                                          "moments": round(run["seconds_moments"] / frames * 1e9, 3)},
             "in_process_wall_s": round(run["seconds_total"], 2)}
        if a.prof:
            pdir = os.path.join(os.path.abspath(a.prof), mode)
            os.makedirs(pdir, exist_ok=True)
            pcmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "--"] + cmd
            wall = BA.run(pcmd, a.timeout, log, cwd=tempfile.gettempdir())
            stats = glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True)
            fam, calls = kernel_families(stats[0])
            key = "moments_diag" if mode == "diagonal" else "moments_full"
            ks = fam[key] / 1e9
            p = {"wall_s_under_profiler": round(wall, 2), "launches": calls[key],
                 "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 4) for k, v in fam.items()},
                 "bytes_per_frame": BYTES_PER_FRAME,
                 "GBps": round(frames * BYTES_PER_FRAME / ks / 1e9, 1) if ks > 0 else None,
                 "bytes_roofline_ms_per_1e6_frames": round(1e6 * BYTES_PER_FRAME / (HBM_TBPS * 1e12) * 1e3, 4),
                 "stats_csv": os.path.relpath(stats[0], os.path.abspath(a.prof))}
            if mode == "full":
                p.update({"fp64_ops_per_frame": OPS_PER_FRAME,
                          "TFLOPS": round(frames * OPS_PER_FRAME / ks / 1e12, 3) if ks > 0 else None,
                          "fraction_of_matrix_peak": round(frames * OPS_PER_FRAME / ks / 1e12 / F64_MATRIX_TFLOPS, 4) if ks > 0 else None,
                          "matrix_roofline_ms_per_1e6_frames": round(1e6 * OPS_PER_FRAME / (F64_MATRIX_TFLOPS * 1e12) * 1e3, 4),
                          "scatter_items_ms_per_1e6_frames": SCATTER_ITEMS_MS_PER_1E6})
            m["prof"] = p
            print("prof %s: %s" % (mode, json.dumps(p)), file=sys.stderr, flush=True)
        res[mode] = m
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

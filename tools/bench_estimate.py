"""Re-estimation throughput: the native estimate tool on synthetic full statistics (mode-3 dumps) of a production-size
pool, plain --ml on the host and --ml --mllt with the covariances resident on the device (aasr_run_estimate).

    python tools/bench_estimate.py [--gauss 50000] [--dim 39] [--runs 2] [--prof DIR] [--out FILE]

Data: --gauss Gaussians x --dim dimensions with covariances B D_g B^T (one mixing matrix, D_g in [0.5, 2]), gamma in
[50, 500], mixtures of 10, all in one dump; a `pre` feature configuration with an undefined lin_transform `mllt`.

Measured:
* --runs wall-time runs of `estimate --ml` and of `estimate --ml --mllt mllt -c CFG`;
* one in-process run of each (aasr_run_estimate): the seconds of reading the dumps, and for MLLT the host-clock seconds
  (transfers included) of the covariance build, of the eight variance passes, of the seven G passes and of the host
  solves;
* --prof DIR: the MLLT run of the tool under `rocprofv3 --kernel-trace --stats` (a run of its own): device ms per launch
  of k_mllt_cov, k_mllt_var, k_mllt_gsum and k_mllt_slab_add, each pass against the bytes roofline (one read of the
  resident covariances, E x GP x 8 bytes, against the HBM peak) and k_mllt_gsum against the FP64 matrix peak
  (2 x dim x E x G operations a pass against 78.6 TFLOP/s).
Every run has its own time limit.  No threshold.  One JSON line on stdout (and in --out)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimate_restate as R  # noqa: E402

ESTIMATE = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "estimate")
HBM_TBPS = 8.0   # MI355X HBM3E peak
F64_MATRIX_TFLOPS = 78.6
ITEM = 256


def make_data(d, G, D, comps=10, seed=7):
    rng = np.random.default_rng(seed)
    S = G // comps
    base, dump = os.path.join(d, "prev"), os.path.join(d, "stats")
    mixtures = [(list(range(comps * s, comps * (s + 1))), [1.0 / comps] * comps) for s in range(S)]
    hmms = [("p%d" % h, [2 * h, 2 * h + 1]) for h in range(S // 2)]
    R.write_model(base, rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, size=(G, D)), mixtures, hmms)
    B = np.eye(D) + 0.3 * rng.normal(size=(D, D)) / np.sqrt(D)
    gamma, mean = rng.uniform(50, 500, size=G), rng.normal(size=(G, D))
    r, c = np.tril_indices(D)
    cov = (B[None] * rng.uniform(0.5, 2.0, size=(G, 1, D))) @ B.T
    m2 = cov[:, r, c] + mean[:, r] * mean[:, c]
    rec = np.zeros(G, np.dtype([("g", "<i4"), ("pos", "<i4"), ("fc", "<i4"), ("gamma", "<f8"), ("aux", "<f8"),
                                ("sx", "<f4", (D,)), ("sxx", "<f4", (len(r),)), ("end", "<i4")], align=False))
    rec["g"], rec["fc"], rec["gamma"], rec["end"] = np.arange(G), gamma.astype(np.int32), gamma, -1
    rec["sx"], rec["sxx"] = gamma[:, None] * mean, gamma[:, None] * m2
    with open(dump + ".gks", "wb") as f:
        f.write(np.array([G, D, R.FULL], "<i4").tobytes())
        f.write(rec.tobytes())
    R.write_mcs(dump + ".mcs", R.FULL, [(p, list(gamma[p]), -100.0) for p, _w in mixtures])
    R.write_lls(dump + ".lls", [("Number of frames", int(gamma.sum()))])
    lst, cfg = os.path.join(d, "list"), os.path.join(d, "prev.cfg")
    open(lst, "w").write(dump + "\n")
    open(cfg, "w").write("module\n{\n  name pre\n  type pre\n  dim %d\n}\nmodule\n{\n  name mllt\n  type lin_transform\n  dim %d\n"
                         "  sources pre\n}\n" % (D, D))
    return base, lst, cfg, os.path.getsize(dump + ".gks")


def run(cmd, timeout, cwd=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return time.time() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gauss", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for the rocprofv3 --kernel-trace --stats run of estimate --mllt")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_estimate_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    G, D = a.gauss, a.dim
    base, lst, cfg, gks_bytes = make_data(d, G, D)
    E, GP = D * (D + 1) // 2, (G + ITEM - 1) // ITEM * ITEM
    res = {"gaussians": G, "dim": D, "gks_MB": round(gks_bytes / 1e6, 1), "data_seconds": round(time.time() - t, 1),
           "resident_covariance_MB": round(E * GP * 8 / 1e6, 1)}
    from aaltoasr_amd import capi
    ml = [ESTIMATE, "-b", base, "-L", lst, "-o", os.path.join(d, "out_ml"), "--ml"]
    mllt = [ESTIMATE, "-b", base, "-L", lst, "-o", os.path.join(d, "out_mllt"), "--ml", "--mllt", "mllt", "-c", cfg]
    for name, cmd in (("ml", ml), ("mllt", mllt)):
        walls = []
        for r in range(a.runs):
            walls.append(round(run(cmd, a.timeout), 2))
            print("run %d estimate %s: %.2f s" % (r, name, walls[-1]), file=sys.stderr, flush=True)
        res[name] = {"options": " ".join(cmd[7:]), "wall_s": walls}
    run_ml = capi.run_estimate(base, lst, os.path.join(d, "in_ml"), opts=capi.EstimateOptions.defaults(no_write=1))
    res["ml"]["read_dumps_s"] = round(run_ml["seconds_read"], 3)
    run_mllt = capi.run_estimate(base, lst, os.path.join(d, "in_mllt"), config=cfg, mllt="mllt",
                                 opts=capi.EstimateOptions.defaults(no_write=1))
    cb, va, gs, hs = run_mllt["seconds_mllt_parts"]
    res["mllt"].update({"read_dumps_s": round(run_mllt["seconds_read"], 3), "mllt_s": round(run_mllt["seconds_mllt"], 3),
                        "host_clock_s": {"covariance_build": round(cb, 4), "variance_pass_each_of_8": round(va / 8, 4),
                                         "g_pass_each_of_7": round(gs / 7, 4), "host_solve_each_of_7": round(hs / 7, 4)}})
    if a.prof:
        pdir = os.path.abspath(a.prof)
        os.makedirs(pdir, exist_ok=True)
        pcmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "--"] + mllt
        wall = run(pcmd, a.timeout, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True)
        k = {}
        for r in csv.DictReader(open(stats[0])):
            for key in ("k_mllt_cov", "k_mllt_var", "k_mllt_gsum", "k_mllt_slab_add"):
                if key in r["Name"]:
                    k[key] = {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)}
        pass_bytes = E * GP * 8
        roof_ms = pass_bytes / (HBM_TBPS * 1e12) * 1e3
        ops = 2.0 * D * E * G
        p = {"wall_s_under_profiler": round(wall, 2), "kernels": k, "pass_bytes": pass_bytes,
             "bytes_roofline_ms_per_pass": round(roof_ms, 4), "stats_csv": os.path.relpath(stats[0], pdir)}
        for key in ("k_mllt_var", "k_mllt_gsum"):
            if key in k and k[key]["avg_ms"] > 0:
                p[key + "_fraction_of_hbm_roofline"] = round(roof_ms / k[key]["avg_ms"], 4)
                p[key + "_TFLOPS"] = round(ops / (k[key]["avg_ms"] * 1e-3) / 1e12, 3)
        if "k_mllt_gsum" in k and k["k_mllt_gsum"]["avg_ms"] > 0:
            p["k_mllt_gsum_fraction_of_matrix_peak"] = round(ops / (k["k_mllt_gsum"]["avg_ms"] * 1e-3) / 1e12 / F64_MATRIX_TFLOPS, 4)
        res["mllt"]["prof"] = p
        print("prof: %s" % json.dumps(p), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

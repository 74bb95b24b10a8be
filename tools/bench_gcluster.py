"""Gaussian-pool clustering time: the device run (aasr_gcluster_arrays: Euclidean pass, four divergence passes, five
centre passes, one synchronisation each) against the NumPy restatement on the CPU.

    python tools/bench_gcluster.py [--gauss 50000] [--clusters 1000] [--dim 39] [--runs 3] [--slice 1000] [--out FILE]

Data: a seeded pool, means N(0, 1), variances exp(U(ln 0.25, ln 4)).

Measured:
* device: --runs in-process runs after one warm-up run; the whole call on the host clock (packing, uploads, the run,
  the map back) and the driver's own clock around the five steps, each to its synchronisation;
* CPU: tools/gcluster_restate.py's divergence pass on the first --slice Gaussians against all the centres, once, and
  that time scaled by gauss / slice x 4 passes.  It is a SCALED figure for a vectorised NumPy restatement, not a run
  of the reference's one-division-per-term loop, which nobody has timed here; the Euclidean pass and the centre sums
  are left out of it.
The runs' maps are compared with each other (the same input gives the same bytes).  No GPU: the script fails.
One JSON line on stdout (and in --out)."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _restate():
    spec = importlib.util.spec_from_file_location("gcluster_restate", os.path.join(ROOT, "tools", "gcluster_restate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gauss", type=int, default=50000)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--slice", type=int, default=1000)
    ap.add_argument("--out")
    a = ap.parse_args()
    from aaltoasr_amd import capi
    if capi.lib().aasr_device_count() < 1:
        raise SystemExit("bench_gcluster: no HIP device; nothing is measured without one")
    rng = np.random.default_rng(20260928)
    mean = rng.standard_normal((a.gauss, a.dim))
    cov = np.exp(rng.uniform(np.log(0.25), np.log(4.0), (a.gauss, a.dim)))
    first, written, _ = capi.gcluster_arrays(mean, cov, clusters=a.clusters)          # warm-up
    calls, steps = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        cluster_of, n, s = capi.gcluster_arrays(mean, cov, clusters=a.clusters)
        calls.append(time.perf_counter() - t0)
        steps.append(s)
        if not np.array_equal(cluster_of, first):
            raise SystemExit("bench_gcluster: two runs on the same input gave different maps")
    GR = _restate()
    sl = min(a.slice, a.gauss)
    ldet = GR.log_det(cov[:sl])
    cm, cc, cl, cv = GR.centres(mean[:a.clusters * 4], cov[:a.clusters * 4], np.arange(min(a.clusters * 4, a.gauss)) % a.clusters,
                                a.clusters)
    t0 = time.perf_counter()
    GR.assign_kl(mean[:sl], cov[:sl], ldet, cm, cc, cl, cv)
    cpu_slice = time.perf_counter() - t0
    res = {"what": "gcluster", "gauss": a.gauss, "clusters": a.clusters, "dim": a.dim, "clusters_written": written,
           "device_call_seconds": [round(x, 4) for x in calls], "device_steps_seconds": [round(x, 4) for x in steps],
           "device_steps_seconds_best": round(min(steps), 4),
           "divisions_per_run": 4 * a.gauss * a.clusters * a.dim,
           "cpu_restatement_slice": sl, "cpu_restatement_slice_seconds": round(cpu_slice, 4),
           "cpu_restatement_4_passes_scaled_seconds": round(cpu_slice * a.gauss / sl * 4, 2),
           "cpu_figure_is": "one NumPy divergence pass on the slice, scaled by gauss / slice x 4; not measured at full size"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

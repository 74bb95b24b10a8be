"""Side benchmark of the state-tying search (not part of bench.py): synthetic statistics injected into an aasr_tie
handle, the split search timed with both hop plans, and tools/tie_restate.py on the same input as the CPU baseline.

    python tools/bench_tie.py [--phones 40] [--labels 40] [--seen 0.25] [--rules 150] [--dim 39] [--restate-trees 1]
                              [--no-device]

Size: `phones` centre phones x 3 states, `labels` context labels of which a fraction `seen` of the left x right pairs
occurs, `rules` random context rules, `dim` dimensions.  The restatement is NumPy on one core and walks `restate-trees`
trees only (it takes about a minute a tree at the default size); its time is reported for those trees and scaled to
all trees by their count.  One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tie_restate as TR  # noqa: E402


def make_input(a):
    rng = np.random.default_rng(a.seed)
    d = a.dim
    labels = ["c%02d" % i for i in range(a.labels)]
    rules = []
    for r in range(a.rules):
        k = int(rng.integers(1, a.labels // 2 + 1))
        rules.append("Q%03d context %s" % (r, ",".join(labels[i] for i in sorted(rng.permutation(a.labels)[:k]))))
    rules_text = "\n".join(rules) + "\n"
    eff_l, eff_r = rng.standard_normal((a.labels, d)), 0.6 * rng.standard_normal((a.labels, d))
    il = np.tril_indices(d)
    names, gamma, sx, sxx = [], [], [], []
    for p in range(a.phones):
        A = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
        cov = A @ A.T
        seen = rng.random((a.labels, a.labels)) < a.seen
        for s in range(3):
            base = rng.standard_normal(d)
            for l, r in zip(*np.nonzero(seen)):
                g = float(rng.integers(20, 200))
                mu = base + (1 + 0.3 * s) * eff_l[l] + eff_r[r] + 0.3 * rng.standard_normal(d)
                m2 = g * (cov * rng.uniform(0.7, 1.4) + np.outer(mu, mu))
                names.append(("%s-p%02d+%s" % (labels[l], p, labels[r]), s))
                gamma.append(g)
                sx.append(g * mu)
                sxx.append(m2[il])
    return rules_text, names, np.array(gamma), np.array(sx), np.array(sxx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--labels", type=int, default=40)
    ap.add_argument("--seen", type=float, default=0.25)
    ap.add_argument("--rules", type=int, default=150)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--sgain", type=float, default=200.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--restate-trees", type=int, default=1)
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    rules_text, names, gamma, sx, sxx = make_input(a)
    out = {"phones": a.phones, "labels": a.labels, "rules": a.rules, "dim": a.dim, "classes": len(names), "count": a.count,
           "sgain": a.sgain}
    if not a.no_device:
        from aaltoasr_amd import capi
        with tempfile.TemporaryDirectory() as tmp:
            rp = os.path.join(tmp, "bench.rules")
            open(rp, "w").write(rules_text)
            clusters = {}
            for hops in (2, 1, 2, 1):          # the first pair warms up (allocations, code load); the second is reported
                t = capi.Tie(a.dim, rp)
                for lab, s in names:
                    t.context_phone(lab, s)
                t.set_stats(gamma, sx, sxx)
                t0 = time.perf_counter()
                t.split(count=a.count, sgain=a.sgain, context=1, hops=hops)
                out["seconds_split_hops%d" % hops] = round(time.perf_counter() - t0, 4)
                out["rounds"] = t.shape()["rounds_split"]
                clusters[hops] = [(c["phone"], c["state"], c["members"]) for c in t.clusters()]
                t.close()
            out["clusters"] = len(clusters[2])
            out["hop_plans_agree"] = clusters[1] == clusters[2]
    if a.restate_trees > 0:
        pool = TR.Pool(TR.read_rules(rules_text))
        keep = []
        for i, (lab, s) in enumerate(names):
            if int(TR.center_phone(lab)[1:]) * 3 + s < a.restate_trees:
                pool.context_phone(lab, s)
                keep.append(i)
        t0 = time.perf_counter()
        r = TR.run(pool, gamma[keep], sx[keep], sxx[keep], count=a.count, sgain=a.sgain, context=1)
        sec = time.perf_counter() - t0
        out.update(restate_trees=a.restate_trees, restate_seconds=round(sec, 2), restate_clusters=len(r["clusters"]),
                   restate_seconds_scaled_to_all_trees=round(sec * a.phones * 3 / a.restate_trees, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

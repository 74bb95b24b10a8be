#!/usr/bin/env python
"""trace_overlap.py -- what a `rocprofv3 --kernel-trace --output-format csv` run of bench.py says about the chunked
score + LNA step (csrc/gmm_score_lna.cc):

    python tools/trace_overlap.py KERNEL_TRACE.csv [...]

Per file, over the last 20 steps (a step begins with k_spectral_fused): the step's span, the per-kernel sums per step, how
much of the LNA kernels' time lies inside scoring-kernel intervals, and the launches of the last whole step with their
queue, stream, start and end."""
import collections
import csv
import sys


def load(path):
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id"), r.get("Stream_Id"))
            for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: r[1])
    return rows


def report(path):
    rows = load(path)
    starts = [i for i, r in enumerate(rows) if "k_spectral_fused" in r[0]][-20:]
    print("%s: %d launches, %d steps" % (path, len(rows), len(starts) - 1))
    total, spans, inside, lna_total = collections.Counter(), [], 0, 0
    for a, b in zip(starts, starts[1:]):
        step = rows[a:b]
        spans.append(rows[b][1] - rows[a][1])
        scoring = [(s, e) for n, s, e, _q, _st in step if "k_gmm_diag_score_pl" in n]
        for n, s, e, _q, _st in step:
            total[n.split("(")[0][-60:]] += e - s
            if "k_state_norm_lna" in n:
                lna_total += e - s
                inside += sum(max(0, min(e, e2) - max(s, s2)) for s2, e2 in scoring)
    n = len(spans)
    print("  step span avg %.3f ms (min %.3f, max %.3f)" % (sum(spans) / n / 1e6, min(spans) / 1e6, max(spans) / 1e6))
    for k, v in total.most_common(8):
        print("  %-62s %.3f ms/step" % (k, v / n / 1e6))
    print("  LNA kernel time inside scoring intervals: %.3f of %.3f ms/step" % (inside / n / 1e6, lna_total / n / 1e6))
    a, b = starts[-2], starts[-1]
    t0 = rows[a][1]
    for name, s, e, q, st in rows[a:b]:
        print("    %-50s queue %s stream %s  %8.3f -> %8.3f ms (%.3f)" % (
            name.split("(")[0][-50:], q, st, (s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6))


if __name__ == "__main__":
    for p in sys.argv[1:]:
        report(p)

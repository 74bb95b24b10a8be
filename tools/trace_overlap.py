#!/usr/bin/env python
"""trace_overlap.py -- what a `rocprofv3 --kernel-trace --output-format csv` run of bench.py says about the chunked
score + LNA step (csrc/gmm_score_lna.cc):

    python tools/trace_overlap.py [--frames F] [--chunk0-frames N] [--baseline OTHER.csv] KERNEL_TRACE.csv [...]

Per file, over the last 20 steps (a step begins with k_spectral_fused): the step's span, the per-kernel sums per step, how
much of the LNA kernels' time lies inside scoring-kernel intervals, and the launches of the last whole step with their
queue, stream, start and end.  Then, per scoring launch in time order and averaged over the steps: its duration, the LNA
time beside it, and in how many of the steps an LNA kernel was already running when it began and still running when it
ended -- a launch that begins under a running LNA grid is placed workgroup by workgroup as that grid drains.  Last, "what
the company costs": the sum of the scoring launches against (F / frames of chunk 0) x the duration of chunk 0, the first
scoring launch of a step, which must be a whole chunk with no LNA kernel beside it.  A schedule that scores the remainder
first has no such launch; --baseline names the trace (same box, same session) of one that has.  F and the frames of chunk
0 default to the bench.py step on 256 CUs: 449 280 and 131 072.

With the library built (no device needed) the plan of the step -- aasr_debug_score_lna_plan for --frames on --cus CUs, the
compiled-in schedule or --share -- gives the frames of every scoring launch and LNA segment, and the per-launch lines add
the launch's rate in frames/us and that of the LNA segment released behind the launch before it, which is the one that
runs beside it: a pace (segment rate over launch rate) below 1 means the segment outlives its launch."""
import argparse
import collections
import csv
import ctypes
import os
import sys


def load(path):
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id"), r.get("Stream_Id"))
            for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: r[1])
    return rows


def steps_of(rows):
    starts = [i for i, r in enumerate(rows) if "k_spectral_fused" in r[0]][-20:]
    return starts, [rows[a:b] for a, b in zip(starts, starts[1:])]


def split(step):
    scoring = [(s, e) for n, s, e, _q, _st in step if "k_gmm_diag_score_pl" in n]
    lna = [(s, e) for n, s, e, _q, _st in step if "k_state_norm_lna" in n]
    return scoring, lna


def chunk0_ms(path):
    """duration of the first scoring launch of a step, averaged; None where an LNA kernel runs beside it in any step"""
    _starts, steps = steps_of(load(path))
    durs = []
    for step in steps:
        scoring, lna = split(step)
        if not scoring:
            return None
        s, e = scoring[0]
        if any(min(e, e2) > max(s, s2) for s2, e2 in lna):
            return None
        durs.append(e - s)
    return sum(durs) / len(durs) / 1e6 if durs else None


def plan_frames(frames, cus, share):
    """(frames per scoring launch in time order, (frames, launch waited for) per LNA segment in side-stream order) of the
    step's plan; None without the library"""
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from aaltoasr_amd import capi
        L = capi.lib()
    except Exception as e:       # the rates are an extra: the rest of the report needs no library
        print("  (no plan, so no rates: %s)" % e)
        return None
    i64, p64 = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.aasr_debug_score_lna_plan.argtypes = [i64, ctypes.c_int, i64, ctypes.c_int, ctypes.c_double, ctypes.c_int, p64, p64, i64,
                                            p64, p64]
    L.aasr_debug_score_lna_plan.restype = i64
    cap = 256
    score, lna = (i64 * (2 * cap))(), (i64 * (3 * cap))()
    ns, nl = i64(0), i64(0)
    if L.aasr_debug_score_lna_plan(frames, cus, 0, -1, share, -1, score, lna, cap, ctypes.byref(ns), ctypes.byref(nl)) <= 0:
        return None
    return ([score[2 * i + 1] for i in range(ns.value)], [(lna[3 * i + 1], lna[3 * i + 2]) for i in range(nl.value)])


def report(path, frames, chunk0_frames, baseline, plan=None):
    rows = load(path)
    starts, steps = steps_of(rows)
    print("%s: %d launches, %d steps" % (path, len(rows), len(starts) - 1))
    total, spans, inside, lna_total = collections.Counter(), [], 0, 0
    per_launch = collections.defaultdict(lambda: [0, 0, 0, 0, 0])   # index -> duration, LNA beside, at start, at end, steps
    seg_ns = collections.defaultdict(lambda: [0, 0])                # LNA segment (side-stream order) -> duration, steps
    for (a, b), step in zip(zip(starts, starts[1:]), steps):
        spans.append(rows[b][1] - rows[a][1])
        scoring, lna = split(step)
        for n, s, e, _q, _st in step:
            total[n.split("(")[0][-60:]] += e - s
            if "k_state_norm_lna" in n:
                lna_total += e - s
                inside += sum(max(0, min(e, e2) - max(s, s2)) for s2, e2 in scoring)
        if plan and len(lna) == len(plan[1]) and len(scoring) == len(plan[0]):
            for k, (s, e) in enumerate(sorted(lna)):
                seg_ns[k][0] += e - s
                seg_ns[k][1] += 1
        for i, (s, e) in enumerate(scoring):
            acc = per_launch[i]
            acc[0] += e - s
            acc[1] += sum(max(0, min(e, e2) - max(s, s2)) for s2, e2 in lna)
            acc[2] += any(s2 < s < e2 for s2, e2 in lna)
            acc[3] += any(s2 < e < e2 for s2, e2 in lna)
            acc[4] += 1
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
    print("  scoring launches, averaged over the steps that have them:")
    score_sum = 0.0
    for i in sorted(per_launch):
        dur, beside, at_start, at_end, cnt = per_launch[i]
        score_sum += dur / n / 1e6
        print("    launch %d: %.3f ms, LNA beside it %.3f ms, an LNA kernel running at its start in %d of %d steps, at its end in %d"
              % (i, dur / cnt / 1e6, beside / cnt / 1e6, at_start, cnt, at_end))
        if plan and seg_ns and i < len(plan[0]):
            rate = plan[0][i] / (dur / cnt / 1e3)
            line = "      %d frames, %.1f frames/us" % (plan[0][i], rate)
            for k, (n_frames, wait) in enumerate(plan[1]):
                if wait == i - 1 and seg_ns[k][1]:
                    seg_rate = n_frames / (seg_ns[k][0] / seg_ns[k][1] / 1e3)
                    line += "; LNA segment beside it: %d frames in %.3f ms, %.1f frames/us, pace %.2f" % (
                        n_frames, seg_ns[k][0] / seg_ns[k][1] / 1e6, seg_rate, seg_rate / rate)
            print(line)
    if plan and seg_ns:
        k = len(plan[1]) - 1
        if plan[1][k][1] == len(plan[0]) - 1 and seg_ns[k][1]:
            ms = seg_ns[k][0] / seg_ns[k][1] / 1e6
            print("    last LNA pass (behind the last launch, alone on the chip): %d frames in %.3f ms, %.1f frames/us"
                  % (plan[1][k][0], ms, plan[1][k][0] / ms / 1e3))
    base_path = baseline or path
    c0 = chunk0_ms(base_path)
    if c0 is None:
        print("  what the company costs: no whole chunk scored alone at the head of the steps of %s (give --baseline)" % base_path)
    else:
        alone = frames / chunk0_frames * c0
        print("  what the company costs: scoring launches %.3f ms/step against %d / %d x %.3f = %.3f ms alone (chunk 0 of %s): %+.3f ms"
              % (score_sum, frames, chunk0_frames, c0, alone, base_path, score_sum - alone))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=449280)
    ap.add_argument("--chunk0-frames", type=int, default=131072)
    ap.add_argument("--baseline", default="")
    ap.add_argument("--cus", type=int, default=256, help="CUs of the box the trace was taken on (the plan's chunk)")
    ap.add_argument("--share", type=float, default=-1.0, help="the schedule's share, where the trace was not taken with the compiled-in one")
    ap.add_argument("traces", nargs="+")
    args = ap.parse_args()
    plan = plan_frames(args.frames, args.cus, args.share)
    for p in args.traces:
        report(p, args.frames, args.chunk0_frames, args.baseline, plan)

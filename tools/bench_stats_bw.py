"""stats --networks throughput: Baum-Welch statistics over HMM networks (features, state scoring, the forward-backward
pass, the occupancies as weighted entries and the weighted accumulation on the device) next to the same tool over .phn
files of the same audio and to logl -H over the same networks.

    python tools/bench_stats_bw.py [--utts 200] [--seconds 2.4] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_logl.py's workload -- tools/bench_align.py's model (D = 39, 50 000 Gaussians, 3 125 states x 16
components), speech-like audio of about --seconds each, per utterance a left-to-right network of 100 random states --
and tools/bench_stats.py's random state segmentations of the same audio for the .phn run.  Default beams.

Measured: --runs alternating wall-time runs of `stats --ml --networks -t`, `stats --ml -t -O` and `logl -H` (model text
parse included in all), from one further run of each network tool with AASR_RECIPE_TIMING=1 the seconds its calling
thread spent per stage (each stage waited for, so they do not overlap in that run), the entries per frame that the
network run reports at -i 1, and with --prof a rocprofv3 --kernel-trace --stats run of its own of the network tool:
the time of k_hmmnet_fb, of the three entry kernels and of k_stats_items_w.  Every run has its own time limit.  One
JSON line on stdout (and in --out)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_logl as BL  # noqa: E402
import bench_stats as BS  # noqa: E402

BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
FAMILIES = (("forward_backward", ("k_hmmnet_fb",)), ("entries", ("k_fb_frame_sums", "k_fb_entry_counts", "k_fb_entry_fill")),
            ("weighted_items", ("k_stats_items_w",)), ("reductions", ("k_stats_pdf_reduce", "k_stats_gauss_reduce")))


def run(cmd, timeout, env=None, cwd=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})), cwd=cwd)
    wall = time.time() - t
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (cmd[0], r.returncode, r.stderr[-2000:]))
    return wall, r


def kernel_families(stats_csv):
    fam = {k: 0.0 for k, _ in FAMILIES}
    fam["other"] = 0.0
    calls = {k: 0 for k, _ in FAMILIES}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        for k, names in FAMILIES:
            if any(n in name for n in names):
                fam[k] += ns
                calls[k] += int(r["Calls"])
                break
        else:
            fam["other"] += ns
    return {k: round(v / 1e6, 3) for k, v in fam.items()}, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=2.4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of stats --networks")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_stats_bw_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.seconds - 0.2, a.seconds + 0.2)
    net_recipe = BL.write_recipes(d, lines, a.utts)["chain"][0]
    phn_recipe = BS.write_segmentations(d, lines)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "model": "D=39, G=50000, S=3125 x 16", "networks": "100 states, 200 emitting arcs, one per utterance"}
    common = ["-b", base, "-c", BA.CFG, "-i", "1"]
    cmds = {"stats_networks": [os.path.join(BIN, "stats")] + common + ["-r", net_recipe, "--ml", "--networks", "-t", "-o",
                                                                        os.path.join(d, "bw")],
            "stats_phn": [os.path.join(BIN, "stats")] + common + ["-r", phn_recipe, "--ml", "-t", "-O", "-o", os.path.join(d, "ph")],
            "logl_networks": [os.path.join(BIN, "logl")] + common + ["-r", net_recipe, "-H"]}
    walls = {k: [] for k in cmds}
    for r in range(a.runs):
        order = list(cmds.items())
        for k, c in (order if r % 2 == 0 else order[::-1]):
            wall, out = run(c, a.timeout)
            walls[k].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, k, wall), file=sys.stderr, flush=True)
            if k == "stats_networks":
                m = re.search(r"Weighted entries: (\d+) over (\d+) frames", out.stderr)
                res["entries"], res["frames"] = int(m.group(1)), int(m.group(2))
                res["max_abs_1_minus_frame_sum"] = float(re.search(r"of a frame: (\S+)", out.stderr).group(1))
                res["retried_utterances"] = out.stderr.count("Could not initialize the utterance segmentation.")
    res["entries_per_frame"] = round(res["entries"] / max(1, res["frames"]), 3)
    res["phn_frames"] = BS.lls_frames(os.path.join(d, "ph"))
    res["wall_s"] = walls
    res["stage_seconds"] = {}
    for k in ("stats_networks", "logl_networks"):
        _, out = run(cmds[k], a.timeout, env={"AASR_RECIPE_TIMING": "1"})
        line = [l for l in out.stderr.splitlines() if " timing: " in l]
        if line:
            res["stage_seconds"][k] = {n.strip(): float(v) for n, v in re.findall(r"([a-z][a-z \-]+?) ([\d.]+) s", line[0].split("timing: ")[1])}
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + \
            cmds["stats_networks"]
        wall, _ = run(cmd, a.timeout, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = kernel_families(stats[0])
        res["prof"] = {"wall_s_under_profiler": round(wall, 2), "kernel_ms": fam, "kernel_calls": calls,
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

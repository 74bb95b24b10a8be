"""lda --networks throughput: the native lda tool over HMM networks (per group the chain's output, the state scores, one
forward-backward batch, the pdf-major entries, the frames at the module's source, one weighted scatter accumulation;
aasr_run_lda_networks_recipe).

    python tools/bench_lda_networks.py [--utts 200] [--seconds 2.4] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_lda.py's recipe -- tools/bench_align.py's model (D = 39, 3 125 states) and speech-like audio, the first
two HMMs renamed _ and __, tests/golden/mfcc_cms_norm.feaconf -- with, per utterance, a left-to-right network of 100
random states from tools/hmmnet_cases.py in place of the segmentation.  Default beams, Baum-Welch.

Measured, per 10^6 frames:
* --runs wall-time runs of `lda --networks --mingamma 1`;
* one further run with AASR_RECIPE_TIMING=1: the seconds the driver's thread spent on input and networks, both feature
  stagings, scoring, forward-backward with the entries, and the accumulation (each stage waited for);
* one in-process run (aasr_run_lda_networks_recipe): device seconds of the two feature stagings and of the scatter
  launches from the driver's events, the weighted entries per frame and the mean entries per work item;
* --prof DIR: one run of the tool under `rocprofv3 --kernel-trace --stats` (a run of its own): device ms of
  k_scatter_entries and k_scatter_slab_add.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_logl as BL  # noqa: E402
import hmmnet_cases as HC  # noqa: E402
from bench_mllr import lin_transform_module  # noqa: E402

LDA = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "lda")
S = 3125
TIMING = re.compile(r"lda timing: input and networks ([\d.]+) s, features \(both stagings\) ([\d.]+) s, scoring ([\d.]+) s, "
                    r"forward-backward and entries ([\d.]+) s, accumulation ([\d.]+) s")


def write_recipe(d, base, lines):
    """the model's first two HMMs renamed _ and __ (its .gk and .mc linked beside the new .ph), a chain per utterance"""
    new = os.path.join(d, "ldanet")
    open(new + ".ph", "w").write(re.sub(r" h1\n", " __\n", re.sub(r" h0\n", " _\n", open(base + ".ph").read())))
    for ext in (".gk", ".mc"):
        if not os.path.exists(new + ext):
            os.symlink(base + ext, new + ext)
    rng = np.random.default_rng(13)
    out = os.path.join(d, "ldanet.recipe")
    with open(out, "w") as f:
        for wav, _, i in lines:
            net = os.path.join(d, "ldanet%04d.hmmnet" % i)
            open(net, "w").write(HC.chain([int(s) for s in rng.integers(0, S, 100)]))
            f.write("audio=%s hmmnet=%s\n" % (wav, net))
    return new, out


def scatter_kernels(stats_csv):
    fam = {"scatter_entries": 0.0, "slab_add": 0.0}
    calls = 0
    for r in csv.DictReader(open(stats_csv)):
        if "k_scatter_entries" in r["Name"]:
            fam["scatter_entries"] += float(r["TotalDurationNs"])
            calls += int(r["Calls"])
        elif "k_scatter_slab_add" in r["Name"]:
            fam["slab_add"] += float(r["TotalDurationNs"])
    return fam, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=2.4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of lda")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_ldanet_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.seconds - 0.2, a.seconds + 0.2)
    model, rec = write_recipe(d, base, lines)
    module = lin_transform_module(BA.CFG)
    from aaltoasr_amd import capi
    cfg_text = open(BA.CFG).read()
    dim = capi.Feat(cfg_text).module_dim(module)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "data_seconds": round(time.time() - t, 1),
           "model": "D=39, G=50000, S=3125 x 16", "networks": "100 states, 200 emitting arcs, one per utterance",
           "lda_options": "--networks -M %s -d %d --mingamma 1" % (module, dim)}
    cmd = [LDA, "--networks", "-b", model, "-c", BA.CFG, "-r", rec, "-M", module, "-d", str(dim), "--mingamma", "1", "-i", "1",
           "-w", os.path.join(d, "out.cfg")]
    walls = []
    for r in range(a.runs):
        wall, _ = BL.run(cmd, a.timeout)
        walls.append(round(wall, 2))
        print("run %d lda --networks: %.2f s" % (r, wall), file=sys.stderr, flush=True)
    _, out = BL.run(cmd, a.timeout, env={"AASR_RECIPE_TIMING": "1"})
    m = TIMING.search(out.stderr)
    e = re.search(r"Weighted entries: (\d+) over (\d+) frames", out.stderr)
    entries, frames = (int(e.group(1)), int(e.group(2))) if e else (0, 0)
    gmm = capi.Gmm.from_files(model + ".gk", model + ".mc", model + ".ph")
    run = capi.run_lda_networks_recipe(cfg_text, gmm, capi.Topology(model + ".ph"), rec, module, dim,
                                       opts=capi.LdaOptions.defaults(mingamma=1.0))
    gmm.close()
    frames = frames or int(run["frames"])
    per = 1e6 / frames
    res.update(frames=frames, weighted_entries=entries, entries_per_frame=round(entries / frames, 3),
               states_with_entries=int((run["state_gamma"] > 0).sum()), wall_s=walls,
               wall_s_per_1e6_frames=round(min(walls) * per, 2) if walls else None,
               device_ms_per_1e6_frames={"features_both_stagings": round(run["seconds_features"] * 1e3 * per, 3),
                                         "scatter": round(run["seconds_scatter"] * 1e3 * per, 3)},
               in_process_wall_s=round(run["seconds_total"], 2))
    # a group holds at most 2^27 scores (network_pass.h): its states' runs are cut into items of 256 entries
    groups = -(-frames * S // (1 << 27))
    res["groups_about"] = groups
    res["entries_per_state_and_group_about"] = round(entries / max(1, groups * res["states_with_entries"]), 1)
    if m:
        res["stage_s_per_1e6_frames"] = dict(zip(("input_and_networks", "features_both_stagings", "scoring",
                                                  "forward_backward_and_entries", "accumulation"),
                                                 (round(float(x) * per, 3) for x in m.groups())))
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        pcmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + cmd
        wall, _ = BL.run(pcmd, a.timeout)
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = scatter_kernels(stats[0])
        res["prof"] = {"wall_s_under_profiler": round(wall, 2),
                       "ms_per_1e6_frames": {k: round(v / 1e6 * per, 3) for k, v in fam.items()},
                       "scatter_launches": calls}
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""logl -H throughput: the native logl tool (features, state scoring and the forward-backward pass over HMM networks
on the device, aasr_run_logl_recipe) against oracle/_ref/logl_refmain, the reference's logl.cc with its own
HmmNetBaumWelch.cc on the adapter classes, on the same files.

    python tools/bench_logl.py [--utts 200] [--seconds 2.4] [--runs 3] [--ref-utts N] [--out FILE]

Data: tools/bench_align.py's model (D = 39, 50 000 Gaussians, 3 125 states x 16 components) and speech-like audio of
about --seconds each (about 300 frames); two recipes over it: `chain`, per utterance a left-to-right network of 100
random states, and `fan`, one network for all utterances whose initial node fans out into 250 chains of ten states
(5 000 emitting arcs) that merge again.  Default beams.

Measured: --runs alternating wall-time runs of both programs per recipe (model text parse included in both; with
--ref-utts N the binary runs the first N utterances and its time is also given scaled by utterances), and from one
further run of `logl` with AASR_RECIPE_TIMING=1 the seconds its calling thread spent on input and networks, features,
scoring and forward-backward (each stage waited for, so the stages do not overlap in that run).
Every run has its own time limit.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import hmmnet_cases as HC  # noqa: E402

LOGL = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "logl")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "logl_refmain")
S = 3125


def write_recipes(d, lines, ref_utts):
    rng = np.random.default_rng(11)
    fan = os.path.join(d, "fan.hmmnet")
    open(fan, "w").write(HC.fan(S, 250, 10, seed=12))
    out = {}
    for tag in ("chain", "fan"):
        rows = []
        for wav, _, i in lines:
            net = fan
            if tag == "chain":
                net = os.path.join(d, "chain%04d.hmmnet" % i)
                open(net, "w").write(HC.chain([int(s) for s in rng.integers(0, S, 100)]))
            rows.append("audio=%s hmmnet=%s\n" % (wav, net))
        full, part = os.path.join(d, tag + ".recipe"), os.path.join(d, tag + "_ref.recipe")
        open(full, "w").write("".join(rows))
        open(part, "w").write("".join(rows[:ref_utts]))
        out[tag] = (full, part)
    return out


def run(cmd, timeout, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    wall = time.time() - t
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (cmd[0], r.returncode, r.stderr[-2000:]))
    return wall, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=2.4)
    ap.add_argument("--ref-utts", type=int, default=0, help="utterances that logl_refmain runs (0: all)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.ref_utts = min(a.ref_utts, a.utts) if a.ref_utts > 0 else a.utts
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_logl_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.seconds - 0.2, a.seconds + 0.2)
    recipes = write_recipes(d, lines, a.ref_utts)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1), "frames": samples // 128,
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16",
           "networks": {"chain": "100 states, 200 emitting arcs, one per utterance", "fan": "250 x 10 states, 5000 emitting arcs"}}
    have_ref = os.access(REFMAIN, os.X_OK)
    for tag, (full, part) in recipes.items():
        def cmd(exe, recipe):
            return [exe, "-b", base, "-c", BA.CFG, "-r", recipe, "-H"]
        order = [("logl", cmd(LOGL, full))] + ([("logl_refmain", cmd(REFMAIN, part))] if have_ref else [])
        walls = {k: [] for k, _ in order}
        totals = {}
        for r in range(a.runs):
            for k, c in (order if r % 2 == 0 else order[::-1]):
                wall, out = run(c, a.timeout)
                walls[k].append(round(wall, 2))
                totals[k] = float(out.stdout.strip().splitlines()[-1].split(":")[-1])
                print("%s run %d %s: %.2f s, total %.3f" % (tag, r, k, wall, totals[k]), file=sys.stderr, flush=True)
        entry = {"wall_s": walls, "total_log_likelihood": totals}
        if have_ref and a.ref_utts < a.utts:
            entry["refmain_utterances"] = a.ref_utts
            entry["refmain_wall_s_scaled_to_the_recipe"] = round(min(walls["logl_refmain"]) * a.utts / a.ref_utts, 1)
        _, out = run(cmd(LOGL, full), a.timeout, env={"AASR_RECIPE_TIMING": "1"})
        m = re.search(r"logl timing: input and networks ([\d.]+) s, features ([\d.]+) s, scoring ([\d.]+) s, "
                      r"forward-backward ([\d.]+) s", out.stderr)
        if m:
            entry["stage_seconds"] = dict(zip(("input_and_networks", "features", "scoring", "forward_backward"),
                                              (float(x) for x in m.groups())))
        res[tag] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Forced alignment throughput: the native align tool (features, scoring and the Viterbi search on the
device, aasr_run_align_recipe) against the reference's own aligner linked on the engine
(oracle/_ref/align_refmain: aku/align.cc + Viterbi.cc + Lattice.cc + PhnReader.cc, per-frame
state_likelihood calls, a sequential search on one CPU core), on one synthetic recipe.

    python tools/bench_align.py [--utts 200] [--min-s 5] [--max-s 20] [--runs 3] [--prof DIR] [--out FILE]

Data: --utts utterances of --min-s .. --max-s seconds cut from a speech-like synthetic signal, a
BASELINE-shaped model (D = 39, 50 000 Gaussians, 3 125 states x 16 components, 625 five-state HMMs) whose
means are drawn from the signal's own feature frames (likelihoods stay inside the float range the
search stores them in), random transcripts of one HMM per ~15 frames, align's default beams.

Measured:
* --prof DIR: one run of the native align under `rocprofv3 --kernel-trace --stats`; per kernel family
  the device time per 10^6 aligned frames (the Viterbi window steps, the scoring, the feature chain);
* --runs alternating wall-time runs of align and align_refmain on the same recipe (model text parse
  included in both), and whether the two wrote the same .phn files.
Every run has its own time limit.  One JSON line on stdout (and in --out)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aaltoasr_amd import synth  # noqa: E402
from oracle import oracle  # noqa: E402

ALIGN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "align")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "align_refmain")
CFG = os.path.join(ROOT, "tests", "golden", "mfcc_cms_norm.feaconf")
PER = 5


def make_data(d, n_utts, min_s, max_s, seed=7):
    rng = np.random.default_rng(seed)
    cfg_text = open(CFG).read()
    base_pcm = synth.make_speechlike_audio(16000 * int(max_s + 1), seed=seed)
    fea = oracle.FeatureChain(cfg_text).generate(base_pcm, 0, 2000)
    S, G = 3125, 50000
    mean, var, off, idx, w = synth.make_model(D=39, G=G, S=S, comps=16, seed=seed + 1)
    mean[:] = fea[rng.integers(0, fea.shape[0], G)] + 0.3 * rng.standard_normal((G, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    base = os.path.join(d, "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    oracle.write_ph(base + ".ph", S, states_per_hmm=PER)
    n_hmm = S // PER
    lines, samples = [], 0
    for i in range(n_utts):
        n = int(16000 * rng.uniform(min_s, max_s))
        pcm = np.roll(base_pcm, int(rng.integers(0, len(base_pcm))))[:n]
        wav = os.path.join(d, "u%04d.wav" % i)
        with wave.open(wav, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(pcm.astype("<i2").tobytes())
        tr = os.path.join(d, "u%04d.phn" % i)
        k = max(1, (n // 128) // (3 * PER))
        open(tr, "w").write("".join("h%d\n" % h for h in rng.integers(0, n_hmm, k)))
        lines.append((wav, tr, i))
        samples += n
    return base, lines, samples


def write_recipe(d, lines, tag):
    p = os.path.join(d, tag + ".recipe")
    with open(p, "w") as f:
        for wav, tr, i in lines:
            f.write("audio=%s transcript=%s alignment=%s\n" % (wav, tr, os.path.join(d, "%s_%04d.out" % (tag, i))))
    return p


def run(cmd, timeout, log, cwd=None):
    """the tool's stderr (-i 1: a line per utterance) goes to the progress log as it is written"""
    with open(log, "a") as f:
        f.write("$ %s\n" % " ".join(cmd))
        f.flush()
        t = time.time()
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=f, timeout=timeout, cwd=cwd)
        wall = time.time() - t
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d), see %s" % (cmd[0], r.returncode, log))
    return wall


def aligned_frames(d, lines, tag):
    """frames the .phn files cover: the last line ends at (frames + 1) x 128 samples"""
    total, files = 0, {}
    for _wav, _tr, i in lines:
        p = os.path.join(d, "%s_%04d.out" % (tag, i))
        b = open(p, "rb").read() if os.path.exists(p) else b""
        files[i] = b
        rows = b.decode().splitlines()
        if rows:
            total += int(rows[-1].split()[1]) // 128 - 1
    return total, files


def kernel_families(stats_csv):
    fam = {"viterbi": 0.0, "scoring": 0.0, "features": 0.0, "other": 0.0}
    calls = {"viterbi": 0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_align_viterbi" in name:
            fam["viterbi"] += ns
            calls["viterbi"] += int(r["Calls"])
        elif "gmm" in name or "score" in name or "frame_operand" in name:
            fam["scoring"] += ns
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
    ap.add_argument("--timeout", type=int, default=900, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of align")
    ap.add_argument("--no-ref", action="store_true", help="time the native tool only")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--log", default="", help="progress log (the tools' -i 1 lines); default: in the work directory")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_align_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = make_data(d, a.utts, a.min_s, a.max_s)
    res = {"utterances": a.utts, "audio_seconds": round(samples / 16000.0, 1),
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5",
           "beams": "align defaults (swins 1000, beam 100, sbeam 100, maxbeam 1600)"}
    print("data: %d utterances, %.0f s of audio, made in %.1f s" % (a.utts, samples / 16000.0, res["data_seconds"]),
          file=sys.stderr, flush=True)
    log = a.log or os.path.join(d, "progress.log")
    common = ["-b", base, "-c", CFG, "-i", "1"]
    tools = [("native", ALIGN)] + ([] if a.no_ref else [("refmain", REFMAIN)])
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        rec = write_recipe(d, lines, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof),
               "--", ALIGN] + common + ["-r", rec]
        wall = run(cmd, a.timeout, log, cwd=tempfile.gettempdir())
        frames, _ = aligned_frames(d, lines, "prof")
        stats = [f for f in glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)]
        fam, calls = kernel_families(stats[0])
        res["prof"] = {"frames": frames, "wall_s_under_profiler": round(wall, 2), "viterbi_launches": calls["viterbi"],
                       "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 2) for k, v in fam.items()},
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    walls = {k: [] for k, _ in tools}
    outputs = {}
    for r in range(a.runs):
        for tag, exe in (tools if r % 2 == 0 else tools[::-1]):
            rec = write_recipe(d, lines, tag)
            wall = run([exe] + common + ["-r", rec], a.timeout, log)
            walls[tag].append(round(wall, 2))
            frames, files = aligned_frames(d, lines, tag)
            outputs[tag] = (frames, files)
            print("run %d %s: %.2f s, %d frames" % (r, tag, wall, frames), file=sys.stderr, flush=True)
    frames = outputs["native"][0]
    res["frames"] = frames
    res["wall_s"] = walls
    res["frames_per_s"] = {k: round(frames / min(v), 1) for k, v in walls.items()}
    if "refmain" in outputs:
        same = sum(outputs["native"][1][i] == outputs["refmain"][1][i] for _w, _t, i in lines)
        res["same_phn_files"] = "%d/%d" % (same, len(lines))
        res["speedup_min_wall"] = round(min(walls["refmain"]) / min(walls["native"]), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

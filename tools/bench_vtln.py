"""VTLN estimation throughput: the native vtln tool (features of every grid point and the log-likelihood of the
segmentations on the device, aasr_run_vtln_recipe) against oracle/_ref/vtln_refmain, the reference's main() on the
adapter classes (a frame at a time through FeatureGenerator::generate and HmmSet::pdf_likelihood), on the same files.

    python tools/bench_vtln.py [--utts 200] [--speakers 10] [--grid 21] [--ref-utts N] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_align.py's recipe (speech-like audio, D = 39, 50 000 Gaussians, 3 125 states x 16 components, 625
five-state HMMs) with tests/golden/mfcc_cms_norm.feaconf and a vtln module between its fft and mel modules; random state
segmentations (whole HMMs, 1-6 frames per state) as tools/bench_stats.py writes them; the utterances dealt to
--speakers speakers in runs, as a recipe sorted by speaker has them.

Measured:
* --runs alternating wall-time runs of `vtln` and of `vtln_refmain` over the recipe (model text parse included in
  both).  With --ref-utts N the binary runs the first N utterances only; its wall time is then reported as measured
  and scaled to the whole recipe by frames, and the result says so.  Without the binary only `vtln` runs;
* --prof DIR: one run of vtln under `rocprofv3 --kernel-trace --stats`; device ms per 10^6 frame evaluations
  (frames x grid points) of the feature chain and of k_segll_*, and k_segll_*'s achieved bandwidth against the bytes
  bound of reading every row once (8 x 39 bytes per frame evaluation at the HBM peak).
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
import bench_stats as BS  # noqa: E402

VTLN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin", "vtln")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "vtln_refmain")
HBM_TBPS = 8.0   # MI355X HBM3E peak


def write_config(d):
    """the benchmark chain with a vtln module on the spectrum"""
    text = open(BA.CFG).read()
    mel = text.index("name mel")
    head, tail = text[:mel], text[mel:]
    tail = tail.replace("sources fft", "sources vtln", 1)
    cut = head.rindex("module")
    text = head[:cut] + "module\n{\n  name vtln\n  type vtln\n  sources fft\n}\n\n" + head[cut:] + tail
    p = os.path.join(d, "vtln.feaconf")
    open(p, "w").write(text)
    return p


def write_recipes(d, srec, n_speakers, ref_utts):
    """bench_stats' recipe with speaker ids (runs of utterances per speaker); the whole one and its first ref_utts lines"""
    lines = open(srec).read().splitlines()
    per = -(-len(lines) // n_speakers)
    out = ["%s speaker=spk%02d" % (l.replace("alignment=", "transcript="), i // per) for i, l in enumerate(lines)]
    full, part = os.path.join(d, "vtln.recipe"), os.path.join(d, "vtln_ref.recipe")
    open(full, "w").write("\n".join(out) + "\n")
    open(part, "w").write("\n".join(out[:ref_utts]) + "\n")
    return full, part, lines


def recipe_frames(lines):
    """the frames of a recipe's segmentations: the last end time of each .phn file"""
    total = 0
    for l in lines:
        seg = [f for f in l.split() if f.startswith(("alignment=", "transcript="))][0].split("=", 1)[1]
        total += int(open(seg).read().split("\n")[-2].split()[1]) // 128
    return total


def kernel_families(stats_csv):
    fam = {"segll": 0.0, "features": 0.0, "other": 0.0}
    calls = {"segll": 0}
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "k_segll_" in name:
            fam["segll"] += ns
            calls["segll"] += int(r["Calls"])
        elif "aasr::k_" in name and "k_gmm_" not in name:   # the chain's kernels; the model's build probes are no part of it
            fam["features"] += ns
        else:
            fam["other"] += ns
    return fam, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--speakers", type=int, default=10)
    ap.add_argument("--grid", type=int, default=21)
    ap.add_argument("--ref-utts", type=int, default=0, help="utterances of the recipe that vtln_refmain runs (0: all)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of vtln")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.ref_utts = min(a.ref_utts, a.utts) if a.ref_utts > 0 else a.utts
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_vtln_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    cfg = write_config(d)
    full, part, rlines = write_recipes(d, BS.write_segmentations(d, lines), a.speakers, min(a.ref_utts, a.utts))
    spkc = os.path.join(d, "in.spkc")
    open(spkc, "w").write("speaker default\n{\n  feature vtln\n  {\n  }\n}\n")
    frames, ref_frames = recipe_frames(rlines), recipe_frames(rlines[:min(a.ref_utts, a.utts)])
    res = {"utterances": a.utts, "speakers": a.speakers, "grid": a.grid, "audio_seconds": round(samples / 16000.0, 1),
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5",
           "frames": frames, "frame_evaluations": frames * a.grid}
    log = os.path.join(d, "progress.log")

    def cmd(exe, recipe, tag):
        return [exe, "-b", base, "-c", cfg, "-r", recipe, "-v", "vtln", "-S", spkc, "-i", "1", "--grid-size", str(a.grid),
                "-o", os.path.join(d, tag + ".spkc"), "-s", os.path.join(d, tag + ".sum")]

    have_ref = os.access(REFMAIN, os.X_OK)
    order = [("vtln", cmd(VTLN, full, "native"))] + ([("vtln_refmain", cmd(REFMAIN, part, "ref"))] if have_ref else [])
    walls = {tag: [] for tag, _ in order}
    for r in range(a.runs):
        for tag, c in (order if r % 2 == 0 else order[::-1]):
            wall = BA.run(c, a.timeout, log)
            walls[tag].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, tag, wall), file=sys.stderr, flush=True)
    res["wall_s"] = walls
    res["frame_evaluations_per_s"] = {"vtln": round(frames * a.grid / min(walls["vtln"]), 1)}
    if have_ref:
        res["refmain_utterances"], res["refmain_frames"] = min(a.ref_utts, a.utts), ref_frames
        res["frame_evaluations_per_s"]["vtln_refmain"] = round(ref_frames * a.grid / min(walls["vtln_refmain"]), 1)
        if ref_frames < frames:   # (a scaling by frames also scales the binary's start-up: an upper bound)
            res["refmain_wall_s_scaled_to_the_recipe"] = round(min(walls["vtln_refmain"]) * frames / ref_frames, 1)
            res["note"] = "vtln_refmain ran the first %d utterances only; its wall time is scaled by frames" % a.ref_utts
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        c = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + \
            cmd(VTLN, full, "prof")
        wall = BA.run(c, a.timeout, log, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam, calls = kernel_families(stats[0])
        evals = frames * a.grid
        seg_s = fam["segll"] / 1e9
        res["prof"] = {"wall_s_under_profiler": round(wall, 2), "segll_launches": calls["segll"],
                       "ms_per_1e6_frame_evaluations": {k: round(v / 1e6 / evals * 1e6, 3) for k, v in fam.items()},
                       "segll_bytes_per_frame_evaluation": 39 * 8,
                       "segll_GBps": round(evals * 39 * 8 / seg_s / 1e9, 1) if seg_s > 0 else None,
                       "roofline_ms_per_1e6_frame_evaluations": round(1e6 * 39 * 8 / (HBM_TBPS * 1e12) * 1e3, 4),
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

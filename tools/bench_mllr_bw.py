"""mllr --networks throughput: CMLLR statistics from Baum-Welch posteriors over HMM networks (features under the
speaker's configuration, state scoring, the forward-backward pass, the frame-major entries and the weighted pass 1 on
the device, then the matrix-pipe passes and one host solve per speaker; aasr_run_mllr_networks_recipe) next to the same
tool over .phn files of the same audio.

    python tools/bench_mllr_bw.py [--utts 200] [--speakers 20] [--runs 3] [--prof DIR] [--out FILE]

Data: tools/bench_mllr.py's recipe -- tools/bench_align.py's model (D = 39, 50 000 Gaussians, 3 125 states x 16
components), speech-like audio of 5 to 20 s, speaker ids dealt to the utterances in blocks, a speaker file whose default
speaker lists the feature configuration's lin_transform module, random state segmentations read with -O for the .phn
run -- with the networks of tools/bench_logl.py: per utterance a left-to-right chain of 100 random states.  Default beams.

Measured: --runs alternating wall-time runs of `mllr -M --networks` and `mllr -M -O` (model text parse included in
both; with --other-mllr PATH also of another build's mllr binary, such as the parent commit's, on the .phn recipe), the
entries per frame and the largest |1 - s_t| that the network run reports at -i 1, its backward retries,
and with --prof a rocprofv3 --kernel-trace --stats run of its own of the network tool: device ms per 10^6 frames of the
forward-backward kernel, the frame-entry kernels, the weighted pass 1 (k_mllr_entry_pass1), pass 2 and the slab pass.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_align as BA  # noqa: E402
import bench_logl as BL  # noqa: E402
import bench_mllr as BM  # noqa: E402
import bench_stats as BS  # noqa: E402
import bench_stats_bw as BSB  # noqa: E402

FAMILIES = (("forward_backward", ("k_hmmnet_fb",)),
            ("frame_entries", ("k_fb_frame_sums", "k_fb_frame_counts", "k_fb_frame_scan", "k_fb_frame_fill")),
            ("pass1_entries", ("k_mllr_entry_pass1",)), ("pass2_rank", ("k_mllr_rank",)), ("slab_add", ("k_mllr_slab_add",)))


def kernel_families(stats_csv):
    fam = {k: 0.0 for k, _ in FAMILIES}
    fam["other"] = 0.0
    for r in csv.DictReader(open(stats_csv)):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        for k, names in FAMILIES:
            if any(n in name for n in names):
                fam[k] += ns
                break
        else:
            fam["other"] += ns
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--speakers", type=int, default=20)
    ap.add_argument("--min-s", type=float, default=5.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per tool run")
    ap.add_argument("--prof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of mllr --networks")
    ap.add_argument("--other-mllr", default="", help="another build's mllr binary, run on the .phn recipe in the same alternation")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="aasr_mllr_bw_")
    os.makedirs(d, exist_ok=True)
    t = time.time()
    base, lines, samples = BA.make_data(d, a.utts, a.min_s, a.max_s)
    per = -(-a.utts // a.speakers)

    def with_speakers(recipe, name):
        rows = open(recipe).read().splitlines()
        path = os.path.join(d, name)
        open(path, "w").write("".join("%s speaker=spk%03d\n" % (r, i // per) for i, r in enumerate(rows)))
        return path

    net_recipe = with_speakers(BL.write_recipes(d, lines, a.utts)["chain"][0], "mllr_net.recipe")
    phn_recipe = with_speakers(BS.write_segmentations(d, lines), "mllr_phn.recipe")
    module = BM.lin_transform_module(BA.CFG)
    spk = os.path.join(d, "in.spkc")
    open(spk, "w").write("speaker default\n{\n  feature %s\n  {\n  }\n}\n" % module)
    res = {"utterances": a.utts, "speakers": a.speakers, "audio_seconds": round(samples / 16000.0, 1),
           "data_seconds": round(time.time() - t, 1), "model": "D=39, G=50000, S=3125 x 16, 625 HMMs x 5",
           "networks": "100 states, 200 emitting arcs, one per utterance"}
    common = [BM.MLLR, "-b", base, "-c", BA.CFG, "-i", "1", "-S", spk, "-M", module]
    cmds = {"mllr_networks": common + ["-r", net_recipe, "--networks", "-o", os.path.join(d, "bw.spkc")],
            "mllr_phn": common + ["-r", phn_recipe, "-O", "-o", os.path.join(d, "ph.spkc")]}
    if a.other_mllr:
        cmds["mllr_phn_other_build"] = [a.other_mllr] + cmds["mllr_phn"][1:-1] + [os.path.join(d, "ph_other.spkc")]
    walls = {k: [] for k in cmds}
    for r in range(a.runs):
        order = list(cmds.items())
        for k, c in (order if r % 2 == 0 else order[::-1]):
            wall, out = BSB.run(c, a.timeout)
            walls[k].append(round(wall, 2))
            print("run %d %s: %.2f s" % (r, k, wall), file=sys.stderr, flush=True)
            if k == "mllr_networks":
                m = re.search(r"Weighted entries: (\d+) over (\d+) frames", out.stderr)
                res["entries"], res["frames"] = int(m.group(1)), int(m.group(2))
                res["max_abs_1_minus_frame_sum"] = float(re.search(r"of a frame: (\S+)", out.stderr).group(1))
                res["backward_retries"] = out.stderr.count("Warning: Backward phase failed")
                res["given_up_utterances"] = out.stderr.count("Could not run Baum-Welch for file")
    frames = max(1, res["frames"])
    res["entries_per_frame"] = round(res["entries"] / frames, 3)
    res["wall_s"] = walls
    res["wall_s_per_1e6_frames"] = {k: round(min(v) / frames * 1e6, 2) for k, v in walls.items()}
    if a.prof:
        os.makedirs(a.prof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(a.prof), "--"] + \
            cmds["mllr_networks"]
        wall, _ = BSB.run(cmd, a.timeout, cwd=tempfile.gettempdir())
        stats = glob.glob(os.path.join(a.prof, "**", "*kernel_stats.csv"), recursive=True)
        fam = kernel_families(stats[0])
        res["prof"] = {"wall_s_under_profiler": round(wall, 2),
                       "ms_per_1e6_frames": {k: round(v / 1e6 / frames * 1e6, 3) for k, v in fam.items()},
                       "kernel_ms": {k: round(v / 1e6, 3) for k, v in fam.items()},
                       "stats_csv": os.path.relpath(stats[0], a.prof)}
        print("prof: %s" % json.dumps(res["prof"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

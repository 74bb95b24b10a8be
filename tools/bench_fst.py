"""bench_fst.py -- side benchmark of the FST token pass (csrc/fst_search.hip); bench.py does not know it.

    python tools/bench_fst.py [--batches 1,16,256,1024] [--frames 500] [--words 300] [--write DIR]

Workload: a synthetic word loop -- a non-emitting hub, `words` words of three phones of three left-to-right states with
self-loops (9 * words + 1 nodes), every word's last state back to the hub with the word as symbol --, random 2-byte
acoustics over 120 models, utterances of about `frames` frames (+-10 %), the default beam (2600) and token limit (5000).
Reports per batch size the seconds of the search alone (aasr_fst_batch_dev + aasr_fst_batch_sync, the acoustics already on
the device), frames/s and utterances/s, the statuses, and one JSON line.  --write DIR also leaves net.fst, model.dur and
u0.lna there, the files a CPU run of the reference decoder needs for the same work (tools/make_fst_golden.py builds its
driver).  Then engine mode from audio (aasr_run_fst_decode_recipe, what fst_decode runs): recipes of --engine-batches
utterances of 4 s of synthetic 16 kHz audio (eight distinct files, repeated), the production feature chain, a model of 120
states x 8 Gaussians, groups of 256 utterances -- seconds from a group's first upload to its last result, and in all
(with reading the audio files)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = 120


def word_loop(words: int, rng) -> bytes:
    lines = [b"#FSTBasic MaxPlus", b"I 0", b"F 0"]
    node = 1
    for w in range(words):
        states = [int(s) for s in rng.integers(0, MODELS, 9)]
        first = node
        lines.append(b"T 0 %d %d , %.4f" % (first, states[0], -float(np.log(words))))
        for k in range(9):
            lines.append(b"T %d %d %d , -0.6931" % (node, node, states[k]))
            if k < 8:
                lines.append(b"T %d %d %d , -0.6931" % (node, node + 1, states[k + 1]))
            else:
                lines.append(b"T %d 0 -1 w%d -0.6931" % (node, w))
            node += 1
    return b"\n".join(lines) + b"\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,256,1024")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--cap-candidates", type=int, default=1 << 18)
    ap.add_argument("--write", default="")
    ap.add_argument("--engine-batches", default="16,256,1024")
    a = ap.parse_args()
    import torch
    from aaltoasr_amd import capi
    L = capi.lib()
    capi.check(L.aasr_set_device(0))
    rng = np.random.default_rng(7)
    work = a.write or tempfile.mkdtemp(prefix="bench_fst_")
    os.makedirs(work, exist_ok=True)
    fst_path = os.path.join(work, "net.fst")
    open(fst_path, "wb").write(word_loop(a.words, rng))
    open(os.path.join(work, "model.dur"), "w").write("4\n%d\n" % MODELS + "".join("%d %.4f %.4f\n" % (i, 2 + i % 7, 1 + (i % 5) / 4) for i in range(MODELS)))
    net = capi.FstNet(fst_path)
    dur = capi.FstDurations(os.path.join(work, "model.dur"))
    rows = []
    for n in [int(x) for x in a.batches.split(",")]:
        T = rng.integers(int(a.frames * 0.9), int(a.frames * 1.1) + 1, n).astype(np.int32)
        codes = rng.integers(0, 12000, (int(T.sum()), MODELS)).astype(">u2")
        if a.write and n == 1:
            open(os.path.join(work, "u0.lna"), "wb").write(struct.pack(">iB", MODELS, 2) + codes.tobytes())
        d_lna = torch.frombuffer(bytearray(codes.tobytes()), dtype=torch.uint8).cuda()
        row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
        opt = capi.FstOptions.defaults(cap_candidates=a.cap_candidates)
        b = C.c_void_p()
        capi.check(L.aasr_fst_batch_create(net.handle, dur.handle, C.byref(opt), n, T.ctypes.data, C.byref(b)))
        over = C.c_int32()
        times = []
        for _ in range(3 if n <= 16 else 2):      # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(L.aasr_fst_batch_dev(b, d_lna.data_ptr(), 2, MODELS, int(T.sum()), row0.ctypes.data, None))
            capi.check(L.aasr_fst_batch_sync(b, None, C.byref(over)))
            times.append(time.perf_counter() - t0)
        statuses = {}
        for u in range(n):
            st = C.c_int32()
            capi.check(L.aasr_fst_batch_result(b, u, C.byref(st), None, None, None, None, None, 0, None))
            statuses[capi.FST_STATUS_NAMES[st.value]] = statuses.get(capi.FST_STATUS_NAMES[st.value], 0) + 1
        sec = min(times[1:])
        rows.append({"utterances": n, "frames": int(T.sum()), "seconds": round(sec, 4), "frames_per_s": round(float(T.sum()) / sec, 1),
                     "utterances_per_s": round(n / sec, 2), "statuses": statuses,
                     "device_mib": round(L.aasr_fst_batch_device_bytes(b) / 2 ** 20, 1)})
        print("batch %5d: %8.4f s  %10.1f frames/s  %8.2f utterances/s  %s  %.0f MiB" % (
            n, sec, rows[-1]["frames_per_s"], rows[-1]["utterances_per_s"], statuses, rows[-1]["device_mib"]), flush=True)
        L.aasr_fst_batch_destroy(b)
        del d_lna
    engine = []
    if a.engine_batches:
        import wave
        from aaltoasr_amd import synth
        from oracle import oracle as O
        cfg_text = synth.make_feature_config()
        mean, var, off, idx, mw = synth.make_model(D=39, G=960, S=MODELS, comps=8, seed=5)
        base = os.path.join(work, "m")
        O.write_gk(base + ".gk", mean, var)
        O.write_mc(base + ".mc", off, idx, mw)
        O.write_ph(base + ".ph", MODELS, states_per_hmm=3)
        wavs = []
        for i in range(8):
            wavs.append(os.path.join(work, "a%d.wav" % i))
            with wave.open(wavs[-1], "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(synth.make_audio(64000, seed=100 + i).astype("<i2").tobytes())
        feat, gmm = capi.Feat(cfg_text), capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
        for n in [int(x) for x in a.engine_batches.split(",")]:
            rec = os.path.join(work, "e%d.recipe" % n)
            open(rec, "w").write("".join("audio=%s\n" % wavs[i % 8] for i in range(n)))
            opts = capi.FstDecodeOptions.defaults()
            opts.fst.cap_candidates = a.cap_candidates
            best = None
            for _ in range(2):      # the first run warms up
                st = capi.run_fst_decode_recipe(feat, gmm, net, rec, os.path.join(work, "e%d.out" % n), opts, dur=dur)
                best = st if best is None or st["seconds_device"] < best["seconds_device"] else best
            lines = open(os.path.join(work, "e%d.out" % n)).read().splitlines()
            engine.append({"utterances": n, "frames": int(best["frames"]), "seconds_device": round(best["seconds_device"], 4),
                           "seconds_total": round(best["seconds_total"], 4), "frames_per_s": round(best["frames"] / best["seconds_device"], 1),
                           "utterances_per_s": round(n / best["seconds_device"], 2),
                           "not_ok": sum(l.split()[-1] in capi.FST_STATUS_NAMES[1:] for l in lines)})
            print("engine %5d: %8.4f s upload to result (%8.4f s in all)  %10.1f frames/s  %8.2f utterances/s  not OK: %d" % (
                n, engine[-1]["seconds_device"], engine[-1]["seconds_total"], engine[-1]["frames_per_s"], engine[-1]["utterances_per_s"],
                engine[-1]["not_ok"]), flush=True)
    print(json.dumps({"bench": "fst_search", "engine": engine, "nodes": net.num_nodes, "arcs": net.num_arcs, "models": MODELS, "rows": rows}))


if __name__ == "__main__":
    main()

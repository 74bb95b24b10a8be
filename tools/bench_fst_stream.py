"""bench_fst_stream.py -- side benchmark of the FST decoder's streaming sessions (csrc/fst_stream.hip); bench.py does not
know it.

    python tools/bench_fst_stream.py [--sessions 1,16,256] [--frames 320] [--chunk 16] [--words 300] [--out FILE]

Workload: tools/bench_fst.py's word loop and settings (9 * words + 1 nodes, random 2-byte acoustics over 120 models, the
default beam and token limit, its duration model), S sessions of `frames` frames each, fed in chunks of `chunk` frames.
Per S, in one process:
  * the whole chunked run -- frames / chunk feeds queued back to back on one stream, no sync between them -- between two
    events on that stream, alternating with a plain aasr_fst_batch over the same frames (the unchanged batch search: the
    yardstick of what chunking costs), the order rotated from repetition to repetition; five repetitions after a warm-up
    of both, the median with min ... max;
  * the latency of one feed, queue to synced result (wall clock, aasr_fst_stream_feed_dev + aasr_fst_stream_sync), median
    and max over the feeds of one more run;
  * from the latency, how many streams a device serves in real time at 125 frames/s: a launch over S sessions has to be
    back before the next chunk has been spoken (chunk / 125 s), so S sessions are served while latency < chunk / 125 s,
    and S * (chunk / 125) / latency is the extrapolation (for S below the device's workgroup slots it is a lower bound).
Results are checked equal (status, log-probability bits, words) between the two paths before anything is reported.
Writes one JSON document to --out (default profiles/fst_stream_bench.json) and prints it as one line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_fst import MODELS, word_loop  # noqa: E402

FRAME_RATE = 125.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,16,256")
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--cap-candidates", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fst_stream_bench.json"))
    a = ap.parse_args()
    import torch
    from aaltoasr_amd import capi
    L = capi.lib()
    capi.check(L.aasr_set_device(0))
    rng = np.random.default_rng(7)
    work = tempfile.mkdtemp(prefix="bench_fst_stream_")
    fst_path = os.path.join(work, "net.fst")
    open(fst_path, "wb").write(word_loop(a.words, rng))
    open(os.path.join(work, "model.dur"), "w").write("4\n%d\n" % MODELS + "".join("%d %.4f %.4f\n" % (i, 2 + i % 7, 1 + (i % 5) / 4) for i in range(MODELS)))
    net = capi.FstNet(fst_path)
    dur = capi.FstDurations(os.path.join(work, "model.dur"))
    stream = torch.cuda.current_stream().cuda_stream
    T, chunk = a.frames, a.chunk
    rows = []
    for n in [int(x) for x in a.sessions.split(",")]:
        codes = rng.integers(0, 12000, (n * T, MODELS)).astype(">u2")
        d_lna = torch.frombuffer(bytearray(codes.tobytes()), dtype=torch.uint8).cuda()
        base = (np.arange(n, dtype=np.int64) * T)
        opt = capi.FstOptions.defaults(cap_candidates=a.cap_candidates)
        frames = np.full(n, T, np.int32)
        b = C.c_void_p()
        capi.check(L.aasr_fst_batch_create(net.handle, dur.handle, C.byref(opt), n, frames.ctypes.data, C.byref(b)))
        s = capi.FstStream(net, n, T, opt, dur=dur)
        feeds = [(base + t, np.full(n, min(chunk, T - t), np.int32)) for t in range(0, T, chunk)]

        def run_batch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(L.aasr_fst_batch_dev(b, d_lna.data_ptr(), 2, MODELS, n * T, base.ctypes.data, stream))
            e1.record()
            over = C.c_int32()
            capi.check(L.aasr_fst_batch_sync(b, stream, C.byref(over)))
            return e0.elapsed_time(e1) / 1e3

        def run_stream():
            s.reset(-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for row0, n_new in feeds:
                s.feed_dev(d_lna, 2, MODELS, row0, n_new, stream)
            e1.record()
            s.sync(stream)
            return e0.elapsed_time(e1) / 1e3

        run_batch()      # the warm-up of both, and the check that they agree
        run_stream()
        statuses = {}
        for u in range(n):
            st, lp, nw = C.c_int32(), C.c_float(), C.c_int32()
            words = np.zeros(T + 1, np.int32)
            capi.check(L.aasr_fst_batch_result(b, u, C.byref(st), C.byref(lp), None, None, C.byref(nw), words.ctypes.data, len(words), None))
            got = s.result(u, want_tokens=False)
            if (got["status"], np.float32(got["logprob"]).tobytes(), got["words"]) != (st.value, np.float32(lp.value).tobytes(), tuple(int(w) for w in words[:nw.value])):
                raise SystemExit("session %d of %d: the chunked search differs from the batch search" % (u, n))
            statuses[capi.FST_STATUS_NAMES[st.value]] = statuses.get(capi.FST_STATUS_NAMES[st.value], 0) + 1
        t_batch, t_stream = [], []
        for r in range(a.reps):      # alternating, the order rotated
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (t_batch if which == 0 else t_stream).append((run_batch, run_stream)[which]())
        s.reset(-1)      # one more run, synced feed by feed: the latency of a feed
        lat = []
        for row0, n_new in feeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.feed_dev(d_lna, 2, MODELS, row0, n_new, stream)
            s.sync(stream)
            lat.append(time.perf_counter() - t0)
        lat_full = [x for x, f in zip(lat, feeds) if int(f[1][0]) == chunk][1:]      # whole chunks, the starting feed apart
        med_b, med_s, med_l = statistics.median(t_batch), statistics.median(t_stream), statistics.median(lat_full)
        budget = chunk / FRAME_RATE
        rows.append({"sessions": n, "frames_each": T, "chunk": chunk, "feeds": len(feeds),
                     "batch_s": {"median": round(med_b, 5), "min": round(min(t_batch), 5), "max": round(max(t_batch), 5)},
                     "chunked_s": {"median": round(med_s, 5), "min": round(min(t_stream), 5), "max": round(max(t_stream), 5)},
                     "chunked_over_batch": round(med_s / med_b, 4),
                     "extra_ms_per_feed": round((med_s - med_b) / len(feeds) * 1e3, 4),
                     "feed_latency_ms": {"median": round(med_l * 1e3, 3), "max": round(max(lat_full) * 1e3, 3), "first": round(lat[0] * 1e3, 3)},
                     "real_time": bool(med_l < budget), "streams_in_real_time": int(n * budget / med_l),
                     "statuses": statuses, "device_mib": round(s.device_bytes / 2 ** 20, 1)})
        print("S %4d: batch %.4f s (%.4f ... %.4f)  chunked %.4f s (%.4f ... %.4f)  x%.3f  feed %.2f ms (max %.2f)  -> %d streams  %s" % (
            n, med_b, min(t_batch), max(t_batch), med_s, min(t_stream), max(t_stream), med_s / med_b, med_l * 1e3, max(lat_full) * 1e3,
            rows[-1]["streams_in_real_time"], statuses), flush=True)
        s.close()
        L.aasr_fst_batch_destroy(b)
        del d_lna
    doc = {"bench": "fst_stream", "nodes": net.num_nodes, "arcs": net.num_arcs, "models": MODELS, "frame_rate": FRAME_RATE,
           "reps": a.reps, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

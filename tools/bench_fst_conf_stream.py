"""bench_fst_conf_stream.py -- side benchmark of the confidence on streaming sessions (csrc/fst_conf_stream.hip); bench.py
does not know it.

    python tools/bench_fst_conf_stream.py [--sessions 1,16,256] [--frames 320] [--chunk 16] [--words 300] [--phones 40] [--out FILE]

Workload: tools/bench_fst_stream.py's (bench_fst.py's word loop, random 2-byte acoustics over 120 models, the default beam
and token limit, its duration model; S sessions of `frames` frames fed in chunks of `chunk`) plus bench_fst_conf.py's phone
loop of `phones` phones of three states with its token limit of 1 000.  Three arrangements do the same work:
  (a) stream    one aasr_fst_conf_stream: per feed one launch whose sibling workgroups run a session's grammar search, its
                phone-loop search and its best-acoustics carry
  (b) pieces    what there was before it: two aasr_fst_stream handles, grammar and phone loop, fed back to back on one
                stream, and the batch frame-best pass (aasr_fst_conf_batch_frame_best_dev) over each chunk
  (c) batch     aasr_fst_conf_batch over the whole utterances
Per S, in one process: the whole run of each -- every feed queued back to back, no sync between them -- between two events
on the stream, alternating repetitions, the order rotated from repetition to repetition, five after a warm-up of each, the
median with min ... max; and for (a) and (b) the latency of one feed, queue to synced result (wall clock), the median over
the whole chunks (the starting feed apart) of alternating synced runs.  The results of (a) and (c) are compared for
equality (every field of aasr_fst_conf_result, by its bytes) before anything is reported.
Writes one JSON document to --out (default profiles/fst_conf_stream_bench.json) and prints it as one line."""
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
import fst_conf_restate as CR  # noqa: E402

FRAME_RATE = 125.0


def spread(v, scale=1e3):
    return {"median": round(statistics.median(v) * scale, 4), "min": round(min(v) * scale, 4), "max": round(max(v) * scale, 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,16,256")
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--phone-token-limit", type=int, default=1000)
    ap.add_argument("--cap-candidates", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--latency-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fst_conf_stream_bench.json"))
    a = ap.parse_args()
    if a.frames % a.chunk:
        raise SystemExit("--frames must be a multiple of --chunk: the frame-best pass of (b) runs over whole chunks")
    import torch
    from aaltoasr_amd import capi
    L = capi.lib()
    capi.check(L.aasr_set_device(0))
    rng = np.random.default_rng(7)
    work = tempfile.mkdtemp(prefix="bench_fst_conf_stream_")
    open(os.path.join(work, "net.fst"), "wb").write(word_loop(a.words, rng))
    open(os.path.join(work, "ploop.fst"), "wb").write(CR.random_phone_loop(rng, MODELS, n_phones=a.phones, states=3))
    open(os.path.join(work, "model.dur"), "w").write("4\n%d\n" % MODELS + "".join("%d %.4f %.4f\n" % (i, 2 + i % 7, 1 + (i % 5) / 4) for i in range(MODELS)))
    net, pnet = capi.FstNet(os.path.join(work, "net.fst")), capi.FstNet(os.path.join(work, "ploop.fst"))
    dur = capi.FstDurations(os.path.join(work, "model.dur"))
    stream = torch.cuda.current_stream().cuda_stream
    T, chunk = a.frames, a.chunk
    rows = []
    for n in [int(x) for x in a.sessions.split(",")]:
        codes = rng.integers(0, 12000, (n * T, MODELS)).astype(">u2")
        d_lna = torch.frombuffer(bytearray(codes.tobytes()), dtype=torch.uint8).cuda()
        base = (np.arange(n, dtype=np.int64) * T)
        o = capi.FstConfOptions.defaults(phone_loop=1)
        o.grammar.cap_candidates = o.phone.cap_candidates = a.cap_candidates
        o.phone.token_limit = a.phone_token_limit
        s = capi.FstConfStream(net, pnet, n, T, o, dur=dur)
        resolved = s.options      # the pieces and the batch get the same capacities
        sg = capi.FstStream(net, n, T, resolved.grammar, dur=dur)
        sp = capi.FstStream(pnet, n, T, resolved.phone, dur=dur)
        fb, cb = C.c_void_p(), C.c_void_p()
        per_chunk, whole = np.full(n, chunk, np.int32), np.full(n, T, np.int32)
        capi.check(L.aasr_fst_conf_batch_create(net.handle, None, None, C.byref(capi.FstConfOptions.defaults()), n, per_chunk.ctypes.data, C.byref(fb)))
        capi.check(L.aasr_fst_conf_batch_create(net.handle, pnet.handle, dur.handle, C.byref(resolved), n, whole.ctypes.data, C.byref(cb)))
        feeds = [(base + t, per_chunk) for t in range(0, T, chunk)]

        def feed_stream(row0, n_new):
            s.feed_dev(d_lna, 2, MODELS, row0, n_new, stream)

        def feed_pieces(row0, n_new):
            sg.feed_dev(d_lna, 2, MODELS, row0, n_new, stream)
            sp.feed_dev(d_lna, 2, MODELS, row0, n_new, stream)
            capi.check(L.aasr_fst_conf_batch_frame_best_dev(fb, d_lna.data_ptr(), 2, MODELS, n * T, row0.ctypes.data, stream))

        def sync_stream():
            s.sync(stream)

        def sync_pieces():
            sg.sync(stream)
            sp.sync(stream)

        def timed(body, sync):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            body()
            e1.record()
            sync()
            return e0.elapsed_time(e1) / 1e3

        def run_stream():
            s.reset(-1)
            return timed(lambda: [feed_stream(*f) for f in feeds], sync_stream)

        def run_pieces():
            sg.reset(-1)
            sp.reset(-1)
            return timed(lambda: [feed_pieces(*f) for f in feeds], sync_pieces)

        def run_batch():
            over = C.c_int32()
            return timed(lambda: capi.check(L.aasr_fst_conf_batch_dev(cb, d_lna.data_ptr(), 2, MODELS, n * T, base.ctypes.data, stream)),
                         lambda: capi.check(L.aasr_fst_conf_batch_sync(cb, stream, C.byref(over))))

        runs = {"stream": run_stream, "pieces": run_pieces, "batch": run_batch}
        for fn in runs.values():      # the warm-up of each, and the check that (a) and (c) agree
            fn()
        statuses = {}
        for u in range(n):
            want, got = capi.FstConfResult(), capi.FstConfResult()
            capi.check(L.aasr_fst_conf_batch_result(cb, u, C.byref(want)))
            capi.check(L.aasr_fst_conf_stream_result(s._h, u, C.byref(got)))
            if bytes(want) != bytes(got) or s.search_result(u)["text"] != sg.result(u, want_tokens=False)["text"]:
                raise SystemExit("session %d of %d: the streamed confidence differs from the batch's" % (u, n))
            key = "%s/%s" % (capi.FST_STATUS_NAMES[want.grammar_status], capi.FST_STATUS_NAMES[want.phone_status])
            statuses[key] = statuses.get(key, 0) + 1
        total = {k: [] for k in runs}
        names = list(runs)
        for r in range(a.reps):      # alternating, the order rotated
            for k in names[r % 3:] + names[:r % 3]:
                total[k].append(runs[k]())
        lat = {"stream": [], "pieces": []}
        for r in range(a.latency_reps):      # synced feed by feed: the latency of a feed
            for k in (("stream", "pieces") if r % 2 == 0 else ("pieces", "stream")):
                (s.reset(-1) if k == "stream" else (sg.reset(-1), sp.reset(-1)))
                feed, sync = (feed_stream, sync_stream) if k == "stream" else (feed_pieces, sync_pieces)
                for i, f in enumerate(feeds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feed(*f)
                    sync()
                    if i > 0:      # (the starting feed clears the tables: apart)
                        lat[k].append(time.perf_counter() - t0)
        row = {"sessions": n, "frames_each": T, "chunk": chunk, "feeds": len(feeds), "statuses_grammar_phone": statuses,
               "stream_total_ms": spread(total["stream"]), "pieces_total_ms": spread(total["pieces"]), "batch_total_ms": spread(total["batch"]),
               "stream_feed_latency_ms": spread(lat["stream"]), "pieces_feed_latency_ms": spread(lat["pieces"]),
               "device_mib": round(s.device_bytes / 2 ** 20, 1)}
        row["stream_over_pieces_total"] = round(row["stream_total_ms"]["median"] / row["pieces_total_ms"]["median"], 4)
        row["stream_over_pieces_latency"] = round(row["stream_feed_latency_ms"]["median"] / row["pieces_feed_latency_ms"]["median"], 4)
        row["stream_over_batch_total"] = round(row["stream_total_ms"]["median"] / row["batch_total_ms"]["median"], 4)
        row["real_time"] = bool(row["stream_feed_latency_ms"]["median"] < chunk / FRAME_RATE * 1e3)
        rows.append(row)
        print("S %4d: (a) %.2f ms (%.2f ... %.2f)  (b) %.2f ms (%.2f ... %.2f)  (c) %.2f ms (%.2f ... %.2f)  a/b %.3f   feed (a) %.3f ms "
              "(%.3f ... %.3f)  (b) %.3f ms (%.3f ... %.3f)  a/b %.3f  %s" % (
                  n, *row["stream_total_ms"].values(), *row["pieces_total_ms"].values(), *row["batch_total_ms"].values(),
                  row["stream_over_pieces_total"], *row["stream_feed_latency_ms"].values(), *row["pieces_feed_latency_ms"].values(),
                  row["stream_over_pieces_latency"], statuses), flush=True)
        s.close()
        sg.close()
        sp.close()
        L.aasr_fst_conf_batch_destroy(fb)
        L.aasr_fst_conf_batch_destroy(cb)
        del d_lna
    doc = {"bench": "fst_conf_stream", "models": MODELS, "words": a.words, "phones": a.phones, "phone_token_limit": a.phone_token_limit,
           "frame_rate": FRAME_RATE, "reps": a.reps, "latency_reps": a.latency_reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

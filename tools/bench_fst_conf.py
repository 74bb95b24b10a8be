"""bench_fst_conf.py -- side benchmark of the FST decoder's confidence (csrc/fst_conf.hip); bench.py does not know it.

    python tools/bench_fst_conf.py [--batches 16,256] [--frames 500] [--words 300] [--phones 40] [--reps 5] [--out FILE]

Workload: bench_fst.py's synthetic word loop and batch (random 2-byte acoustics over 120 models, utterances of about
`frames` frames, the default beam and token limit) plus a phone loop of `phones` phones of three states, searched with
the default beam and a token limit of --phone-token-limit (1000: on random acoustics the beam cuts nothing, and 5000
tokens of a phone loop over 500 frames make more distinct phone sequences than the largest derived history table holds).
Per batch size, in one process, alternating repetitions (one of each per round, the order rotated from round to round,
the first round dropped as warm-up), each between two events on the stream:

    confidence    aasr_fst_conf_batch_dev: both searches, the frame-best pass with its sums, the two token-record launches
    two_searches  aasr_fst_batch_dev on the grammar, then on the phone loop: what the searches cost without the confidence
    frame_best    aasr_fst_conf_batch_frame_best_dev alone
    confidence_2  the same as `confidence` on a second confidence batch, allocated after the plain batches: what the
                  placement of the tables alone changes
    inner_searches  aasr_fst_batch_dev on the first confidence batch's own two inner batches: the same memory as
                  `confidence`, without the added launches

Reports the median and the spread (min ... max) of each in milliseconds, the frame-best pass's achieved bytes per second
(the LNA bytes it reads once / its median time) beside the HBM figure, and writes all of it as JSON to --out
(default profiles/fst_conf_bench.json)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fst import MODELS, word_loop  # noqa: E402
import fst_conf_restate as CR  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0      # float4 copy measured / specification


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--phone-token-limit", type=int, default=1000)
    ap.add_argument("--cap-candidates", type=int, default=1 << 18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fst_conf_bench.json"))
    a = ap.parse_args()
    import torch
    from aaltoasr_amd import capi
    L = capi.lib()
    capi.check(L.aasr_set_device(0))
    rng = np.random.default_rng(7)
    work = tempfile.mkdtemp(prefix="bench_fst_conf_")
    open(os.path.join(work, "net.fst"), "wb").write(word_loop(a.words, rng))
    open(os.path.join(work, "ploop.fst"), "wb").write(CR.random_phone_loop(rng, MODELS, n_phones=a.phones, states=3))
    open(os.path.join(work, "model.dur"), "w").write("4\n%d\n" % MODELS + "".join("%d %.4f %.4f\n" % (i, 2 + i % 7, 1 + (i % 5) / 4) for i in range(MODELS)))
    net, pnet = capi.FstNet(os.path.join(work, "net.fst")), capi.FstNet(os.path.join(work, "ploop.fst"))
    dur = capi.FstDurations(os.path.join(work, "model.dur"))
    rows = []
    for n in [int(x) for x in a.batches.split(",")]:
        T = rng.integers(int(a.frames * 0.9), int(a.frames * 1.1) + 1, n).astype(np.int32)
        frames = int(T.sum())
        codes = rng.integers(0, 12000, (frames, MODELS)).astype(">u2")
        d_lna = torch.frombuffer(bytearray(codes.tobytes()), dtype=torch.uint8).cuda()
        row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
        o = capi.FstConfOptions.defaults(phone_loop=1)
        o.grammar.cap_candidates = o.phone.cap_candidates = a.cap_candidates
        o.phone.token_limit = a.phone_token_limit
        cb, gb, pb, cb2 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(L.aasr_fst_conf_batch_create(net.handle, pnet.handle, dur.handle, C.byref(o), n, T.ctypes.data, C.byref(cb)))
        resolved = capi.FstConfOptions()
        L.aasr_fst_conf_batch_options(cb, C.byref(resolved))      # the plain batches get the same capacities
        capi.check(L.aasr_fst_batch_create(net.handle, dur.handle, C.byref(resolved.grammar), n, T.ctypes.data, C.byref(gb)))
        capi.check(L.aasr_fst_batch_create(pnet.handle, dur.handle, C.byref(resolved.phone), n, T.ctypes.data, C.byref(pb)))
        capi.check(L.aasr_fst_conf_batch_create(net.handle, pnet.handle, dur.handle, C.byref(resolved), n, T.ctypes.data, C.byref(cb2)))
        args = (d_lna.data_ptr(), 2, MODELS, frames, row0.ctypes.data, None)
        work_items = {"confidence": lambda: capi.check(L.aasr_fst_conf_batch_dev(cb, *args)),
                      "two_searches": lambda: (capi.check(L.aasr_fst_batch_dev(gb, *args)), capi.check(L.aasr_fst_batch_dev(pb, *args))),
                      "frame_best": lambda: capi.check(L.aasr_fst_conf_batch_frame_best_dev(cb, *args)),
                      "confidence_2": lambda: capi.check(L.aasr_fst_conf_batch_dev(cb2, *args)),
                      "inner_searches": lambda: (capi.check(L.aasr_fst_batch_dev(L.aasr_fst_conf_batch_grammar(cb), *args)),
                                                 capi.check(L.aasr_fst_batch_dev(L.aasr_fst_conf_batch_phone(cb), *args)))}
        ms = {k: [] for k in work_items}
        for rep in range(a.reps + 1):
            names = list(work_items)
            for k in names[rep % len(names):] + names[:rep % len(names)]:
                fn = work_items[k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep > 0:
                    ms[k].append(e0.elapsed_time(e1))
        over = C.c_int32()
        capi.check(L.aasr_fst_conf_batch_sync(cb, None, C.byref(over)))
        statuses = {}
        for u in range(n):
            r = capi.FstConfResult()
            capi.check(L.aasr_fst_conf_batch_result(cb, u, C.byref(r)))
            key = "%s/%s" % (capi.FST_STATUS_NAMES[r.grammar_status], capi.FST_STATUS_NAMES[r.phone_status])
            statuses[key] = statuses.get(key, 0) + 1
        row = {"utterances": n, "frames": frames, "statuses_grammar_phone": statuses, "lna_bytes": frames * MODELS * 2}
        for k, v in ms.items():
            row[k + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        row["confidence_minus_two_searches_ms"] = round(row["confidence_ms"]["median"] - row["two_searches_ms"]["median"], 4)
        row["confidence_minus_inner_searches_ms"] = round(row["confidence_ms"]["median"] - row["inner_searches_ms"]["median"], 4)
        row["frame_best_bytes_per_s"] = round(row["lna_bytes"] / (row["frame_best_ms"]["median"] * 1e-3), 1)
        rows.append(row)
        print("batch %5d (%d frames): confidence %.3f ms (%.3f ... %.3f)  two searches %.3f ms (%.3f ... %.3f)  frame best %.4f ms "
              "(%.4f ... %.4f) = %.1f GB/s  second confidence batch %.3f ms (%.3f ... %.3f)  inner searches %.3f ms (%.3f ... %.3f)  %s" % (
                  n, frames, *row["confidence_ms"].values(), *row["two_searches_ms"].values(), *row["frame_best_ms"].values(),
                  row["frame_best_bytes_per_s"] / 1e9, *row["confidence_2_ms"].values(), *row["inner_searches_ms"].values(), statuses), flush=True)
        L.aasr_fst_conf_batch_destroy(cb)
        L.aasr_fst_conf_batch_destroy(cb2)
        L.aasr_fst_batch_destroy(gb)
        L.aasr_fst_batch_destroy(pb)
        del d_lna
    result = {"bench": "fst_conf", "models": MODELS, "words": a.words, "phones": a.phones, "reps": a.reps, "phone_token_limit": a.phone_token_limit,
              "hbm_tb_per_s": {"measured_float4_copy": HBM_MEASURED_TBS, "spec": HBM_SPEC_TBS}, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

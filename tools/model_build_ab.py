"""model_build_ab.py -- digests of what the host-side model builder (csrc/gmm_*.cc) makes the device compute.

    AASR_LIBDIR=<dir with libaasr.so> python tools/model_build_ab.py            one line per case
    AASR_LIBDIR=<dir with libaasr.so> python tools/model_build_ab.py --time    host-side times, one JSON line

A fixed list of small models that together reach every build path: the paired and the independent track layouts,
outlier routing, engine parts (planner and pivot groups), the centred form, factor rows (full covariances, a mixed pool
read from .gk files, PCGMM / SCGMM pools: the shared Cholesky), CMLLR transforms walked over one handle (in place, rebuild,
dimension parts, f64), Gaussian clustering and the model cache.  Every case prints its name and the SHA-256 of the raw
output bytes, computed twice in the process (a case that does not repeat says so and prints both).  Run it once per
library, one process each, and compare the outputs line for line: a change to the builder that alters no packed byte
leaves every line as it was.

--time: wall time of Gmm.from_arrays on the BASELINE-sized model (50 000 Gaussians, 3 125 states, 39 dimensions) and
of one set_cmllr speaker change on it (global transform, in place).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aaltoasr_amd import capi, synth  # noqa: E402
from oracle import oracle  # noqa: E402

PRECS = (("f16x2", 4), ("bf16x3", 3), ("f32", 0), ("f64", 1))


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def emit(name, fn) -> None:
    """fn() -> (arrays, note).  Errors are results too: the same model must be refused with the same words."""
    res = []
    for _ in range(2):
        try:
            arrays, note = fn()
            res.append((sha(*arrays), note))
        except capi.AasrError as e:
            res.append(("error-%d" % e.code, e.msg))
    (h, note), (h2, _) = res
    print("%-52s %s%s  %s" % (name, h, "" if h == h2 else " NOT-REPEATED " + h2, note), flush=True)


def lna_codes(g, frames) -> np.ndarray:
    """2-byte LNA codes through the engine's own score layout (aasr_gmm_score_lna_dev)."""
    import torch
    F = frames.shape[0]
    d_f = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).cuda()
    d_scr = torch.empty(g.score_scratch_floats(F), dtype=torch.float32, device="cuda")
    d_by = torch.zeros((F, g.num_states * 2), dtype=torch.uint8, device="cuda")
    g.score_lna_dev(d_f, d_scr, d_by, True, 2)
    torch.cuda.synchronize()
    return d_by.cpu().numpy()


def layout_note(g) -> str:
    lay, parts = g.own_layout(), g.engine_parts()
    note = "layout=%d 2term=%d routing=%d/%d centred=%d" % (g.active_layout(), lay["two_term_rows"], lay["routing"],
                                                            lay["outlier_comps"], lay["all_centred"])
    if parts:
        note += " parts=" + ",".join("%d:%d:%d" % (p["arith"], p["states"], p["pivot_groups"]) for p in parts["parts"])
    return note


def everything(g, frames, per_gaussian=True):
    out = [g.score(frames), lna_codes(g, frames)]
    if per_gaussian:
        out.append(g.gauss_loglik(frames))
    return out, layout_note(g)


def diag_cases(tag, model, frames, precs=PRECS, per_gaussian=True):
    g = capi.Gmm.from_arrays(*model)
    for pname, prec in precs:
        def run():
            g.set_precision(prec)
            arrays, note = everything(g, frames, per_gaussian)
            if prec == 1:
                arrays.append(g.score_f64(frames.astype(np.float64)))
            return arrays, note
        emit("%s %s" % (tag, pname), run)
    g.close()


def transforms(n, D, seed, zero_diag=None):
    rng = np.random.default_rng(seed)
    W = np.empty((n, D, D + 1))
    for t in range(n):
        W[t][:, 1:] = np.eye(D) * rng.uniform(0.8, 1.2, D) + 0.05 * rng.standard_normal((D, D))
        W[t][:, 0] = 0.2 * rng.standard_normal(D)
    if zero_diag is not None:
        W[zero_diag][2, 1 + 2] = 0.0
    return W


def transform_walk(tag, model, frames, prec=None):
    """none -> global -> regression classes with unadapted Gaussians -> another global -> classes, one with a zero on
    its diagonal -> a global transform with a zero on the diagonal -> none, on ONE handle."""
    G, D = model[0].shape
    g = capi.Gmm.from_arrays(*model)
    if prec is not None:
        g.set_precision(prec)
    zeros = np.zeros(G, np.int32)
    classes = np.random.default_rng(5).integers(-1, 3, G).astype(np.int32)
    steps = (("none", None, None), ("global", zeros, transforms(1, D, 1)), ("classes", classes, transforms(3, D, 2)),
             ("global2", zeros, transforms(1, D, 3)), ("classes0", classes, transforms(3, D, 4, zero_diag=1)),
             ("global0", zeros, transforms(1, D, 6, zero_diag=0)), ("none2", None, None))
    for sname, g2t, W in steps:
        # the step is taken once, the scores twice
        try:
            g.set_cmllr(g2t, W) if W is not None else g.set_cmllr()
        except capi.AasrError as e:
            print("%-52s error-%d  %s" % ("%s %s" % (tag, sname), e.code, e.msg), flush=True)
            continue

        def run():
            if prec == 1:
                return [g.score(frames), g.score_f64(frames.astype(np.float64))], layout_note(g)
            arrays = [g.score(frames), lna_codes(g, frames)]
            if W is None:
                arrays.append(g.gauss_loglik(frames))   # (not built for adapted pools)
            return arrays, layout_note(g)
        emit("%s %s" % (tag, sname), run)
    g.close()


def spd(rng, d, scale=1.0):
    a = rng.standard_normal((d, d)) * 0.3
    return scale * (a @ a.T + 0.5 * np.eye(d))


def sym(rng, d, scale):
    a = rng.standard_normal((d, d))
    return scale * 0.5 * (a + a.T)


def pcgmm_entries(rng, d, K, G, n_diag):
    basis = np.array([spd(rng, d)] + [sym(rng, d, 0.5 / (K * np.sqrt(d))) for _ in range(K - 1)])
    entries = [("precision_subspace", 7, basis)]
    for _ in range(G):
        kk = int(rng.integers(1, K + 1))
        lam = np.concatenate([[rng.uniform(0.5, 2.0)], rng.uniform(-0.4, 0.4, kk - 1)])
        entries.append(("pcgmm", 7, rng.standard_normal(d) * 0.8, lam))
    for _ in range(n_diag):
        entries.insert(int(rng.integers(1, len(entries) + 1)), ("diag", rng.standard_normal(d), np.exp(rng.uniform(-1, 1, d))))
    return entries


def scgmm_entries(rng, d, K, G):
    thetas = []
    for b in range(K):
        P = spd(rng, d) if b == 0 else sym(rng, d, 0.5 / (K * np.sqrt(d)))
        thetas.append(np.concatenate([rng.standard_normal(d) * (0.5 if b == 0 else 0.1), oracle.map_m2v(P)]))
    entries = [("exponential_subspace", 3, np.array(thetas))]
    for _ in range(G):
        kk = int(rng.integers(1, K + 1))
        lam = np.concatenate([[rng.uniform(0.5, 2.0)], rng.uniform(-0.4, 0.4, kk - 1)])
        entries.append(("scgmm", 3, lam))
    return entries


def file_cases(tmp):
    """Pools read from .gk / .mc / .ph files: mixed full and diagonal, PCGMM, SCGMM; the model cache."""
    d, S = 13, 12
    frames = synth.make_frames(200, D=d, seed=77)

    def scored(base):
        g = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
        for pname, prec in PRECS[:3]:
            def run():
                g.set_precision(prec)
                return [g.score(frames), g.gauss_loglik(frames)], layout_note(g)
            emit("%s %s" % (os.path.basename(base), pname), run)
        return g

    rng = np.random.default_rng(61)
    G = 40
    mean = rng.standard_normal((G, d))
    cov = np.array([spd(rng, d, 2.0) for _ in range(G)])
    var = np.exp(rng.uniform(-1, 1, (G, d)))
    is_full = (np.arange(G) % 3 != 0)
    _, _, off, idx, w = synth.make_model(D=d, G=G, S=S, comps=6, seed=62, tied=True)
    base = os.path.join(tmp, "mixed_gk")
    oracle.write_gk_full(base + ".gk", mean, cov, is_full=is_full, var=var)
    oracle.write_mc(base + ".mc", off, idx, w)
    oracle.write_ph(base + ".ph", S)
    scored(base).close()
    for name, entries in (("pcgmm_gk", pcgmm_entries(np.random.default_rng(63), d, 6, 36, 4)),
                          ("scgmm_gk", scgmm_entries(np.random.default_rng(64), d, 5, 40))):
        Gs = sum(1 for e in entries if e[0] in ("pcgmm", "scgmm", "diag"))
        _, _, off, idx, w = synth.make_model(D=d, G=Gs, S=S, comps=6, seed=65, tied=True)
        base = os.path.join(tmp, name)
        oracle.write_gk_subspace(base + ".gk", d, entries)
        oracle.write_mc(base + ".mc", off, idx, w)
        oracle.write_ph(base + ".ph", S)
        scored(base).close()
    # the model cache: a diagonal model through files, the cache written, read back, scored
    model = synth.make_model(D=39, G=256, S=32, comps=8, seed=66)
    base = os.path.join(tmp, "cached")
    oracle.write_gk(base + ".gk", model[0], model[1])
    oracle.write_mc(base + ".mc", *model[2:])
    oracle.write_ph(base + ".ph", 32)
    fr = synth.make_frames(200, seed=67)
    g = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
    g.write_cache(base + ".cache")
    emit("model cache, file", lambda: ([open(base + ".cache", "rb").read()], "%d bytes" % os.path.getsize(base + ".cache")))
    emit("model cache, from files", lambda: everything(g, fr))
    g.close()
    g = capi.Gmm.from_cache(base + ".cache")
    emit("model cache, read back", lambda: everything(g, fr))
    g.close()


def cases() -> None:
    fr = synth.make_frames(300, seed=41)
    plain = synth.make_model(D=39, G=256, S=32, comps=8, seed=40)
    diag_cases("plain", plain, fr)
    diag_cases("plain tied", synth.make_model(D=39, G=256, S=32, comps=8, seed=42, tied=True), fr)
    mean, var, off, idx, w = plain
    off2 = off.copy()
    off2[6:] -= 8    # state 5 without components
    diag_cases("plain, empty state", (mean, var, off2, np.delete(idx, np.s_[40:48]), np.delete(w, np.s_[40:48])), fr)
    diag_cases("plain, partial tile", synth.make_model(D=39, G=37 * 8, S=37, comps=8, seed=43), fr)
    # independent tracks: ragged mixtures, four states over the two-term limits
    ragged = synth.push_states_over_the_f16_limits(synth.make_model(D=39, G=4000, S=150, comps_range=(1, 40), seed=430),
                                                   [3, 4, 77, 149])
    diag_cases("independent tracks", ragged, fr, PRECS[:3], per_gaussian=False)
    # outlier routing: HYB tables and centred records
    routed, _ = synth.sharpen_outliers(synth.make_model(D=39, G=64 * 8, S=64, comps=8, seed=44), [(3, 1), (10, 2), (40, 1)])
    diag_cases("outlier routing", routed, fr, PRECS[:3])
    # engine parts: most states over the limits of the one-pivot two-term rows
    S = 64
    parts = synth.push_states_over_the_f16_limits(synth.make_model(D=39, G=S * 8, S=S, comps=8, seed=470),
                                                  list(range(0, S, 2)) + [1])
    diag_cases("engine parts", parts, fr, PRECS[:3])
    # ill-conditioned: the centred form throughout, and its per-Gaussian view
    diag_cases("ill-conditioned", (mean, var * 1e-4, off, idx, w), fr, PRECS[2:])   # (no split-term rows for such a model)
    # full covariances, one of them not positive definite
    rng = np.random.default_rng(45)
    d, G = 13, 48
    fmean = rng.standard_normal((G, d))
    fcov = np.array([spd(rng, d, 2.0) for _ in range(G)])
    fcov[5] = -np.eye(d)
    _, _, foff, fidx, fw = synth.make_model(D=d, G=G, S=12, comps=6, seed=46, tied=True)
    ffr = synth.make_frames(200, D=d, seed=47)
    g = capi.Gmm.from_full(fmean, fcov, foff, fidx, fw)
    for pname, prec in PRECS[:3]:
        def run():
            g.set_precision(prec)
            return [g.score(ffr), g.gauss_loglik(ffr)], layout_note(g)
        emit("full covariance %s" % pname, run)
    g.close()
    with tempfile.TemporaryDirectory() as tmp:
        file_cases(tmp)
    # transforms on one handle
    transform_walk("walk plain", plain, fr)
    transform_walk("walk outlier-routed", routed, fr)
    transform_walk("walk engine parts", parts, fr)
    wide = synth.make_model(D=80, G=1200, S=100, comps=12, seed=31)
    transform_walk("walk D=80", wide, synth.make_frames(200, D=80, seed=9))
    transform_walk("walk plain f64", plain, fr, prec=1)
    # Gaussian clustering
    for tag, model in (("clustered plain", plain), ("clustered engine parts", parts)):
        g = capi.Gmm.from_arrays(*model)
        g2c = synth.make_clustering(model[0], 16)
        g.set_clustering(16, [(int(a), int(c)) for a, c in enumerate(g2c)])
        g.set_clustering_min_evals(0.25, 0.25)
        emit(tag, lambda: ([g.score(fr), lna_codes(g, fr)], layout_note(g)))
        g.close()


def times() -> None:
    model = synth.make_model(D=39, G=50000, S=3125, comps=16)
    warm = capi.Gmm.from_arrays(*synth.make_model())   # library load, device start-up
    warm.close()
    t0 = time.perf_counter()
    g = capi.Gmm.from_arrays(*model)
    build_s = time.perf_counter() - t0
    fr = synth.make_frames(256, seed=48)
    g.score(fr)
    zeros = np.zeros(50000, np.int32)
    change = []
    for seed in range(5):
        W = transforms(1, 39, 100 + seed)
        t0 = time.perf_counter()
        g.set_cmllr(zeros, W)
        change.append(time.perf_counter() - t0)
    note = layout_note(g)
    g.close()
    print(json.dumps({"libdir": os.environ.get("AASR_LIBDIR", "lib"), "from_arrays_s": round(build_s, 4),
                      "set_cmllr_ms": [round(1e3 * c, 4) for c in change], "layout": note}), flush=True)


if __name__ == "__main__":
    times() if "--time" in sys.argv else cases()

"""Writes tests/golden/oracle_vectors.npz: outputs of the CPU oracle on seeded
inputs for the parts of the path the reference holds no golden vectors for
(GMM scoring, clustering, CMLLR, LNA packing, full-precision features).  The
inputs are regenerated from the seeds by the tests; only the expected outputs
are stored.  Re-run after an intended oracle change:  python tools/make_golden.py

`python tools/make_golden.py --reference` writes tests/golden/reference_outputs.npz: what the
reference's own code compiled into oracle/_ref (KissFFT, util.hh's safe_log / str2float, the
recogniser's LNA reader) returns on the seeded inputs of tests/test_oracle_golden.py, so that those
oracle pins hold where oracle/_ref could not be built.  Needs oracle/_ref."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aaltoasr_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402


def vectors():
    O.build()
    out = {}
    # (1) config[0]-shaped model: D=39, G=256, S=32 x 8, 200 frames incl. far ones
    model = synth.make_model(D=39, G=256, S=32, comps=8)
    frames = synth.make_frames(200)
    frames[::25] *= 6.0                      # float-underflow / floor paths
    om = O.DiagModel(*model)
    ll, lik = om.score(frames.astype(np.float64), want_lik=True)
    out["cfg0_state_loglik"] = ll
    for nb in (2, 4):
        lp, by = O.lna_encode(lik, True, nb)
        out["cfg0_lna%d_lp" % nb] = lp
        out["cfg0_lna%d_bytes" % nb] = by
    out["cfg0_gauss_loglik_f1_4"] = om.gauss_loglik(frames[1:4].astype(np.float64))
    # (2) tied pool, ragged mixtures
    model = synth.make_model(D=39, G=2048, S=128, tied=True, comps_range=(1, 23))
    frames = synth.make_frames(120, seed=77)
    out["tied_state_loglik"] = O.DiagModel(*model).score(frames.astype(np.float64))
    # (3) clustering
    model = synth.make_model(D=39, G=2048, S=128, comps=16)
    g2c = synth.make_clustering(model[0], 64)
    om = O.DiagModel(*model)
    om.set_clustering(64, [(g, int(c)) for g, c in enumerate(g2c)], 0.0, 0.25)
    s, n = om.score_clustered(synth.make_frames(150, seed=78).astype(np.float64), want_counts=True)
    out["cluster_state_loglik"], out["cluster_exact_counts"] = s, n
    out["cluster_g2c"] = g2c
    # (4) full covariance
    rng = np.random.default_rng(synth.SEED + 5)
    D, G = 8, 64
    mean = rng.standard_normal((G, D))
    a = rng.standard_normal((G, D, D)) * 0.4
    cov = a @ a.transpose(0, 2, 1) + 0.1 * np.eye(D)
    _, _, off, idx, w = synth.make_model(D=D, G=G, S=8, comps=8)
    out["full_state_loglik"] = O.FullModel(mean, cov, off, idx, w).score(synth.make_frames(100, D=D, seed=79))
    # (5) features of the reference's own test audio at full precision
    pcm, _ = O.read_wav_pcm16(os.path.join(ROOT, "tests", "golden", "short.wav"))
    for name in ("mfcc_p_dd", "mfcc_cms_norm"):
        ch = O.FeatureChain(open(os.path.join(ROOT, "tests", "golden", name + ".feaconf")).read())
        out["fea_" + name] = ch.generate(pcm, -15, 106)
    return out


# ---- inputs of the reference pins in tests/test_oracle_golden.py (shared: the stored outputs belong to them)

FFT_SIZES = (8, 32, 128, 256, 512, 1024, 6, 18, 200, 320, 400, 480, 600, 750, 1000, 14, 56, 220, 364, 442, 552)
FFT_REPS = 20
SAFE_LOG_ARGS = (0.0, 1e-60, 1e-50, 9.99e-51, 1.0000001e-50, 1.0, 3.3e-7, 1e300)
STR2FLOAT_ARGS = ("0.97", "1e-3", "5.5112", "-6.36855e-05", "16777217", "0.1", "3.4e38")
LNA_READS = ((0, 1), (0, 8), (1, 8), (1, 57))      # (order, buffer size) of LnaReaderCircular


def fft_inputs():
    """(n, x) float32 in the order the pin draws them."""
    rng = np.random.default_rng(2)
    for n in FFT_SIZES:
        for _ in range(FFT_REPS):
            yield n, (rng.standard_normal(n) * 10 ** rng.uniform(-3, 4)).astype(np.float32)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def lna_pin_file(path, nbytes):
    """The LNA file the reader pin opens: the oracle's phone_probs restatement on seeded likelihoods.
    Returns (F, S, log-probs)."""
    rng = np.random.default_rng(11)
    F, S = 57, 43
    lik = np.exp(rng.uniform(-60, 3, (F, S)))
    lik[3, :] = 0.0                       # Z == 0 row
    lik[5, 7] = 1e-300                    # far below the 2-byte range
    lp, by = O.lna_encode(lik, True, nbytes)
    with open(path, "wb") as f:
        f.write(O.lna_header(S, nbytes))
        f.write(by.tobytes())
    return F, S, lp


def reference_vectors(tmpdir):
    O.build()
    K, A = O.ref_kissfft(), O.ref_aku()
    if K is None or A is None or O.ref_lna() is None:
        raise SystemExit("oracle/_ref is not built: the reference outputs cannot be recorded here")
    out = {}
    pf = C.POINTER(C.c_float)
    fft = []
    cfgs = {}
    for n, x in fft_inputs():
        cfg = cfgs.setdefault(n, K.kiss_fftr_alloc(n, 0, None, None))
        y = np.zeros((n // 2 + 1) * 2, np.float32)
        K.kiss_fftr(cfg, x.ctypes.data_as(pf), y.ctypes.data_as(pf))
        fft.append(digest(y))
    out["kissfft_sha256"] = np.array(fft).reshape(len(FFT_SIZES), FFT_REPS, 32)
    out["safe_log"] = np.array([A.ref_safe_log(x) for x in SAFE_LOG_ARGS], np.float64)
    ok = C.c_int()
    out["str2float"] = np.array([A.ref_str2float(s.encode(), C.byref(ok)) for s in STR2FLOAT_ARGS], np.float32)
    for nb in (2, 4):
        path = os.path.join(tmpdir, "x%d.lna" % nb)
        F, S, _ = lna_pin_file(path, nb)
        out["lna%d_file_sha256" % nb] = digest(np.frombuffer(open(path, "rb").read(), np.uint8))
        out["lna%d_reads" % nb] = np.array([O.ref_lna_read(path, F + 5, S, buf_size=b, order=o) for o, b in LNA_READS])
    return out


if __name__ == "__main__":
    if "--reference" in sys.argv:
        import tempfile
        path = os.path.join(ROOT, "tests", "golden", "reference_outputs.npz")
        with tempfile.TemporaryDirectory() as d:
            np.savez_compressed(path, **reference_vectors(d))
    else:
        path = os.path.join(ROOT, "tests", "golden", "oracle_vectors.npz")
        np.savez_compressed(path, **vectors())
    print("wrote", path, os.path.getsize(path), "bytes")

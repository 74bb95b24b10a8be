"""CMLLR estimation on the device: the statistics handle (csrc/mllr.cc, mllr_accum.hip) and the mllr tool.

Yardstick: tools/mllr_restate.py.  collect() is MllrTrainer::collect_data in double, frame by frame and Gaussian by
Gaussian in the reference's order; collect(extended=True) forms the same sums in np.longdouble in another order.

Tolerances of the accumulators, relative to the largest entry of the quantity: the restatement's own distance to the
extended sums, measured on the CPU on the inputs of every handle case of this module (same seeds) -- largest values
G 2.9e-14 and k 5.0e-14 (39 dimensions, 3 149 frames), beta 9.7e-15 (15 dimensions, 1 139 frames); at 39 dimensions with
16 components and 2 310 frames G 1.7e-14, k 6.2e-15, beta 8.1e-15 -- times a margin of 4 (at most 8 was allowed) for the
different grouping of the sums (the engine adds a frame's Gaussians first and the frames in chunks on the matrix pipe):
TOL below, which every case's restatement must meet against the extended sums, on the host.  The handle is held to the
case's own figure: within 4 x that case's restatement-to-extended distance (not below 4 roundings of a double, 8.9e-16) of
the restatement, and within twice that of the extended sums.
Closed loop, both modes: the written file read back through the speaker configuration must score strictly higher along
the segmentation, log |det A| included, than the input file (s1 in feature mode: the composed transform).
Speaker-file numbers may differ from the restatement's by one unit of the last printed digit; such flips are counted and
must stay below 1 % of the numbers.  The solver's tolerance: tests/test_mllr_host.py.

Kernel instances: d + 1 padded to 1, 2, 3 or 4 blocks of 16, i.e. dimensions 1-15, 16-31, 32-47, 48-63; 64 is refused.
A chunk is 1 024 frames."""
import importlib.util
import os
import re
import subprocess
import wave
from decimal import Decimal

import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
TOL = {"G": 4 * 2.9e-14, "k": 4 * 5.0e-14, "beta": 4 * 9.7e-15}
CHUNK = 1024
EPS = 2.0 ** -52


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MR = _load("mllr_restate")


def run_handle(capi, gmm, x, pdf, cuts=None, h=None):
    import torch
    own = h is None
    h = h or capi.Mllr(gmm)
    d_x = torch.tensor(x, device="cuda")
    cuts = cuts or [0, len(pdf)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            h.accumulate_dev(d_x[a:b], pdf[a:b])
    out = h.fetch()
    if own:
        h.close()
    return out


def errs(got, want):
    return {"G": MR.rel_err(got[0], want[0]), "k": MR.rel_err(got[1], want[1]),
            "beta": abs(float(got[2]) - float(want[2])) / max(float(want[2]), 1e-300)}


def check(capi, model, x, pdf, cuts_list=(None,)):
    want = MR.collect(model, x, pdf)
    ext = MR.collect(model, x, pdf, extended=True)
    e = errs(want, ext)
    print("restatement against extended sums", {q: "%.3g" % v for q, v in e.items()})
    assert all(e[q] <= TOL[q] for q in TOL), e                       # the two references, on the host
    # the handle's bound is the case's own: 4 x this case's distance, no less than 4 roundings of a double (sums of a
    # few terms, where the restatement can be exact and the other grouping is a rounding or two away)
    tol = {q: 4 * max(e[q], 4 * EPS) for q in TOL}
    gmm = capi.Gmm.from_arrays(*model)
    outs = []
    for cuts in cuts_list:
        got = run_handle(capi, gmm, x, pdf, cuts)
        e1, e2 = errs(got, want), errs(got, ext)
        print("cuts %s: handle against restatement %s, against extended %s" %
              (cuts, {q: "%.3g" % v for q, v in e1.items()}, {q: "%.3g" % v for q, v in e2.items()}))
        assert all(e1[q] <= tol[q] for q in TOL), ("restatement", e1, tol)
        assert all(e2[q] <= 2 * tol[q] for q in TOL), ("extended", e2, tol)
        assert (got[0] == got[0].transpose(0, 2, 1)).all()           # mirrored at fetch
        outs.append(got)
    gmm.close()
    return outs, want


@pytest.mark.parametrize("M", [16, 1])
def test_39_dimensions(capi, M):
    """several chunks in one call, then uneven cuts (other chunk boundaries), with skipped frames between"""
    rng = np.random.default_rng(100 + M)
    model, x, pdf = MR.make_case(rng, 39, [M, max(1, M // 2), M, 1], [900, 500, 700, 150], skipped=60)
    F = len(pdf)
    assert F > 2 * CHUNK and (pdf == -1).sum() == 60
    check(capi, model, x, pdf, [None, [0, 1, 7, CHUNK + 3, F // 2 + 5, F - 1, F]])


@pytest.mark.parametrize("D", [1, 15, 16, 31, 32, 47, 48, 63])
def test_dimension_instances(capi, D):
    """the narrowest and the widest dimension of every instance (15 | 16, 31 | 32, 47 | 48 are the boundaries)"""
    rng = np.random.default_rng(200 + D)
    model, x, pdf = MR.make_case(rng, D, [3, 1, 2], [500, 300, 330], skipped=9)
    check(capi, model, x, pdf, [None, [0, 2, len(pdf) // 3, len(pdf)]])


def test_dimension_64_is_refused(capi):
    rng = np.random.default_rng(3)
    gmm = capi.Gmm.from_arrays(*MR.FS.make_model(rng, 64, [2, 1]))
    with pytest.raises(capi.AasrError) as ei:
        capi.Mllr(gmm)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "64" in ei.value.msg
    gmm.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 77])
def test_frame_counts(capi, n):
    rng = np.random.default_rng(300 + n)
    a = n // 2
    model, x, pdf = MR.make_case(rng, 39, [4, 2], [n - a, a])
    assert len(pdf) == n
    check(capi, model, x, pdf)


def test_underflowing_frames_add_nothing_and_bad_variances(capi):
    """pdf 0: frames so far out that every likelihood is 0 -- no sum, nothing added; pdf 1: Gaussians with a zero and a
    negative variance (precision 0 in the likelihood, no weight in that dimension's sums: the stats handle's rule)"""
    rng = np.random.default_rng(41)
    model = MR.FS.make_model(rng, 39, [3, 2, 4])
    mean, var, off, idx, w = model
    x, pdf = MR.FS.make_frames(rng, model, [200, 300, 250], skipped=20)
    x[pdf == 0] += 60.0
    var[idx[off[1]], 5] = 0.0
    var[idx[off[1] + 1], 11] = -1.0
    post = MR.posteriors(model, x, pdf)
    assert all(post[f][1].sum() == 0 for f in np.nonzero(pdf == 0)[0])
    (got,), want = check(capi, model, x, pdf)
    only0 = pdf == 0
    gmm = capi.Gmm.from_arrays(*model)
    G, k, beta = run_handle(capi, gmm, np.ascontiguousarray(x[only0]), np.ascontiguousarray(pdf[only0]))
    gmm.close()
    assert beta == 0.0 and not G.any() and not k.any()
    assert np.isfinite(got[0]).all() and got[2] == pytest.approx(float((pdf > 0).sum()), rel=1e-12)


def test_reset_between_speakers_and_equal_bytes(capi):
    rng = np.random.default_rng(42)
    model, x, pdf = MR.make_case(rng, 39, [5, 3], [1500, 900], skipped=11)
    gmm = capi.Gmm.from_arrays(*model)
    a = run_handle(capi, gmm, x, pdf)
    b = run_handle(capi, gmm, x, pdf)
    for p, q in zip(a[:2], b[:2]):
        assert p.tobytes() == q.tobytes()                            # no atomics, fixed order
    assert a[2] == b[2]
    h = capi.Mllr(gmm)
    run_handle(capi, gmm, x[:700], pdf[:700], h=h)
    h.reset()
    c = run_handle(capi, gmm, x, pdf, h=h)                           # the second speaker starts from zero
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[2] == a[2]
    h.close()
    gmm.close()


def test_recovery_of_a_known_transform(capi):
    """frames drawn from the model, pushed through the inverse of a known affine map: the auxiliary function (from the
    extended statistics) at the engine's W is not below the identity's, and not below its value at the restatement's W by
    more than 1e-9 -- the CPU probe measured 9.1e-12 between the two solvers at |Q| = 1.3e4, times about 100."""
    rng = np.random.default_rng(43)
    D = 39
    model, x, pdf = MR.make_case(rng, D, [4, 4, 4, 2], [800, 700, 600, 200])
    A = np.eye(D) + 0.15 * rng.standard_normal((D, D)) / np.sqrt(D)
    y = np.ascontiguousarray((x - 0.3 * rng.standard_normal(D)) @ np.linalg.inv(A).T)
    gmm = capi.Gmm.from_arrays(*model)
    G, k, beta = run_handle(capi, gmm, y, pdf)
    gmm.close()
    W = capi.mllr_solve(G, k, beta)
    Ge, ke, be = MR.collect(model, y, pdf, extended=True)
    Wr = MR.solve(*MR.collect(model, y, pdf))
    q, qr, q0 = (MR.auxiliary(w, Ge, ke, be) for w in (W, Wr, np.eye(D, D + 1, 1)))
    print("Q engine %.12g restatement %.12g identity %.12g; W against restatement %.3g" % (q, qr, q0, MR.rel_err(W, Wr)))
    assert q >= q0 and q >= qr - 1e-9


# ---- the tool -------------------------------------------------------------------------------------------------------

N_HMM, PER, COMPS, SPF = 6, 3, 4, 128


def write_ph(path):
    with open(path, "w") as f:
        f.write("PHONE\n%d\n" % N_HMM)
        for h in range(N_HMM):
            f.write("%d 5 h%d\n-1 -2 %d %d %d\n0 1 2 1.0\n1 0\n" % (h + 1, h, 3 * h, 3 * h + 1, 3 * h + 2))
            f.write("2 2 2 0.5 3 0.5\n3 2 3 0.5 4 0.5\n4 2 4 0.5 1 0.5\n")


def write_wav(path, pcm):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.astype("<i2").tobytes())


def vec(v):
    return " ".join("%.6g" % t for t in np.asarray(v).ravel())


def varied_audio(n_samples, seed):
    """synth.make_audio's ingredients (white noise and three tones) with gains and tone frequencies redrawn every 100 ms.
    The stationary signal of synth.make_audio gives features that barely move around their mean: the second moments
    G_i are then close to singular, the estimate has entries of several hundred and its sixth digit depends on the last
    bits of the statistics -- no yardstick for a writer that prints six digits."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n_samples)
    seg = 1600
    for a in range(0, n_samples, seg):
        t = np.arange(a, min(n_samples, a + seg)) / 16000.0
        g_noise, g_tone = np.exp(rng.uniform(np.log(0.05), 0.0, 2))
        x[a:a + seg] = g_noise * 2000.0 * rng.standard_normal(len(t))
        for fj in rng.uniform(150.0, 3800.0, 3):
            x[a:a + seg] += g_tone * 6000.0 * np.sin(2 * np.pi * fj * t)
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def setup(capi, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("mllr")
    S, D = N_HMM * PER, 39
    cfg_text = synth.make_feature_config()
    open(str(d / "f.cfg"), "w").write(cfg_text)
    ft = capi.Feat(cfg_text)
    rng = np.random.default_rng(12)
    utts = []
    for u in range(6):
        pcm = varied_audio(16000 * 3 + 1500 * u, seed=200 + u)
        wav = str(d / ("u%d.wav" % u))
        write_wav(wav, pcm)
        utts.append(dict(wav=wav, pcm=pcm, eof=ft.eof_frame(len(pcm)), phn=str(d / ("u%d.phn" % u)), spk="s%d" % (u // 2)))
    fea = np.concatenate([ft.run(x["pcm"], 0, x["eof"], dtype=np.float64) for x in utts])
    G = COMPS * S
    mean, var, off, idx, w = synth.make_model(D=D, G=G, S=S, comps=COMPS, seed=24)
    # a model the data does not fit as it is: means around the frames of a shifted, scaled copy
    mean[:] = 1.2 * fea[rng.integers(0, len(fea), G)] + 0.4 + 0.3 * rng.standard_normal((G, D))
    var[:] = rng.uniform(0.5, 2.0, var.shape)
    base = str(d / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    write_ph(base + ".ph")
    lines = []
    for x in utts:   # state segmentations of our own making
        t, seg = 0, []
        while t < x["eof"] - 10:
            h = int(rng.integers(0, N_HMM))
            for k in range(3):
                n = int(rng.integers(1, 6))
                seg.append("%d %d h%d.%d\n" % (t * SPF, (t + n) * SPF, h, k))
                t += n
        open(x["phn"], "w").write("".join(seg))
        lines.append("audio=%s transcript=%s alignment=%s speaker=%s" % (x["wav"], x["phn"], x["phn"], x["spk"]))
    open(str(d / "r.rcp"), "w").write("\n".join(lines) + "\n")
    # input speaker files: feature mode -- s1 comes with a transform of its own (the composition), the others with none
    old_A = (np.eye(D) + 0.05 * rng.standard_normal((D, D))).astype(np.float32)
    old_b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    blocks = {"s1": "    matrix %s\n    bias %s\n" % (vec(old_A), vec(old_b))}
    text = "speaker default\n{\n  feature transform\n  {\n  }\n}\n"
    text += "speaker s1\n{\n  feature transform\n  {\n%s  }\n}\n" % blocks["s1"]
    open(str(d / "fea.spkc"), "w").write(text)
    open(str(d / "model.spkc"), "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    return dict(dir=d, cfg_text=cfg_text, base=base, model=(mean, var, off, idx, w), utts=utts, blocks=blocks,
                topo=capi.Topology(base + ".ph"), D=D)


def run_tool(st, spkc, out, *extra):
    cmd = [os.path.join(BIN, "mllr"), "-b", st["base"], "-c", str(st["dir"] / "f.cfg"), "-r", str(st["dir"] / "r.rcp"),
           "-S", str(st["dir"] / spkc), "-o", out, "-i", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def restate_speakers(capi, st, feature_mode):
    """per speaker W (and in feature mode the composed float A, b) from the engine's own f64 features"""
    out = {}
    for spk in ("s0", "s1", "s2"):
        ft = capi.Feat(st["cfg_text"])
        block = st["blocks"].get(spk, "") if feature_mode else None
        if feature_mode:
            ft.set_parameters("transform", "{\n%s}\n" % block)
        xs, ps = [], []
        for u in st["utts"]:
            if u["spk"] != spk:
                continue
            start, pdf, _ = capi.stats_read_segmentation(st["topo"], u["phn"], ft.frame_rate, 0, 0, u["eof"], False)
            xs.append(ft.run(u["pcm"], start, len(pdf), dtype=np.float64))
            ps.append(pdf)
        x, pdf = np.concatenate(xs), np.concatenate(ps)
        G, k, beta = MR.collect(st["model"], x, pdf)
        W = MR.solve(G, k, beta)
        We = MR.solve(*[np.asarray(a, np.float64) for a in MR.collect(st["model"], x, pdf, extended=True)])
        out[spk] = dict(W=W, We=We, beta=beta, x=x, pdf=pdf)
        if feature_mode and block:
            old = [np.array(l.split()[1:], np.float32) for l in block.strip().split("\n")]
            out[spk]["old"] = (old[0].reshape(st["D"], st["D"]), old[1])
    return out


def parse_spkc(text):
    """-> {speaker: {key: [tokens]}} of the one module block of every speaker"""
    out = {}
    for m in re.finditer(r"speaker (\S+)\n\{\n(.*?)\n\}\n", text, re.S):
        keys = {}
        for line in m.group(2).split("\n"):
            t = line.split()
            if len(t) >= 2 and t[0] not in ("feature", "model"):
                keys[t[0]] = t[1:]
        out[m.group(1)] = keys
    return out


def count_flips(got, want):
    """numbers printed with %g: equal strings, or one unit of the last printed digit apart (a flip); anything else fails"""
    assert len(got) == len(want), (len(got), len(want))
    flips = 0
    for a, b in zip(got, want):
        if a == b:
            continue
        # %g prints six significant digits (and drops trailing zeros): one unit of the sixth digit of either
        # number (they differ where a power of ten lies between the two), compared in exact decimal arithmetic
        da, db = Decimal(a), Decimal(b)
        assert abs(da - db) in (Decimal(1).scaleb(da.adjusted() - 5), Decimal(1).scaleb(db.adjusted() - 5)), (a, b)
        flips += 1
    return flips


def fmt(v):
    return ["%g" % t for t in np.asarray(v).ravel()]


def test_tool_feature_mode(capi, setup, tmp_path):
    st = setup
    out = str(tmp_path / "out.spkc")
    r = run_tool(st, "fea.spkc", out, "-M", "transform")
    assert r.stdout == "s0: s1: s2: "                                 # no newline in feature mode
    assert r.stderr.count("Calculating transform for s") == 3 and "Processing file: %s (1/6)" % st["utts"][0]["wav"] in r.stderr
    want = restate_speakers(capi, st, True)
    got = parse_spkc(open(out).read())
    assert set(got) == {"default", "s0", "s1", "s2"}
    flips = total = selfflips = 0
    for spk, ws in want.items():
        A, b = MR.compose(ws["W"], *ws.get("old", (None, None)))
        Ae, be = MR.compose(ws["We"], *ws.get("old", (None, None)))
        print("%s: largest |W| %.3g" % (spk, np.abs(ws["W"]).max()))
        selfflips += count_flips(fmt(Ae), fmt(A)) + count_flips(fmt(be), fmt(b))
        flips += count_flips(got[spk]["matrix"], fmt(A)) + count_flips(got[spk]["bias"], fmt(b))
        total += A.size + b.size
    print("flips %d, of the restatement from extended statistics %d, of %d numbers" % (flips, selfflips, total))
    assert selfflips <= 0.01 * total and flips <= 0.01 * total
    # -O reads the alignment= files (the same here); -B 2 -I 1 / 2 concatenated as train.pl does with cat
    run_tool(st, "fea.spkc", str(tmp_path / "o.spkc"), "-M", "transform", "-O")
    assert open(str(tmp_path / "o.spkc")).read() == open(out).read()
    halves = ""
    for k in (1, 2):
        run_tool(st, "fea.spkc", str(tmp_path / ("h%d.spkc" % k)), "-M", "transform", "-B", "2", "-I", str(k))
        halves += open(str(tmp_path / ("h%d.spkc" % k))).read()
    assert "utterance" not in halves and halves.count("speaker default") == 1
    assert halves == open(out).read()
    # closed loop: each file read back and applied through the speaker configuration, the f64 features recomputed under
    # it, the engine's own scoring along the segmentation plus frames * log |det A| of the transform the file carries
    D = st["D"]
    gmm = capi.Gmm.from_files(st["base"] + ".gk", st["base"] + ".mc", st["base"] + ".ph")
    for spk, ws in want.items():
        ll = []
        for path in (str(st["dir"] / "fea.spkc"), out):
            keys = parse_spkc(open(path).read()).get(spk, {})
            logdet = np.linalg.slogdet(np.array(keys["matrix"], np.float64).reshape(D, D))[1] if "matrix" in keys else 0.0
            ft = capi.Feat(st["cfg_text"])
            sc = capi.SpeakerConfig(ft)
            sc.read_file(path)
            sc.set_speaker(spk)
            xs = []
            for u in st["utts"]:
                if u["spk"] == spk:
                    start, pdf, _ = capi.stats_read_segmentation(st["topo"], u["phn"], ft.frame_rate, 0, 0, u["eof"], False)
                    xs.append(ft.run(u["pcm"], start, len(pdf), dtype=np.float64))
            x = np.concatenate(xs)
            s = gmm.score_f64(x)
            ll.append(float(s[np.arange(len(ws["pdf"])), ws["pdf"]].sum()) + len(ws["pdf"]) * logdet)
            del sc
        print("%s: log-likelihood with log |det A| %.6f -> %.6f over %d frames" % (spk, ll[0], ll[1], len(ws["pdf"])))
        assert ll[1] > ll[0]
    gmm.close()


def test_tool_model_mode_and_closed_loop(capi, setup, tmp_path):
    st = setup
    out = str(tmp_path / "out.spkc")
    r = run_tool(st, "model.spkc", out)
    want = restate_speakers(capi, st, False)
    lines = r.stdout.split("\n")
    assert [l.split(":")[0] for l in lines[:3]] == ["s0", "s1", "s2"] and "No regression tree used" in r.stderr
    for l, spk in zip(lines, ("s0", "s1", "s2")):
        assert l == "%s: %g frames, 1 transform matrices" % (spk, want[spk]["beta"])
    got = parse_spkc(open(out).read())
    flips = total = 0
    for spk, ws in want.items():
        # the yardstick first: the restatement from extended statistics prints the same digits on these inputs
        print("%s: largest |W| %.3g" % (spk, np.abs(ws["W"]).max()))
        assert count_flips(fmt(ws["We"]), fmt(ws["W"])) <= 0.01 * ws["W"].size
        assert got[spk]["unitmode"] == ["UNIT_NO"]
        flips += count_flips(got[spk]["w1"], fmt(ws["W"]))
        total += ws["W"].size
    print("flips %d of %d numbers" % (flips, total))
    assert flips <= 0.01 * total
    halves = ""
    for k in (1, 2):
        run_tool(st, "model.spkc", str(tmp_path / ("h%d.spkc" % k)), "-B", "2", "-I", str(k))
        halves += open(str(tmp_path / ("h%d.spkc" % k))).read()
    assert halves == open(out).read()
    # closed loop: the file read back, the engine's own scoring along the segmentation (log |det A| included)
    ft = capi.Feat(st["cfg_text"])
    for spk, ws in want.items():
        ll = []
        for path in (str(st["dir"] / "model.spkc"), out):
            gmm = capi.Gmm.from_files(st["base"] + ".gk", st["base"] + ".mc", st["base"] + ".ph")
            sc = capi.SpeakerConfig(ft, gmm)
            sc.read_file(path)
            sc.set_speaker(spk)
            s = gmm.score_f64(ws["x"])
            ll.append(float(s[np.arange(len(ws["pdf"])), ws["pdf"]].sum()))
            del sc
            gmm.close()
        print("%s: log-likelihood %.6f -> %.6f over %d frames" % (spk, ll[0], ll[1], len(ws["pdf"])))
        assert ll[1] > ll[0]

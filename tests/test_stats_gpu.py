"""ML statistics on the device (csrc/stats_accum.hip) and the native stats tool, against a restatement
in double of Mixture::accumulate / DiagonalStatisticsAccumulator::accumulate summed in frame order
(aku/Distributions.cc:249-260, 2134-2161) over the engine's own f64 features and the oracle's double
Gaussian log-likelihoods:
1. lib/bin/stats --ml -t on a synthetic recipe (WAV audio, random state segmentations, a tied model with
   unused Gaussians, recipe start/end times, a segmentation longer than the audio, an empty file and a
   state far from every frame) -- feacount exact, gamma within 1e-12, every .gks float within one ulp,
   .mcs structure exact and values within 1e-9, .phs byte-identical, .lls within 1e-9;
2. -B 2 -I 1 plus -I 2 equal the single run, and two runs write identical bytes;
3. align then stats -O over the .phn files that align wrote;
4. the handle: many utterances per call equal per-utterance calls, and a state of 10^5 frames (split
   across workgroups) matches the restatement;
5. known answer: frames drawn from known per-state Gaussians through a `pre` module give back their
   means and variances;
6. -S with a VTLN speaker file (two speakers with different warps alternating, -U with an utterance warp)
   against the restatement over features computed under each utterance's warp;
7. a model with a mixture of no components: its frames add safe_log(0) to the .lls and nothing else."""
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

pytestmark = pytest.mark.gpu

N_HMM, PER, COMPS = 10, 3, 4
SPF = 128


def write_ph(path, n_hmm=N_HMM):
    """3-state left-to-right HMMs, pdf = 3 h + j, a skip from state 0 to state 2 on every HMM"""
    rng = np.random.default_rng(3)
    with open(path, "w") as f:
        f.write("PHONE\n%d\n" % n_hmm)
        for h in range(n_hmm):
            f.write("%d 5 h%d\n-1 -2 %d %d %d\n0 1 2 1.0\n1 0\n" % (h + 1, h, 3 * h, 3 * h + 1, 3 * h + 2))
            a = rng.uniform(0.3, 0.7)
            f.write("2 3 2 %.4f 3 %.4f 4 %.4f\n" % (a, (1 - a) * 0.8, (1 - a) * 0.2))
            b = rng.uniform(0.3, 0.7)
            f.write("3 2 3 %.4f 4 %.4f\n" % (b, 1 - b))
            c = rng.uniform(0.3, 0.7)
            f.write("4 2 4 %.4f 1 %.4f\n" % (c, 1 - c))


def _write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def random_segmentation(rng, n_frames, start=0, far_state=None):
    """state-segmented lines from `start`: whole HMMs, states in order (sometimes the 0 -> 2 skip)"""
    lines, t = [], start
    while t < start + n_frames:
        h = int(rng.integers(0, N_HMM))
        states = [0, 2] if rng.random() < 0.2 else [0, 1, 2]
        for k in states:
            d = int(rng.integers(1, 7))
            lines.append((t, t + d, "h%d" % h, k))
            t += d
    if far_state is not None:
        h = far_state // PER   # the far state is the HMM's last one
        for k in range(3):
            lines.append((t, t + 2, "h%d" % h, k))
            t += 2
    return lines


def write_phn(path, lines):
    with open(path, "w") as f:
        for s, e, lab, k in lines:
            f.write("%d %d %s.%d\n" % (s * SPF, e * SPF, lab, k))


@pytest.fixture(scope="module")
def setup(capi, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("stats")
    S = N_HMM * PER
    cfg_text = synth.make_feature_config()
    cfg = str(d / "f.cfg")
    open(cfg, "w").write(cfg_text)
    ft = capi.Feat(cfg_text)
    rng = np.random.default_rng(11)
    utts = []
    for u in range(6):
        pcm = synth.make_audio(16000 * 2 + 1000 * u, seed=100 + u)
        wav = str(d / ("u%d.wav" % u))
        _write_wav(wav, pcm)
        eof = ft.eof_frame(len(pcm))
        utts.append(dict(wav=wav, pcm=pcm, eof=eof, phn=str(d / ("u%d.phn" % u))))
    fea = np.concatenate([ft.run(x["pcm"], 0, x["eof"], dtype=np.float64) for x in utts])
    G = COMPS * S + 7   # the last 7 Gaussians belong to no mixture
    mean, var, off, idx, w = synth.make_model(D=39, G=G, S=S, comps=COMPS, seed=23)
    mean[:] = fea[rng.integers(0, len(fea), G)] + 0.3 * rng.standard_normal((G, 39))
    var[:] = rng.uniform(0.5, 2.0, var.shape)
    idx[:] = rng.integers(0, COMPS * S, len(idx))   # tied: Gaussians shared between mixtures
    far = S - 1   # every Gaussian of this state far from every frame: total 0
    far_g = COMPS * S + np.arange(COMPS) % 7
    idx[off[far]:off[far + 1]] = far_g
    mean[far_g] = 1e3
    var[far_g] = 1e-2
    base = str(d / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    write_ph(base + ".ph")
    # segmentations: one longer than the audio, one empty, one with start/end times, one with the far state
    recipe = []
    for u, x in enumerate(utts):
        if u == 1:
            lines = random_segmentation(rng, x["eof"] + 40)
        elif u == 4:
            lines = []
        elif u == 5:
            lines = random_segmentation(rng, x["eof"] - 60, far_state=far)
        else:
            lines = random_segmentation(rng, x["eof"] - 20)
        write_phn(x["phn"], lines)
        line = "audio=%s transcript=%s alignment=%s speaker=s%d" % (x["wav"], x["phn"], x["phn"], u % 2)
        # recipe keys persist across lines (aku/Recipe.cc): every line sets its times
        line += " start-time=0.2 end-time=1.1" if u == 2 else " start-time=0 end-time=0"
        recipe.append(line)
    rcp = str(d / "r.rcp")
    open(rcp, "w").write("\n".join(recipe) + "\n")
    topo = capi.Topology(base + ".ph")
    return dict(dir=d, cfg=cfg, cfg_text=cfg_text, base=base, model=(mean, var, off, idx, w), S=S, G=G, utts=utts,
                recipe=rcp, topo=topo, far=far)


def restate(capi, oracle, st, recipe_lines, ophn=False, transitions=True, warps=None):
    """the statistics of stats --ml [-t] over the recipe, in double, frame by frame; warps: per recipe line the
    vtln module's warp_factor its features are computed with"""
    mean, var, off, idx, w = st["model"]
    topo = st["topo"]
    ft = capi.Feat(st["cfg_text"])
    fr = ft.frame_rate
    dm = oracle.DiagModel(mean, var, off, idx, w)
    w = dm.mix_w   # normalised as Mixture::read leaves them
    G, D, S = len(mean), mean.shape[1], len(off) - 1
    out = dict(feacount=np.zeros(G, np.int64), gamma=np.zeros(G), aux=np.zeros(G), sx=np.zeros((G, D)),
               sxx=np.zeros((G, D)), mix_gamma=np.zeros(len(idx)), count=np.zeros(S, np.int64), mll=np.zeros(S))
    probs = [p for s in range(topo.num_states()) for _, p in topo.transitions(s)]
    out["tr"] = np.zeros(len(probs))
    lls, frames = 0.0, 0
    for li, line in enumerate(recipe_lines):
        info = dict(kv.split("=", 1) for kv in line.split())
        if warps is not None:
            ft.set_parameters("vtln", "{\n  warp_factor %s\n}\n" % warps[li])
        pcm = oracle.read_wav_pcm16(info["audio"])[0]
        eof = ft.eof_frame(len(pcm))
        first = last = 0
        t0, t1 = float(info.get("start-time", 0)), float(info.get("end-time", 0))
        if t0 > 0 or t1 > 0:
            first, last = int(np.float32(t0) * np.float32(fr)), int(np.float32(t1) * np.float32(fr))
        seg = capi.stats_read_segmentation(topo, info["alignment" if ophn else "transcript"], fr, first, last, eof,
                                           transitions)
        if seg is None or len(seg[1]) == 0:
            continue
        start, pdf, tr = seg
        x = ft.run(pcm, start, len(pdf), dtype=np.float64)
        gl = dm.gauss_loglik(x)
        for f in range(len(pdf)):
            p = int(pdf[f])
            recs = range(off[p], off[p + 1])
            lik = [np.exp(gl[f, idx[r]]) for r in recs]
            total = 0.0
            for r, l in zip(recs, lik):
                total += w[r] * l
            sl = np.log(1e-50) if total < 1e-50 else np.log(total)   # util::safe_log
            out["mll"][p] += 1.0 * sl
            lls += sl
            if total > 0:
                out["count"][p] += 1
                for r, l in zip(recs, lik):
                    g = 1.0 * w[r] * l / total
                    gi = idx[r]
                    out["mix_gamma"][r] += g
                    out["feacount"][gi] += 1
                    out["gamma"][gi] += g
                    out["aux"][gi] += abs(g)
                    gx = g * x[f]
                    out["sx"][gi] += gx
                    out["sxx"][gi] += gx * x[f]
            if transitions and tr[f] >= 0:
                out["tr"][tr[f]] += 1.0
                lls += np.log(probs[tr[f]])
        frames += len(pdf)
    out["lls"], out["frames"] = lls, frames
    return out


def read_gks(path):
    b = open(path, "rb").read()
    G, D, mode = struct.unpack_from("<3i", b, 0)
    at = 12
    out = {}
    for _ in range(G):
        g, flag = struct.unpack_from("<2i", b, at)
        at += 8
        if flag == 0:
            fc, gam, aux = struct.unpack_from("<idd", b, at)
            at += 20
            sx = np.frombuffer(b, "<f4", D, at).astype(np.float64)
            sxx = np.frombuffer(b, "<f4", D, 4 * D + at).astype(np.float64)
            at += 8 * D
            end, = struct.unpack_from("<i", b, at)
            at += 4
            assert end == -1
            out[g] = (fc, gam, aux, sx, sxx)
        else:
            assert flag == -1
    assert at == len(b)
    return (G, D, mode), out


def read_mcs(path):
    lines = open(path).read().split("\n")
    n, mode = int(lines[0]), int(lines[1])
    at, out = 2, {}
    for i in range(n):
        assert int(lines[at]) == i
        at += 1
        if lines[at] != "-1":
            out[i] = lines[at].split()
            at += 1
        assert lines[at] == "-1"
        at += 1
    return (n, mode), out


def one_ulp(v):
    v = np.float32(v)
    return float(np.spacing(np.abs(v)))


def check_against(st, base, want, transitions=True):
    mean, var, off, idx, w = st["model"]
    (G, D, mode), gks = read_gks(base + ".gks")
    assert (G, D, mode) == (st["G"], mean.shape[1], 1)
    acc = set(np.nonzero(want["feacount"])[0].tolist())
    assert set(gks) == acc
    assert not (set(range(G - 7, G)) & acc)   # the far Gaussians and those of no mixture
    for g, (fc, gam, aux, sx, sxx) in gks.items():
        assert fc == want["feacount"][g]
        assert gam == pytest.approx(want["gamma"][g], rel=1e-12, abs=1e-300)
        assert aux == pytest.approx(want["aux"][g], rel=1e-12, abs=1e-300)
        for got_v, want_v in ((sx, want["sx"][g]), (sxx, want["sxx"][g])):
            lim = np.array([one_ulp(v) for v in want_v])
            assert (np.abs(got_v - want_v) <= lim).all(), (g, got_v - want_v, lim)
    (n, mode), mcs = read_mcs(base + ".mcs")
    assert (n, mode) == (len(off) - 1, 1)
    assert set(mcs) == set(np.nonzero(want["count"])[0].tolist())
    for p, f in mcs.items():
        M = off[p + 1] - off[p]
        assert f[0] == "0" and int(f[1]) == M and len(f) == 2 + 2 * M + 2
        for k in range(M):
            assert int(f[2 + 2 * k]) == idx[off[p] + k]
            assert float(f[3 + 2 * k]) == pytest.approx(want["mix_gamma"][off[p] + k], rel=1e-9, abs=1e-12)
        assert f[-2] == "0"
        assert float(f[-1]) == pytest.approx(want["mll"][p], rel=1e-9)
    if st["far"] is not None:
        assert st["far"] not in mcs
    topo = st["topo"]
    src = [(s, o) for s in range(topo.num_states()) for o, _ in topo.transitions(s)]
    txt = "%d\n" % len(src) + "".join("%d %d %g\n" % (s, o, c) for (s, o), c in zip(src, want["tr"]) if c > 0)
    assert open(base + ".phs").read() == txt
    lls = open(base + ".lls").read().split("\n")
    assert lls[0].startswith("Numerator loglikelihood: ") and lls[1].startswith("Number of frames: ")
    assert int(lls[1].split(": ")[1]) == want["frames"]
    assert float(lls[0].split(": ")[1]) == pytest.approx(want["lls"], rel=1e-9)


def run_stats(st, out, *extra):
    cmd = [os.path.join(BIN, "stats"), "-b", st["base"], "-c", st["cfg"], "-r", st["recipe"], "-o", out, "--ml",
           "-F", "0", "-W", "0", "-A", "1", "-i", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stderr


def test_stats_tool_matches_restatement(capi, oracle, setup, tmp_path):
    out = str(tmp_path / "o")
    err = run_stats(setup, out, "-t")
    lines = open(setup["recipe"]).read().split("\n")[:-1]
    want = restate(capi, oracle, setup, lines)
    check_against(setup, out, want)
    assert err.count("Processing file: ") == len(lines)
    assert " (0.20-1.10)" in err
    assert "Could not initialize the utterance segmentation.\nGiving up for this file\n" in err
    assert "Finished collecting statistics (0/0)\n" in err
    total = float(err.split("Total num log likelihood: ")[1].split()[0])
    assert total == pytest.approx(want["lls"], rel=1e-5)
    # a second run writes the same bytes
    out2 = str(tmp_path / "p")
    run_stats(setup, out2, "-t")
    for ext in (".gks", ".mcs", ".phs", ".lls"):
        assert open(out + ext, "rb").read() == open(out2 + ext, "rb").read(), ext


def test_stats_batches_sum_to_the_single_run(capi, oracle, setup, tmp_path):
    lines = open(setup["recipe"]).read().split("\n")[:-1]
    whole = str(tmp_path / "all")
    run_stats(setup, whole, "-t")
    parts, wants = [], []
    for k in (1, 2):
        out = str(tmp_path / ("b%d" % k))
        run_stats(setup, out, "-t", "-B", "2", "-I", str(k))
        first, n = capi.recipe_batch_range(len(lines), 2, k)
        want = restate(capi, oracle, setup, lines[first:first + n])
        check_against(setup, out, want)   # every half within the tolerances of the single run's check
        parts.append(out)
        wants.append(want)
    assert sum(w["frames"] for w in wants) == restate(capi, oracle, setup, lines)["frames"]
    # what the halves hold adds up to the single run: counts exactly, the rest to rounding
    g_whole = read_gks(whole + ".gks")[1]
    g_parts = [read_gks(p + ".gks")[1] for p in parts]
    assert set(g_whole) == set(g_parts[0]) | set(g_parts[1])
    for g, (fc, gam, aux, sx, sxx) in g_whole.items():
        got = [p[g] for p in g_parts if g in p]
        assert sum(x[0] for x in got) == fc
        assert sum(x[1] for x in got) == pytest.approx(gam, rel=1e-12)
        assert sum(x[2] for x in got) == pytest.approx(aux, rel=1e-12)
        for j, whole_v in ((3, sx), (4, sxx)):
            lim = np.array([one_ulp(v) for v in whole_v]) + sum(np.array([one_ulp(v) for v in x[j]]) for x in got)
            assert (np.abs(sum(x[j] for x in got) - whole_v) <= lim).all(), g
    m_whole = read_mcs(whole + ".mcs")[1]
    m_parts = [read_mcs(p + ".mcs")[1] for p in parts]
    assert set(m_whole) == set(m_parts[0]) | set(m_parts[1])
    for p, f in m_whole.items():
        got = [m[p] for m in m_parts if p in m]
        for i in range(3, len(f) - 2, 2):   # component gammas
            assert sum(float(x[i]) for x in got) == pytest.approx(float(f[i]), rel=1e-9, abs=1e-12)
        assert sum(float(x[-1]) for x in got) == pytest.approx(float(f[-1]), rel=1e-9)
    def phs(path):
        rows = open(path).read().splitlines()
        return int(rows[0]), {(int(a), int(b)): float(c) for a, b, c in (r.split() for r in rows[1:])}
    n_whole, t_whole = phs(whole + ".phs")
    halves = [phs(p + ".phs") for p in parts]
    assert all(n == n_whole for n, _ in halves)
    summed = {}
    for _, t in halves:
        for k, v in t.items():
            summed[k] = summed.get(k, 0.0) + v
    assert summed == t_whole
    ll = [float(open(p + ".lls").read().split("\n")[0].split(": ")[1]) for p in parts]
    assert sum(ll) == pytest.approx(float(open(whole + ".lls").read().split("\n")[0].split(": ")[1]), rel=1e-9)


def test_stats_no_train_writes_only_lls(capi, oracle, setup, tmp_path):
    out = str(tmp_path / "n")
    run_stats(setup, out, "-n", "-t")
    assert os.path.exists(out + ".lls") and not os.path.exists(out + ".gks") and not os.path.exists(out + ".mcs")
    want = restate(capi, oracle, setup, open(setup["recipe"]).read().split("\n")[:-1], transitions=False)
    assert float(open(out + ".lls").read().split("\n")[0].split(": ")[1]) == pytest.approx(want["lls"], rel=1e-9)


def test_align_then_stats_ophn(capi, oracle, setup, tmp_path):
    d = tmp_path
    lines = []
    for u, x in enumerate(setup["utts"]):
        if u == 4:
            continue
        tr = str(d / ("t%d.phn" % u))
        with open(tr, "w") as f:
            for h in np.random.default_rng(u).integers(0, N_HMM, 12):
                f.write("h%d\n" % h)
        lines.append("audio=%s transcript=%s alignment=%s" % (x["wav"], tr, str(d / ("a%d.phn" % u))))
    rcp = str(d / "a.rcp")
    open(rcp, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([os.path.join(BIN, "align"), "-b", setup["base"], "-c", setup["cfg"], "-r", rcp,
                        "--beam", "1000", "--sbeam", "1000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = dict(setup, recipe=rcp)
    out = str(d / "o")
    run_stats(st, out, "-t", "-O")
    check_against(st, out, restate(capi, oracle, st, lines, ophn=True))


def test_batched_equals_single_and_a_heavy_state(capi, oracle, setup):
    import torch
    mean, var, off, idx, w = setup["model"]
    gmm = capi.Gmm.from_arrays(mean, var, off, idx, w)
    rng = np.random.default_rng(5)
    F = 100_000 + 3000
    x = mean[rng.integers(0, COMPS * setup["S"], F)] + 0.7 * rng.standard_normal((F, 39))
    pdf = rng.integers(0, setup["S"] - 1, F).astype(np.int32)
    pdf[:100_000] = 7   # one state holds 10^5 frames
    rng.shuffle(pdf)
    d_x = torch.tensor(x, device="cuda")
    one = capi.Stats(gmm, setup["topo"], len(idx))
    d_ll = torch.zeros(F, dtype=torch.float64, device="cuda")
    one.accumulate_dev(d_x, pdf, d_ll)
    a = one.fetch()
    many = capi.Stats(gmm, setup["topo"], len(idx))
    cuts = [0, 17, 1000, 1001, 50_000, 77_777, F]
    for b, e in zip(cuts[:-1], cuts[1:]):
        many.accumulate_dev(d_x[b:e], pdf[b:e])
    bb = many.fetch()
    assert (a["feacount"] == bb["feacount"]).all() and (a["count"] == bb["count"]).all()
    np.testing.assert_allclose(a["gamma"], bb["gamma"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(a["sum_x"], bb["sum_x"], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(a["mixture_ll"], bb["mixture_ll"], rtol=1e-12)
    # the heavy state against the restatement
    sel = pdf == 7
    dm = oracle.DiagModel(mean, var, off, idx, w)
    w = dm.mix_w
    gl = dm.gauss_loglik(x[sel])
    recs = np.arange(off[7], off[8])
    lik = np.exp(gl[:, idx[recs]])
    tot = np.zeros(len(lik))
    for k in range(len(recs)):
        tot = tot + w[recs[k]] * lik[:, k]
    gam = (w[recs] * lik) / tot[:, None]
    np.testing.assert_allclose(a["mix_gamma"][recs], gam.sum(0), rtol=1e-11)
    np.testing.assert_allclose(d_ll.cpu().numpy()[sel], np.log(np.maximum(tot, 1e-50)), rtol=1e-13, atol=1e-12)
    assert sel.sum() >= 100_000 and a["count"][7] == int((tot > 0).sum())
    gmm.close()


def test_known_answer_pre_module(capi, oracle, tmp_path):
    """frames of a pre module drawn from known diagonal Gaussians, one per state, segmented by state:
    the ML estimates from the .gks recover the generating parameters"""
    d = tmp_path
    D, S = 6, 3 * 2
    rng = np.random.default_rng(17)
    mu = rng.uniform(-3, 3, (S, D))
    sd = rng.uniform(0.5, 2.0, (S, D))
    cfg = "module\n{\n name pre\n type pre\n dim %d\n}\n" % D
    open(str(d / "k.cfg"), "w").write(cfg)
    base = str(d / "k")
    with open(base + ".ph", "w") as f:
        f.write("PHONE\n2\n")
        for h in range(2):
            f.write("%d 5 h%d\n-1 -2 %d %d %d\n0 1 2 1.0\n1 0\n2 2 2 0.5 3 0.5\n3 2 3 0.5 4 0.5\n4 2 4 0.5 1 0.5\n"
                    % (h + 1, h, 3 * h, 3 * h + 1, 3 * h + 2))
    oracle.write_gk(base + ".gk", mu + 0.5, (sd * 1.5) ** 2)
    oracle.write_mc(base + ".mc", np.arange(S + 1), np.arange(S), np.ones(S))
    lines = []
    for u in range(4):
        segs, frames, t = [], [], 0
        for rep in range(40):
            h = int(rng.integers(0, 2))
            for k in range(3):
                n = int(rng.integers(20, 60))
                s = 3 * h + k
                frames.append(mu[s] + sd[s] * rng.standard_normal((n, D)))
                segs.append((t, t + n, "h%d" % h, k))
                t += n
        fea = str(d / ("u%d.fea" % u))
        oracle.write_feature_file(fea, np.concatenate(frames).astype(np.float32))
        phn = str(d / ("u%d.phn" % u))
        write_phn(phn, segs)
        lines.append("audio=%s transcript=%s" % (fea, phn))
    rcp = str(d / "k.rcp")
    open(rcp, "w").write("\n".join(lines) + "\n")
    out = str(d / "o")
    r = subprocess.run([os.path.join(BIN, "stats"), "-b", base, "-c", str(d / "k.cfg"), "-r", rcp, "-o", out, "--ml"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, gks = read_gks(out + ".gks")
    assert set(gks) == set(range(S))
    for s in range(S):
        fc, gam, aux, sx, sxx = gks[s]
        assert gam == pytest.approx(fc, rel=1e-12)   # one component: gamma 1 on every frame
        m = sx / gam
        v = sxx / gam - m * m
        n = gam
        assert np.all(np.abs(m - mu[s]) < 5 * sd[s] / np.sqrt(n)), s
        assert np.all(np.abs(v / sd[s] ** 2 - 1) < 5 * np.sqrt(2 / n)), s


VTLN_CFG = """module
{
  name audiofile
  type audiofile
  sample_rate 16000
}
module
{
  name fft
  type fft
  magnitude 0
  sources audiofile
}
module
{
  name vtln
  type vtln
  sources fft
}
module
{
  name mel
  type mel
  sources vtln
}
module
{
  name mfcc
  type dct
  dim 12
  sources mel
}
module
{
  name d1
  type delta
  sources mfcc
}
module
{
  name merged
  type merge
  sources mfcc d1
}
"""

SPKC = """speaker s1
{
  feature vtln
  {
    warp_factor 0.92
  }
}
speaker s2
{
  feature vtln
  {
    warp_factor 1.08
  }
}
utterance default
{
  vtln
  {
  }
}
utterance u7
{
  vtln
  {
    warp_factor 1.02
  }
}
"""


def test_stats_speaker_vtln(capi, oracle, setup, tmp_path):
    """-S: features under each speaker's warp, the speakers alternating inside one group of utterances; -U: the
    last utterance carries an utterance warp (the last, so that no later set_speaker stores it as its speaker's)"""
    d = tmp_path
    cfg = str(d / "v.cfg")
    open(cfg, "w").write(VTLN_CFG)
    ft = capi.Feat(VTLN_CFG)
    D = ft.dim
    utts = [setup["utts"][u] for u in (0, 1, 2, 3, 5, 0)]
    fea = np.concatenate([ft.run(x["pcm"], 0, x["eof"], dtype=np.float64) for x in utts])
    rng = np.random.default_rng(41)
    S = N_HMM * PER
    G = COMPS * S + 7
    mean, var, off, idx, w = synth.make_model(D=D, G=G, S=S, comps=COMPS, seed=29)
    mean[:] = fea[rng.integers(0, len(fea), G)] + 0.3 * rng.standard_normal((G, D))
    var[:] = rng.uniform(0.3, 1.5, var.shape)
    idx[:] = rng.integers(0, COMPS * S, len(idx))
    base = str(d / "v")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    write_ph(base + ".ph")
    spk = str(d / "v.spkc")
    open(spk, "w").write(SPKC)
    speakers = ["s1", "s2", "s1", "s2", "s1", "s2"]
    lines = []
    for i, (x, sp) in enumerate(zip(utts, speakers)):
        line = "audio=%s transcript=%s speaker=%s start-time=0 end-time=0" % (x["wav"], x["phn"], sp)
        if i == len(utts) - 1:
            line += " utterance=u7"
        lines.append(line)
    rcp = str(d / "v.rcp")
    open(rcp, "w").write("\n".join(lines) + "\n")
    st = dict(setup, cfg=cfg, cfg_text=VTLN_CFG, base=base, model=(mean, var, off, idx, w), G=G, recipe=rcp,
              topo=capi.Topology(base + ".ph"), far=None)
    warp = {"s1": "0.92", "s2": "1.08"}
    # -S alone: every utterance under its speaker's warp
    out = str(d / "o")
    run_stats(st, out, "-t", "-S", spk)
    check_against(st, out, restate(capi, oracle, st, lines, warps=[warp[sp] for sp in speakers]))
    # -U: the last utterance under its own warp
    out_u = str(d / "u")
    run_stats(st, out_u, "-t", "-S", spk, "-U")
    check_against(st, out_u, restate(capi, oracle, st, lines, warps=[warp[sp] for sp in speakers[:-1]] + ["1.02"]))
    # the warps matter: the statistics of one warp for all differ
    flat = restate(capi, oracle, st, lines, warps=["1.0"] * len(lines))
    got = read_gks(out + ".gks")[1]
    assert any(abs(got[g][1] - flat["gamma"][g]) > 1e-6 * max(1.0, flat["gamma"][g]) for g in got)


def test_stats_mixture_without_components(capi, oracle, setup, tmp_path):
    """a state whose mixture has no components: total 0 on its frames -- safe_log(0) into the .lls and its
    mixture_ll, nothing accumulated, the same bytes on every run"""
    mean, var, off, idx, w = setup["model"]
    empty = 4
    M = off[empty + 1] - off[empty]
    keep = np.r_[0:off[empty], off[empty + 1]:len(idx)]
    off2 = off.copy()
    off2[empty + 1:] -= M
    idx2, w2 = idx[keep], w[keep]
    base = str(tmp_path / "e")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off2, idx2, w2)
    write_ph(base + ".ph")
    st = dict(setup, base=base, model=(mean, var, off2, idx2, w2))
    lines = open(setup["recipe"]).read().split("\n")[:-1]
    want = restate(capi, oracle, st, lines)
    assert want["count"][empty] == 0 and want["mll"][empty] < 0   # the state has frames
    outs = []
    for tag in ("a", "b"):
        out = str(tmp_path / tag)
        run_stats(st, out, "-t")
        outs.append(out)
    check_against(st, outs[0], want)
    assert empty not in read_mcs(outs[0] + ".mcs")[1]
    for ext in (".gks", ".mcs", ".phs", ".lls"):
        assert open(outs[0] + ext, "rb").read() == open(outs[1] + ext, "rb").read(), ext

"""lda --networks (csrc/lda.cc, csrc/aku/main_lda.cc): the LDA matrix from Baum-Welch posteriors over the recipe's HMM
networks, the states' sums accumulated on the device from weighted entries, against tools/lda_networks_restate.py.  The
reference's own -H cannot run, so that restatement -- what aku/lda.cc:147-372 would compute from pdf_probs() -- is the
yardstick.

Fixture (modelled on tests/test_mllr_bw_gpu.py): three 2 s recordings, the production feature chain with three cepstra
up to its 12-dimensional normalization, then a lin_transform `lda` of 6 rows with a defined, well-conditioned matrix
(identity rows plus small noise); an 18-state diagonal model of dimension 6 in HMMs of three, the first two labelled _ and
__, with broad variances fitted to the engine's output frames; four windows of 55 frames a recording, each with a network
of its own (chains of six states, one fan a recording).  The restatement runs on the oracle's double state likelihoods
of the engine's own f64 frames at the chain's output and sums the engine's own f64 frames at the module's source; the
tool runs under AASR_PREC=1.

Every run asks for -d 6, and the driver refuses a -d other than the module's dimension, so the module has 6 rows and the
model that scores its output 6 dimensions: with 8 rows the eighth and ninth eigenvalue of W^-1 B lie so close on this data
that the two reference-side routes of the restatement no longer agree on the rows.

Conditions on the inputs, asserted in the fixture on the CPU side: with wide beams every utterance ends OK at its first
attempt and its smallest positive occupancy is above 1e-200; with default beams max |1 - s_t| is at most 0.02; at least
target_dim + 1 states have a restated gamma of --mingamma or more and none lies within 1e-6 relative of it; the restated W
is positive definite.

Bounds: the matrix by tests/test_lda_gpu.py's rule -- rows matched by |cosine|, max(8 x the distance between the eig and
eigh routes, 5e-6); gamma within 1e-12 relative of the restated gamma (tests/test_stats_bw_gpu.py's bound for gamma);
the sum of gamma within 1e-9 x frames of the number of frames."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmmnet_cases as HC  # noqa: E402
import lda_networks_restate as LN  # noqa: E402
import test_mllr_gpu as MG  # noqa: E402

pytestmark = pytest.mark.gpu
LR, BW, RS = LN.LR, LN.BW, LN.RS
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
S, PER, COMPS = 18, 3, 3
D_SRC, TD = 12, 6
SILENCE = list(range(2 * PER))
MINGAMMA = 12.5
SPANS = ((0.05, 0.49), (0.5, 0.94), (0.95, 1.39), (1.4, 1.84))
RECS = ("r0", "r1", "r2")
PREC64 = {"AASR_PREC": "1"}
WIDE = ("-F", "1e9", "-W", "1e9")
WRITTEN = 5e-6      # "%g": six significant digits


class World:
    pass


def build_world(capi, oracle, d):
    w = World()
    w.dir = d
    rng = np.random.default_rng(23)
    text = synth.make_feature_config(dim_cep=3)
    head = text[:text.index("module\n{\n  name transform")]
    a = np.eye(TD, D_SRC) + 0.05 * rng.standard_normal((TD, D_SRC))
    w.cfg_text = head + ("module\n{\n  name lda\n  type lin_transform\n  dim %d\n  matrix %s\n  sources normalization\n}\n"
                         % (TD, MG.vec(a)))
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(w.cfg_text)
    w.fr = 125.0
    w.windows = [tuple(capi.recipe_frame_limits(a_, b_, w.fr)) for a_, b_ in SPANS]
    assert [b_ - a_ for a_, b_ in w.windows] == [55] * 4, w.windows
    w.T = 240
    ft = capi.Feat(w.cfg_text)
    assert ft.dim == TD and ft.module_dim("normalization") == D_SRC
    w.pcm, w.wav, w.y, w.x = {}, {}, {}, {}
    for i, rec in enumerate(RECS):
        w.pcm[rec] = MG.varied_audio(16000 * 2, seed=500 + i)
        w.wav[rec] = str(d / (rec + ".wav"))
        MG.write_wav(w.wav[rec], w.pcm[rec])
        w.y[rec] = ft.run(w.pcm[rec], 0, w.T, dtype=np.float64)                           # what the model scores
        w.x[rec] = ft.run(w.pcm[rec], 0, w.T, module="normalization", dtype=np.float64)   # what is summed
    ally = np.concatenate([w.y[rec] for rec in RECS])
    G = COMPS * S
    mean, var, off, idx, mw = synth.make_model(D=TD, G=G, S=S, comps=COMPS, seed=37)
    mean[:] = ally[rng.integers(0, len(ally), G)] + 0.3 * rng.standard_normal((G, TD)) * ally.std(0)[None, :]
    var[:] = rng.uniform(3.0, 8.0, var.shape) * ally.var(0)[None, :]       # broad: the state posteriors stay soft
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    ph = open(w.base + ".ph").read().replace(" h0\n", " _\n").replace(" h1\n", " __\n")
    assert " _\n" in ph and " __\n" in ph
    open(w.base + ".ph", "w").write(ph)
    w.dm = oracle.DiagModel(mean, var, off, idx, mw)
    w.sp = np.full(S, 0.5)
    w.lines = []
    for i, rec in enumerate(RECS):
        for j in range(4):
            t = HC.fan(S, 3, 3, seed=60 + i) if j == 2 else HC.chain([int(s) for s in rng.choice(S, 6, replace=False)])
            net = str(d / ("%s_%d.hmmnet" % (rec, j)))
            open(net, "w").write(t)
            w.lines.append((rec, j, net))
    w.recipe = write_recipe(w, "all.rcp", w.lines)
    w.ll = {rec: w.dm.score(w.y[rec]) for rec in RECS}
    w.cache = {}
    return w


def write_recipe(w, name, lines):
    path = str(w.dir / name)
    with open(path, "w") as f:
        for rec, j, net in lines:
            f.write("audio=%s hmmnet=%s start-time=%s end-time=%s\n" % (w.wav[rec], net, SPANS[j][0], SPANS[j][1]))
    return path


def restate(w, fw=1e9, bw=1e9, ac=1.0, viterbi=False, mingamma=MINGAMMA, no_silence=False, maxmem=3000, lines=None):
    """the restated pipeline over the fixture's lines (or `lines`), with lda.cc:186-202's retries -> LN.pipeline's
    dictionary plus the utterances, the tolerance of the matrix and the expected retry messages"""
    key = (fw, bw, ac, viterbi, mingamma, no_silence, maxmem, tuple(lines or ()))
    if key in w.cache:
        return w.cache[key]
    utts, xs, messages = [], [], []
    for rec, j, net in (lines or w.lines):
        a, b = w.windows[j]
        parsed = HC.parse(open(net).read(), w.sp)
        for k in range(1, 6):
            e = BW.entries(parsed, w.ll[rec][a:b], fw, k * bw, ac, viterbi)
            if e["status"] != RS.FAILED_BACKWARD:
                break
            if k < 5:
                messages.append("Warning: Backward phase failed, increasing beam to %.1f" % ((k + 1) * bw))
        e["attempts"] = k
        utts.append(e)
        xs.append(w.x[rec][a:b])
    x = np.concatenate(xs)
    row0 = np.concatenate([[0], np.cumsum([len(q) for q in xs])])[:-1]
    o = LN.pipeline(utts, row0, x, S, TD, mingamma=mingamma, maxmem=maxmem, silence=SILENCE if no_silence else ())
    other = LR.solve(o["gamma"], o["sum_x"], o["sum_xx"], o["selected"], 1e6, TD, route="eigh")
    o["tol"] = max(8 * LR.rel_err(LR.match_rows(other, o["lda"]), o["lda"]), WRITTEN)
    o.update(utts=utts, x=x, row0=row0, messages=messages,
             frames=sum(e["T"] for e in utts if e["status"] == RS.OK))
    w.cache[key] = o
    return o


def check_conditions(w):
    wide = restate(w)
    for e in wide["utts"]:
        assert e["status"] == RS.OK and e["attempts"] == 1 and e["min_positive_occ"] > 1e-200, e["min_positive_occ"]
    per_frame = len(wide["rows"]) / float(len(wide["x"]))
    print("entries a frame %.2f, smallest occupancy %.3g" % (per_frame, min(e["min_positive_occ"] for e in wide["utts"])))
    assert per_frame > 1.5                                       # Baum-Welch: a frame belongs to several states
    dflt = restate(w, fw=15.0, bw=200.0)
    dev = max(e["max_dev"] for e in dflt["utts"])
    print("default beams: max |1 - s_t| %.3g" % dev)
    assert all(e["status"] == RS.OK for e in dflt["utts"]) and dev <= 0.02
    for o in (wide, restate(w, viterbi=True), restate(w, no_silence=True)):
        g = o["gamma"]
        print("gamma", np.round(g, 2).tolist())
        assert o["selected"].sum() >= TD + 1
        assert (np.abs(g - MINGAMMA) > 1e-6 * MINGAMMA).all()
        _, _, _, W = LR.w_and_b(g, o["sum_x"], o["sum_xx"], o["selected"], 1e6)
        assert np.linalg.eigvalsh(W).min() > 0


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = build_world(capi, oracle, tmp_path_factory.mktemp("lda_networks"))
    check_conditions(w)
    return w


def run_tool(w, out, *extra, recipe=None, ok=True):
    cmd = [os.path.join(BIN, "lda"), "--networks", "-b", w.base, "-c", w.cfg, "-r", recipe or w.recipe, "-M", "lda",
           "-d", str(TD), "-w", out, "--mingamma", str(MINGAMMA), "-i", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **PREC64))
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def written_matrix(out):
    text = open(out).read()
    m = re.search(r"matrix ([^\n]*)", text[text.index("name lda"):])
    return np.array(m.group(1).split(), np.float64).reshape(TD, -1)


def compare(tag, got, want, tol):
    err = LR.rel_err(LR.match_rows(got, want), want)
    print("%s: written matrix %.3g from the restatement (tolerance %.3g)" % (tag, err, tol))
    assert err <= tol


def differs(got, other, tol):
    """some row of got has no parallel partner among other's rows within tol"""
    unit = lambda m: m / np.linalg.norm(m, axis=1, keepdims=True)
    return float((1 - np.abs(unit(got) @ unit(other).T).max(axis=1)).max()) > tol


@pytest.fixture(scope="module")
def wide_runs(world, tmp_path_factory):
    """the tool under wide beams in both segmentation modes, once"""
    d = tmp_path_factory.mktemp("lda_networks_out")
    out = {}
    for mode in ("bw", "vit"):
        path = str(d / (mode + ".cfg"))
        out[mode] = (path, run_tool(world, path, "--segmode", mode, *WIDE))
    return out


def test_baum_welch_under_wide_beams(world, wide_runs, capi):
    w = world
    path, r = wide_runs["bw"]
    want = restate(w)
    assert r.stderr.count("Processing file: ") == 12 and "Warning" not in r.stderr and "Could not" not in r.stderr, r.stderr
    assert "Reserving memory" in r.stdout and "Compute the LDA" in r.stdout
    assert "Collecting statistics for %d states" % want["selected"].sum() in r.stdout, r.stdout
    entries = [l for l in r.stderr.splitlines() if l.startswith("Weighted entries: ")]
    assert entries == ["Weighted entries: %d over %d frames" % (len(want["rows"]), want["frames"])], r.stderr
    assert len([l for l in r.stderr.splitlines() if l.startswith("Largest |1 - sum of PDF probabilities| of a frame: ")]) == 1
    got = written_matrix(path)
    assert got.shape == (TD, D_SRC)
    compare("Baum-Welch", got, want["lda"], want["tol"])
    # the states' gamma through the library call
    gmm = capi.Gmm.from_files(w.base + ".gk", w.base + ".mc", w.base + ".ph")
    gmm.set_precision(1)
    res = capi.run_lda_networks_recipe(w.cfg_text, gmm, capi.Topology(w.base + ".ph"), w.recipe, "lda", TD,
                                       opts=capi.LdaOptions.defaults(mingamma=MINGAMMA),
                                       networks=capi.LdaNetworkOptions.defaults(networks=1, fw_beam=1e9, bw_beam=1e9))
    gmm.close()
    g, wg = res["state_gamma"], want["gamma"]
    rel = np.abs(g - wg) / np.where(wg > 0, wg, 1.0)
    print("gamma: largest relative difference %.3g; sum %.12g over %d frames" % (rel.max(), g.sum(), res["frames"]))
    assert ((wg > 0) == (g > 0)).all() and rel.max() <= 1e-12
    assert res["frames"] == want["frames"] == 12 * 55 and abs(g.sum() - res["frames"]) <= 1e-9 * res["frames"]
    assert res["seconds_scatter"] > 0 and res["seconds_features"] > 0


def test_viterbi_mode_counts_whole_frames(world, wide_runs, capi):
    w = world
    want = restate(w, viterbi=True)
    assert (want["weights"] == 1.0).all() and len(want["rows"]) == want["frames"]
    compare("Viterbi", written_matrix(wide_runs["vit"][0]), want["lda"], want["tol"])
    gmm = capi.Gmm.from_files(w.base + ".gk", w.base + ".mc", w.base + ".ph")
    gmm.set_precision(1)
    res = capi.run_lda_networks_recipe(w.cfg_text, gmm, capi.Topology(w.base + ".ph"), w.recipe, "lda", TD,
                                       opts=capi.LdaOptions.defaults(mingamma=MINGAMMA),
                                       networks=capi.LdaNetworkOptions.defaults(networks=1, viterbi=1, fw_beam=1e9, bw_beam=1e9))
    gmm.close()
    counts = np.diff(want["cnt"]).astype(np.float64)
    assert res["state_gamma"].tolist() == counts.tolist() == want["gamma"].tolist()


def test_posteriors_not_paths_were_accumulated(world, wide_runs):
    soft, hard = written_matrix(wide_runs["bw"][0]), written_matrix(wide_runs["vit"][0])
    tol = max(restate(world)["tol"], restate(world, viterbi=True)["tol"])
    assert differs(soft, hard, tol)


def test_default_forward_beam_with_scale_and_a_narrow_backward_beam(world, tmp_path):
    w = world
    want = restate(w, fw=15.0, bw=20.0, ac=0.5)
    print("attempts", [e["attempts"] for e in want["utts"]], "status", [e["status"] for e in want["utts"]])
    out = str(tmp_path / "narrow.cfg")
    r = run_tool(w, out, "-A", "0.5", "-W", "20")
    warn = [l for l in r.stderr.splitlines() if l.startswith("Warning: Backward phase failed, increasing beam to ")]
    assert warn == want["messages"], (warn, want["messages"])
    gave_up = sum(1 for e in want["utts"] if e["status"] != RS.OK)
    assert r.stderr.count("Could not run Baum-Welch for file ") == gave_up
    compare("-A 0.5 -W 20", written_matrix(out), want["lda"], want["tol"])
    assert differs(written_matrix(out), restate(w)["lda"], want["tol"])     # the options matter


def test_a_line_that_gives_up_adds_nothing(world, tmp_path):
    """a chain longer than its window fails its backward pass at every beam: four warnings, the two give-up lines, and
    the matrix of the other lines -- whose rows in the frame buffer lie on both sides of the given-up line's"""
    w = world
    long_net = str(tmp_path / "long.hmmnet")
    open(long_net, "w").write(HC.chain([s % S for s in range(60)]))
    lines = w.lines[:5] + [("r1", 0, long_net)] + w.lines[5:]
    want = restate(w, fw=15.0, bw=200.0, lines=lines)
    assert [e["status"] == RS.OK for e in want["utts"]] == [True] * 5 + [False] + [True] * 7
    assert want["utts"][5]["attempts"] == 5 and want["frames"] == 12 * 55
    out = str(tmp_path / "gaveup.cfg")
    r = run_tool(w, out, recipe=write_recipe(w, "gaveup.rcp", lines))
    warn = [l for l in r.stderr.splitlines() if l.startswith("Warning: Backward phase failed, increasing beam to ")]
    assert warn == want["messages"] == ["Warning: Backward phase failed, increasing beam to %.1f" % (k * 200.0) for k in (2, 3, 4, 5)]
    assert r.stderr.count("Could not run Baum-Welch for file %s\n" % w.wav["r1"]) == 1
    assert r.stderr.count("The HMM network may be incorrect or initial beam too low.\n") == 1
    assert "Weighted entries: %d over %d frames" % (len(want["rows"]), 12 * 55) in r.stderr, r.stderr
    compare("a given-up line", written_matrix(out), want["lda"], want["tol"])
    compare("a given-up line against the run without it", written_matrix(out), restate(w, fw=15.0, bw=200.0)["lda"],
            restate(w, fw=15.0, bw=200.0)["tol"])


def test_no_silence_and_the_memory_cap(world, tmp_path):
    w = world
    want = restate(w, no_silence=True)
    assert want["selected"][SILENCE].sum() == 0 and restate(w)["selected"][SILENCE].sum() > 0
    out = str(tmp_path / "nosil.cfg")
    r = run_tool(w, out, "--no-silence", *WIDE)
    assert "Discarding %d silence states" % len(SILENCE) in r.stdout
    assert "Collecting statistics for %d states" % want["selected"].sum() in r.stdout, r.stdout
    compare("--no-silence", written_matrix(out), want["lda"], want["tol"])
    assert differs(written_matrix(out), restate(w)["lda"], want["tol"])
    # -m: at 12 dimensions a megabyte holds more accumulators than there are states, so the only cap within reach is
    # none at all: lda_select leaves no state and the solve says so
    assert LN.select(restate(w)["gamma"], MINGAMMA, 1, D_SRC).tolist() == restate(w)["selected"].tolist()
    assert LN.select(restate(w)["gamma"], MINGAMMA, 0, D_SRC).sum() == 0
    r = run_tool(w, str(tmp_path / "m0.cfg"), "-m", "0", *WIDE, ok=False)
    assert "Collecting statistics at maximum for 0 states" in r.stdout
    assert "exception: lda: 0 selected classes cannot carry %d dimensions" % TD in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "m0.cfg"))


def test_the_written_configuration_whitens_the_selected_posteriors(world, wide_runs, oracle):
    w = world
    path, _ = wide_runs["bw"]
    want = restate(w)
    feats = {}
    for rec in RECS:
        r = subprocess.run([os.path.join(BIN, "feacat"), "-c", path, "--raw-output", "-H", w.wav[rec]], capture_output=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        dim = int(np.frombuffer(r.stdout[:4], np.int32)[0])
        feats[rec] = np.frombuffer(r.stdout[4:], np.float32).reshape(-1, dim).astype(np.float64)
        assert dim == TD
    y = np.concatenate([feats[rec][w.windows[j][0]:w.windows[j][1]] for rec, j, _ in w.lines])
    assert len(y) == len(want["x"])
    cls_of = np.repeat(np.arange(S), np.diff(want["cnt"]))
    keep = want["selected"][cls_of] == 1
    wt, rows = want["weights"][keep], want["rows"][keep]
    mean = (wt[:, None] * y[rows]).sum(0) / wt.sum()
    c = y[rows] - mean
    cov = (wt[:, None] * c).T @ c / wt.sum()
    dev = float(np.abs(cov - np.eye(TD)).max())
    print("posterior-weighted covariance of the projected features - I: %.3g" % dev)
    assert dev <= max(want["tol"], 2e-5)      # float features of a float matrix, as tests/test_lda_gpu.py bounds them

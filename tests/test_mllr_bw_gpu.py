"""mllr --networks (csrc/mllr.cc, csrc/aku/main_mllr.cc): CMLLR statistics from Baum-Welch posteriors over the recipe's
HMM networks on the device, against tools/mllr_bw_restate.py.

Fixture: three speakers, one 2 s recording each (tests/test_mllr_gpu.py's varied audio), the production feature chain
with three cepstra (12 dimensions: four windows of 55 frames a speaker are 220 frames, more than (D + 1)^2 = 169), 18
states in HMMs of three with broad variances, so that a frame belongs to several pdfs.  Every window has a network of its
own from tools/hmmnet_cases.py: chains of six states, and one fan a speaker.  The restatement runs on the oracle's
double state likelihoods of the engine's own f64 features; the tool runs under AASR_PREC=1 unless a test says otherwise.

Conditions on the inputs, asserted in the fixture on the CPU side: with wide beams every utterance ends OK and its
smallest positive occupancy is above 1e-200 (the device makes no entry where the reference makes one of weight 0); with
default beams max |1 - s_t| is at most 0.02; all three speakers solve, and the restatement from extended statistics
prints the same digits as the one in double but for at most 1 % of the numbers.

Bounds: those of tests/test_mllr_gpu.py's tool tests -- speaker-file numbers may differ from the restatement's by one
unit of the last printed digit, and such flips stay below 1 % of the numbers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmmnet_cases as HC  # noqa: E402
import mllr_bw_restate as MB  # noqa: E402
import test_mllr_gpu as MG  # noqa: E402

pytestmark = pytest.mark.gpu
MR, BW, RS = MB.MR, MB.BW, MB.RS
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
S, PER, COMPS, SPF = 18, 3, 3, 128
SPANS = ((0.05, 0.49), (0.5, 0.94), (0.95, 1.39), (1.4, 1.84))
SPEAKERS = ("s0", "s1", "s2")
PREC64 = {"AASR_PREC": "1"}
WIDE = ("-F", "1e9", "-W", "1e9")


class World:
    pass


def engine_features(capi, w, pcm, block):
    """the engine's own f64 features of a whole recording under a speaker's `transform` parameters (None: as configured)"""
    ft = capi.Feat(w.cfg_text)
    if block is not None:
        ft.set_parameters("transform", "{\n%s}\n" % block)
    return ft.run(pcm, 0, w.T, dtype=np.float64)


def build_world(capi, oracle, d, features=engine_features):
    w = World()
    w.dir = d
    rng = np.random.default_rng(17)
    w.cfg_text = synth.make_feature_config(dim_cep=3)
    w.D = D = 12
    w.cfg = str(d / "f.cfg")
    open(w.cfg, "w").write(w.cfg_text)
    w.fr = 125.0
    w.windows = [tuple(capi.recipe_frame_limits(a, b, w.fr)) for a, b in SPANS]
    assert [b - a for a, b in w.windows] == [55] * 4, w.windows
    w.pcm, w.wav = {}, {}
    for i, spk in enumerate(SPEAKERS):
        w.pcm[spk] = MG.varied_audio(16000 * 2, seed=300 + i)
        w.wav[spk] = str(d / (spk + ".wav"))
        MG.write_wav(w.wav[spk], w.pcm[spk])
    w.T = 240                                                        # the frames taken of every recording (the windows end at 230)
    # input speaker files: feature mode -- s1 comes with a transform of its own (the composition), the others with none
    old_A = (np.eye(D) + 0.05 * rng.standard_normal((D, D))).astype(np.float32)
    old_b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    w.blocks = {"s1": "    matrix %s\n    bias %s\n" % (MG.vec(old_A), MG.vec(old_b))}
    old = [np.array(l.split()[1:], np.float32) for l in w.blocks["s1"].strip().split("\n")]   # as the file's digits read
    w.old = {"s1": (old[0].reshape(D, D), old[1])}
    text = "speaker default\n{\n  feature transform\n  {\n  }\n}\n"
    text += "speaker s1\n{\n  feature transform\n  {\n%s  }\n}\n" % w.blocks["s1"]
    open(str(d / "fea.spkc"), "w").write(text)
    open(str(d / "model.spkc"), "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    # the frames of both modes: feature mode under the speaker's input transform, model mode as configured
    # (a speaker without a block of its own takes the default speaker's empty one: no matrix, no bias)
    w.fea = {True: {spk: features(capi, w, w.pcm[spk], w.blocks.get(spk, "")) for spk in SPEAKERS}}
    w.fea[False] = {spk: features(capi, w, w.pcm[spk], None) for spk in SPEAKERS}
    assert all(len(x) == w.T for x in w.fea[True].values())
    allf = np.concatenate([w.fea[False][spk] for spk in SPEAKERS])
    G = COMPS * S
    mean, var, off, idx, mw = synth.make_model(D=D, G=G, S=S, comps=COMPS, seed=31)
    # a model the data does not fit as it is: means around the frames of a shifted, scaled copy; broad variances keep the
    # state posteriors soft
    mean[:] = 1.2 * allf[rng.integers(0, len(allf), G)] + 0.4 + 0.3 * rng.standard_normal((G, D))
    var[:] = rng.uniform(3.0, 8.0, var.shape) * allf.var(0)[None, :]
    w.model = (mean, var, off, idx, mw)
    w.base = str(d / "m")
    oracle.write_gk(w.base + ".gk", mean, var)
    oracle.write_mc(w.base + ".mc", off, idx, mw)
    oracle.write_ph(w.base + ".ph", S, states_per_hmm=PER)
    w.dm = oracle.DiagModel(mean, var, off, idx, mw)
    w.sp = np.full(S, 0.5)
    # a network per (speaker, window): chains of six states, the third window of every speaker a fan
    w.texts, w.nets, w.lines = {}, {}, []
    for i, spk in enumerate(SPEAKERS):
        for j in range(4):
            if j == 2:
                t = HC.fan(S, 3, 3, seed=40 + i)
            else:
                t = HC.chain([int(s) for s in rng.choice(S, 6, replace=False)])
            w.texts[spk, j] = t
            w.nets[spk, j] = str(d / ("%s_%d.hmmnet" % (spk, j)))
            open(w.nets[spk, j], "w").write(t)
            w.lines.append((spk, j, w.nets[spk, j]))
    w.recipe = write_recipe(w, "all.rcp", w.lines)
    return w


def write_recipe(w, name, lines, key="hmmnet"):
    path = str(w.dir / name)
    with open(path, "w") as f:
        for spk, j, net in lines:
            f.write("audio=%s %s=%s start-time=%s end-time=%s speaker=%s\n" % (w.wav[spk], key, net, SPANS[j][0], SPANS[j][1], spk))
    return path


def entries_with_retries(net, ll, fw, bw, viterbi=False):
    """aku/mllr.cc:87-102: up to five attempts, attempt k with backward beam k x bw; -> the last attempt's entries, k"""
    for k in range(1, 6):
        e = BW.entries(net, ll, fw, k * bw, 1.0, viterbi)
        if e["status"] != RS.FAILED_BACKWARD:
            break
    return e, k


def restate(w, feature_mode, lines=None, fw=1e9, bw=1e9, viterbi=False, extended=True):
    """per speaker the statistics and W of mllr --networks over its lines (default: the fixture's), in double"""
    out = {}
    for spk in SPEAKERS:
        mine = [(j, net) for s_, j, net in (lines or w.lines) if s_ == spk]
        if not mine:
            continue
        x_all = w.fea[feature_mode][spk]
        ll_all = w.dm.score(x_all)
        utts, xs = [], []
        for j, net in mine:
            a, b = w.windows[j]
            e, k = entries_with_retries(HC.parse(open(net).read(), w.sp), ll_all[a:b], fw, bw, viterbi)
            e["attempts"] = k
            utts.append(e)
            xs.append(x_all[a:b])
        x = np.concatenate(xs)
        row0 = np.concatenate([[0], np.cumsum([len(q) for q in xs])])[:-1]
        lists = MB.frame_lists(utts, row0, len(x))
        G, k_, beta = MB.collect(w.model, x, lists)
        o = dict(utts=utts, lists=lists, x=x, beta=beta, W=MR.solve(G, k_, beta),
                 lls=sum(e["result"].forward_total for e in utts if e["status"] == RS.OK))
        if extended:
            o["We"] = MR.solve(*[np.asarray(q, np.float64) for q in MB.collect(w.model, x, lists, extended=True)])
        out[spk] = o
    return out


def check_conditions(w):
    total = selfflips = 0
    for mode in (True, False):
        want = restate(w, mode)
        for spk, o in want.items():
            for e in o["utts"]:
                assert e["status"] == RS.OK and e["attempts"] == 1 and e["min_positive_occ"] > 1e-200, (spk, e["min_positive_occ"])
            assert len(o["x"]) > (w.D + 1) ** 2
            assert np.mean([len(l) for l in o["lists"]]) > 1.5       # Baum-Welch: a frame belongs to several pdfs
            old = w.old.get(spk, (None, None)) if mode else (None, None)
            A, b = MR.compose(o["W"], *old)
            Ae, be = MR.compose(o["We"], *old)
            selfflips += MG.count_flips(MG.fmt(Ae), MG.fmt(A)) + MG.count_flips(MG.fmt(be), MG.fmt(b))
            total += A.size + b.size
            print("%s %s: largest |W| %.3g, entries a frame %.2f, smallest occupancy %.3g" %
                  ("feature" if mode else "model", spk, np.abs(o["W"]).max(), np.mean([len(l) for l in o["lists"]]),
                   min(e["min_positive_occ"] for e in o["utts"])))
        w.want_wide = w.__dict__.get("want_wide", {})
        w.want_wide[mode] = want
    print("the restatement from extended statistics against the one in double: %d flips of %d numbers" % (selfflips, total))
    assert selfflips <= 0.01 * total
    dflt = restate(w, True, fw=15.0, bw=200.0, extended=False)
    dev = max(e["max_dev"] for o in dflt.values() for e in o["utts"])
    print("default beams: max |1 - s_t| %.3g" % dev)
    assert all(e["status"] == RS.OK for o in dflt.values() for e in o["utts"]) and dev <= 0.02
    w.want_default = dflt


@pytest.fixture(scope="module")
def world(capi, oracle, tmp_path_factory):
    w = build_world(capi, oracle, tmp_path_factory.mktemp("mllr_bw"))
    check_conditions(w)
    return w


def run_tool(w, spkc, out, *extra, recipe=None, env=PREC64, networks=True):
    cmd = [os.path.join(BIN, "mllr"), "-b", w.base, "-c", w.cfg, "-r", recipe or w.recipe, "-S", str(w.dir / spkc), "-o", out,
           "-i", "1"] + (["--networks"] if networks else []) + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def flips_against(w, got, want, feature_mode):
    flips = total = 0
    for spk, o in want.items():
        if feature_mode:
            A, b = MR.compose(o["W"], *w.old.get(spk, (None, None)))
            flips += MG.count_flips(got[spk]["matrix"], MG.fmt(A)) + MG.count_flips(got[spk]["bias"], MG.fmt(b))
            total += A.size + b.size
        else:
            assert got[spk]["unitmode"] == ["UNIT_NO"]
            flips += MG.count_flips(got[spk]["w1"], MG.fmt(o["W"]))
            total += o["W"].size
    print("flips %d of %d numbers" % (flips, total))
    assert flips <= 0.01 * total
    return flips


def test_feature_mode_against_the_restatement(world, tmp_path):
    w = world
    out = str(tmp_path / "out.spkc")
    r = run_tool(w, "fea.spkc", out, "-M", "transform", *WIDE)
    assert r.stdout == "s0: s1: s2: "
    assert r.stderr.count("Calculating transform for s") == 3 and r.stderr.count("Processing file: ") == 12
    assert "Warning" not in r.stderr and "Could not" not in r.stderr, r.stderr
    want = w.want_wide[True]
    got = MG.parse_spkc(open(out).read())
    assert set(got) == {"default", "s0", "s1", "s2"}
    flips_against(w, got, want, True)
    total = [l for l in r.stderr.splitlines() if l.startswith("Total log likelihood: ")]
    lls = sum(o["lls"] for o in want.values())
    assert len(total) == 1 and abs(float(total[0].split(": ")[1]) - lls) <= 1e-6 + 1e-12 * abs(lls), (total, lls)
    assert len([l for l in r.stderr.splitlines() if l.startswith("Largest |1 - sum of PDF probabilities| of a frame: ")]) == 1
    run_tool(w, "fea.spkc", str(tmp_path / "again.spkc"), "-M", "transform", *WIDE)          # a second run: the same file
    assert open(str(tmp_path / "again.spkc")).read() == open(out).read()
    halves = ""
    for k in (1, 2):                                                 # -B 2 -I 1 / 2 concatenated as train.pl does with cat
        run_tool(w, "fea.spkc", str(tmp_path / ("h%d.spkc" % k)), "-M", "transform", *WIDE, "-B", "2", "-I", str(k))
        halves += open(str(tmp_path / ("h%d.spkc" % k))).read()
    assert "utterance" not in halves and halves.count("speaker default") == 1
    assert halves == open(out).read()


def test_a_single_path_network_is_the_phn_mode_byte_for_byte(world, capi, tmp_path):
    """networks without self loops, one arc a frame: every frame has one pdf and occ / s_t is exactly 1.0, so the weighted
    pass leaves the plain pass's bytes and the speaker file of mllr --networks is that of mllr over the .phn files that
    state the same path and windows"""
    w = world
    rng = np.random.default_rng(5)
    topo = capi.Topology(w.base + ".ph")
    net_lines, phn_lines = [], []
    for spk in SPEAKERS:
        for j, (a, b) in enumerate(w.windows):
            states = np.repeat(rng.integers(0, S, 40), rng.integers(2, 6, 40))[:b - a].tolist()
            assert len(states) == b - a
            text = "#FSTBasic MaxPlus\nI 0\nF %d\n" % len(states)
            text += "".join("T %d %d %d\n" % (i, i + 1, 2 * s + (0 if i + 1 < len(states) and states[i + 1] == s else 1))
                            for i, s in enumerate(states))
            net, phn = str(tmp_path / ("%s_%d.hmmnet" % (spk, j))), str(tmp_path / ("%s_%d.phn" % (spk, j)))
            open(net, "w").write(text)
            with open(phn, "w") as f:
                for i, s in enumerate(states):
                    f.write("%d %d h%d.%d\n" % ((a + i) * SPF, (a + i + 1) * SPF, s // PER, s % PER))
            seg = capi.stats_read_segmentation(topo, phn, w.fr, a, b, w.T, False)
            assert seg[0] == a and seg[1].tolist() == states
            net_lines.append((spk, j, net))
            phn_lines.append((spk, j, phn))
    rn = write_recipe(w, "single_net.rcp", net_lines)
    rp = write_recipe(w, "single_phn.rcp", phn_lines, key="transcript")
    a, b = str(tmp_path / "a.spkc"), str(tmp_path / "b.spkc")
    run_tool(w, "fea.spkc", a, "-M", "transform", *WIDE, recipe=rn)
    run_tool(w, "fea.spkc", b, "-M", "transform", recipe=rp, networks=False)
    got = MG.parse_spkc(open(a).read())
    assert set(got) == {"default", "s0", "s1", "s2"} and all("matrix" in got[s] for s in SPEAKERS)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_viterbi_mode(world, tmp_path):
    w = world
    want = restate(w, True, viterbi=True, extended=False)
    assert all(len(l) == 1 and l[0][1] == 1.0 for o in want.values() for l in o["lists"])
    out = str(tmp_path / "vit.spkc")
    run_tool(w, "fea.spkc", out, "-M", "transform", "--segmode", "vit", *WIDE)
    flips_against(w, MG.parse_spkc(open(out).read()), want, True)


def test_model_mode(world, tmp_path):
    w = world
    out = str(tmp_path / "model.spkc")
    r = run_tool(w, "model.spkc", out, *WIDE)
    want = w.want_wide[False]
    lines = r.stdout.split("\n")
    assert "No regression tree used" in r.stderr
    for l, spk in zip(lines, SPEAKERS):
        assert l == "%s: %g frames, 1 transform matrices" % (spk, want[spk]["beta"])
    flips_against(w, MG.parse_spkc(open(out).read()), want, False)


def loglik(w, capi, gmm, spk, path):
    """the forward totals of the speaker's networks on the engine's own scores of the features under the speaker file
    `path`, plus frames x log |det A| of the transform it carries"""
    keys = MG.parse_spkc(open(path).read()).get(spk, {})
    logdet = np.linalg.slogdet(np.array(keys["matrix"], np.float64).reshape(w.D, w.D))[1] if "matrix" in keys else 0.0
    ft = capi.Feat(w.cfg_text)
    sc = capi.SpeakerConfig(ft)
    sc.read_file(path)
    sc.set_speaker(spk)
    ll = gmm.score_f64(ft.run(w.pcm[spk], 0, w.T, dtype=np.float64))
    del sc
    total = 0.0
    for j, (a, b) in enumerate(w.windows):
        r = RS.forward_backward(HC.parse(w.texts[spk, j], w.sp), ll[a:b], 1e9, 1e9)
        assert r.status == RS.OK
        total += r.forward_total + (b - a) * logdet
    return total


def test_default_precision_and_default_beams(world, capi, tmp_path):
    """no bound fixed in advance on the numbers: the difference from the AASR_PREC=1 run is printed; asserted is the
    closed loop -- for every speaker the Baum-Welch likelihood of its networks under the written transform, log |det A|
    included, exceeds the one under the input file"""
    w = world
    out, ref = str(tmp_path / "dflt.spkc"), str(tmp_path / "f64.spkc")
    r = run_tool(w, "fea.spkc", out, "-M", "transform", env=None)
    run_tool(w, "fea.spkc", ref, "-M", "transform")
    assert "Warning: Sum of PDF probabilities" not in r.stderr
    got, want = MG.parse_spkc(open(out).read()), MG.parse_spkc(open(ref).read())
    worst = 0.0
    for spk in SPEAKERS:
        for key in ("matrix", "bias"):
            worst = max(worst, MR.rel_err(np.array(got[spk][key], np.float64), np.array(want[spk][key], np.float64)))
    print("default precision against AASR_PREC=1, default beams: largest relative difference of A, b %.3g" % worst)
    flips_against(w, want, w.want_default, True)                     # (the AASR_PREC=1 run at default beams, as a by-product)
    gmm = capi.Gmm.from_files(w.base + ".gk", w.base + ".mc", w.base + ".ph")
    for spk in SPEAKERS:
        before, after = loglik(w, capi, gmm, spk, str(w.dir / "fea.spkc")), loglik(w, capi, gmm, spk, out)
        print("%s: log-likelihood with log |det A| %.6f -> %.6f" % (spk, before, after))
        assert after > before
    gmm.close()


def test_retries_and_giving_up(world, tmp_path):
    """One line fails its backward pass once (tests/test_stats_bw_gpu.py's decoy branch: next to the real path of three
    states a branch longer than the window that holds every frame's best state), one line -- a chain longer than its
    window -- fails five times.  W is taken from the restatement's pruning-margin report.  The given-up line adds
    nothing: the speaker's transform is the restatement's without it."""
    w = world
    spk = "s0"
    a, b_ = w.windows[0]
    ll = w.dm.score(w.fea[True][spk])[a:b_]
    order = np.argsort(ll.sum(axis=0))
    real = [int(order[0]), int(order[1]), int(order[2])]
    n = b_ - a
    decoy = [int(ll[max(0, min(n - 1, n - 1 - k))].argmax()) for k in range(n + 4, -1, -1)]
    bld = HC.Builder()
    init, fin = bld.node(), bld.node()
    for states in (real, decoy):
        nodes = [bld.node() for _ in states]
        bld.eps(init, nodes[0])
        for i, s in enumerate(states):
            bld.emit(nodes[i], nodes[i], 2 * s)
            bld.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else fin, 2 * s + 1)
    text = bld.text(init, fin)
    net = str(tmp_path / "retry.hmmnet")
    open(net, "w").write(text)
    long_net = str(tmp_path / "long.hmmnet")
    open(long_net, "w").write(HC.chain([s % S for s in range(n + 5)]))
    kept = [(spk, 0, net)] + [(spk, j, w.nets[spk, j]) for j in (1, 2, 3)]
    rnet = HC.parse(text, w.sp)
    chosen = None
    for W in [round(10 * 1.12 ** k, 1) for k in range(40)]:
        r1 = RS.forward_backward(rnet, ll, 1e9, float(W))
        r2 = RS.forward_backward(rnet, ll, 1e9, 2.0 * W)
        if r1.status == RS.FAILED_BACKWARD and r2.status == RS.OK and min(r1.min_margin, r2.min_margin) >= 0.05:
            want = restate(w, True, lines=kept, fw=1e9, bw=float(W), extended=False)[spk]
            others = [e for e in want["utts"][1:]]
            if all(e["status"] == RS.OK and e["attempts"] == 1 and e["result"].min_margin >= 0.05 for e in others):
                chosen = W
                break
    assert chosen, "no backward beam separates the two runs on this fixture"
    W = chosen
    assert want["utts"][0]["attempts"] == 2 and want["utts"][0]["status"] == RS.OK
    recipe = write_recipe(w, "retry.rcp", [kept[0], (spk, 0, long_net)] + kept[1:])
    out = str(tmp_path / "r.spkc")
    r = run_tool(w, "fea.spkc", out, "-M", "transform", "-F", "1e9", "-W", str(W), recipe=recipe)
    warn = [l for l in r.stderr.splitlines() if l.startswith("Warning: Backward phase failed, increasing beam to ")]
    assert warn == ["Warning: Backward phase failed, increasing beam to %.1f" % (2.0 * W)] + \
        ["Warning: Backward phase failed, increasing beam to %.1f" % (k * W) for k in (2, 3, 4, 5)], r.stderr
    assert r.stderr.count("Could not run Baum-Welch for file %s\n" % w.wav[spk]) == 1
    assert r.stderr.count("The HMM network may be incorrect or initial beam too low.\n") == 1
    assert r.stdout == "s0: "
    got = MG.parse_spkc(open(out).read())
    flips_against(w, got, {spk: want}, True)

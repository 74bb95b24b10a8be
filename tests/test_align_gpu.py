"""The forced aligner on the device (csrc/align_viterbi.hip) and the native align tool:
1. with wide beams and one window it finds the path of a plain global Viterbi over the oracle's
   likelihoods (no reference binary involved);
2. the align tool writes the same .phn files, byte for byte, and prints the same log-likelihoods and
   retry messages as oracle/_ref/align_refmain (aku/align.cc + Viterbi.cc + Lattice.cc + PhnReader.cc
   linked with the engine), over windows and moves, --phoseg, --no-force-end, start/end times, -S, a
   topology with skip transitions and unequal probabilities, and beams tight enough to retry;
3. 300 utterances in one batch equal 300 single-utterance searches and the plain Viterbi;
4. edge cases: a one-frame utterance and a transcript longer than the utterance.
The windowed search itself -- ring wraps, moves, both beams, retries, ties, float64 rows -- is compared with a plain
restatement at the kernel's interface in tests/test_align_windows_gpu.py."""
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from viterbi_restate import global_viterbi  # noqa: E402
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
REFBIN = os.path.join(ROOT, "oracle", "_ref")

pytestmark = pytest.mark.gpu

N_HMM, PER = 12, 3


def write_ph(path, n_hmm=N_HMM):
    """3-state HMMs, pdf = 3 h + j, unequal probabilities, a skip from state 0 to state 2 and one from
    state 1 straight into the next HMM on every third HMM."""
    rng = np.random.default_rng(5)
    with open(path, "w") as f:
        f.write("PHONE\n%d\n" % n_hmm)
        for h in range(n_hmm):
            f.write("%d 5 h%d\n" % (h + 1, h))
            f.write("-1 -2 %d %d %d\n" % (3 * h, 3 * h + 1, 3 * h + 2))
            f.write("0 1 2 1.0\n1 0\n")
            a = rng.uniform(0.3, 0.8)
            if h % 3 == 0:
                f.write("2 3 2 %.4f 3 %.4f 4 %.4f\n" % (a, (1 - a) * 0.7, (1 - a) * 0.3))
                b = rng.uniform(0.3, 0.8)
                f.write("3 3 3 %.4f 4 %.4f 1 %.4f\n" % (b, (1 - b) * 0.8, (1 - b) * 0.2))
            else:
                f.write("2 2 2 %.4f 3 %.4f\n" % (a, 1 - a))
                b = rng.uniform(0.3, 0.8)
                f.write("3 2 3 %.4f 4 %.4f\n" % (b, 1 - b))
            c = rng.uniform(0.3, 0.8)
            f.write("4 2 4 %.4f 1 %.4f\n" % (c, 1 - c))


def _write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def topo_tables(topo, n_states):
    """transitions per state as lists of (offset, log prob as float32)"""
    out = []
    for s in range(n_states):
        out.append([(o, np.float32(np.log(p))) for o, p in topo.transitions(s)])
    return out


@pytest.fixture(scope="module")
def model(capi, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("align")
    S = N_HMM * PER
    cfg_text = synth.make_feature_config()
    cfg = str(d / "f.cfg")
    open(cfg, "w").write(cfg_text)
    pcm = synth.make_audio(16000 * 4, seed=81)
    ft = capi.Feat(cfg_text)
    T = ft.last_frame(len(pcm)) + 1
    fea = ft.run(pcm, 0, T, dtype=np.float64)
    rng = np.random.default_rng(19)
    G = 4 * S
    mean, var, off, idx, w = synth.make_model(D=39, G=G, S=S, comps=3, seed=29)
    mean[:] = fea[rng.integers(0, T, G)] + 0.3 * rng.standard_normal((G, 39))
    var[:] = rng.uniform(0.6, 1.6, var.shape)
    base = str(d / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    write_ph(base + ".ph")
    topo = capi.Topology(base + ".ph")
    return dict(dir=d, cfg=cfg, cfg_text=cfg_text, base=base, arrays=(mean, var, off, idx, w), S=S, topo=topo,
                fea=fea)


def test_topology_state_index_is_checked_against_the_model(capi, model, tmp_path):
    mean, var, off, idx, w = model["arrays"]
    small = capi.Gmm.from_arrays(mean, var, off[:31], idx[:off[30]], w[:off[30]])   # 30 states, the .ph needs 36
    with pytest.raises(capi.AasrError) as e:
        model["topo"].validate(small)
    assert "h10" in str(e.value)
    model["topo"].validate(capi.Gmm.from_arrays(mean, var, off, idx, w))


def _scores(capi, model, frames):
    import torch
    gmm = capi.Gmm.from_arrays(*model["arrays"])
    gmm.set_precision(0)
    ll = gmm.score(frames.astype(np.float32))
    return gmm, ll, torch.from_numpy(ll).cuda()


def test_matches_a_plain_viterbi(capi, oracle, model):
    """wide beams, swins >= T: the committed path is the global best path over the oracle's
    double-precision likelihoods, the end forced to the last position"""
    import torch
    fea = model["fea"]
    T = fea.shape[0]
    topo = model["topo"]
    rng = np.random.default_rng(3)
    trans = topo_tables(topo, model["S"])
    ll_ref = oracle.DiagModel(*model["arrays"]).score(fea)
    gmm, _, d_ll = _scores(capi, model, fea)
    trs, spans = [], []
    for u in range(4):
        n = int(rng.integers(8, 30))
        trs.append([int(x) for x in rng.integers(0, N_HMM, n)])
        a = int(rng.integers(0, T // 3))
        spans.append((a, int(rng.integers(a + PER * n + 20, T))))
    opts = capi.AlignOptions.defaults(swins=T + 8, beam=1e6, sbeam=100000, maxbeam=1e6)
    res = capi.align_batch(gmm, topo, trs, d_ll, [a for a, _ in spans], [0] * 4, [0] * 4,
                           [b - a for a, b in spans], opts)
    for u, (t, (a, b)) in enumerate(zip(trs, spans)):
        states = [s for h in t for s in topo.hmm_states(h)]
        want = global_viterbi(ll_ref[a:b], states, trans)
        r = res[u]
        assert r["status"] == capi.ALIGN_OK and r["n_fail"] == 0
        assert np.array_equal(r["positions"], want), u
    torch.cuda.synchronize()


def test_batch_equals_single(capi, oracle, model):
    """300 utterances of 1-3000 frames (rows drawn from a long synthetic score matrix) in one batch,
    one window step per call, equal the same utterances searched one at a time."""
    rng = np.random.default_rng(11)
    frames = synth.make_frames(6000, seed=5)
    gmm, ll, d_ll = _scores(capi, model, frames)
    topo = model["topo"]
    trs, row0, eof = [], [], []
    for u in range(300):
        T = 1 if u == 0 else int(rng.integers(1, 3001))
        n = max(1, min(int(rng.integers(1, 120)), T // 4))
        trs.append([int(x) for x in rng.integers(0, N_HMM, n)])
        row0.append(int(rng.integers(0, 6000 - T + 1)))
        eof.append(T)
    opts = capi.AlignOptions.defaults(swins=300, beam=20.0, sbeam=10, maxbeam=500.0)
    batch = capi.align_batch(gmm, topo, trs, d_ll, row0, [0] * 300, [0] * 300, eof, opts, windows=1)
    assert batch[0]["calls"] >= 2
    for u in range(0, 300, 7):
        one = capi.align_batch(gmm, topo, [trs[u]], d_ll, [row0[u]], [0], [0], [eof[u]], opts)[0]
        b = batch[u]
        assert b["status"] == one["status"] and b["n_fail"] == one["n_fail"], u
        assert np.array_equal(b["positions"], one["positions"]), u
        assert b["loglik"] == one["loglik"], u
    assert any(b["status"] == capi.ALIGN_OK and b["n_fail"] == 0 for b in batch)
    # the beams are tight enough that some searches restart from scratch with doubled beams and then finish
    retried = [u for u, b in enumerate(batch) if b["status"] == capi.ALIGN_OK and b["n_fail"] > 0]
    assert retried
    for u in retried[:5]:
        one = capi.align_batch(gmm, topo, [trs[u]], d_ll, [row0[u]], [0], [0], [eof[u]], opts)[0]
        assert np.array_equal(batch[u]["positions"], one["positions"]) and batch[u]["n_fail"] == one["n_fail"], u


def test_batch_equals_plain_viterbi(capi, oracle, model):
    """utterances of 1-3000 frames in one batch, wide beams and one window: the plain Viterbi"""
    rng = np.random.default_rng(13)
    frames = synth.make_frames(3000, seed=6)
    gmm, ll, d_ll = _scores(capi, model, frames)
    ll_ref = oracle.DiagModel(*model["arrays"]).score(frames.astype(np.float32).astype(np.float64))
    topo = model["topo"]
    trans = topo_tables(topo, model["S"])
    trs, row0, eof = [], [], []
    for u in range(24):
        T = 1 if u == 0 else int(rng.integers(2, 3001))
        n = 1 if u == 0 else max(1, min(int(rng.integers(1, 100)), T // 5))
        trs.append([int(x) for x in rng.integers(0, N_HMM, n)] if u else [1])
        row0.append(int(rng.integers(0, 3000 - T + 1)))
        eof.append(T)
    opts = capi.AlignOptions.defaults(swins=3000, beam=1e6, sbeam=1000, maxbeam=1e6)
    res = capi.align_batch(gmm, topo, trs, d_ll, row0, [0] * 24, [0] * 24, eof, opts)
    for u in range(1, 24):
        states = [s for h in trs[u] for s in topo.hmm_states(h)]
        want = global_viterbi(ll_ref[row0[u]:row0[u] + eof[u]], states, trans)
        assert res[u]["status"] == capi.ALIGN_OK, u
        assert np.array_equal(res[u]["positions"], want), u
    # one frame, three states: the forced end is out of range at every beam -> given up, nothing committed
    assert res[0]["status"] == capi.ALIGN_GAVE_UP and len(res[0]["positions"]) == 0


# ------------------------------------------------------------- against the reference aligner --

@pytest.fixture(scope="module")
def world(capi, model):
    if not os.access(os.path.join(REFBIN, "align_refmain"), os.X_OK):
        pytest.skip("oracle/_ref/align_refmain was not built (no reference tree in the build container)")
    d = model["dir"]
    rng = np.random.default_rng(23)
    utts = []
    secs = [3.0, 2.2, 4.1, 1.5, 2.7, 3.3, 0.03, 0.5]
    for i, s in enumerate(secs):
        n = int(16000 * s)
        wav = str(d / ("u%d.wav" % i))
        _write_wav(wav, synth.make_audio(n, seed=90 + i))
        frames = max(1, int(n / 128))
        if i == 6:
            labels = ["h1"]                       # a one-frame-ish utterance, one HMM
        elif i == 7:
            labels = ["h%d" % x for x in rng.integers(0, N_HMM, 40)]   # more states than frames: end unreachable
        else:
            labels = ["h%d" % x for x in rng.integers(0, N_HMM, max(2, frames // 9))]
        tr = str(d / ("u%d.phn" % i))
        if i == 1:   # timed lines with state fields and comments
            lines = []
            for k, l in enumerate(labels):
                for j in range(PER):
                    lines.append("%d %d %s.%d%s" % (k * 384 + j * 128, k * 384 + j * 128 + 128, l, j,
                                                    " word%d" % k if j == 0 else ""))
            open(tr, "w").write("\n".join(lines) + "\n")
        else:
            open(tr, "w").write("".join("%s%s\n" % (l, " c%d" % k if k % 4 == 0 else "") for k, l in enumerate(labels)))
        utts.append((wav, tr, i))
    spk = str(d / "s.spkc")
    with open(spk, "w") as f:
        for name in ("s1", "s2"):
            f.write("speaker %s\n{\n  feature normalization\n  {\n    scale %s\n  }\n}\n"
                    % (name, " ".join("%.3f" % x for x in rng.uniform(0.8, 1.2, 39))))
    return dict(dir=d, utts=utts, spk=spk)


def _recipe(world, tag, times=False, speakers=False):
    lines = []
    for wav, tr, i in world["utts"]:
        out = world["dir"] / ("%s_%d.phn" % (tag, i))
        extra = ""
        if times:   # recipe keys persist from line to line: the other lines reset them
            extra = " start-time=0.512 end-time=2.8" if i == 2 else " start-time=0 end-time=0"
        if speakers:
            extra += " speaker=%s" % ("s1" if i % 2 else "s2")
        lines.append("audio=%s transcript=%s alignment=%s%s" % (wav, tr, out, extra))
    p = world["dir"] / (tag + ".recipe")
    p.write_text("\n".join(lines) + "\n")
    return str(p)


CASES = {
    "default": [],
    "swins64": ["--swins", "64"],
    "swins150": ["--swins", "150"],
    "phoseg": ["--phoseg", "--swins", "150"],
    "noforce": ["--no-force-end", "--swins", "64"],
    "times": ["--swins", "150"],
    "speakers": ["--swins", "150"],
    "tight": ["--beam", "40", "--sbeam", "30", "--maxbeam", "400", "--swins", "150"],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_files_as_the_reference_aligner(capi, model, world, case):
    args = CASES[case]
    if case == "speakers":
        args = args + ["-S", world["spk"]]
    outs = {}
    for tag, exe in (("ref", os.path.join(REFBIN, "align_refmain")), ("eng", os.path.join(BIN, "align"))):
        recipe = _recipe(world, "%s_%s" % (case, tag), times=case == "times", speakers=case == "speakers")
        r = subprocess.run([exe, "-b", model["base"], "-c", model["cfg"], "-r", recipe, "-i", "2"] + args,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (tag, r.stderr[-3000:])
        files = {}
        for _wav, _tr, i in world["utts"]:
            p = world["dir"] / ("%s_%s_%d.phn" % (case, tag, i))
            files[i] = p.read_bytes() if p.exists() else None
        msgs = [l for l in r.stderr.splitlines()
                if re.match(r"(File log likelihood|Total data log likelihood|Too low beams|Have to stop|Restoring original|Processing file)", l)]
        outs[tag] = (files, msgs)
    ref_files, ref_msgs = outs["ref"]
    eng_files, eng_msgs = outs["eng"]
    for i in ref_files:
        assert eng_files[i] == ref_files[i], (case, i, (ref_files[i] or b"")[:400], (eng_files[i] or b"")[:400])
    assert eng_msgs == ref_msgs
    if case == "tight":
        # a search that missed the forced end, restarted with doubled beams and finished -- on an utterance
        # whose end is reachable (u6 and u7 never finish)
        current, failed, retried_ok = None, set(), set()
        for m in ref_msgs:
            if m.startswith("Processing file:"):
                current = m.split()[2]
            elif m.startswith("Too low beams"):
                failed.add(current)
            elif m.startswith("File log likelihood") and current in failed:
                retried_ok.add(current)
        assert any(not f.endswith(("u6.wav", "u7.wav")) for f in retried_ok), ref_msgs
        assert any(m.startswith("Restoring original beam") for m in ref_msgs)

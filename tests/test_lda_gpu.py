"""The native lda tool end to end (csrc/lda.cc, lib/bin/lda) on a handful of short synthetic utterances, a .ph with _ and
__ and random state segmentations, against the pipeline restated in NumPy: the oracle's feature chain at the transform
module's source, the segmentation reader through capi, in-order sums and the NumPy solve (tools/lda_restate.py).

Rows are matched by |cosine| and compared up to sign.  Tolerance, as tests/test_lda_host.py: per input 8 x the distance
between the two reference-side routes (np.linalg.eig on W^-1 B, np.linalg.eigh on the Cholesky-reduced problem), not
below the float the matrix is written in (the configuration holds "%g" values: 6 significant digits, 5e-6 relative)."""
import importlib.util
import os
import subprocess
import wave

import numpy as np
import pytest

from aaltoasr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
pytestmark = pytest.mark.gpu

LABELS = ["_", "__", "a", "b", "c", "e", "f", "d"]     # d: the rare HMM, in one segmentation only
PER, SPF, TD = 3, 128, 12
WRITTEN = 5e-6      # "%g": six significant digits


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LR = _load("lda_restate")


def write_ph(path):
    """3-state left-to-right HMMs, pdf = 3 h + j"""
    with open(path, "w") as f:
        f.write("PHONE\n%d\n" % len(LABELS))
        for h, lab in enumerate(LABELS):
            f.write("%d 5 %s\n-1 -2 %d %d %d\n0 1 2 1.0\n1 0\n" % (h + 1, lab, 3 * h, 3 * h + 1, 3 * h + 2))
            f.write("2 2 2 0.6 3 0.4\n3 2 3 0.6 4 0.4\n4 2 4 0.6 1 0.4\n")


def write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def random_phn(path, rng, n_frames, rare=False):
    """whole HMMs, states in order, from frame 0 past n_frames; `rare`: HMM d appears here (its last state once)"""
    t = 0
    with open(path, "w") as f:
        while t < n_frames:
            h = int(rng.integers(0, len(LABELS) - 1))
            for k in range(PER):
                n = int(rng.integers(2, 7))
                f.write("%d %d %s.%d\n" % (t * SPF, (t + n) * SPF, LABELS[h], k))
                t += n
        if rare:
            for k, n in enumerate((4, 3, 2)):
                f.write("%d %d d.%d\n" % (t * SPF, (t + n) * SPF, k))
                t += n


def lda_config(dim=TD):
    """the production graph up to its normalization, then an undefined lin_transform `lda` of `dim` rows"""
    text = synth.make_feature_config()
    head = text[:text.index("module\n{\n  name transform")]
    return head + "module\n{\n  name lda\n  type lin_transform\n  dim %d\n  sources normalization\n}\n" % dim


@pytest.fixture(scope="module")
def setup(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("lda")
    cfg_text = lda_config()
    open(str(d / "f.cfg"), "w").write(cfg_text)
    write_ph(str(d / "m.ph"))
    ft = capi.Feat(cfg_text)
    rng = np.random.default_rng(19)
    lines = []
    for u in range(4):
        pcm = synth.make_audio(16000 + 3000 * u, seed=300 + u)
        wav, phn, ali = str(d / ("u%d.wav" % u)), str(d / ("u%d.phn" % u)), str(d / ("u%d.ali" % u))
        write_wav(wav, pcm)
        eof = ft.eof_frame(len(pcm))
        # u1's segmentation runs past the audio's end: those frames count nowhere; u3 holds the rare HMM
        random_phn(phn, rng, eof + 30 if u == 1 else eof - 25, rare=(u == 3))
        random_phn(ali, rng, eof - 25)
        lines.append("audio=%s transcript=%s alignment=%s speaker=s%d" % (wav, phn, ali, 1 + u % 2))
    open(str(d / "r.rcp"), "w").write("\n".join(lines) + "\n")
    return dict(dir=d, cfg_text=cfg_text, lines=lines, topo=capi.Topology(str(d / "m.ph")))


def restate(capi, oracle, st, cfg_text, source, td, ophn=False, mingamma=1.0, no_silence=False, warps=None):
    """-> (lda by the NumPy route, tolerance, selected, frames [n x D] and states of the selected frames)"""
    # (the oracle's chain stops before the undefined transform: it takes an identity only where dim == source dim)
    chain = oracle.FeatureChain(cfg_text[:cfg_text.index("module\n{\n  name lda")])
    ft = capi.Feat(cfg_text)
    fr = ft.frame_rate
    S = st["topo"].num_states()
    xs, states = [], []
    for li, line in enumerate(st["lines"]):
        info = dict(kv.split("=", 1) for kv in line.split())
        if warps is not None:
            chain.set_parameters("vtln", {"warp_factor": warps[li]})
        pcm = oracle.read_wav_pcm16(info["audio"])[0]
        seg = capi.stats_read_segmentation(st["topo"], info["alignment" if ophn else "transcript"], fr, 0, 0,
                                           ft.eof_frame(len(pcm)), False)
        start, pdf, _ = seg
        xs.append(chain.generate(pcm, start, len(pdf), source))
        states.append(np.asarray(pdf, np.int32))
    x, states = np.concatenate(xs), np.concatenate(states)
    count = np.bincount(states, minlength=S).astype(np.float64)
    sel = (count >= mingamma).astype(np.int32)
    if no_silence:
        sel[:2 * PER] = 0
    cls = np.where(sel[states] == 1, states, -1).astype(np.int32)
    g, sx, sxx = LR.scatter_in_order(x, cls, S)
    want = LR.solve(g, sx, sxx, sel, 1e6, td)
    other = LR.solve(g, sx, sxx, sel, 1e6, td, route="eigh")
    tol = max(8 * LR.rel_err(LR.match_rows(other, want), want), WRITTEN)
    return want, tol, sel, x[cls >= 0], count, g


def run_lda(st, out, *extra, cfg="f.cfg", dim=TD):
    d = st["dir"]
    cmd = [os.path.join(BIN, "lda"), "-p", str(d / "m.ph"), "-c", str(d / cfg), "-r", str(d / "r.rcp"), "-M", "lda",
           "-d", str(dim), "-w", out, "--mingamma", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def written_matrix(capi, out, rows):
    import re
    text = open(out).read()
    block = text[text.index("name lda"):]
    m = re.search(r"matrix ([^\n]*)", block)
    return np.array(m.group(1).split(), np.float64).reshape(rows, -1), text


def differs(got, other, tol):
    """some row of got has no parallel partner among other's rows within tol (no bijection is asked of unequal results)"""
    unit = lambda m: m / np.linalg.norm(m, axis=1, keepdims=True)
    return float((1 - np.abs(unit(got) @ unit(other).T).max(axis=1)).max()) > tol


def compare(tag, got, want, tol):
    err = LR.rel_err(LR.match_rows(got, want), want)
    print("%s: written matrix %.3g from the restatement (tolerance %.3g)" % (tag, err, tol))
    assert err <= tol


def test_pipeline_against_the_restatement_and_the_whitened_features(capi, oracle, setup, tmp_path):
    out = str(tmp_path / "out.cfg")
    run_lda(setup, out)
    want, tol, sel, x, count, _ = restate(capi, oracle, setup, setup["cfg_text"], "normalization", TD)
    assert sel.sum() == (count > 0).sum() >= (len(LABELS) - 1) * PER
    got, text = written_matrix(capi, out, TD)
    compare("pipeline", got, want, tol)
    # the engine's convention on the written matrix: the largest entry of every row positive
    assert all(row[np.abs(row).argmax()] > 0 for row in got)
    # out.cfg through feacat: the selected frames' covariance is the identity
    d = setup["dir"]
    feats = []
    for li, line in enumerate(setup["lines"]):
        info = dict(kv.split("=", 1) for kv in line.split())
        raw = str(tmp_path / ("u%d.fea" % li))
        r = subprocess.run([os.path.join(BIN, "feacat"), "-c", out, "--raw-output", "-H", info["audio"]],
                           capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = r.stdout
        dim = int(np.frombuffer(data[:4], np.int32)[0])
        fea = np.frombuffer(data[4:], np.float32).reshape(-1, dim).astype(np.float64)
        pcm = oracle.read_wav_pcm16(info["audio"])[0]
        ft = capi.Feat(setup["cfg_text"])
        start, pdf, _ = capi.stats_read_segmentation(setup["topo"], info["transcript"], ft.frame_rate, 0, 0,
                                                     ft.eof_frame(len(pcm)), False)
        feats.append(fea[start:start + len(pdf)])
    y = np.concatenate(feats)
    cov = np.cov(y.T, bias=True)
    dev = float(np.abs(cov - np.eye(TD)).max())
    print("covariance of the projected features - I: %.3g" % dev)
    assert dev <= max(tol, 2e-5)      # float features of a float matrix: 2^-17 relative on sums of 39 products


def test_mingamma_drops_a_state_from_the_sums_and_the_data_mean(capi, oracle, setup, tmp_path):
    """HMM d's last state has 2 frames: --mingamma 3 leaves it out, of the class sums and so of the data mean"""
    out = str(tmp_path / "mg.cfg")
    rare = (len(LABELS) - 1) * PER + 2
    res = capi.run_lda_recipe(setup["cfg_text"], setup["topo"], str(setup["dir"] / "r.rcp"), "lda", TD, out=out,
                              opts=capi.LdaOptions.defaults(mingamma=3.0))
    want, tol, sel, x, count, g = restate(capi, oracle, setup, setup["cfg_text"], "normalization", TD, mingamma=3.0)
    assert count[rare] == 2 and sel[rare] == 0 and sel.sum() == (count >= 3).sum() >= TD + 1
    assert res["state_gamma"][rare] == 0.0                          # the handle received nothing for it
    assert (res["state_gamma"] == g).all() and res["frames"] == count.sum()
    compare("mingamma 3", written_matrix(capi, out, TD)[0], want, tol)
    all_in = restate(capi, oracle, setup, setup["cfg_text"], "normalization", TD)[0]
    assert differs(written_matrix(capi, out, TD)[0], all_in, 10 * tol)


def test_ophn_and_no_silence(capi, oracle, setup, tmp_path):
    out = str(tmp_path / "o.cfg")
    run_lda(setup, out, "-O", "--no-silence")
    want, tol, sel, _, _, _ = restate(capi, oracle, setup, setup["cfg_text"], "normalization", TD, ophn=True,
                                      no_silence=True)
    assert sel[:2 * PER].sum() == 0
    compare("-O --no-silence", written_matrix(capi, out, TD)[0], want, tol)


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
module
{
  name lda
  type lin_transform
  dim 8
  sources merged
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
"""


def test_speaker_vtln_changes_the_source_features(capi, oracle, setup, tmp_path):
    d = setup["dir"]
    open(str(d / "v.cfg"), "w").write(VTLN_CFG)
    open(str(d / "v.spkc"), "w").write(SPKC)
    out = str(tmp_path / "v.cfg")
    run_lda(setup, out, "-S", str(d / "v.spkc"), cfg="v.cfg", dim=8)
    warps = ["0.92" if "speaker=s1" in line else "1.08" for line in setup["lines"]]
    want, tol, _, _, _, _ = restate(capi, oracle, setup, VTLN_CFG, "merged", 8, warps=warps)
    got = written_matrix(capi, out, 8)[0]
    compare("-S vtln", got, want, tol)
    flat = restate(capi, oracle, setup, VTLN_CFG, "merged", 8, warps=["1.0"] * 4)[0]
    assert differs(got, flat, 10 * tol)                             # the warps matter

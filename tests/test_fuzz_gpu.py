"""Fixed-seed slices of the randomised parity sweeps (tools/fuzz_parity.py, fuzz_features.py, fuzz_fullcov.py, fuzz_recipe.py, fuzz_speakers.py)
as part of the suite, so that a discrepancy found by a sweep can never sit in a scratch log:
every random model / feature graph of these seeds must agree with the oracle -- scores within
1e-4 wherever the reference's float storage can hold the likelihood (below its flush point,
where the LNA output is the floor whatever the value, the engine's value must flush too), clustered
exact-evaluation counts bit for bit, model-side CMLLR (one global or per-class transforms, plain
and clustered) likewise, feature modules to the per-module tolerance.  Seed 1 is
the sweep whose iteration 26 had differing cluster counts in round 1 (tied empty clusters); seed
104 (iterations 0..249) holds the round-2 find: a one-dimensional model with kappa 416 and a frame
12 sigma out, 1.18e-4 in the expanded form until the 2-norm conditioning limit routed it."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# seed 3002 (iterations 0..299) holds round 3's find: a one-dimensional model, 8.85e-5 off with the two-term fp16 form at
# kappa2 <= 80 (no averaging over dimensions); models of fewer than 8 dimensions now get a limit of 45 and this one takes
# the three-term form
@pytest.mark.parametrize("seed,n", [(1, 40), (7, 25), (20260928, 25), (104, 250), (3002, 300)])
def test_scoring_sweep(capi, oracle, seed, n):
    worst, fails = _load("fuzz_parity").run(seed, n)
    assert not fails, "\n".join(fails)
    assert any(k.startswith("clustered") for k in worst) and any("layouts=4" in k for k in worst)
    assert any(k.startswith("cmllr") for k in worst) and "cmllr clustered refused" not in worst
    assert worst["f64"] <= 1e-12 and worst.get("f64 clustered", 0.0) <= 1e-12       # AASR_PREC_F64: the oracle's values
    assert worst.get("f64 cmllr", 0.0) <= 1e-11
    assert max(v for k, v in worst.items() if k.endswith("(ll > -104)")) <= 1e-4


@pytest.mark.parametrize("seed,n", [(1, 40), (5, 40)])
def test_feature_graph_sweep(capi, oracle, seed, n):
    worst, fails = _load("fuzz_features").run(seed, n)
    assert not fails, "\n".join(fails)
    assert {"fft", "mel", "dct", "delta", "merge"} <= set(worst)


@pytest.mark.parametrize("seed,n", [(1, 60), (3, 40)])
def test_full_covariance_sweep(capi, oracle, seed, n):
    """tools/fuzz_fullcov.py: random full-covariance pools (spectra over two decades, non-SPD entries, ragged /
    tied / zero-weight mixtures), both precisions, against oracle.FullModel."""
    worst, fails = _load("fuzz_fullcov").run(seed, n)
    assert not fails, "\n".join(fails)
    assert worst["refused"] <= 1 and worst["full prec=0"] <= 1e-4 and worst["full prec=3"] <= 1e-4


@pytest.mark.parametrize("seed,n", [(11, 60), (12, 60)])
def test_full_covariance_sweep_over_feature_scales(capi, oracle, seed, n):
    """The same sweep with the pools moved to other units (feature standard deviations 0.01 ... 100, i.e. variances up to
    10^4): coefficients ~ 1 / scale against frame components ~ scale.  Without per-column scales the two-term fp16 rows'
    `lo` terms are subnormals there (3e-8 absolute, times the other operand); with them a pool scores as its normalised
    twin does.  The pools must still GET the two-term rows (a refusal would pass trivially)."""
    mod = _load("fuzz_fullcov")
    worst, fails = mod.run(seed, n, scales=True)
    assert not fails, "\n".join(fails)
    # (pools in very small units are refused at creation as before: their constants, + D log(1 / scale), leave the
    # in-register epilogue no f32 exponent headroom -- DESIGN "full covariance")
    assert worst["full prec=4"] <= 1e-4 and worst["full prec=3"] <= 1e-4 and worst["refused"] <= n // 3


def test_unnormalised_full_covariance_pool_keeps_the_two_term_rows(capi, oracle):
    """configs[4]'s pool in miniature with features of standard deviation 40: AASR_PREC_F16X2 still runs the fp16 factor
    rows (aasr_gmm_effective_precision) and agrees with the oracle as the pool in unit scale does."""
    import numpy as np
    from aaltoasr_amd import synth
    from conftest import assert_ll
    Dc, Gc, Sc = 39, 256, 16
    rng = np.random.default_rng(77)
    mean = rng.standard_normal((Gc, Dc))
    a = rng.standard_normal((Gc, Dc, Dc)) * 0.3
    cov = a @ a.transpose(0, 2, 1) + 0.1 * np.eye(Dc)
    _, _, off, idx, w = synth.make_model(D=Dc, G=Gc, S=Sc, comps=16)
    frames = synth.make_frames(500, D=Dc, seed=78)
    for fs in (1.0, 40.0, 300.0):
        g = capi.Gmm.from_full(mean * fs, cov * fs * fs, off, idx, w)
        g.set_precision(4)
        assert g.effective_precision() == 4, fs
        fr = (frames.astype(np.float64) * fs).astype(np.float32)
        want = oracle.FullModel(mean * fs, cov * fs * fs, off, idx, w).score(fr.astype(np.float64))
        worst = assert_ll(g.score(fr), want, "feature scale %g" % fs)
        assert worst <= 6e-5, (fs, worst)
        g.close()


@pytest.mark.parametrize("seed,n", [(1, 30), (19, 40)])
def test_recipe_driver_sweep(capi, oracle, seed, n):
    """tools/fuzz_recipe.py: random recipes (segment times that stay in force, -B / -I slices, tiny files, 2- / 4-byte,
    -N, clustered models) through aasr_run_recipe against the oracle's phone_probs restatement, and every file
    against the same utterance run alone."""
    worst, fails = _load("fuzz_recipe").run(seed, n)
    assert not fails, "\n".join(fails)
    assert worst["files"] >= n and worst["code"] <= 1 and worst["lp"] <= 1e-4


@pytest.mark.parametrize("seed,n", [(1, 12)])
def test_speaker_configuration_sweep(capi, oracle, seed, n):
    """tools/fuzz_speakers.py: random .spkc files (VTLN, normalisation, feature transform, model-side CMLLR as a
    global transform or per mixture / Gaussian groups, utterance entries, defaults) through phone_probs -S."""
    worst, fails = _load("fuzz_speakers").run(seed, n)
    assert not fails, "\n".join(fails)
    assert worst["files"] >= n and worst["visible"] > 10000 and worst["ll"] <= 1e-4


def test_subspace_pool_sweep(capi, oracle):
    """tools/fuzz_subspace.py: random PCGMM / SCGMM / mixed 'variable' pools (parity unpinned, as tests/test_subspace_gpu.py)."""
    worst, fails = _load("fuzz_subspace").run(2, 30)
    assert not fails, "\n".join(fails)
    assert max(worst["pcgmm"], worst["scgmm"], worst["mixed"]) <= 1e-4


def test_wide_model_sweep(capi, oracle):
    """tools/fuzz_wide.py: models of feature dimension 64 ... 200 (scored as dimension parts) -- plain, AASR_PREC_F64,
    clustered, under one transform or regression classes, clustered under them."""
    worst, fails = _load("fuzz_wide").run(3, 25)
    assert not fails, fails[:5]



@pytest.mark.parametrize("seed,n", [(1, 10), (2, 10)])
def test_fitted_model_sweep(capi, oracle, seed, n):
    """tools/fuzz_fitted.py: models fitted to random mixtures of separated, differently scaled blobs -- the conditioning
    that needs the engine's pivot groups (gmm_plan_engine_parts) -- on the public layout, through the LNA pass on the
    engine's own layout, and under Gaussian clustering over the parts, against the oracle."""
    worst, fails = _load("fuzz_fitted").run(seed, n)
    assert not fails, "\n".join(fails)
    assert worst.get("n parts", 0) >= 3 and worst.get("lna code steps", 0) <= 1


@pytest.mark.parametrize("seed,n", [(1, 12), (5, 12)])
def test_stats_sweep(capi, oracle, seed, n):
    """tools/fuzz_stats.py: the statistics handle on random models of 1 ... 192 dimensions and largest mixtures of 0 ... 118
    (ragged, tied, zero weights), 0 to a few thousand frames per pdf, skipped frames, uneven call cuts, against the
    in-order restatement in double with the tolerances of tests/test_stats_gpu.py.  The seeds' sizes were chosen from the
    models' shapes alone (fuzz_stats.shapes_of: both draw all four sub-block sizes); the shapes that ran are asserted."""
    mod = _load("fuzz_stats")
    worst, fails = mod.run(seed, n)
    assert not fails, "\n".join(fails)
    assert worst["shapes"] == mod.shapes_of(seed, n)
    assert len({s[1] for s in worst["shapes"]}) >= 3 and {s[2] for s in worst["shapes"]} == {0, 1}
    assert len({s[0] for s in worst["shapes"]}) >= 5

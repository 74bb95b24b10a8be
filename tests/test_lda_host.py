"""LDA estimation, the host side (no GPU): the solver, the state selection, the tool's refusals.

Yardstick: tools/lda_restate.py -- lda.cc:380-446 in NumPy with np.linalg.eig (dgeev, the reference's routine) and
np.linalg.inv.  The inputs are per-class sums with a known generalised spectrum (neighbouring eigenvalues of W^-1 B a
factor 1.6 apart, those of the projected covariance a factor 1.35), checked here, so that every eigenvector is well
conditioned.  Rows are matched by |cosine| (a bijection) and compared up to sign.

Tolerance: no figure is picked.  Per input, the distance between two reference-side routes -- np.linalg.eig on W^-1 B
and np.linalg.eigh on the Cholesky-reduced problem -- relative to the largest entry, times 8 for the Jacobi solve's
different rounding path.  Measured when this was written: routes 4.4e-15 (6 dimensions) and 3.4e-9 (39 dimensions,
where the unsymmetric route loses digits to the spectrum's range of 1.6^38); the engine 4.5e-15 and 3.4e-9 from the
np.linalg.eig route, lda Sigma lda^T - I at most 6.9e-16 and 2.0e-10."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LR = _load("lda_restate")


@pytest.mark.parametrize("d,K,td", [(6, 9, 3), (39, 60, 20)])
def test_solver_against_the_restated_solver(capi, d, K, td):
    g, sx, sxx = LR.known_spectrum_case(np.random.default_rng(d), d, K, td)
    sel = np.ones(K, np.int32)
    want, lam, ev, cov = LR.solve(g, sx, sxx, sel, 1e6, td, details=True)
    # the separation that makes the eigenvectors well conditioned
    assert (lam[:td] / lam[1:td + 1] >= 1.5).all() and lam[td] > 0
    evs = np.sort(ev)
    assert (evs[1:] / evs[:-1] >= 1.3).all()
    other = LR.solve(g, sx, sxx, sel, 1e6, td, route="eigh")
    routes = LR.rel_err(LR.match_rows(other, want), want)
    tol = 8 * routes
    got = capi.lda_solve(g, sx, LR.pack(sxx), sel, 1e6, td)
    err = LR.rel_err(LR.match_rows(got, want), want)
    white = float(np.abs(got @ cov @ got.T - np.eye(td)).max())
    print("d %d: routes %.3g, engine %.3g, whitening %.3g (tolerance %.3g)" % (d, routes, err, white, tol))
    assert err <= tol
    assert white <= tol
    # the engine's own convention: rows by falling eigenvalue of the projected covariance, the largest entry positive
    order = np.argsort(-ev, kind="stable")
    unit = lambda m: m / np.linalg.norm(m, axis=1, keepdims=True)
    assert (np.abs(unit(want[order]) @ unit(got).T).argmax(axis=1) == np.arange(td)).all()
    for row in got:
        assert row[np.abs(row).argmax()] > 0


def test_max_gamma_and_the_mask_reach_the_solver(capi):
    d, K, td = 6, 12, 3
    g, sx, sxx = LR.known_spectrum_case(np.random.default_rng(3), d, K, td)
    scale = np.linspace(0.5, 2.0, K)
    g, sx, sxx = g * scale, sx * scale[:, None], sxx * scale[:, None, None]
    sel = np.ones(K, np.int32)
    sel[[2, 7]] = 0
    for mg in (1e6, 500.0):
        want = LR.solve(g, sx, sxx, sel, mg, td)
        tol = 8 * LR.rel_err(LR.match_rows(LR.solve(g, sx, sxx, sel, mg, td, route="eigh"), want), want)
        got = capi.lda_solve(g, sx, LR.pack(sxx), sel, mg, td)
        assert LR.rel_err(LR.match_rows(got, want), want) <= tol
    capped, free = capi.lda_solve(g, sx, LR.pack(sxx), sel, 500.0, td), capi.lda_solve(g, sx, LR.pack(sxx), sel, 1e6, td)
    assert np.abs(capped - free).max() > 1e-6 * np.abs(free).max()


def test_solver_error_returns(capi):
    d, K, td = 6, 9, 3
    g, sx, sxx = LR.known_spectrum_case(np.random.default_rng(1), d, K, td)
    P = LR.pack(sxx)
    sel = np.zeros(K, np.int32)
    sel[:td] = 1                                                   # fewer classes than target_dim + 1
    with pytest.raises(capi.AasrError) as ei:
        capi.lda_solve(g, sx, P, sel, 1e6, td)
    assert ei.value.code == capi.AASR_ERR_INVALID and "selected classes" in ei.value.msg
    # W not positive definite: every class's second moment equals its mean's outer product (no spread)
    flat = LR.pack(np.stack([np.outer(sx[c], sx[c]) / g[c] for c in range(K)]))
    with pytest.raises(capi.AasrError) as ei:
        capi.lda_solve(g, sx, flat, np.ones(K, np.int32), 1e6, td)
    assert ei.value.code == capi.AASR_ERR_INVALID and "not positive definite" in ei.value.msg
    # a projected covariance with a non-positive eigenvalue.  Consistent sums cannot give one (the data covariance is
    # (W + B) / gamma without the cap), so the input is crafted: class 0 gets a negative definite "covariance" and
    # 10^9 frames, which the cap of 400 keeps from W and B but not from the data covariance
    cbar = np.mean([LR.moments(g[c], sx[c], sxx[c])[1] for c in range(K)], axis=0)
    g2, sx2, sxx2 = g.copy(), sx.copy(), sxx.copy()
    m0 = sx[0] / g[0]
    g2[0] = 1e9
    sx2[0] = g2[0] * m0
    sxx2[0] = g2[0] * (np.outer(m0, m0) - 0.5 * cbar)
    with pytest.raises(capi.AasrError) as ei:
        capi.lda_solve(g2, sx2, LR.pack(sxx2), np.ones(K, np.int32), 400.0, td)
    assert ei.value.code == capi.AASR_ERR_INVALID and "non-positive eigenvalue" in ei.value.msg


def test_selection(capi):
    count = np.array([10, 60, 60, 5, 80, 60, 0, 70], np.float64)
    # no cap: every state at or above mingamma
    assert capi.lda_select(count, 50, 3000, 39).tolist() == [0, 1, 1, 0, 1, 1, 0, 1]
    assert capi.lda_select(count, 60.5, 3000, 39).tolist() == [0, 0, 0, 0, 1, 0, 0, 1]
    # the cap: maxmem 10^6 / (8 dim^2) states, largest count first; dim 250 -> 2 per MB
    assert capi.lda_select(count, 50, 1, 250).tolist() == [0, 0, 0, 0, 1, 0, 0, 1]
    # ... and a tie at the cap goes to the lower state index: 80, 70, then the first two of the three 60s
    assert capi.lda_select(count, 50, 2, 250).tolist() == [0, 1, 1, 0, 1, 0, 0, 1]
    assert capi.lda_select(count, 50, 0, 250).tolist() == [0] * 8
    # --no-silence drops its states after the cap was spent on them
    assert capi.lda_select(count, 50, 2, 250, silence=[4, 1]).tolist() == [0, 0, 1, 0, 0, 0, 0, 1]
    with pytest.raises(capi.AasrError):
        capi.lda_select(count, 50, 2, 250, silence=[8])


# ---- the tool's refusals: before the device is opened (this runs without one) ---------------------------------------

PH3 = "PHONE\n3\n" + "".join("%d 3 %s\n-1 -2 %d\n0 1 2 1.0\n1 0\n2 2 2 0.5 1 0.5\n" % (i + 1, lab, i)
                             for i, lab in enumerate(("_", "__", "a")))
CFG = ("module\n{\n  name a\n  type audiofile\n}\nmodule\n{\n  name n\n  type normalization\n  sources a\n}\n"
       "module\n{\n  name lda\n  type lin_transform\n  dim 5\n  sources n\n}\n")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lda_host")
    open(str(d / "m.ph"), "w").write(PH3)
    open(str(d / "nosil.ph"), "w").write(PH3.replace(" __\n", " b\n"))
    open(str(d / "f.cfg"), "w").write(CFG)
    open(str(d / "r.rcp"), "w").write("audio=a.wav transcript=a.phn\n")
    open(str(d / "lines.rcp"), "w").write("audio=a.wav transcript=a.phn start-line=3 end-line=5\n")
    open(str(d / "model.spkc"), "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    return d


def run_tool(files, *extra, ph="m.ph", recipe="r.rcp", dim="5", module="lda"):
    cmd = [os.path.join(BIN, "lda"), "-p", str(files / ph), "-c", str(files / "f.cfg"), "-r", str(files / recipe),
           "-M", module, "-d", dim] + list(extra)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("extra,named", [(["-H"], "-H"), (["--mpv"], "--mpv"), (["--vit"], "--vit")])
def test_refused_options(files, extra, named):
    r = run_tool(files, *extra)
    assert r.returncode == 1 and "exception: lda: " + named in r.stderr and "not supported" in r.stderr, r.stderr
    assert "hip" not in r.stderr.lower()


def test_dimension_module_and_silence_checks_come_before_the_device(files):
    r = run_tool(files, dim="4")
    assert r.returncode == 1 and "exception: lda: -d 4 but module lda has dimension 5" in r.stderr, r.stderr
    r = run_tool(files, module="n")
    assert r.returncode == 1 and "exception: Module n is not a transform module" in r.stderr, r.stderr
    r = run_tool(files, ph="nosil.ph")
    assert r.returncode == 1 and "exception: lda: no HMM __ in the model" in r.stderr, r.stderr
    r = run_tool(files, recipe="lines.rcp")
    assert r.returncode == 1 and "start-line / end-line" in r.stderr, r.stderr
    r = run_tool(files, "-S", str(files / "model.spkc"))
    assert r.returncode == 1 and "speaker files with model transforms" in r.stderr, r.stderr
    for res in (r,):
        assert "hip" not in res.stderr.lower()


def test_an_accepted_command_line_reaches_the_device_and_fails_there(files):
    """the counterpart of the refusals: what is not refused goes on to open the device, and says so when there is none"""
    r = run_tool(files)
    assert r.returncode == 1 and "lda:" not in r.stderr, r.stderr

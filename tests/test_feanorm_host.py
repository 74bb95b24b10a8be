"""Feature normalization and PCA, the host side (no GPU): the PCA solver and the tool's refusals.

Yardstick: tools/feanorm_restate.py -- the covariance's eigenvectors by np.linalg.eigh (dsyev, the reference's routine)
as rows, ascending, and the two scalings of the tool.  The inputs are sample covariances of data with a prescribed,
well-separated spectrum (neighbouring eigenvalues a factor 1.35 apart, checked here), so that every eigenvector is well
conditioned.  Rows correspond by index (both sides ascending) and are compared up to sign.

Tolerance: no figure is picked.  Per input, the distance between two NumPy routes -- np.linalg.eigh of the covariance
and the SVD of the centred data -- relative to the largest entry, times 8 for the Jacobi solve's different rounding
path.  The identities (A S Sigma S A^T diagonal, unit variance or unit determinant) are held to the same bound."""
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


FR = _load("feanorm_restate")


def spectrum_case(d, n=6000, ratio=1.35):
    """-> centred data [n x d], its covariance, a float scale vector"""
    rng = np.random.default_rng(d)
    lam = 3.0 * ratio ** -np.arange(d)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    z, _ = np.linalg.qr(rng.standard_normal((n, d)))             # orthonormal columns: the sample spectrum is lam exactly
    x = (z * np.sqrt(n * lam)) @ Q.T + rng.uniform(-2, 2, d)
    xc = x - x.mean(axis=0)
    scale = rng.uniform(0.3, 2.0, d).astype(np.float32).astype(np.float64)
    return xc, xc.T @ xc / n, scale


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("d", [6, 39])
def test_pca_against_the_restated_solver(capi, d, unit):
    xc, cov, scale = spectrum_case(d)
    want, ev = FR.pca(cov, scale, unit)
    assert (ev[1:] / ev[:-1] >= 1.3).all() and ev[0] > 0          # the separation that conditions the eigenvectors
    other, _ = FR.pca(cov, scale, unit, route="svd", centred=xc)
    routes = FR.rel_err(FR.match_sign(other, want), want)
    tol = 8 * routes
    got, gev = capi.feanorm_pca(cov, scale, unit)
    err = FR.rel_err(FR.match_sign(got, want), want)
    # what the transform promises on normalized features (x - mean) * scale, whose covariance is S Sigma S
    S = np.diag(scale)
    out = got @ S @ cov @ S @ got.T
    off = float(np.abs(out - np.diag(np.diag(out))).max() / np.abs(out).max())
    print("d %d, unit determinant %d: routes %.3g, engine %.3g, off-diagonal %.3g (tolerance %.3g)" % (d, unit, routes, err, off, tol))
    assert err <= tol and off <= tol
    assert np.abs(gev - ev).max() <= tol * ev.max()
    if unit:
        assert abs(abs(np.linalg.det(got)) - 1) <= d * tol
        # rows still by ascending eigenvalue: the projected variances rise
        assert (np.diff(np.diag(out)) > 0).all()
    else:
        assert np.abs(np.diag(out) - 1).max() <= tol
        rayleigh = np.array([r @ cov @ r / (r @ r) for r in got * scale[None, :] * np.sqrt(gev)[:, None]])
        assert (np.diff(rayleigh) > 0).all()                        # rows by ascending eigenvalue
    for row in got:                                                  # the sign convention
        assert row[np.abs(row).argmax()] > 0
    assert got.tobytes() == FR.fix_sign(got).tobytes()
    # without a scale vector: ones
    plain, _ = capi.feanorm_pca(cov, None, unit)
    wplain, _ = FR.pca(cov, None, unit)
    assert FR.rel_err(FR.match_sign(plain, wplain), wplain) <= tol


def test_a_singular_or_indefinite_covariance_is_an_error(capi):
    for cov in (np.diag([2.0, 1.0, 0.0]), np.array([[1.0, 2.0], [2.0, 1.0]])):
        for unit in (False, True):
            with pytest.raises(capi.AasrError) as ei:
                capi.feanorm_pca(cov, None, unit)
            assert ei.value.code == capi.AASR_ERR_INVALID and "non-positive eigenvalue" in ei.value.msg


# ---- the tool's refusals: before the device is opened (this runs without one) ---------------------------------------

CFG = ("module\n{\n  name a\n  type audiofile\n  sample_rate 16000\n}\nmodule\n{\n  name fft\n  type fft\n  sources a\n}\n"
       "module\n{\n  name mel\n  type mel\n  sources fft\n}\nmodule\n{\n  name c\n  type dct\n  dim 12\n  sources mel\n}\n"
       "module\n{\n  name d\n  type delta\n  sources c\n}\nmodule\n{\n  name m\n  type merge\n  sources c d\n}\n"
       "module\n{\n  name n\n  type normalization\n  sources m\n}\n"
       "module\n{\n  name pca\n  type lin_transform\n  sources n\n}\n"
       "module\n{\n  name small\n  type lin_transform\n  sources c\n}\n")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("feanorm_host")
    open(str(d / "f.cfg"), "w").write(CFG)
    open(str(d / "r.rcp"), "w").write("audio=a.wav\n")
    open(str(d / "s.spkc"), "w").write("speaker default\n{\n}\nutterance default\n{\n}\n")
    open(str(d / "model.spkc"), "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    return d


def run_tool(files, *args):
    cmd = [os.path.join(BIN, "feanorm"), "-c", str(files / "f.cfg"), "-r", str(files / "r.rcp")] + list(args)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


def test_the_references_refusals_come_before_the_device(files):
    spk = str(files / "s.spkc")
    cases = [(["--utt", "o.spkc", "-S", spk], "exception: --utt requires the normalization module (--module)"),
             (["-M", "n", "--utt", "o.spkc"], "exception: --utt requires --speakers"),
             (["-M", "m"], "exception: Module m is not a normalization module"),
             (["-M", "n", "-P", "d"], "exception: Module d is not a linear transformation module"),
             (["-M", "nowhere"], "exception: unknown module requested: nowhere"),
             (["-M", "n", "-P", "nowhere"], "exception: unknown module requested: nowhere"),
             (["-M", "n", "-P", "small"],
              "exception: feanorm: the source of module small has dimension 12 but the statistics have dimension 24"),
             (["-M", "n", "-b", "0"], "exception: feanorm: the block size must be at least 1"),
             (["-M", "n", "-S", str(files / "model.spkc")], "speaker files with model transforms")]
    for args, message in cases:
        r = run_tool(files, *args)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert "hip" not in r.stderr.lower(), (args, r.stderr)


def test_the_warning_without_a_module(files, tmp_path):
    r = run_tool(files, "-w", str(tmp_path / "o.cfg"))
    assert "Warning: No --module given, configuration will be written unaltered" in r.stderr, r.stderr
    assert "Warning" not in run_tool(files, "-M", "n", "-w", str(tmp_path / "o.cfg")).stderr


def test_an_accepted_command_line_reaches_the_device_and_fails_there(files):
    """the counterpart of the refusals: what is not refused goes on to open the device, and says so when there is none"""
    r = run_tool(files, "-M", "n", "-P", "pca", "--cov", "-p")
    assert r.returncode == 1 and "feanorm:" not in r.stderr and "Module" not in r.stderr, r.stderr

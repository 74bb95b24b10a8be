"""CMLLR estimation, the host side (no GPU): the solver, the composition with an existing transform, the tool's refusals.

Yardstick: tools/mllr_restate.py -- MllrTrainer::collect_data and MllTrainerComponent::calculate_transform restated in
Python, in the reference's order and in double, the LU steps by LAPACK dgetrf / dgetri (scipy), which is what the
reference's LapackPP calls.

Tolerance of the solver, TOL_W = 5e-13 relative to W's largest entry: measured on the CPU when this was written, the
engine's solver (its own LU) against the restated one on the same statistics: 1.6e-15 (39 dimensions, 16 components,
2 100 frames), 2.8e-15 (16 dimensions), 4.3e-15 (63 dimensions); the restated solver with a plain LU in place of LAPACK:
1.0e-15 / 2.4e-15 / 2.9e-15; the 20 d row rounds do not amplify the rounding.  The bound is the largest figure times a
margin of about 100.  For orientation, double against extended-precision statistics moves W by 2.2e-14 ... 1.1e-13.

The written speaker file is checked in tests/test_mllr_gpu.py: a speaker configuration needs a feature handle, and that
needs a device."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
TOL_W = 5e-13


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MR = _load("mllr_restate")


def known_transform_stats(seed, D, M=4, n=900):
    """frames drawn from the model and pushed through the inverse of a known affine map; the restated statistics"""
    rng = np.random.default_rng(seed)
    model, x, pdf = MR.make_case(rng, D, [M, M, M, 2], [n // 3, n // 3, n // 4, n // 12])
    A = np.eye(D) + 0.15 * rng.standard_normal((D, D)) / np.sqrt(D)
    b = 0.3 * rng.standard_normal(D)
    y = np.ascontiguousarray((x - b) @ np.linalg.inv(A).T)          # A y + b = x
    return model, y, pdf, A, b


@pytest.mark.parametrize("D", [2, 16, 39])
def test_solver_against_the_restated_solver(capi, D):
    model, y, pdf, A, b = known_transform_stats(40 + D, D)
    G, k, beta = MR.collect(model, y, pdf)
    want = MR.solve(G, k, beta)
    got = capi.mllr_solve(G, k, beta)
    err = MR.rel_err(got, want)
    print("D %d: engine against restated solver %.3g; plain LU against LAPACK %.3g" %
          (D, err, MR.rel_err(MR.solve(G, k, beta, lapack=False), want)))
    assert err <= TOL_W
    # it does not lower the auxiliary function
    assert MR.auxiliary(got, G, k, beta) >= MR.auxiliary(np.eye(D, D + 1, 1), G, k, beta)


def test_solver_stops_at_a_zero_pivot(capi):
    D = 3
    model, y, pdf, _, _ = known_transform_stats(7, D, n=200)
    G, k, beta = MR.collect(model, y, pdf)
    G[1] = 0.0
    with pytest.raises(capi.AasrError) as ei:
        capi.mllr_solve(G, k, beta)
    assert ei.value.code == capi.AASR_ERR_INVALID and "zero pivot in G_1" in ei.value.msg
    with pytest.raises(capi.AasrError) as ei:                       # no frames at all: every G_i is zero
        capi.mllr_solve(np.zeros_like(G), np.zeros_like(k), 0.0)
    assert "zero pivot in G_0" in ei.value.msg


def test_composition_and_float_conversion(capi):
    rng = np.random.default_rng(5)
    D = 5
    W = np.concatenate([rng.standard_normal((D, 1)), np.eye(D) + 0.1 * rng.standard_normal((D, D))], 1)
    A, b = capi.mllr_compose(W)
    assert A.dtype == np.float32 and (A == W[:, 1:].astype(np.float32)).all() and (b == W[:, 0].astype(np.float32)).all()
    old_A = (np.eye(D) + 0.2 * rng.standard_normal((D, D))).astype(np.float32)
    old_b = rng.standard_normal(D).astype(np.float32)
    A2, b2 = capi.mllr_compose(W, old_A, old_b)
    wA, wb = MR.compose(W, old_A, old_b)
    # A <- A A_old in double, narrowed once; the in-place product of MllrTrainer.cc:127 leaves b <- b_old
    assert np.abs(A2.astype(np.float64) - W[:, 1:] @ old_A.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(A2).max()
    assert np.abs(A2 - wA).max() <= 2.0 ** -23 * np.abs(wA).max()
    assert (b2 == wb).all() and (b2 == old_b).all()
    with pytest.raises(capi.AasrError):
        capi.mllr_compose(W, old_A, None)


# ---- the tool's refusals: before the device is opened (this runs without one) ---------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mllr_host")
    gk = str(d / "m.gk")
    open(gk, "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(str(d / "m.mc"), "w").write("1\n1 0 1.0\n")
    open(str(d / "m.ph"), "w").write("PHONE\n1\n1 3 a\n-1 -2 0\n0 1 2 1.0\n1 0\n2 2 2 0.5 1 0.5\n")
    open(str(d / "full.gk"), "w").write("1 2 full_cov\n0 0 1 0 0 1\n")
    for e in ("mc", "ph"):
        open(str(d / ("full." + e)), "w").write(open(str(d / ("m." + e))).read())
    open(str(d / "f.cfg"), "w").write("module\n{\n  name a\n  type audiofile\n}\n")
    open(str(d / "r.rcp"), "w").write("audio=a.wav transcript=a.phn speaker=s1\n")
    open(str(d / "lines.rcp"), "w").write("audio=a.wav transcript=a.phn speaker=s1 start-line=3 end-line=5\n")
    open(str(d / "s.spkc"), "w").write("speaker default\n{\n}\n")
    open(str(d / "m.mcs"), "w").write("0\n")
    return d


def run_tool(files, *extra, base="m", recipe="r.rcp"):
    cmd = [os.path.join(BIN, "mllr"), "-b", str(files / base), "-c", str(files / "f.cfg"), "-r", str(files / recipe),
           "-S", str(files / "s.spkc")] + list(extra)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("extra,named", [
    (["-H"], "-H"),
    (["--segmode", "vit"], "--segmode"),
    (["-R", "tree"], "-R"),
    (["--snl"], "--snl"),
    (["--rsamp"], "--rsamp"),
])
def test_refused_options(files, extra, named):
    r = run_tool(files, *extra)
    assert r.returncode == 1 and "exception: mllr: " + named in r.stderr and "not supported" in r.stderr, r.stderr
    assert "hip" not in r.stderr.lower()


def test_tree_generation_is_refused_and_a_bad_unit_rejected(files):
    r = run_tool(files, "-s", str(files / "m.mcs"), "-t", "4")
    assert r.returncode == 1 and "tree generation (-s with -t > 1)" in r.stderr
    r = run_tool(files, "-s", str(files / "m.mcs"), "-t", "4", "-u", "WORD")
    assert r.returncode == 1 and "exception: WORD is not a valid unit identifier" in r.stderr
    for u in ("PHONE", "MIX", "GAUSSIAN"):
        assert "tree generation" in run_tool(files, "-s", str(files / "m.mcs"), "-t", "2", "-u", u).stderr


def test_recipe_line_limits_and_other_pools_are_refused(files):
    r = run_tool(files, recipe="lines.rcp")
    assert r.returncode == 1 and "start-line / end-line" in r.stderr
    r = run_tool(files, base="full")
    assert r.returncode == 1 and "only diagonal Gaussians are supported" in r.stderr and "full_cov" in r.stderr


def test_an_accepted_command_line_reaches_the_device_and_fails_there(files):
    """the counterpart of the refusals: what is not refused goes on to open the device, and says so when there is none"""
    r = run_tool(files, "-M", "t")
    assert r.returncode == 1 and "mllr:" not in r.stderr

"""The native estimate tool end to end with --mllt (lib/bin/estimate, csrc/estimate.cc, csrc/mllt.hip) on a generated
case: 200 Gaussians x 8 dimensions whose covariances B D_g B^T share one mixing matrix B (condition <= 4), D_g diagonal
in [0.5, 2], gamma in [50, 500], ten Gaussians without statistics, mode-3 dumps split over two list entries.

A is compared with the in-order double restatement (tools/estimate_restate.py).  The tolerance is measured on the CPU,
not on the code under test: the restatement runs over the same statistics with the Gaussians in 8 seeded random orders,
s is the largest entry difference between any two of those runs relative to max |A|, and the device may differ by
max(16 s, 2^-24) -- 16 because eight orders under-sample the worst one, 2^-24 because the matrix lands in float."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimate_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

G, D, S, COMPS = 200, 8, 20, 10
NO_STATS = list(range(7, G, 20))
WRITTEN = 5e-6      # "%g": six significant digits


def _config(a_old):
    return ("module\n{\n  name pre\n  type pre\n  dim %d\n}\nmodule\n{\n  name mllt\n  type lin_transform\n  dim %d\n  matrix %s\n"
            "  sources pre\n}\n" % (D, D, " ".join("%.6g" % x for x in a_old.ravel())))


def build_case(tmp):
    """the model, the two dumps, the list and the configuration; the statistics as the tool reads them"""
    rng = np.random.default_rng(2024)
    q1, _ = np.linalg.qr(rng.normal(size=(D, D)))
    q2, _ = np.linalg.qr(rng.normal(size=(D, D)))
    B = (q1 * np.linspace(1.0, 3.0, D)) @ q2
    assert np.linalg.cond(B) <= 4
    prev = os.path.join(tmp, "prev")
    mixtures = [(list(range(COMPS * s, COMPS * (s + 1))), list(rng.uniform(0.5, 1.5, size=COMPS))) for s in range(S)]
    hmms = [("p%d" % h, [2 * h, 2 * h + 1]) for h in range(S // 2)]
    R.write_model(prev, rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, size=(G, D)), mixtures, hmms)
    gamma = rng.uniform(50, 500, size=G)
    mean = rng.normal(size=(G, D))
    r, c = np.tril_indices(D)
    bases = [os.path.join(tmp, "part%d" % n) for n in range(2)]
    parts = [[None] * G, [None] * G]
    for g in range(G):
        if g in NO_STATS:
            continue
        cov = (B * rng.uniform(0.5, 2.0, size=D)) @ B.T
        m2 = (cov + np.outer(mean[g], mean[g]))[r, c]
        f = rng.uniform(0.2, 0.8)
        for n, share in enumerate((f, 1 - f)):
            parts[n][g] = (int(share * gamma[g]) + 1, share * gamma[g], share * gamma[g] * mean[g], share * gamma[g] * m2)
    for n, base in enumerate(bases):
        R.write_gks(base + ".gks", D, R.FULL, parts[n])
        R.write_mcs(base + ".mcs", R.FULL, [(p, [0.5 * gamma[k] if k not in NO_STATS else 0.0 for k in p], -100.0) for p, _w in mixtures])
        R.write_lls(base + ".lls", [("Number of frames", 1000)])
    lst = os.path.join(tmp, "list")
    open(lst, "w").write("\n".join(bases) + "\n")
    a_old = (np.eye(D) + 0.1 * rng.normal(size=(D, D))).astype(np.float32)
    a_old = np.array(["%.6g" % x for x in a_old.ravel()], np.float32).reshape(D, D)    # what the configuration holds
    cfg = os.path.join(tmp, "prev.cfg")
    open(cfg, "w").write(_config(a_old))
    r_model = R.Model(prev)
    for b in bases:
        r_model.add_dump(b)
    return dict(tmp=tmp, prev=prev, bases=bases, lst=lst, cfg=cfg, a_old=a_old, arrays=r_model.mllt_arrays(), r_model=r_model)


@pytest.fixture(scope="module")
def world(capi, tmp_path_factory):
    w = build_case(str(tmp_path_factory.mktemp("estimate_mllt")))
    arrays, prev, lst, cfg = w["arrays"], w["prev"], w["lst"], w["cfg"]
    # the device's A, and the tool's run
    h = capi.Mllt(*arrays[:3], arrays[3].astype(np.int32))
    A, mean_new, var_new = h.estimate(0.1)
    out = os.path.join(w["tmp"], "out")
    res = subprocess.run([os.path.join(BIN, "estimate"), "-b", prev, "-L", lst, "-o", out, "--ml", "--mllt", "mllt", "-c", cfg,
                          "-i", "1"], capture_output=True, text=True, timeout=300)
    w.update(h=h, A=A, mean=mean_new, var=var_new, out=out, res=res)
    return w


def test_tool_runs_and_writes_the_composed_matrix(world):
    assert world["res"].returncode == 0, world["res"].stderr
    assert "MLLT in" in world["res"].stdout
    text = open(world["out"] + ".cfg").read()
    m = re.search(r"matrix ([^\n]*)", text[text.index("name mllt"):])
    got = np.array(m.group(1).split(), np.float64).reshape(D, D)
    want = (world["A"] @ world["a_old"].astype(np.float64)).astype(np.float32).astype(np.float64)
    assert np.abs(got - want).max() <= WRITTEN * np.abs(want).max()
    assert np.abs(got - world["a_old"]).max() > 0.05       # and it is not the old matrix


def test_written_gaussians(world):
    tok = open(world["out"] + ".gk").read().split()
    assert tok[:3] == [str(G), str(D), "variable"]
    rows = np.array(tok[3:]).reshape(G, 1 + 2 * D)
    prev = R.Model(world["prev"])
    ok = world["arrays"][3]
    for g in range(G):
        if ok[g]:
            want = ["%g" % x for x in world["mean"][g]] + ["%g" % x for x in world["var"][g]]
        else:
            want = ["%g" % x for x in prev.mean[g]] + ["%g" % x for x in prev.var[g]]    # unchanged
        assert list(rows[g, 1:]) == want, g
    assert sorted(np.flatnonzero(~ok)) == NO_STATS
    # the mixtures as in the ML update
    world["r_model"].estimate_mixtures()
    assert open(world["out"] + ".mc").read().split() == world["r_model"].mc_tokens()


def test_likelihood_rises_and_covariances_diagonalise(world):
    gamma, sx, sxx, ok = world["arrays"]
    A, h = world["A"], world["h"]
    assert abs(abs(np.linalg.det(A)) - 1) <= 8 * D * 2.0 ** -53
    var0 = np.maximum(h.variances(np.eye(D)), 0.1)
    q1, q0 = R.mllt_objective(A, gamma, world["var"], ok), R.mllt_objective(np.eye(D), gamma, var0, ok)
    print("objective %.6f at the result, %.6f at A = I" % (q1, q0))
    assert q1 >= q0
    cov = R.unpack_lower(R.covariances(gamma, sx, sxx, ok), D)

    def off_mass(T):
        m = np.einsum("ij,gjk,lk->gil", T, cov, T)
        return float((m ** 2).sum() - (np.einsum("gii->gi", m) ** 2).sum())
    print("off-diagonal mass %.6g at the result, %.6g at A = I" % (off_mass(A), off_mass(np.eye(D))))
    assert off_mass(A) < off_mass(np.eye(D))


def test_A_against_the_restatement(world):
    gamma, sx, sxx, ok = world["arrays"]
    want, _mean, _var = R.estimate_mllt(gamma, sx, sxx, ok, 0.1)
    rng = np.random.default_rng(8)
    runs = [want] + [R.estimate_mllt(gamma, sx, sxx, ok, 0.1, order=list(rng.permutation(G)))[0] for _ in range(8)]
    s = max(np.abs(a - b).max() for i, a in enumerate(runs) for b in runs[:i]) / np.abs(want).max()
    err = np.abs(world["A"] - want).max() / np.abs(want).max()
    tol = max(16 * s, 2.0 ** -24)
    print("MLLT A: device against the in-order restatement %.3g; spread s of 8 orders %.3g; tolerance %.3g" % (err, s, tol))
    assert s <= 1e-6, "the fixture is too ill-conditioned"
    assert err <= tol


def test_written_model_loads_and_scores(world, tmp_path):
    rng = np.random.default_rng(3)
    fea = str(tmp_path / "u.fea")
    with open(fea, "wb") as f:
        f.write(struct.pack("=i", D))
        f.write(rng.standard_normal((60, D)).astype(np.float32).tobytes())
    recipe = str(tmp_path / "r.recipe")
    open(recipe, "w").write("audio=%s lna=%s\n" % (fea, tmp_path / "u.lna"))
    r = subprocess.run([os.path.join(BIN, "phone_probs"), "-b", world["out"], "-c", world["out"] + ".cfg", "-r", recipe,
                        "--lnabytes=4", "-N"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(str(tmp_path / "u.lna")) > 60 * S


def test_mode_1_dumps_are_refused(capi, world, tmp_path):
    base = str(tmp_path / "diag")
    gamma, sx, sxx, ok = world["arrays"]
    diag = [i * (i + 1) // 2 + i for i in range(D)]
    R.write_gks(base + ".gks", D, R.ML, [(10, gamma[g], sx[g], sxx[g][diag]) if ok[g] else None for g in range(G)])
    open(base + ".mcs", "w").write(open(world["bases"][0] + ".mcs").read().replace("\n3\n", "\n1\n", 1))
    lst = str(tmp_path / "list")
    open(lst, "w").write(base + "\n")
    out = str(tmp_path / "never")
    res = subprocess.run([os.path.join(BIN, "estimate"), "-b", world["prev"], "-L", lst, "-o", out, "--ml", "--mllt", "mllt",
                          "-c", world["cfg"]], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "stats --mllt" in res.stderr and not os.path.exists(out + ".gk")
    h = capi.Estimate.from_base(world["prev"])
    h.add_dump(base)
    with pytest.raises(capi.AasrError, match="stats --mllt"):
        h.run_mllt()
    # a module that is no transform, and one of another size, are refused as well
    bad = str(tmp_path / "bad.cfg")
    open(bad, "w").write(_config(world["a_old"]).replace("dim %d\n  matrix" % D, "dim %d\n  matrix" % (D - 1)))
    res = subprocess.run([os.path.join(BIN, "estimate"), "-b", world["prev"], "-L", world["lst"], "-o", out, "--ml", "--mllt",
                          "pre", "-c", world["cfg"]], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "Module pre is not a transform module" in res.stderr
    res = subprocess.run([os.path.join(BIN, "estimate"), "-b", world["prev"], "-L", world["lst"], "-o", out, "--ml", "--mllt",
                          "mllt", "-c", bad], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "is not %d x %d" % (D, D) in res.stderr

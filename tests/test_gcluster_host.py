"""Gaussian-pool clustering, the host side (no GPU): the restatement on a case worked by hand, the .gcl bytes, the tool's
refusals -- every one of them is made before the device is opened -- and the loud failure without a device.

Yardstick: tools/gcluster_restate.py (aku/gcluster.cc's diagonal mode in NumPy, operation by operation)."""
import importlib.util
import math
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


GR = _load("gcluster_restate")


def _write_gk(path, mean, var):
    with open(path, "w") as f:
        f.write("%d %d variable\n" % mean.shape)
        for m, v in zip(mean, var):
            f.write("diag " + " ".join(repr(float(x)) for x in list(m) + list(v)) + "\n")


def _tool(capi, *args):
    return subprocess.run([os.path.join(BIN, "gcluster")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_restatement_on_a_case_worked_by_hand():
    """dim 1, six Gaussians of variance 1 at 0 1 2 10 11 12, two clusters.  libc's rand() from seed 1 gives
    1804289383, 846930886, ...: position 0 takes 0 + 1804289383 % 6 = 1, position 1 takes 1 + 846930886 % 5 = 2, so
    the centres start at the means 1 and 2.  Euclidean pass: 0 1 | 2 10 11 12, centres 0.5 and 8.75.  With unit
    variances the divergence is t^2 / 2: 2 moves over (1.125 against 22.78), the map is 0 0 0 1 1 1 from then on, the
    centres 1 and 11."""
    mean = np.array([[0.0], [1.0], [2.0], [10.0], [11.0], [12.0]])
    cov = np.ones((6, 1))
    r = GR.run(mean, cov, 2)
    assert list(r["perm"][:2]) == [1, 2]
    assert [list(m) for m in r["maps"]] == [[0, 0, 1, 1, 1, 1]] + [[0, 0, 0, 1, 1, 1]] * 4
    assert list(r["dists"][0]) == [1.0, 0.0, 0.0, 8.0, 9.0, 10.0]
    assert list(r["dists"][1]) == [0.125, 0.125, 1.125, 0.78125, 2.53125, 5.28125]
    assert list(r["dists"][2]) == [0.5, 0.0, 0.5, 0.5, 0.0, 0.5]
    assert r["lines"] == ["Iteration 1: Average Kullback-Leibler divergence = 1.66146"] + \
        ["Iteration %d: Average Kullback-Leibler divergence = 0.333333" % i for i in (2, 3, 4)]
    assert r["c_mean"].tolist() == [[1.0], [11.0]] and r["c_cov"].tolist() == [[1.0], [1.0]]
    assert r["gcl"] == b"2\n0 0\n1 0\n2 0\n3 1\n4 1\n5 1\n"
    # the gap of Gaussian 2 in the first divergence pass: 1.125 against 6.75^2 / 2
    assert r["gaps"][1][2] == (22.78125 - 1.125) / 22.78125
    # one pair with unequal variances: (ldet_c - ldet_g + (cov_g + t^2) / cov_c - dim) / 2
    idx, dist, gap = GR.assign_kl([[0.0]], [[2.0]], GR.log_det([[2.0]]), [[1.0]], [[4.0]], GR.log_det([[4.0]]), [1])
    assert idx[0] == 0 and dist[0] == (math.log(4.0) - math.log(2.0) + 0.75 - 1.0) / 2.0 and gap[0] == math.inf
    # the centres: sums in Gaussian order times 1 / count, a cluster without members is invalid and all zero
    cm, cc, cl, cv = GR.centres(mean, cov * 2.0, [2, 0, 2, 2, 0, 2], 3)
    assert cm.tolist() == [[12.0 * 0.5], [0.0], [((0.0 + 2.0) + 10.0 + 12.0) * 0.25]] and list(cv) == [1, 0, 1]
    assert cc.tolist() == [[2.0], [0.0], [2.0]] and list(cl) == [math.log(2.0), 0.0, math.log(2.0)]


def test_restatement_rules_of_the_scan():
    """strict < from (1e100, 0): ties go to the lower index, invalid centres are skipped by the divergence pass only,
    nothing usable leaves (0, 1e100) -- also when centre 0 is invalid -- and NaN never wins."""
    mean, cov = np.array([[0.0], [5.0]]), np.ones((2, 1))
    c_mean, c_cov = np.array([[1.0], [-1.0], [1.0]]), np.ones((3, 1))
    zeros = np.zeros(3)
    idx, dist, gap = GR.assign_kl(mean, cov, np.zeros(2), c_mean, c_cov, zeros, [1, 1, 1])
    assert list(idx) == [0, 0] and gap[0] == 0.0 and gap[1] == 0.0         # an exact tie on either side
    idx, dist, _ = GR.assign_kl(mean, cov, np.zeros(2), c_mean, c_cov, zeros, [0, 1, 1])
    assert list(idx) == [1, 2] and list(dist) == [0.5, 8.0]
    idx, dist, _ = GR.assign_kl(mean, cov, np.zeros(2), c_mean, c_cov, zeros, [0, 0, 0])
    assert list(idx) == [0, 0] and list(dist) == [1e100, 1e100]
    idx, dist, _ = GR.assign_euclid(mean, c_mean)
    assert list(idx) == [0, 0] and list(dist) == [1.0, 4.0]
    idx, dist, _ = GR.assign_kl(mean, cov, np.zeros(2), c_mean, np.array([[np.nan], [1.0], [1.0]]), zeros, [1, 1, 1])
    assert list(idx) == [1, 2]


def test_gcl_bytes_and_the_renumbering(oracle, tmp_path):
    valid = np.array([1, 0, 1, 0, 1], np.int32)
    n, of = GR.renumber([4, 0, 2, 2, 4, 0], valid)
    assert n == 3 and list(of) == [2, 0, 1, 1, 2, 0]
    data = GR.gcl_bytes(n, of)
    assert data == b"3\n0 2\n1 0\n2 1\n3 1\n4 2\n5 0\n"
    p = tmp_path / "m.gcl"
    p.write_bytes(data)
    # the engine's reader takes it (its last pair twice, PDFPool::read_clustering's quirk); 3 > 0.3 * 6 would be refused
    nn, pairs = oracle.read_gcl(str(p), 10)
    assert nn == 3 and pairs == [(g, int(c)) for g, c in enumerate(of)] + [(5, 0)]
    with pytest.raises(ValueError):
        GR.renumber([0, 0], np.zeros(2, np.int32))


@pytest.fixture()
def pool(tmp_path):
    rng = np.random.default_rng(5)
    path = str(tmp_path / "p.gk")
    _write_gk(path, rng.standard_normal((8, 3)), np.exp(rng.standard_normal((8, 3))))
    return path, str(tmp_path / "p.gcl")


@pytest.mark.parametrize("args,message", [
    (["-C", "1"], "exception: Invalid number of clusters"),
    (["-C", "4", "-t", "0"], "exception: Invalid number of iterations"),
    (["-C", "9"], "exception: Not enough Gaussians to cluster!"),
    (["-C", "4", "-F"], "-F/--full (full-covariance cluster centres) is not supported"),
    (["-C", "4", "-R", "tree"], "exception: Both tree and model must be given"),
    (["-C", "4", "-b", "base"], "exception: Both tree and model must be given"),
    (["-C", "4", "-R", "tree", "-b", "base"], "-R/--regtree with -b/--base"),
])
def test_tool_refusals_come_before_the_device(capi, pool, args, message):
    gk, out = pool
    r = _tool(capi, "-g", gk, "-o", out, *args)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_tool_missing_gk_and_missing_file(capi, pool):
    gk, out = pool
    r = _tool(capi, "-o", out)
    assert r.returncode == 1 and "option -g --gk=FILE required" in r.stderr
    r = _tool(capi, "-g", gk + ".none", "-o", out, "-C", "4")
    assert r.returncode == 1 and "could not open" in r.stderr
    r = _tool(capi, "-g", gk, "-C", "4")
    assert r.returncode == 1 and "option -o --out=FILE required" in r.stderr


def test_tool_help_lists_the_reference_options(capi):
    r = _tool(capi, "--help")
    assert r.returncode == 0 and r.stdout.startswith("usage: gcluster [OPTION...]\n")
    for opt in ("-h, --help", "-g, --gk=FILE", "-o, --out=FILE", "-F, --full", "-C, --clusters=INT", "-t, --iterations=INT",
                "-R, --regtree=FILE", "-b, --base=BASENAME", "-i, --info=INT"):
        assert opt in r.stdout, opt
    # -t is parsed and checked, and changes nothing in the single-group run: the help says so
    line = [l for l in r.stdout.splitlines() if "--iterations=INT" in l][0]
    assert "four are made whatever is given" in line


def test_library_checks_and_no_cpu_fallback(capi):
    """The option checks of the run entries are the tool's; the step entries refuse bad arguments; and without a
    device every compute entry is AASR_ERR_NO_DEVICE -- with one, the step entry simply computes."""
    rng = np.random.default_rng(2)
    mean, cov = rng.standard_normal((8, 3)), np.exp(rng.standard_normal((8, 3)))
    for C_, msg in ((1, "Invalid number of clusters"), (9, "Not enough Gaussians to cluster!")):
        with pytest.raises(capi.AasrError) as ei:
            capi.gcluster_arrays(mean, cov, clusters=C_)
        assert ei.value.code == capi.AASR_ERR_INVALID and msg in ei.value.msg
    with pytest.raises(capi.AasrError) as ei:
        capi.gcluster_centres(mean, cov, [0, 1, 2, 3, 0, 1, 2, 0], 3)
    assert ei.value.code == capi.AASR_ERR_INVALID and "out of range" in ei.value.msg
    assert capi.gcluster_chunk() >= 1
    ldet = GR.log_det(cov)
    args = (mean, cov, ldet, mean[:3], cov[:3], ldet[:3], [1, 1, 1])
    if capi.lib().aasr_device_count() > 0:
        idx, dist = capi.gcluster_assign(*args)
        want = GR.assign_kl(*args)
        assert (idx == want[0]).all() and (dist == want[1]).all()
        return
    for call in (lambda: capi.gcluster_assign(*args), lambda: capi.gcluster_assign(*args, euclid=True),
                 lambda: capi.gcluster_centres(mean, cov, [0, 1, 2, 2, 0, 1, 2, 0], 3),
                 lambda: capi.gcluster_arrays(mean, cov, clusters=3)):
        with pytest.raises(capi.AasrError) as ei:
            call()
        assert ei.value.code == capi.AASR_ERR_NO_DEVICE

"""Gaussian-pool clustering on the device against tools/gcluster_restate.py (aku/gcluster.cc's diagonal mode in NumPy):
integer maps, and == on float64 distances and centres.  No tolerance anywhere.

What makes exactness a fair demand is checked on the inputs, on the CPU side: in every seeded case every Gaussian's
best and second-best candidate lie more than 1e-9 apart, relative (GR's gap), so no map hangs on a last bit.  Rows
that are duplicated on purpose tie exactly on both sides and are the one exemption, named where it is made.

Shapes are the smallest at which each mechanism can break: one dimension; a pool that is no multiple of the 64
Gaussians of a workgroup; more centres than one chunk (capi.gcluster_chunk()) and one past it; 80 dimensions (two
waves of the centre kernel) and 300 (two of its workgroups); as many centres as Gaussians."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
MIN_GAP = 1e-9


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GR = _load("gcluster_restate")


def make_pool(seed, D, G):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((G, D)), np.exp(rng.uniform(np.log(0.25), np.log(4.0), (G, D)))


def make_case(seed, D, G, C):
    """A pool and the centres of a random map in which every cluster has a member (G == C: one each)."""
    mean, cov = make_pool(seed, D, G)
    rng = np.random.default_rng(seed + 1)
    cmap = np.concatenate([np.arange(C), rng.integers(0, C, G - C)])[rng.permutation(G)]
    return (mean, cov, GR.log_det(cov)) + GR.centres(mean, cov, cmap, C)


# C None: one centre past the kernel's chunk
ASSIGN_SHAPES = [(1, 70, 3), (39, 257, 5), (39, 1000, 130), (39, 257, None), (80, 300, 17), (5, 64, 64)]


@pytest.mark.parametrize("D,G,C", ASSIGN_SHAPES)
def test_assign_steps_equal_the_restatement(capi, D, G, C):
    if C is None:
        C = capi.gcluster_chunk() + 1
    mean, cov, ldet, cm, cc, cl, cv = make_case(1000 + D + G + C, D, G, C)
    assert cv.all()
    for euclid in (False, True):
        want_idx, want_dist, gap = GR.assign_euclid(mean, cm) if euclid else GR.assign_kl(mean, cov, ldet, cm, cc, cl, cv)
        assert gap.min() > MIN_GAP, "bad fixture: gap %g" % gap.min()
        idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc, cl, cv, euclid=euclid)
        assert np.array_equal(idx, want_idx), (euclid, np.flatnonzero(idx != want_idx)[:10])
        assert np.array_equal(dist, want_dist), (euclid, np.abs(dist - want_dist).max())
        assert len(np.unique(idx)) > 1


def test_invalid_clusters_are_skipped_by_the_divergence_and_used_by_the_norm(capi):
    chunk = capi.gcluster_chunk()
    D, G, C = 7, 200, 2 * chunk + 5
    mean, cov, ldet, cm, cc, cl, cv = make_case(77, D, G, C)
    everyone = GR.assign_kl(mean, cov, ldet, cm, cc, cl, cv)[0]
    cv = cv.copy()
    cv[0] = cv[C - 1] = 0
    cv[chunk:2 * chunk] = 0                                # a whole chunk
    want_idx, want_dist, gap = GR.assign_kl(mean, cov, ldet, cm, cc, cl, cv)
    assert gap.min() > MIN_GAP
    moved = everyone != want_idx
    assert moved.sum() >= 20 and (cv[everyone[moved]] == 0).all()   # the invalid centres would have won these
    idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc, cl, cv)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    assert (cv[idx] != 0).all()
    # as the reference leaves an emptied cluster: zeros, so that its terms are x / 0
    cm0, cc0 = cm * (cv[:, None] != 0), cc * (cv[:, None] != 0)
    idx, dist = capi.gcluster_assign(mean, cov, ldet, cm0, cc0, cl, cv)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    # the Euclidean pass knows no validity
    e_idx, e_dist, e_gap = GR.assign_euclid(mean, cm)
    assert e_gap.min() > MIN_GAP and (cv[e_idx] == 0).any()
    idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc, cl, cv, euclid=True)
    assert np.array_equal(idx, e_idx) and np.array_equal(dist, e_dist)


def test_all_invalid_clusters_leave_index_0_and_1e100(capi):
    chunk = capi.gcluster_chunk()
    mean, cov, ldet, cm, cc, cl, cv = make_case(78, 3, 130, chunk + 3)
    idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc, cl, np.zeros_like(cv))
    assert (idx == 0).all() and (dist == 1e100).all()
    # a distance that is NaN or not below 1e100 never wins either: only centre 2 is usable
    cc2 = cc.copy()
    cc2[:2] = np.nan
    cl2 = cl.copy()
    cl2[3:] = 1e101
    want = GR.assign_kl(mean, cov, ldet, cm, cc2, cl2, cv)
    assert (want[0] == 2).all()
    idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc2, cl2, cv)
    assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])


def test_exact_ties_go_to_the_lower_index_across_chunks_and_waves(capi):
    """Identical centres at a < b with b in the next chunk (and, as the kernel deals a chunk's centres to its waves, in
    an earlier wave's hands than a), plus a pair inside one chunk; the Gaussians at those centres are in the pool
    several times.  Exempt from the gap condition: exactly the rows whose two best candidates are such a pair."""
    chunk = capi.gcluster_chunk()
    D, G, C = 6, 320, 2 * chunk
    mean, cov = make_pool(79, D, G)
    pairs = [(chunk - 1, chunk), (2, chunk // 2 + 1)]
    for a, b in pairs:                                      # centre j is Gaussian j
        mean[b], cov[b] = mean[a], cov[a]
        for dup in (a + 100, b + 150, G - 1 - a):
            mean[dup], cov[dup] = mean[a], cov[a]
    ldet = GR.log_det(cov)
    cm, cc, cl, cv = mean[:C].copy(), cov[:C].copy(), ldet[:C].copy(), np.ones(C, np.int32)
    for euclid in (False, True):
        want_idx, want_dist, gap = GR.assign_euclid(mean, cm) if euclid else GR.assign_kl(mean, cov, ldet, cm, cc, cl, cv)
        tied = gap == 0.0
        assert (gap[~tied] > MIN_GAP).all()
        assert set(want_idx[tied]) == {a for a, _ in pairs} and tied.sum() >= 10
        idx, dist = capi.gcluster_assign(mean, cov, ldet, cm, cc, cl, cv, euclid=euclid)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
        for a, b in pairs:
            assert (idx != b).all() and (idx[[a, b, a + 100, b + 150, G - 1 - a]] == a).all()


@pytest.mark.parametrize("D,G,C", [(1, 70, 3), (39, 300, 6), (80, 300, 6), (300, 70, 4)])
def test_centres_are_the_in_order_sums_bit_for_bit(capi, D, G, C):
    mean, cov = make_pool(500 + D, D, G)
    mean *= 10.0 ** np.random.default_rng(D).integers(-3, 4, (G, 1))   # sums whose order shows in the last bits
    cmap = np.random.default_rng(D + 1).integers(2, C, G)
    cmap[G // 3] = 0                                        # one member
    cmap[[0, G // 2, G - 1]] = 2                            # (and cluster 2 reaches over the whole range; cluster 1: nobody)
    want = GR.centres(mean, cov, cmap, C)
    assert list(want[3][:3]) == [1, 0, 1]
    shuffled = GR.centres(mean[::-1], cov[::-1], cmap[::-1], C)
    assert not np.array_equal(shuffled[0], want[0])         # the order is visible in these sums
    got = capi.gcluster_centres(mean, cov, cmap, C)
    for g, w, what in zip(got, want, ("mean", "cov", "ldet", "valid")):
        assert np.array_equal(g, w), what
    assert np.array_equal(got[0][0], mean[G // 3]) and (got[0][1] == 0).all() and (got[1][1] == 0).all()


def _run_tool(*args):
    r = subprocess.run([os.path.join(BIN, "gcluster")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


def pool_600():
    return synth.make_model(D=39, G=600, S=75, comps=8, seed=synth.SEED + 41)


@pytest.fixture(scope="module")
def run_600(capi, oracle, tmp_path_factory):
    """The 600-Gaussian pool through the tool, once: (model, want, paths, the tool's output)."""
    d = tmp_path_factory.mktemp("gcluster600")
    model = pool_600()
    base = str(d / "m")
    oracle.write_gk(base + ".gk", model[0], model[1])
    oracle.write_mc(base + ".mc", model[2], model[3], model[4])
    oracle.write_ph(base + ".ph", 75)
    want = GR.run(model[0], model[1], 12)
    r = _run_tool("-g", base + ".gk", "-o", base + ".gcl", "-C", 12, "-i", 1)
    return model, want, base, r


def test_tool_end_to_end_equals_the_restatement(run_600):
    model, want, base, r = run_600
    for step, gap in enumerate(want["gaps"]):
        assert gap.min() > MIN_GAP, "bad fixture: step %d gap %g" % (step, gap.min())
    assert open(base + ".gcl", "rb").read() == want["gcl"]
    assert r.stdout.splitlines() == want["lines"] + ["Wrote %d clusters" % want["n"]]
    assert want["n"] == 12 and len(want["lines"]) == 4
    err = r.stderr.splitlines()
    assert "make initial clusters" in err and err.index("make initial clusters") < err.index("start clustering")
    # -t is checked and changes nothing; -i 2 adds the Gaussians' lines in front of every iteration's
    r2 = _run_tool("-g", base + ".gk", "-o", base + ".t9.gcl", "-C", 12, "-t", 9, "-i", 2)
    assert open(base + ".t9.gcl", "rb").read() == want["gcl"]
    lines = r2.stdout.splitlines()
    assert len(lines) == 4 * 601 + 1 and lines[600] == want["lines"][0]
    assert lines[601 + 5] == "Gaussian 5 in cluster %d, distance %g" % (want["maps"][2][5], want["dists"][2][5])


def test_empty_cluster_is_left_out_and_the_ids_are_renumbered(capi, oracle, tmp_path):
    """The Gaussian the permutation picks second is made a copy of the one it picks first: two identical centres, the
    Euclidean pass gives every tie to the first, the second has no members and is invalid for good.  Exempt from the
    gap condition: the rows that go to the doubled centre in the Euclidean pass (exact ties)."""
    D, G, C = 5, 90, 6
    mean, cov = make_pool(80, D, G)
    perm = GR.permutation(G)
    mean[perm[1]], cov[perm[1]] = mean[perm[0]], cov[perm[0]]
    want = GR.run(mean, cov, C)
    assert want["n"] == C - 1 and want["c_valid"][1] == 0
    for step, (gap, cmap) in enumerate(zip(want["gaps"], want["maps"])):
        exempt = (cmap == 0) if step == 0 else np.zeros(G, bool)
        assert (gap[~exempt] > MIN_GAP).all(), step
    gk, out = str(tmp_path / "e.gk"), str(tmp_path / "e.gcl")
    oracle.write_gk(gk, mean, cov)
    r = _run_tool("-g", gk, "-o", out, "-C", C, "-i", 1)
    data = open(out, "rb").read()
    assert data == want["gcl"] and data.startswith(b"%d\n" % (C - 1))
    assert r.stdout.splitlines()[-1] == "Wrote %d clusters" % (C - 1)
    ids = np.array([int(l.split()[1]) for l in data.decode().splitlines()[1:]])
    assert sorted(set(ids)) == list(range(C - 1))
    cluster_of, n, _ = capi.gcluster_arrays(mean, cov, clusters=C)
    assert n == C - 1 and np.array_equal(cluster_of, want["cluster_of"])


def test_full_covariance_pool_clusters_by_its_diagonals(capi, oracle, tmp_path):
    D, G, C = 4, 60, 5
    rng = np.random.default_rng(81)
    mean = rng.standard_normal((G, D))
    A = rng.standard_normal((G, D, D))
    cov = A @ np.swapaxes(A, 1, 2) + 0.5 * np.eye(D)
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    diag = np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2))
    want = GR.run(mean, diag, C)
    for step, gap in enumerate(want["gaps"]):
        assert gap.min() > MIN_GAP, step
    gk, out = str(tmp_path / "f.gk"), str(tmp_path / "f.gcl")
    oracle.write_gk_full(gk, mean, cov)
    _run_tool("-g", gk, "-o", out, "-C", C)
    assert open(out, "rb").read() == want["gcl"]


def test_round_trip_into_clustered_scoring(capi, oracle, run_600):
    """The written file loads (12 <= 0.3 * 600), and Gmm.cluster(12) on the same model is the same clustering: it
    hands aasr_gmm_set_clustering the pairs the file's reader produces, the last pair twice included, so the state
    log-likelihoods of clustered scoring are equal, not close."""
    model, want, base, _ = run_600
    n, pairs = oracle.read_gcl(base + ".gcl", 600)
    assert n == 12 and pairs[:-1] == [(g, int(c)) for g, c in enumerate(want["cluster_of"])] and pairs[-1] == pairs[-2]
    frames = synth.make_frames(64, seed=synth.SEED + 42)
    scores = []
    for how in ("file", "cluster", "pairs"):
        gm = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
        if how == "file":
            gm.read_clustering(base + ".gcl")
        elif how == "cluster":
            assert gm.cluster(12) == 12
        else:
            gm.set_clustering(n, pairs)
        assert gm.num_clusters == 12
        gm.set_clustering_min_evals(0.0, 0.25)
        scores.append(gm.score(frames))
        gm.close()
    assert np.array_equal(scores[0], scores[1]) and np.array_equal(scores[0], scores[2])
    plain = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
    assert np.abs(plain.score(frames) - scores[0]).max() > 1e-3      # clustered scoring did take part

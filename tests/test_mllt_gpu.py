"""The MLLT kernels (csrc/mllt.hip) through the aasr_mllt handle: the variance pass and the G sums on the FP64 matrix
pipe against np.longdouble restatements over the handle's own resident covariances.

Bounds, first order in 2^-53 for any order of the sums in double, no measurement in them:
  variances  |err| <= (dim^2 + 2) 2^-52 sum_jk |a_ij S_jk a_ik|          per value,
  G sums     |err| <= (G + 2) 2^-52 sum_g |w_gi S_g(a, b)|                per entry, given the same variances.
Dimensions 1, 3, 16, 17, 39 (one tile, below and across a tile edge, the production width) and 63; 64 is refused.
Pools of 1, item - 1, item, item + 1 and 3 items + 5 Gaussians; a Gaussian without statistics in the first and in the
last position of an item; a gamma of 1e-30.  The same bytes from two runs and under slab bounds of one and three
items."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimate_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

ITEM = 256
CASES = [(1, 1), (1, ITEM + 1), (3, ITEM - 1), (16, ITEM), (17, ITEM + 1), (39, 3 * ITEM + 5), (39, 1), (63, ITEM + 1),
         (5, 3 * ITEM + 5)]


def make_statistics(d, G, seed):
    """gamma, sum_x, packed sum_xx of G Gaussians with covariance B D_g B^T and the flags: no statistics for the first
    Gaussian and the last of the first item (where the pool has them), a gamma of 1e-30 in the middle"""
    rng = np.random.default_rng(seed)
    B = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    gamma = rng.uniform(50, 500, size=G)
    ok = np.ones(G, np.int32)
    if G > 2:
        ok[0] = 0
        gamma[G // 2] = 1e-30
    if G >= ITEM:
        ok[ITEM - 1] = 0
    mean = rng.normal(size=(G, d))
    r, c = np.tril_indices(d)
    sxx = np.empty((G, R.tri(d)))
    for g in range(G):
        S = (B * rng.uniform(0.5, 2.0, size=d)) @ B.T
        sxx[g] = gamma[g] * (S + np.outer(mean[g], mean[g]))[r, c]
    sx = gamma[:, None] * mean
    # a Gaussian without statistics may hold anything: its sums must not be read into the result
    sx[ok == 0] = np.nan
    sxx[ok == 0] = np.nan
    return gamma, sx, sxx, ok


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "d%d-g%d" % c)
def case(request, capi):
    d, G = request.param
    gamma, sx, sxx, ok = make_statistics(d, G, 100 * d + G)
    h = capi.Mllt(gamma, sx, sxx, ok)
    cov = h.covariances()
    rng = np.random.default_rng(d)
    A = np.eye(d) + 0.2 * rng.normal(size=(d, d))
    yield dict(d=d, G=G, gamma=gamma, ok=ok, h=h, cov=cov, A=A, sx=sx, sxx=sxx)
    h.close()


def test_covariances(case):
    d, ok, cov = case["d"], case["ok"].astype(bool), case["cov"]
    assert np.isfinite(cov).all() and (cov[~ok] == 0).all()
    want = R.covariances(case["gamma"], case["sx"], case["sxx"], ok, np.longdouble)
    # the scaling by the rounded 1 / gamma, the product of two rounded means and the difference: at most
    # 3 u |S| + 7 u |mean_i mean_j| with u = 2^-53
    r, c = np.tril_indices(d)
    mean = np.where(ok[:, None], case["sx"] / case["gamma"][:, None], 0)
    mag = np.abs(want) + 2 * np.abs(mean[:, r] * mean[:, c])
    assert (np.abs(cov - want) <= 4 * 2.0 ** -53 * mag).all()


def test_variances_against_longdouble(case):
    d, h, A, cov = case["d"], case["h"], case["A"], case["cov"]
    got = h.variances(A)
    want = R.variances(A, cov.astype(np.longdouble))
    bound = (d * d + 2) * 2.0 ** -52 * R.variance_bound(A, cov)
    err = np.abs(got - want)
    print("variances d=%d G=%d: worst error / bound %.3g" % (d, case["G"], float((err / np.where(bound > 0, bound, 1)).max())))
    assert (err <= bound).all()
    assert (got[case["ok"] == 0] == 0).all() and (got[case["ok"] == 1] > 0).all()
    assert h.variances(A).tobytes() == got.tobytes()


def test_g_sums_against_longdouble(case):
    d, G, h, cov, ok = case["d"], case["G"], case["h"], case["cov"], case["ok"].astype(bool)
    var = np.maximum(h.variances(case["A"]), 0.1)
    got = h.g_sums(var)
    w = np.where(ok[:, None], case["gamma"][:, None] / var, 0.0)           # the same doubles as the handle's
    want = np.einsum("gi,ge->ie", w.astype(np.longdouble), cov.astype(np.longdouble))
    bound = (G + 2) * 2.0 ** -52 * np.einsum("gi,ge->ie", np.abs(w), np.abs(cov))
    err = np.abs(got - want)
    print("G sums d=%d G=%d: worst error / bound %.3g" % (d, G, float((err / np.where(bound > 0, bound, 1)).max())))
    assert (err <= bound).all()
    shape = h.launch_shape()
    items = (G + ITEM - 1) // ITEM
    assert shape == {"pb": (d + 15) // 16, "items": items, "launches": 1}
    # the same bytes from a second run, and under slab bounds of one and of three items
    assert h.g_sums(var).tobytes() == got.tobytes()
    slab = 16 * ((d + 15) // 16) * 16 * ((R.tri(d) + 15) // 16) * 8
    for n in (1, 3):
        h.set_slab_bytes(n * slab)
        assert h.g_sums(var).tobytes() == got.tobytes()
        assert h.launch_shape()["launches"] == (items + n - 1) // n
    h.set_slab_bytes(64 << 20)


def test_dimension_64_is_refused(capi):
    d, G = 64, 2
    with pytest.raises(capi.AasrError) as ei:
        capi.Mllt(np.ones(G), np.zeros((G, d)), np.zeros((G, R.tri(d))))
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "64" in ei.value.msg


def test_whole_loop_is_consistent(capi):
    """aasr_mllt_estimate on a small pool (the comparison of A with the restatement is tests/test_estimate_gpu.py's):
    unit determinant, a likelihood no worse than at A = I, and the returned means and variances are exactly A mean_g in
    double and the floored variance pass under the returned A."""
    d, G = 6, ITEM + 9
    gamma, sx, sxx, ok = make_statistics(d, G, 4242)
    k = G // 2                                   # (no 1e-30 here: the loop's sums are not the test's subject)
    gamma[k], sx[k], sxx[k] = 77.0, sx[k] * (77.0 / 1e-30), sxx[k] * (77.0 / 1e-30)
    h = capi.Mllt(gamma, sx, sxx, ok)
    A, mean, var = h.estimate(0.1)
    okb = ok.astype(bool)
    assert abs(abs(np.linalg.det(A)) - 1) <= 8 * d * 2.0 ** -53
    assert var.tobytes() == np.where(okb[:, None], np.maximum(h.variances(A), 0.1), 0).tobytes()
    want = np.zeros((G, d))
    for g in np.flatnonzero(okb):
        inv = 1 / gamma[g]
        for i in range(d):
            acc = 0.0
            for j in range(d):
                acc += A[i, j] * (sx[g, j] * inv)
            want[g, i] = acc
    assert mean.tobytes() == want.tobytes()
    var0 = np.maximum(h.variances(np.eye(d)), 0.1)
    assert R.mllt_objective(A, gamma, var, okb) >= R.mllt_objective(np.eye(d), gamma, var0, okb)
    t = h.times()
    assert t["cov_build"] > 0 and t["variances"] > 0 and t["g_sums"] > 0 and t["host_solve"] > 0

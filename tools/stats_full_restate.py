"""stats_full_restate.py -- NumPy restatement of the full second moments that stats collects with --full-stats
(csrc/stats_full_accum.hip): FullStatisticsAccumulator::accumulate (aku/Distributions.cc:133-141) under
Mixture::accumulate, the yardstick of tests/test_stats_full_gpu.py.

It builds on fuzz_stats.py: the records of gmm_build_f64, the posteriors operation by operation, the in-order sum.  Per
mixture component (record) the sum of gamma x x^T over the frames with a positive total in frame order, every entry as
dsyr forms it, (gamma x_j) x_i for j <= i; per pool Gaussian the records that share it added in record order.  The
second moments are packed lower triangles, row-major with j <= i: the layout of the mode-3 .gks and of
aasr_stats_full_moments.  extended=True: the same posteriors (double), every sum in np.longdouble by np.sum -- a
reference that shares no summation order with the kernel.

The device sums a Gaussian's frames in another grouping (256-row work items, four rows a matrix instruction, the items
of all its records one after the other), so it is compared with fuzz_stats.TOL["sum_xx"], not with ==.

    python tools/stats_full_restate.py [D M FRAMES]     (the distance between the two restatements, for a look)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_stats as FS  # noqa: E402
import estimate_restate as ER  # noqa: E402

TOL = FS.TOL["sum_xx"]          # (relative, absolute) per entry against restate_full()
TOL_EXT = (2 * TOL[0], 2 * TOL[1])   # against the extended-precision sums


def tri(d):
    return d * (d + 1) // 2


def restate_full(model, mix_w, x, pdf, extended=False):
    """sum_xx_full [G x D (D + 1) / 2] of the frames x [F x D] with pdfs pdf[] (< 0: skipped)"""
    mean, var, off, idx, _ = model
    G, D, S = len(mean), mean.shape[1], len(off) - 1
    rmean, rprec, rcst, rw = FS.records(model, mix_w)
    acc = np.longdouble if extended else np.float64
    add = (lambda t: t.astype(acc).sum(axis=0)) if extended else FS._in_order
    r, c = np.tril_indices(D)       # row-major, c <= r
    out = np.zeros((G, tri(D)), acc)
    for s in range(S):
        rows = np.nonzero(pdf == s)[0]          # ascending: frame order
        if len(rows) == 0 or off[s + 1] == off[s]:
            continue
        rs = slice(off[s], off[s + 1])
        xs = x[rows]
        gam, ok, _sl, _total = FS.posteriors(xs, rmean[rs], rprec[rs], rcst[rs], rw[rs])
        g, xo = gam[ok], xs[ok]
        if len(xo) == 0:
            continue
        xi, xj = xo[:, r].astype(acc), xo[:, c].astype(acc)
        for k in range(off[s + 1] - off[s]):    # record order
            out[idx[off[s] + k]] += add((g[:, k, None].astype(acc) * xj) * xi)
    return out


def distance(got, want, tol=TOL):
    """the largest entry error in units of the tolerance (an exact 0 against 0 is 0), and where"""
    g, w = np.asarray(got, np.float64), np.asarray(want).astype(np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    if g.size == 0:
        return 0.0, None
    if not np.isfinite(g).all():
        return np.inf, None
    diff, lim = np.abs(g - w), tol[1] + tol[0] * np.abs(w)
    ratio = np.where(diff == 0, 0.0, diff / lim)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    return float(ratio[at]), at


def write_gks_full(path, feacount, gamma, sum_x, sum_xx_full):
    """the mode-3 .gks by the restatement's own writer (estimate_restate.write_gks; aux_gamma 0)"""
    G, D = np.shape(sum_x)
    ER.write_gks(path, D, ER.FULL, [None if feacount[g] <= 0 else (int(feacount[g]), float(gamma[g]), sum_x[g], sum_xx_full[g])
                                    for g in range(G)])


if __name__ == "__main__":
    D, M, F = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (39, 4, 600)
    rng = np.random.default_rng(1)
    model = FS.make_model(rng, D, [M, 1, max(1, M // 2)])
    x, pdf = FS.make_frames(rng, model, [F, 5, F // 3], skipped=7)
    w = model[4].copy()
    for s in range(3):
        w[model[2][s]:model[2][s + 1]] /= w[model[2][s]:model[2][s + 1]].sum()
    a, b = restate_full(model, w, x, pdf), restate_full(model, w, x, pdf, extended=True)
    print("in-order restatement against the extended-precision sums: %.3g of the tolerance" % distance(a, b)[0])

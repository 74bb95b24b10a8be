"""aku/gcluster.cc (diagonal mode, one group) restated in NumPy: the yardstick of tests/test_gcluster_host.py and
tests/test_gcluster_gpu.py, compared with == and nothing wider.

Arithmetic: float64, one IEEE operation at a time (NumPy's elementwise add, subtract, multiply, divide and sqrt are
correctly rounded and never fused), in the reference's orders: distances summed over the dimensions in order, centre
sums over the members in Gaussian order, log-determinants with the C library's log (math.log) in dimension order.

* permutation: fill_random_permutation with libc's rand() after srand(1), what a fresh process has.
* assign_euclid / assign_kl: one assignment pass -> (index, distance, gap); gap is every Gaussian's relative distance
  between its best and second-best candidate, (d2 - d1) / max(|d1|, |d2|) -- inf with one candidate, 0 for an exact
  tie.  A kernel that rounds one operation differently can only change a map where this gap is at rounding level.
* centres: compute_cluster_statistics.
* run: make_initial_clusters, refine_clustering(4), save_clustering -> the five maps, distances and gaps, the
  "Iteration" lines of -i 1 and the .gcl bytes.
* norm2 is NOT dnrm2: the reference's BLAS norm scales its sum and can differ in the last place from the square root of
  the in-order sum that is restated (and computed by the kernel) here.
"""
import ctypes
import math

import numpy as np

NONE = 1e100        # the reference's starting minimum
PASSES = 4          # gcluster.cc:455, whatever -t says


def permutation(num):
    libc = ctypes.CDLL(None)
    libc.srand(1)
    p = list(range(num))
    for i in range(num):
        pos = i + libc.rand() % (num - i)
        p[i], p[pos] = p[pos], p[i]
    return np.array(p, np.int64)


def _log(x):
    if x > 0:
        return math.log(x) if x != math.inf else math.inf
    return -math.inf if x == 0 else math.nan


def log_det(cov):
    """[n x d] -> [n]: sum_k log(cov[k]) in dimension order"""
    out = np.zeros(len(cov))
    for i, row in enumerate(np.asarray(cov, np.float64)):
        t = 0.0
        for v in row:
            t = t + _log(float(v))
        out[i] = t
    return out


def _pick(d, usable):
    """strict < from (1e100, index 0) over the usable columns in ascending order; NaN never wins"""
    with np.errstate(all="ignore"):
        cand = usable[None, :] & (d < NONE)
    masked = np.where(cand, d, np.inf)
    idx = masked.argmin(axis=1)                      # the first of equal values
    found = cand.any(axis=1)
    idx = np.where(found, idx, 0).astype(np.int32)
    dist = np.where(found, masked[np.arange(len(d)), idx], NONE)
    if d.shape[1] > 1:
        two = np.partition(masked, 1, axis=1)[:, :2]
        with np.errstate(all="ignore"):
            gap = (two[:, 1] - two[:, 0]) / np.maximum(np.abs(two[:, 0]), np.abs(two[:, 1]))
        gap = np.where(np.isinf(two[:, 1]), np.inf, np.where(two[:, 1] == two[:, 0], 0.0, gap))
    else:
        gap = np.full(len(d), np.inf)
    return idx, dist, gap


def assign_euclid(mean, c_mean):
    mean, c_mean = np.asarray(mean, np.float64), np.asarray(c_mean, np.float64)
    acc = np.zeros((len(mean), len(c_mean)))
    for k in range(mean.shape[1]):
        t = mean[:, k, None] - c_mean[None, :, k]
        acc = acc + t * t
    return _pick(np.sqrt(acc), np.ones(len(c_mean), bool))


def assign_kl(mean, cov, ldet, c_mean, c_cov, c_ldet, c_valid):
    mean, cov, c_mean, c_cov = (np.asarray(a, np.float64) for a in (mean, cov, c_mean, c_cov))
    ldet, c_ldet = np.asarray(ldet, np.float64), np.asarray(c_ldet, np.float64)
    dim = mean.shape[1]
    acc = np.zeros((len(mean), len(c_mean)))
    with np.errstate(all="ignore"):
        for k in range(dim):
            t = mean[:, k, None] - c_mean[None, :, k]
            acc = acc + (cov[:, k, None] + t * t) / c_cov[None, :, k]
        kl = (c_ldet[None, :] - ldet[:, None] + acc - float(dim)) / 2.0
    return _pick(kl, np.asarray(c_valid) != 0)


def centres(mean, cov, cmap, n_clusters):
    """-> c_mean, c_cov [C x d], c_ldet [C] (0 for a cluster without members), c_valid [C] int32"""
    mean, cov = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    d = mean.shape[1]
    sm, sc = np.zeros((n_clusters, d)), np.zeros((n_clusters, d))
    count = np.zeros(n_clusters, np.int64)
    for i, c in enumerate(cmap):                     # Gaussian order
        sm[c] = sm[c] + mean[i]
        sc[c] = sc[c] + cov[i]
        count[c] += 1
    valid = (count > 0).astype(np.int32)
    for c in range(n_clusters):
        if count[c] > 0:
            scale = 1 / float(count[c])
            sm[c] = sm[c] * scale
            sc[c] = sc[c] * scale
    ldet = np.where(valid != 0, log_det(np.where(valid[:, None] != 0, sc, 1.0)), 0.0)
    return sm, sc, ldet, valid


def gcl_bytes(n, cluster_of):
    return ("%d\n" % n + "".join("%d %d\n" % (g, c) for g, c in enumerate(cluster_of))).encode()


def renumber(cmap, valid):
    """save_clustering: the valid clusters numbered in order -> (count, cluster of every Gaussian)"""
    real = np.cumsum(valid != 0) - 1
    real = np.where(valid != 0, real, -1)
    n = int((valid != 0).sum())
    if n == 0:
        raise ValueError("No valid clusters!")
    return n, real[np.asarray(cmap)].astype(np.int32)


def run(mean, cov, n_clusters):
    mean, cov = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    G = len(mean)
    if n_clusters < 2:
        raise ValueError("Invalid number of clusters")
    if G < n_clusters:
        raise ValueError("Not enough Gaussians to cluster!")
    ldet = log_det(cov)
    perm = permutation(G)
    maps, dists, gaps, lines = [], [], [], []
    idx, dist, gap = assign_euclid(mean, mean[perm[:n_clusters]])
    maps.append(idx), dists.append(dist), gaps.append(gap)
    cm, cc, cl, cv = centres(mean, cov, idx, n_clusters)
    for it in range(PASSES):
        idx, dist, gap = assign_kl(mean, cov, ldet, cm, cc, cl, cv)
        maps.append(idx), dists.append(dist), gaps.append(gap)
        cm, cc, cl, cv = centres(mean, cov, idx, n_clusters)
        total = 0.0
        for v in dist:
            total = total + float(v)
        lines.append("Iteration %i: Average Kullback-Leibler divergence = %g" % (it + 1, total / float(G)))
    n, cluster_of = renumber(maps[-1], cv)
    return {"perm": perm, "maps": maps, "dists": dists, "gaps": gaps, "lines": lines, "n": n, "cluster_of": cluster_of,
            "gcl": gcl_bytes(n, cluster_of), "c_mean": cm, "c_cov": cc, "c_ldet": cl, "c_valid": cv}

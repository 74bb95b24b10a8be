"""CMLLR estimation restated in Python: the yardstick of tests/test_mllr_*.py and tools/bench_mllr.py.

collect():  MllrTrainer::collect_data / MllTrainerComponent::collect_data (aku/MllrTrainer.cc:22-60, 147-163) in double,
            frame by frame and Gaussian by Gaussian in the reference's order -- or (extended=True) the same sums in
            np.longdouble, weights summed over the Gaussians first and the frames contracted by einsum, which shares no
            summation order with either the reference or the kernel.
solve():    MllTrainerComponent::calculate_transform / calculate_alpha (:165-253) with LAPACK dgetrf / dgetri through
            scipy, which is what LapackPP's LUFactorizeIP / LaLUInverseIP call.
compose():  MllrTrainer::calculate_transform(LinTransformModule *) (:98-145).
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FS = _load("fuzz_stats")


def posteriors(model, x, pdf, dtype=np.float64):
    """per frame the posteriors of its mixture's components WITHOUT the mixture weights (MllrTrainer.cc:40-49):
    prior * lik / sum lik with prior 1; 0 where that is not > 0 (:153).  -> list of (first record, values)"""
    mean, var, off, idx, _ = model
    rmean, rprec, rcst, _ = FS.records(model, np.ones(len(idx)))
    out = [None] * len(pdf)
    for s in np.unique(pdf[pdf >= 0]):
        rows = np.nonzero(pdf == s)[0]
        r = slice(off[s], off[s + 1])
        M = off[s + 1] - off[s]
        xx = x[rows].astype(dtype)
        ll = np.zeros((len(rows), M), dtype)
        for d in range(x.shape[1]):
            df = xx[:, d, None] - rmean[None, r, d].astype(dtype)
            ll += df * df * rprec[None, r, d].astype(dtype)
        ll *= dtype(-0.5)
        ll += rcst[None, r].astype(dtype)
        with np.errstate(all="ignore"):
            lik = np.exp(ll)
            total = np.zeros(len(rows), dtype)
            for k in range(M):
                total = total + lik[:, k]
            g = dtype(1.0) * lik / total[:, None]
        g = np.where(g > 0, g, dtype(0.0))
        for j, f in enumerate(rows):
            out[f] = (off[s], g[j])
    return out


def scales(model):
    """per record 1 / covar and mean / covar; a non-positive variance weighs nothing (the engine's rule, as its
    precision is 0 in the likelihood)"""
    mean, var, off, idx, _ = model
    ok = var > 0
    v = np.where(ok, var, 1.0)
    return np.where(ok, 1.0 / v, 0.0)[idx], np.where(ok, mean / v, 0.0)[idx]


def collect(model, x, pdf, extended=False):
    """-> G [D][D+1][D+1], k [D][D+1], beta"""
    D = x.shape[1]
    dtype = np.longdouble if extended else np.float64
    iv, mv = scales(model)
    post = posteriors(model, x, pdf, dtype)
    G, k, beta = np.zeros((D, D + 1, D + 1), dtype), np.zeros((D, D + 1), dtype), dtype(0.0)
    if extended:
        w, u = np.zeros((len(pdf), D), dtype), np.zeros((len(pdf), D), dtype)
        for f, pg in enumerate(post):
            if pg is None:
                continue
            r0, g = pg
            w[f] = (iv[r0:r0 + len(g)].astype(dtype) * g[:, None]).sum(0)
            u[f] = (mv[r0:r0 + len(g)].astype(dtype) * g[:, None]).sum(0)
            beta += g.sum()
        xi = np.concatenate([np.ones((len(pdf), 1), dtype), x.astype(dtype)], 1)
        for i in range(D):
            G[i] = (xi * w[:, i, None]).T @ xi
        k = u.T @ xi
        return G, k, beta
    for f, pg in enumerate(post):
        if pg is None:
            continue
        r0, g = pg
        xi = np.concatenate([[1.0], x[f]])
        fft = np.outer(xi, xi)
        for j, prob in enumerate(g):
            if not prob > 0:
                continue
            k += (mv[r0 + j] * prob)[:, None] * xi[None, :]
            G += (iv[r0 + j] * prob)[:, None, None] * fft[None]
            beta += prob
    return G, k, beta


def _inv(a, lapack=True):
    if lapack:
        from scipy.linalg import lapack as lp
        lu, piv, info = lp.dgetrf(a)
        assert info == 0, info
        inv, info = lp.dgetri(lu, piv)
        assert info == 0, info
        return inv, np.prod(np.diag(lu))
    # a plain LU with partial pivoting (the engine's own solver restated, for the LAPACK-vs-plain figure)
    n = len(a)
    lu, perm = a.astype(np.float64).copy(), np.arange(n)
    for c in range(n):
        p = c + int(np.argmax(np.abs(lu[c:, c])))
        if p != c:
            lu[[c, p]] = lu[[p, c]]
            perm[[c, p]] = perm[[p, c]]
        lu[c + 1:, c] /= lu[c, c]
        lu[c + 1:, c + 1:] -= np.outer(lu[c + 1:, c], lu[c, c + 1:])
    det = np.prod(np.diag(lu))
    inv = np.zeros((n, n))
    for c in range(n):
        y = np.zeros(n)
        y[c] = 1.0
        for i in range(n):
            y[i] -= lu[i, :i] @ y[:i]
        for i in range(n - 1, -1, -1):
            y[i] = (y[i] - lu[i, i + 1:] @ y[i + 1:]) / lu[i, i]
        inv[:, perm[c]] = y
    return inv, det


def solve(G, k, beta, lapack=True):
    """calculate_transform: W [D][D+1]; G, k, beta as doubles (extended statistics are rounded first)"""
    G, k, beta = np.asarray(G, np.float64), np.asarray(k, np.float64), float(beta)
    D = len(k)
    inv_G = [_inv(G[i], lapack)[0] for i in range(D)]
    trans = np.zeros((D, D + 1))
    trans[np.arange(D), np.arange(D) + 1] = 1.0
    for rnd in range(20 * D):
        row = rnd % D
        A, detA = _inv(np.ascontiguousarray(trans[:, 1:].T), lapack)
        A = detA * A
        p = np.concatenate([[0.0], A[row]])
        Gi, kr = inv_G[row], k[row]
        c2 = p @ (Gi @ p)
        c1 = p @ (Gi @ kr)
        a1 = (-c1 + np.sqrt(c1 * c1 + 4 * c2 * beta)) / (2 * c2)
        a2 = (-c1 - np.sqrt(c1 * c1 + 4 * c2 * beta)) / (2 * c2)
        m1 = beta * np.log(abs(a1 * c2 + c1)) - (c2 / 2) * a1 * a1
        m2 = beta * np.log(abs(a2 * c2 + c1)) - (c2 / 2) * a2 * a2
        alpha = a1 if m1 > m2 else a2
        p = alpha * p + kr
        trans[row] = Gi.T @ p
    return trans


def compose(W, old_A=None, old_b=None):
    """-> float32 A, b.  With an old transform: A <- A old_A; line 127 multiplies old_A into b IN PLACE (dgemv with
    beta = 0 clears its output first, and the output is its input), so the new bias is lost and b <- old_b."""
    A, b = W[:, 1:].copy(), W[:, 0].copy()
    if old_A is not None:
        b = np.asarray(old_b, np.float32).astype(np.float64)
        A = A @ np.asarray(old_A, np.float32).astype(np.float64)
    return A.astype(np.float32), b.astype(np.float32)


def auxiliary(W, G, k, beta):
    """the CMLLR auxiliary function beta log |det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i), in extended precision"""
    W = np.asarray(W, np.longdouble)
    q = np.longdouble(beta) * np.longdouble(np.linalg.slogdet(np.asarray(W[:, 1:], np.float64))[1])
    for i in range(len(W)):
        q -= np.longdouble(0.5) * (W[i] @ (np.asarray(G[i], np.longdouble) @ W[i]) - 2 * (W[i] @ np.asarray(k[i], np.longdouble)))
    return q


def rel_err(a, b):
    """largest difference relative to the largest entry of b"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def make_case(rng, D, sizes, counts, skipped=0, scale=1.0):
    model = FS.make_model(rng, D, sizes)
    x, pdf = FS.make_frames(rng, model, counts, skipped=skipped)
    return model, x * scale, pdf

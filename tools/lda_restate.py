"""aku/lda.cc restated in NumPy: the yardstick of tests/test_lda_host.py, tests/test_lda_gpu.py and
tests/test_scatter_gpu.py.

* scatter_in_order: FullStatisticsAccumulator::accumulate frame by frame in double, (gamma x_j) x_i as dsyr forms it;
  with dtype=np.longdouble the same sums in extended precision.
* solve: lda.cc:380-446 with np.linalg.eig (dgeev, the reference's routine) and np.linalg.inv; route="eigh" takes the
  Cholesky-reduced symmetric problem instead (a second reference-side route, for the tolerance).
* match_rows: two results row by row by |cosine|, up to sign.
* known_spectrum_case: per-class sums whose W^-1 B has a prescribed, well-separated spectrum.
"""
import numpy as np


def pack(full):
    """[..., d, d] symmetric -> packed lower triangle, row-major with j <= i"""
    d = full.shape[-1]
    i, j = np.tril_indices(d)
    return np.ascontiguousarray(full[..., i, j])


def unpack(packed, d):
    i, j = np.tril_indices(d)
    full = np.zeros(packed.shape[:-1] + (d, d), packed.dtype)
    full[..., i, j] = packed
    full[..., j, i] = packed
    return full


def scatter_in_order(x, cls, n_classes, weight=None, dtype=np.float64):
    """-> gamma [C], sum_x [C x d], sum_xx [C x d x d] (lower triangle filled, mirrored)"""
    n, d = x.shape
    x = x.astype(dtype)
    w = np.ones(n, dtype) if weight is None else np.asarray(weight).astype(dtype)
    g = np.zeros(n_classes, dtype)
    sx = np.zeros((n_classes, d), dtype)
    sxx = np.zeros((n_classes, d, d), dtype)
    for t in range(n):
        c = cls[t]
        if c < 0:
            continue
        g[c] += w[t]
        sx[c] += w[t] * x[t]
        sxx[c] += np.outer(x[t], w[t] * x[t])        # entry (i, j) = x_i (gamma x_j)
    low = np.tril(np.ones((d, d), bool))
    sxx = np.where(low, sxx, np.swapaxes(sxx, 1, 2))
    return g, sx, sxx


def moments(gamma, sx, sxx):
    mean = sx / gamma
    return mean, sxx * (1 / gamma) - np.outer(mean, mean)


def w_and_b(gamma, sx, sxx, selected, max_gamma):
    """data mean / covariance and B, W of lda.cc:380-403; sxx full [C x d x d]"""
    sel = [c for c in range(len(gamma)) if selected[c]]
    d = sx.shape[1]
    g_all, sx_all, sxx_all = 0.0, np.zeros(d), np.zeros((d, d))
    for c in sel:
        g_all = g_all + gamma[c]
        sx_all = sx_all + sx[c]
        sxx_all = sxx_all + sxx[c]
    mean, cov = moments(g_all, sx_all, sxx_all)
    B, W = np.zeros((d, d)), np.zeros((d, d))
    for c in sel:
        m, s = moments(gamma[c], sx[c], sxx[c])
        g = min(gamma[c], max_gamma)
        B += g * np.outer(m - mean, m - mean)
        W += g * s
    return mean, cov, B, W


def solve(gamma, sx, sxx, selected, max_gamma, target_dim, route="eig", details=False):
    """lda [target_dim x d], rows in whatever order the eigen-solver returns; sxx full [C x d x d]"""
    _, cov, B, W = w_and_b(gamma, sx, sxx, selected, max_gamma)
    if route == "eig":
        lam, vec = np.linalg.eig(np.linalg.inv(W) @ B)
        lam, vec = lam.real, vec.real
    else:
        L = np.linalg.cholesky(W)
        Li = np.linalg.inv(L)
        lam, y = np.linalg.eigh(Li @ B @ Li.T)
        vec = Li.T @ y
        vec = vec / np.linalg.norm(vec, axis=0)
    order = np.argsort(-lam, kind="stable")
    lam, vec = lam[order], vec[:, order]
    pca = vec[:, :target_dim]
    fea_cov = pca.T @ cov @ pca
    if route == "eig":
        ev, evec = np.linalg.eig(fea_cov)
        ev, evec = ev.real, evec.real
    else:
        ev, evec = np.linalg.eigh(fea_cov)
    lda = np.diag(1 / np.sqrt(ev)) @ evec.T @ pca.T
    if details:
        return lda, lam, ev, cov
    return lda


def match_rows(got, want):
    """-> got's rows reordered and signed to match want's, by |cosine|; the matching must be a bijection"""
    gn = got / np.linalg.norm(got, axis=1, keepdims=True)
    wn = want / np.linalg.norm(want, axis=1, keepdims=True)
    cos = wn @ gn.T
    pick = np.abs(cos).argmax(axis=1)
    assert sorted(pick) == list(range(len(got))), pick
    assert (np.abs(cos)[np.arange(len(pick)), pick] > 0.99).all()
    sign = np.sign(cos[np.arange(len(pick)), pick])
    return got[pick] * sign[:, None]


def rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def known_spectrum_case(rng, d, n_classes, target_dim, gamma=400.0, ratio=1.6, fea_ratio=1.35):
    """Per-class sums (gamma, sum_x, sum_xx full) with W = K g A A^T and B = A diag(lam) A^T: the eigenvalues of
    W^-1 B are lam / (K g) with neighbours `ratio` apart, its unit eigenvectors the normalised columns of A^-T, and the
    projected covariance's eigenvalues neighbours `fea_ratio` apart."""
    K = n_classes
    lam = K * gamma * 4.0 * ratio ** -np.arange(d)
    U = rng.standard_normal((d, d))
    U /= np.linalg.norm(U, axis=0)                               # columns of A^-T up to their lengths s
    f = fea_ratio ** rng.permutation(d).astype(float)               # the projected covariance's spectrum, any order
    s = np.sqrt((1 + lam / (K * gamma)) / f)
    A = np.linalg.inv((U * s).T)
    Q, _ = np.linalg.qr(np.concatenate([np.ones((K, 1)), rng.standard_normal((K, d))], 1))
    Mz = Q[:, 1:] * np.sqrt(lam / gamma)                         # class means in z: weighted mean 0, g M^T M = diag(lam)
    E = rng.standard_normal((K, d, d))
    E = 0.15 * (E + np.swapaxes(E, 1, 2)) / np.sqrt(d)
    E -= E.mean(axis=0)                                          # within-class covariances I + E_c, their mean I
    x0 = rng.standard_normal(d)
    g = np.full(K, gamma)
    sx = np.zeros((K, d))
    sxx = np.zeros((K, d, d))
    for c in range(K):
        m = A @ Mz[c] + x0
        cov = A @ (np.eye(d) + E[c]) @ A.T
        sx[c] = gamma * m
        sxx[c] = gamma * (cov + np.outer(m, m))
    return g, sx, sxx

"""aku/feanorm.cc restated in NumPy: the yardstick of tests/test_moments_gpu.py, tests/test_feanorm_host.py and
tests/test_feanorm_gpu.py.  Written from the behaviour the tool documents (include/aasr.h), frame by frame.

* cut: an utterance's rows in blocks of the block size -> segments (first row, length, utterance).
* segment_sums: per segment, frame by frame in the given dtype: the count, sum x and sum x^2 (diagonal) or sum x x^T
  (full; entry (i, j) grows by x_i x_j); with dtype=np.longdouble the same sums in extended precision.
* blocked: global += segment / block_size, count += length / block_size, over the kept segments in order.
* normalization / utterance_normalization: the mean and scale with the float roundings of the tool.
* pca: the covariance's eigenvectors (np.linalg.eigh, ascending, as dsyev) as rows and the two scalings;
  route="svd" takes the singular vectors of the centred data instead (a second route, for the tolerance).
* match_sign / fix_sign: two results row by row up to sign; the engine's sign convention.
* run: the whole tool over per-utterance feature arrays.
"""
import numpy as np


def cut(rows_per_utt, block_size, first_utt=0):
    """-> int32 [m x 3]: first row, length, utterance; the utterances' rows follow each other in one buffer"""
    segs, row = [], 0
    for u, n in enumerate(rows_per_utt):
        for k in range(0, n, block_size):
            segs.append((row + k, min(block_size, n - k), first_utt + u))
        row += n
    return np.array(segs, np.int32).reshape(-1, 3)


def segment_sums(x, segs, full=False, dtype=np.float64):
    """-> count [m], sum_x [m x d], sum_xx [m x d] or [m x d x d]"""
    d = x.shape[1]
    x = x.astype(dtype)
    m = len(segs)
    c, sx = np.zeros(m, dtype), np.zeros((m, d), dtype)
    sxx = np.zeros((m, d, d) if full else (m, d), dtype)
    for s, (first, n, _) in enumerate(segs):
        for t in range(first, first + n):
            c[s] += 1
            sx[s] += x[t]
            sxx[s] += np.outer(x[t], x[t]) if full else x[t] * x[t]
    return c, sx, sxx


def pack(full):
    """[..., d, d] symmetric -> packed lower triangle, row-major with j <= i"""
    i, j = np.tril_indices(full.shape[-1])
    return np.ascontiguousarray(full[..., i, j])


def blocked(c, sx, sxx, block_size, keep=None):
    """-> count, sum_x [d], sum_xx: the blocked sums over the segments with keep != 0, in order"""
    dtype = sx.dtype
    bs = dtype.type(block_size)
    g, gx, gxx = dtype.type(0), np.zeros(sx.shape[1:], dtype), np.zeros(sxx.shape[1:], dtype)
    for s in range(len(c)):
        if keep is not None and not keep[s]:
            continue
        gx = gx + sx[s] / bs
        gxx = gxx + sxx[s] / bs
        g = g + c[s] / bs
    return g, gx, gxx


def normalization(count, gx, gxx):
    """-> mean, scale (float32, as the tool rounds them) and the double mean; gxx: the diagonal second moments"""
    m = gx / count
    var = (gxx / count - m * m).astype(np.float32)            # sqrtf takes a float
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.float32(1) / np.sqrt(var)
    return m.astype(np.float32), scale.astype(np.float32), m


def utterance_normalization(c, sx, sxx):
    """the utterance's segments' sums added in order, undivided -> mean, scale (float32); sxx: diagonal second moments"""
    ux, uxx, n = np.zeros_like(sx[0]), np.zeros_like(sxx[0]), sx.dtype.type(0)
    for s in range(len(c)):
        ux, uxx, n = ux + sx[s], uxx + sxx[s], n + c[s]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = ux / n
        sd = np.sqrt((uxx / n - m * m).astype(np.float32)).astype(np.float64)
    sd = np.where(sd <= 0, 1.0, sd)                             # a NaN is not <= 0: it stays
    return m.astype(np.float32), (1 / sd).astype(np.float32)


def covariance(count, gx, gxx_full):
    m = gx / count
    return gxx_full / count - np.outer(m, m)


def fix_sign(a):
    """every row's entry of largest magnitude (the first such) positive"""
    big = np.abs(a).argmax(axis=1)
    return a * np.where(a[np.arange(len(a)), big] < 0, -1.0, 1.0)[:, None]


def pca(cov, scale=None, unit_determinant=False, route="eigh", centred=None):
    """-> (pca [d x d], eigenvalues ascending).  route="svd": from the centred data [n x d] whose covariance cov is."""
    d = cov.shape[0]
    if route == "eigh":
        ev, vec = np.linalg.eigh(cov)
        rows = vec.T
    else:
        _, s, vt = np.linalg.svd(centred / np.sqrt(len(centred)), full_matrices=False)
        ev, rows = (s * s)[::-1], vt[::-1]
    tr = rows.copy()
    sc = np.ones(d) if scale is None else np.asarray(scale, np.float64)
    if unit_determinant:
        tr = tr / sc[None, :]
        tr = tr * (1 / abs(np.linalg.det(tr)) ** (1 / d))
    else:
        tr = tr / np.sqrt(ev)[:, None]
        tr = tr / sc[None, :]
    return fix_sign(tr), ev


def match_sign(got, want):
    """got's rows signed to match want's; the rows must correspond one to one"""
    s = np.sign(np.sum(got * want, axis=1))
    assert (s != 0).all()
    return got * s[:, None]


def rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def run(feats, at_eof, block_size, full=False, dtype=np.float64):
    """feats: per utterance its frames [n x d] (the rows the tool takes); at_eof: per utterance whether the input's end
    stopped it (otherwise the recipe's end time did, and a trailing partial block stays out of the global sums).
    -> dict: count, mean_acc (dtype), second (diagonal, dtype), cov (full), keep, per-utterance (mean, scale)"""
    x = np.concatenate(feats)
    rows = [len(f) for f in feats]
    segs = cut(rows, block_size)
    keep = np.array([1 if (n == block_size or at_eof[u]) else 0 for _, n, u in segs], np.int32)
    c, sx, sxx = segment_sums(x, segs, full, dtype)
    g, gx, gxx = blocked(c, sx, sxx, block_size, keep)
    diag = np.diagonal(gxx).copy() if full else gxx
    seg_diag = np.diagonal(sxx, axis1=1, axis2=2) if full else sxx
    out = {"count": g, "sum_x": gx, "second": diag, "segs": segs, "keep": keep, "utt": []}
    out["mean"], out["scale"], out["mean_acc"] = normalization(g, gx, diag)
    if full:
        out["cov"] = covariance(g, gx, gxx)
    for u in range(len(feats)):
        pick = [s for s in range(len(segs)) if segs[s][2] == u]
        out["utt"].append(utterance_normalization(c[pick], sx[pick], seg_diag[pick]) if pick else None)
    return out

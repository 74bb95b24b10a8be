"""mllr_bw_restate.py -- NumPy restatement, in double, of the CMLLR statistics over HMM networks (mllr --networks):
tools/stats_bw_restate.py's entries (forward-backward occupancies, the per-frame sum and division of
HmmNetBaumWelch::next_frame) regrouped by frame, then MllrTrainer::collect_data (aku/MllrTrainer.cc:22-60, 147-163) once
per (pdf, probability) of a frame as train_mllr calls it (aku/mllr.cc:136-141).

    e = BW.entries(net, ll, fw_beam=.., bw_beam=.., viterbi=..)                 # one utterance (stats_bw_restate)
    lists = frame_lists([e0, e1, ...], [row0_0, row0_1, ...], n_rows)            # per frame row [(pdf, weight), ...]
    off, pdf, weight = flatten(lists)                                            # aasr_fb_batch_frame_entries_dev's arrays
    G, k, beta = collect(model, x, lists)                                        # what capi.Mllr.fetch returns

Order: a frame's entries come in the order of its network's pdf list (the order in which s_t is summed); collect() walks
the frames in row order, a frame's entries in list order, an entry's Gaussians in mixture order, and adds every
Gaussian's term to G, k and beta as the reference does.  Per entry (pdf, p) the value of Gaussian g is p * lik_g / sum_g
lik_g, the mixture weights unused, and what is not > 0 adds nothing; an entry whose pdf the model does not have is
skipped.  collect(extended=True) forms the same sums in np.longdouble, a frame's weights summed first and the frames
contracted by matrix products, which shares no summation order with the reference or the kernel.  solve() and compose()
are tools/mllr_restate.py's.  Nothing here touches the device or the library."""
from __future__ import annotations

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import mllr_restate as MR  # noqa: E402
import stats_bw_restate as BW  # noqa: E402

FS, RS = BW.FS, BW.RS
solve, compose = MR.solve, MR.compose


def frame_lists(utts, row0, n_rows) -> list:
    """The entries of a batch grouped by frame row: per row of the frame buffer [(global pdf, weight), ...] in the
    order of the utterance's pdf list; rows that no utterance that ran owns stay empty."""
    lists = [[] for _ in range(n_rows)]
    for u, e in enumerate(utts):
        if e["status"] != RS.OK:
            continue
        for j, p in enumerate(e["pdfs"]):          # pdf-list order: a frame's list fills in that order
            for t, w in zip(e["frames"][j], e["weights"][j]):
                lists[row0[u] + int(t)].append((int(p), float(w)))
    return lists


def flatten(lists):
    """-> off [rows + 1] int64, pdf int32, weight float64: the arrays of aasr_fb_batch_frame_entries_dev"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    pdf = np.array([p for l in lists for p, _ in l], np.int32)
    weight = np.array([w for l in lists for _, w in l], np.float64)
    return off, pdf, weight


def unflatten(off, pdf, weight) -> list:
    return [[(int(pdf[e]), float(weight[e])) for e in range(int(off[r]), int(off[r + 1]))] for r in range(len(off) - 1)]


def posteriors(model, x, lists, dtype=np.float64) -> list:
    """per frame, per entry (first record, values): p * lik_g / sum_g lik_g without the mixture weights
    (MllrTrainer.cc:40-49 with the entry's probability as the prior), 0 where that is not > 0 (:153); None for an entry
    whose pdf the model does not have.  The likelihoods as mllr_restate.posteriors forms them."""
    mean, var, off, idx, _ = model
    S = len(off) - 1
    rmean, rprec, rcst, _ = FS.records(model, np.ones(len(idx)))
    rows = np.array([r for r, l in enumerate(lists) for _ in l], np.int64)
    pdfs = np.array([p for l in lists for p, _ in l], np.int64)
    wgts = np.array([w for l in lists for _, w in l], np.float64)
    flat = [None] * len(rows)
    for s in np.unique(pdfs):
        if s < 0 or s >= S:
            continue
        sel = np.nonzero(pdfs == s)[0]
        r = slice(off[s], off[s + 1])
        M = off[s + 1] - off[s]
        xx = x[rows[sel]].astype(dtype)
        ll = np.zeros((len(sel), M), dtype)
        for d in range(x.shape[1]):
            df = xx[:, d, None] - rmean[None, r, d].astype(dtype)
            ll += df * df * rprec[None, r, d].astype(dtype)
        ll *= dtype(-0.5)
        ll += rcst[None, r].astype(dtype)
        with np.errstate(all="ignore"):
            lik = np.exp(ll)
            total = np.zeros(len(sel), dtype)
            for k in range(M):
                total = total + lik[:, k]
            g = wgts[sel].astype(dtype)[:, None] * lik / total[:, None]
        g = np.where(g > 0, g, dtype(0.0))
        for j, e in enumerate(sel):
            flat[e] = (off[s], g[j])
    out, at = [], 0
    for l in lists:
        out.append(flat[at:at + len(l)])
        at += len(l)
    return out


def collect(model, x, lists, extended=False):
    """-> G [D][D+1][D+1], k [D][D+1], beta over the frame rows x with their entry lists"""
    assert len(lists) == len(x)
    D = x.shape[1]
    dtype = np.longdouble if extended else np.float64
    iv, mv = MR.scales(model)
    post = posteriors(model, x, lists, dtype)
    G, k, beta = np.zeros((D, D + 1, D + 1), dtype), np.zeros((D, D + 1), dtype), dtype(0.0)
    if extended:
        w, u = np.zeros((len(x), D), dtype), np.zeros((len(x), D), dtype)
        for f, entries in enumerate(post):
            for pg in entries:
                if pg is None:
                    continue
                r0, g = pg
                w[f] += (iv[r0:r0 + len(g)].astype(dtype) * g[:, None]).sum(0)
                u[f] += (mv[r0:r0 + len(g)].astype(dtype) * g[:, None]).sum(0)
                beta += g.sum()
        xi = np.concatenate([np.ones((len(x), 1), dtype), x.astype(dtype)], 1)
        for i in range(D):
            G[i] = (xi * w[:, i, None]).T @ xi
        k = u.T @ xi
        return G, k, beta
    for f, entries in enumerate(post):
        if not entries:
            continue
        xi = np.concatenate([[1.0], x[f]])
        fft = np.outer(xi, xi)
        for pg in entries:
            if pg is None:
                continue
            r0, g = pg
            for j, prob in enumerate(g):
                if not prob > 0:
                    continue
                k += (mv[r0 + j] * prob)[:, None] * xi[None, :]
                G += (iv[r0 + j] * prob)[:, None, None] * fft[None]
                beta += prob
    return G, k, beta


def add(a, b):
    return tuple(p + q for p, q in zip(a, b))


def path_weighted(net, ll, model, x, ac_scale=1.0, viterbi=False):
    """The expected statistics by enumeration: the sum over the paths of (path probability) x (mllr_restate.collect
    along the path's state sequence) -- in Viterbi mode the best path's alone.  -> G, k, beta"""
    paths = BW.enumerate_paths(net, ll, ac_scale)
    m = max(p[0] for p in paths)
    if viterbi:
        probs = [1.0 if p[0] == m else 0.0 for p in paths]
    else:
        z = sum(np.exp(p[0] - m) for p in paths)
        probs = [float(np.exp(p[0] - m) / z) for p in paths]
    total = None
    for pr, (_, arcs) in zip(probs, paths):
        if pr == 0.0:
            continue
        pdf = np.array([net.emitting[a][2] for a in arcs], np.int32)
        one = MR.collect(model, x, pdf)
        part = tuple(pr * np.asarray(q, np.float64) for q in one)
        total = part if total is None else add(total, part)
    return total

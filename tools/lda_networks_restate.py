"""lda_networks_restate.py -- NumPy restatement, in double, of LDA over HMM networks (lda --networks): what
aku/lda.cc:147-372 would compute from HmmNetBaumWelch's pdf_probs() -- the reference's own -H cannot run, so this is the
yardstick of tests/test_scatter_weighted_gpu.py and tests/test_lda_networks_gpu.py.

    e = BW.entries(net, ll, fw_beam=.., bw_beam=.., ac_scale=.., viterbi=..)    # one utterance (stats_bw_restate)
    cnt, rows, weights = BW.group([e0, e1, ...], [row0_0, ...], num_states)     # aasr_fb_batch_entries_dev's order
    g, sx, sxx = scatter_entries_in_order(x, cnt, rows, weights, num_states)    # FullStatisticsAccumulator::accumulate
    out = pipeline(utts, row0, x_source, num_states, target_dim, ...)           # selection, then lda_restate.solve

scatter_entries_in_order adds the entries of a class one after the other, entry e of class c adding weights[e] xi xi^T for
frame row rows[e] ((gamma x_j) x_i as dsyr forms it); with dtype=np.longdouble the same sums in extended precision.  An
entry of weight 0 adds nothing and does not look at its row, as the device's does not.  select() is lda.cc:113-115,
247-263 on the summed gamma (a tie goes to the lower state index, as aasr_lda_select decides it).  Nothing here touches
the device or the library."""
from __future__ import annotations

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import lda_restate as LR  # noqa: E402
import stats_bw_restate as BW  # noqa: E402

RS = BW.RS


def scatter_entries_in_order(x, cnt, rows, weights, n_classes, dtype=np.float64):
    """-> gamma [C], sum_x [C x d], sum_xx [C x d x d] (lower triangle filled, mirrored)"""
    d = x.shape[1]
    xx = x.astype(dtype)
    w = np.asarray(weights).astype(dtype)
    g = np.zeros(n_classes, dtype)
    sx = np.zeros((n_classes, d), dtype)
    sxx = np.zeros((n_classes, d, d), dtype)
    for c in range(n_classes):
        for e in range(int(cnt[c]), int(cnt[c + 1])):
            if w[e] == 0:
                continue
            v = xx[rows[e]]
            g[c] += w[e]
            sx[c] += w[e] * v
            sxx[c] += np.outer(v, w[e] * v)          # entry (i, j) = x_i (gamma x_j)
    low = np.tril(np.ones((d, d), bool))
    sxx = np.where(low, sxx, np.swapaxes(sxx, 1, 2))
    return g, sx, sxx


def entries_of_classes(cls, n_classes, weight=None):
    """The entry list of a hard labelling: one entry per frame with cls >= 0 in the order of the row list that
    aasr_scatter_accumulate_dev builds (class after class, frames ascending) -> cnt, rows, weights (ones without weight)"""
    cls = np.asarray(cls)
    rows = np.concatenate([np.nonzero(cls == c)[0] for c in range(n_classes)] + [np.zeros(0, np.int64)]).astype(np.int32)
    cnt = np.zeros(n_classes + 1, np.int64)
    cnt[1:] = np.cumsum([int((cls == c).sum()) for c in range(n_classes)])
    w = np.ones(len(rows)) if weight is None else np.asarray(weight, np.float64)[rows]
    return cnt, rows, w


def select(gamma, mingamma, maxmem, dim, silence=()):
    """lda.cc:113-115, 247-263 -> 0 / 1 per state"""
    n = len(gamma)
    maxpos = max(0, int(min(maxmem * 1000.0 * 1000.0 / (float(dim) * dim * 8), float(n))))
    order = sorted(range(n), key=lambda s: (-gamma[s], s))
    sel = np.zeros(n, np.int32)
    for s in order[:maxpos]:
        if gamma[s] >= mingamma:
            sel[s] = 1
    for s in silence:
        sel[s] = 0
    return sel


def pipeline(utts, row0, x_source, num_states, target_dim, mingamma=50.0, maxgamma=1e6, maxmem=3000, silence=(),
             route="eig") -> dict:
    """utts: BW.entries() of the batch's utterances (those that gave up add nothing), row0: the frame row of every
    utterance's first frame in x_source, the frames at the module's source.  -> gamma, selected, lda and the sums"""
    cnt, rows, weights = BW.group(utts, row0, num_states)
    g, sx, sxx = scatter_entries_in_order(x_source, cnt, rows, weights, num_states)
    sel = select(g, mingamma, maxmem, x_source.shape[1], silence)
    sel = np.where(g > 0, sel, 0).astype(np.int32)
    lda = LR.solve(g, sx, sxx, sel, maxgamma, target_dim, route=route)
    return {"gamma": g, "sum_x": sx, "sum_xx": sxx, "selected": sel, "lda": lda, "cnt": cnt, "rows": rows,
            "weights": weights}

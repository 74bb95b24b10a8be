"""stats_bw_restate.py -- NumPy restatement, in double, of Baum-Welch statistics over HMM networks (stats --networks):
tools/hmmnet_restate.py's forward_backward for the occupancies, HmmNetBaumWelch::next_frame's per-frame sum and
division (aku/HmmNetBaumWelch.cc:714-789) in dense form for the entries, and Mixture::accumulate /
DiagonalStatisticsAccumulator::accumulate (aku/Distributions.cc:249-260, 2134-2161) with the entry's weight as gamma,
operation by operation as csrc/stats_weighted.hip states them, on top of tools/fuzz_stats.py's records.

    e = entries(net, ll, fw_beam=.., bw_beam=.., ac_scale=.., viterbi=..)      # one utterance
    cnt, rows, weights = group([e0, e1, ...], [row0_0, row0_1, ...], num_states) # the order of aasr_fb_batch_entries_dev
    want = accumulate(model, mix_w, x, cnt, rows, weights)                       # the dictionary of capi.Stats.fetch

entries() reports the smallest positive occupancy (the reference counts an arc whose posterior underflowed to exactly
0 as an entry of weight 0, the device makes none: tests choose inputs that stay far from that) and max |1 - s_t|.
compare_dumps() reads the .gks / .mcs files that the stats tool writes and compares them under the bounds that
tests/test_stats_gpu.py::check_against uses for the .phn mode.  Nothing here touches the device or the library."""
from __future__ import annotations

import math
import os
import struct
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import fuzz_stats as FS  # noqa: E402
import hmmnet_restate as RS  # noqa: E402


def entries(net, ll, fw_beam=15.0, bw_beam=200.0, ac_scale=1.0, viterbi=False) -> dict:
    """One utterance: the forward-backward result and its normalised entries, per pdf of the network's pdf list the
    frames (ascending) with occ > 0 and their weights occ / s_t, s_t summed in pdf-list order."""
    r = RS.forward_backward(net, ll, fw_beam, bw_beam, ac_scale, viterbi)
    out = {"result": r, "status": r.status, "pdfs": list(net.pdfs), "frames": [], "weights": [], "s": None,
           "min_positive_occ": math.inf, "max_dev": 0.0, "T": len(ll)}
    if r.status != RS.OK:
        return out
    occ = r.pdf_occ
    s = np.zeros(len(occ))
    for j in range(occ.shape[1]):          # pdf-list order, one addition after the other
        s = s + occ[:, j]
    out["s"] = s
    pos = occ[occ > 0]
    out["min_positive_occ"] = float(pos.min()) if pos.size else math.inf
    out["max_dev"] = float(np.abs(1.0 - s).max())
    for j in range(occ.shape[1]):
        t = np.nonzero(occ[:, j] > 0)[0]
        out["frames"].append(t)
        out["weights"].append(occ[t, j] / s[t])
    return out


def group(utts, row0, num_states):
    """The entries of a batch in the order of aasr_fb_batch_entries_dev: global pdf ascending, within a pdf the
    utterances in batch order, frames ascending -> cnt [num_states + 1], rows, weights"""
    per = [[] for _ in range(num_states)]
    for u, e in enumerate(utts):
        if e["status"] != RS.OK:
            continue
        for j, p in enumerate(e["pdfs"]):
            per[p].append((e["frames"][j] + row0[u], e["weights"][j]))
    cnt = np.zeros(num_states + 1, np.int64)
    rows, weights = [], []
    for p in range(num_states):
        for f, w in per[p]:
            rows.append(f)
            weights.append(w)
            cnt[p + 1] += len(f)
    cnt = np.cumsum(cnt)
    rows = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    weights = np.concatenate(weights) if weights else np.zeros(0)
    return cnt, rows, weights


def weighted_posteriors(x, wgt, rmean, rprec, rcst, rw):
    """fuzz_stats.posteriors with Mixture::accumulate's gamma: gamma * w_k * lik / total left to right, and
    gamma * safe_log(total)"""
    n, M = len(x), len(rw)
    ll = np.zeros((n, M))
    for d in range(x.shape[1]):
        df = x[:, d, None] - rmean[None, :, d]
        ll += df * df * rprec[None, :, d]
    ll *= -0.5
    ll += rcst[None, :]
    with np.errstate(under="ignore"):
        lik = np.exp(ll)
        total = np.zeros(n)
        for k in range(M):
            total = total + rw[k] * lik[:, k]
        ok = total > 0
        gam = np.zeros((n, M))
        gam[ok] = wgt[ok, None] * rw[None, :] * lik[ok] / total[ok, None]
        with np.errstate(divide="ignore"):
            sl = np.where(total < FS.SAFE_FLOOR, np.log(FS.SAFE_FLOOR), np.log(np.where(total > 0, total, 1.0)))
        return gam, ok, wgt * sl


def accumulate(model, mix_w, x, cnt, rows, weights) -> dict:
    """The statistics of the weighted entries (cnt[s] the first entry of pdf s in rows / weights) over the frames x: the
    entries of a pdf summed in their order, per pool Gaussian its records in record order.  -> capi.Stats.fetch's keys"""
    mean, var, off, idx, _ = model
    G, D, S, K = len(mean), mean.shape[1], len(off) - 1, len(idx)
    rmean, rprec, rcst, rw = FS.records(model, mix_w)
    racc_g, racc_a = np.zeros(K), np.zeros(K)
    racc_x, racc_xx = np.zeros((K, D)), np.zeros((K, D))
    count, mll = np.zeros(S, np.int64), np.zeros(S)
    for s in range(S):
        e = slice(int(cnt[s]), int(cnt[s + 1]))
        if e.stop == e.start:
            continue
        r = slice(off[s], off[s + 1])
        xs, wgt = x[rows[e]], np.asarray(weights[e], np.float64)
        gam, ok, wsl = weighted_posteriors(xs, wgt, rmean[r], rprec[r], rcst[r], rw[r])
        count[s] += int(ok.sum())
        mll[s] += FS._in_order(wsl[:, None])[0]
        g, xo = gam[ok], xs[ok]
        racc_g[r] += FS._in_order(g)
        racc_a[r] += FS._in_order(np.abs(g))
        for k in range(off[s + 1] - off[s]):
            gx = g[:, k, None] * xo
            racc_x[off[s] + k] += FS._in_order(gx)
            racc_xx[off[s] + k] += FS._in_order(gx * xo)
    out = dict(feacount=np.zeros(G, np.int64), gamma=np.zeros(G), aux_gamma=np.zeros(G), sum_x=np.zeros((G, D)),
               sum_xx=np.zeros((G, D)))
    rec_pdf = np.repeat(np.arange(S), np.diff(off))
    for k in range(K):
        gi = idx[k]
        out["feacount"][gi] += count[rec_pdf[k]]
        out["gamma"][gi] += racc_g[k]
        out["aux_gamma"][gi] += racc_a[k]
        out["sum_x"][gi] += racc_x[k]
        out["sum_xx"][gi] += racc_xx[k]
    out.update(count=count, mixture_ll=mll, mix_gamma=racc_g)
    return out


def add(a: dict, b: dict) -> dict:
    return {k: a[k] + b[k] for k in a}


def enumerate_paths(net, ll, ac_scale=1.0):
    """Every path from the initial to the final node that emits exactly T frames -> [(score, [emitting arc per frame])],
    the walk of hmmnet_restate.brute_force with the arcs kept.  For networks of a few nodes only."""
    ll = np.asarray(ll, np.float64)
    T = ll.shape[0]
    paths = []

    def walk(node, t, acc, arcs):
        if t == T and node == net.final:
            paths.append((acc, list(arcs)))
        for a in net.out_eps[node]:
            walk(net.eps[a][1], t, acc + net.eps[a][2], arcs)
        if t < T:
            for a in net.out_em[node]:
                e = net.emitting[a]
                s = RS.arc_score(e, ll[t], ac_scale)
                if s > RS.ZERO:
                    walk(e[1], t + 1, acc + s, arcs + [a])

    walk(net.initial, 0, 0.0, [])
    return paths


def path_weighted(net, ll, model, mix_w, x, ac_scale=1.0, viterbi=False) -> dict:
    """The expected statistics by enumeration: the sum over the paths of (path probability) x (the statistics of the
    path's state sequence with gamma 1) -- in Viterbi mode the best path's alone.  Counts are left out: an entry is
    counted once however many paths share it."""
    paths = enumerate_paths(net, ll, ac_scale)
    m = max(p[0] for p in paths)
    if viterbi:
        probs = [1.0 if p[0] == m else 0.0 for p in paths]
    else:
        z = sum(math.exp(p[0] - m) for p in paths)
        probs = [math.exp(p[0] - m) / z for p in paths]
    S = len(model[2]) - 1
    total = None
    for pr, (_, arcs) in zip(probs, paths):
        if pr == 0.0:
            continue
        pdf = np.array([net.emitting[a][2] for a in arcs], np.int32)
        one = FS.restate(model, mix_w, x, pdf)
        part = {k: pr * np.asarray(one[k], np.float64) for k in ("gamma", "aux_gamma", "sum_x", "sum_xx", "mix_gamma",
                                                                  "mixture_ll")}
        total = part if total is None else add(total, part)
    assert S == len(total["mixture_ll"])
    return total


# ---- the dumps of the stats tool ------------------------------------------------------------------------------------

def read_gks(path):
    """-> (pool size, dim, mode), {gaussian: (feacount, gamma, aux gamma, sum x, sum xx)} of the accumulated Gaussians"""
    b = open(path, "rb").read()
    G, D, mode = struct.unpack_from("<3i", b, 0)
    at, out = 12, {}
    for _ in range(G):
        g, flag = struct.unpack_from("<2i", b, at)
        at += 8
        if flag == 0:
            fc, gam, aux = struct.unpack_from("<idd", b, at)
            at += 20
            sx = np.frombuffer(b, "<f4", D, at).astype(np.float64)
            sxx = np.frombuffer(b, "<f4", D, 4 * D + at).astype(np.float64)
            at += 8 * D
            end, = struct.unpack_from("<i", b, at)
            at += 4
            assert end == -1
            out[g] = (fc, gam, aux, sx, sxx)
        else:
            assert flag == -1
    assert at == len(b)
    return (G, D, mode), out


def read_mcs(path):
    """-> (pdfs, mode), {pdf: the fields of its line} of the accumulated mixtures"""
    lines = open(path).read().split("\n")
    n, mode = int(lines[0]), int(lines[1])
    at, out = 2, {}
    for i in range(n):
        assert int(lines[at]) == i
        at += 1
        if lines[at] != "-1":
            out[i] = lines[at].split()
            at += 1
        assert lines[at] == "-1"
        at += 1
    return (n, mode), out


def _close(got, want, rel, abs_):
    return abs(got - want) <= max(abs_, rel * abs(want))


def compare_dumps(base, want, model, worst=None) -> list:
    """[failure text] of base.gks / base.mcs against a restatement, under the bounds of the .phn mode's check
    (tests/test_stats_gpu.py::check_against): the set of accumulated Gaussians and feacount exact; gamma and aux gamma
    within 1e-12 relative; every float of sum x / sum xx within one float ulp of the restatement's value; the set of
    accumulated mixtures, their component lists exact; component gammas within 1e-9 relative (1e-12 absolute);
    mixture_ll within 1e-9 relative.  worst: {quantity: largest error in units of its bound}, updated."""
    mean, _, off, idx, _ = model
    fails = []
    worst = {} if worst is None else worst

    def note(q, err, lim):
        worst[q] = max(worst.get(q, 0.0), float(err / lim) if lim > 0 else (0.0 if err == 0 else math.inf))

    (G, D, mode), gks = read_gks(base + ".gks")
    if (G, D, mode) != (len(mean), mean.shape[1], 1):
        fails.append("gks header %s" % ((G, D, mode),))
    acc = set(np.nonzero(want["feacount"])[0].tolist())
    if set(gks) != acc:
        fails.append("accumulated Gaussians differ: %s" % sorted(set(gks) ^ acc)[:8])
    for g, (fc, gam, aux, sx, sxx) in gks.items():
        if g not in acc:
            continue
        if fc != want["feacount"][g]:
            fails.append("feacount of %d: %d against %d" % (g, fc, want["feacount"][g]))
        for q, got_v, want_v in (("gamma", gam, want["gamma"][g]), ("aux_gamma", aux, want["aux_gamma"][g])):
            note(q, abs(got_v - want_v), max(1e-300, 1e-12 * abs(want_v)))
            if not _close(got_v, want_v, 1e-12, 1e-300):
                fails.append("%s of %d: %.17g against %.17g" % (q, g, got_v, want_v))
        for q, got_v, want_v in (("sum_x", sx, want["sum_x"][g]), ("sum_xx", sxx, want["sum_xx"][g])):
            lim = np.spacing(np.abs(want_v.astype(np.float32))).astype(np.float64)
            err = np.abs(got_v - want_v)
            note(q, (err / lim).max(), 1.0)
            if not (err <= lim).all():
                fails.append("%s of %d: off by %s float ulps" % (q, g, (err / lim).max()))
    (n, mode), mcs = read_mcs(base + ".mcs")
    if (n, mode) != (len(off) - 1, 1):
        fails.append("mcs header %s" % ((n, mode),))
    if set(mcs) != set(np.nonzero(want["count"])[0].tolist()):
        fails.append("accumulated mixtures differ")
    for p, f in mcs.items():
        M = off[p + 1] - off[p]
        if f[0] != "0" or int(f[1]) != M or len(f) != 2 + 2 * M + 2 or f[-2] != "0":
            fails.append("mixture %d: line %s" % (p, f))
            continue
        for k in range(M):
            if int(f[2 + 2 * k]) != idx[off[p] + k]:
                fails.append("mixture %d component %d: Gaussian %s" % (p, k, f[2 + 2 * k]))
            got_v, want_v = float(f[3 + 2 * k]), want["mix_gamma"][off[p] + k]
            note("mix_gamma", abs(got_v - want_v), max(1e-12, 1e-9 * abs(want_v)))
            if not _close(got_v, want_v, 1e-9, 1e-12):
                fails.append("mixture %d component %d: gamma %s against %.12g" % (p, k, f[3 + 2 * k], want_v))
        got_v, want_v = float(f[-1]), want["mixture_ll"][p]
        note("mixture_ll", abs(got_v - want_v), 1e-9 * abs(want_v))
        if not _close(got_v, want_v, 1e-9, 0.0):
            fails.append("mixture %d: mixture_ll %s against %.12g" % (p, f[-1], want_v))
    return fails

"""Randomised sweep of the statistics handle (csrc/stats.cc, stats_accum.hip) over everything that picks the
accumulation kernel's launch shape: dimensions 1 ... 192 (the ten dimension instances), largest mixtures 0 ... 118 (the
four sub-block sizes, records staged in LDS or not), ragged / tied / zero-weight mixtures, 0 to a few thousand frames per
pdf, skipped frames and uneven call cuts -- against restate() below, Mixture::accumulate /
DiagonalStatisticsAccumulator::accumulate in double with the frames of a pdf summed in frame order.
`python tools/fuzz_stats.py SEED N`; exits non-zero on a failure.

The restatement and the comparison live here so that tests/test_stats_shapes_gpu.py checks with the same code."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SAFE_FLOOR = 1e-50           # util::safe_log
MAX_DIM, MAX_COMPS = 192, 118
# the tolerances of tests/test_stats_gpu.py: (rtol, atol) per quantity; counts are compared exactly
TOL = {"gamma": (1e-12, 1e-300), "aux_gamma": (1e-12, 1e-300), "mixture_ll": (1e-12, 0.0), "mix_gamma": (1e-11, 1e-300),
       "sum_x": (1e-10, 1e-9), "sum_xx": (1e-10, 1e-9), "frame_ll": (1e-13, 1e-12)}
EXACT = ("feacount", "count")


def dimp_for(D):
    """the dimension instance of stats_items_launch that a model of D dimensions runs (0: none)"""
    for n in (8, 16, 24, 32, 40, 48, 64, 96, 128, 192):
        if D <= n:
            return n
    return 0


def launch_shape(D, max_comps):
    """(block, lds_recs) by the rule of stats.cc, None where the model is refused -- for choosing cases on the CPU; the
    tests assert the shapes they expect as literals"""
    rec = 2 * dimp_for(D) + 2
    b = 256
    while b > 64 and b * (max_comps + 2) * 8 > 48 * 1024:
        b -= 64
    if b * (max_comps + 2) * 8 > 60 * 1024:
        return None
    return b, int((b * (max_comps + 2) + max_comps * rec) * 8 + b * 8 <= 64 * 1024)


def write_ph(path):
    """a topology of one HMM over state 0: all that a statistics handle without transitions needs"""
    with open(path, "w") as f:
        f.write("PHONE\n1\n1 5 h0\n-1 -2 0 0 0\n0 1 2 1.0\n1 0\n2 2 2 0.5 3 0.5\n3 2 3 0.5 4 0.5\n4 2 4 0.5 1 0.5\n")


def make_model(rng, D, sizes, spare=3, zero_weights=0):
    """A ragged, tied model: mixture s has sizes[s] components drawn from a pool half their number (Gaussians shared
    between mixtures), every mixture of two or more holds one Gaussian twice, `spare` pool Gaussians belong to no
    mixture.  Means within a few sigma of each other in every dimension count, so that posteriors are shared."""
    sizes = np.asarray(sizes, np.int64)
    K = int(sizes.sum())
    used = max(1, K // 2)
    G = used + spare
    mean = rng.standard_normal((G, D)) * (2.0 / np.sqrt(D))
    var = rng.uniform(1.0, 3.0, (G, D))     # precisions <= 1: every log-likelihood is negative, no sum of them cancels
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    idx = rng.integers(0, used, K).astype(np.int32)
    for s in range(len(sizes)):
        if sizes[s] >= 2:
            idx[off[s] + sizes[s] - 1] = idx[off[s]]
    w = rng.uniform(0.05, 1.0, K)
    for _ in range(zero_weights):
        s = int(rng.choice(np.nonzero(sizes >= 2)[0]))
        w[off[s] + int(rng.integers(0, sizes[s]))] = 0.0
    return mean, var, off, idx, w


def make_frames(rng, model, counts, skipped=0):
    """counts[s] frames for pdf s drawn near its mixture's Gaussians, `skipped` frames of pdf -1, all shuffled"""
    mean, var, off, idx, _ = model
    D = mean.shape[1]
    xs, ps = [], []
    for s, n in enumerate(counts):
        if n == 0:
            continue
        M = off[s + 1] - off[s]
        centre = mean[idx[off[s] + rng.integers(0, M, n)]] if M else np.zeros((n, D))
        xs.append(centre + rng.standard_normal((n, D)) * rng.uniform(0.7, 1.3))
        ps.append(np.full(n, s, np.int32))
    if skipped:
        xs.append(rng.standard_normal((skipped, D)) * 50.0)
        ps.append(np.full(skipped, -1, np.int32))
    if not xs:
        return np.zeros((0, D)), np.zeros(0, np.int32)
    x, p = np.concatenate(xs), np.concatenate(ps)
    order = rng.permutation(len(p))
    return np.ascontiguousarray(x[order]), np.ascontiguousarray(p[order])


def records(model, mix_w):
    """gmm_build_f64 restated: per mixture component its mean, precision (1 / variance, 0 for a variance <= 0), the
    constant log(sqrt(prod precision)) -- the product itself (0) where it is not positive -- and the normalised weight"""
    mean, var, off, idx, _ = model
    with np.errstate(divide="ignore"):
        prec = np.where(var > 0, 1.0 / np.where(var > 0, var, 1.0), 0.0)
    prod = np.ones(len(mean))
    for d in range(mean.shape[1]):
        prod = prod * prec[:, d]
    with np.errstate(divide="ignore"):
        cst = np.where(prod > 0, np.log(np.sqrt(np.where(prod > 0, prod, 1.0))), prod)
    return mean[idx], prec[idx], cst[idx], np.asarray(mix_w, np.float64)


def posteriors(x, rmean, rprec, rcst, rw, dtype=np.float64):
    """Per frame of one pdf: the Gaussian log-likelihoods operation by operation as the kernel header states (sum of
    df * df * precision over the dimensions in order, * -0.5, + constant, exp), the total in component order, the
    posteriors 1.0 * w * lik / total, safe_log(total).  dtype = np.longdouble: the same in extended precision."""
    n, M = len(x), len(rw)
    x = x.astype(dtype)
    ll = np.zeros((n, M), dtype)
    for d in range(x.shape[1]):
        df = x[:, d, None] - rmean[None, :, d].astype(dtype)
        ll += df * df * rprec[None, :, d].astype(dtype)
    ll *= dtype(-0.5)
    ll += rcst[None, :].astype(dtype)
    with np.errstate(under="ignore"):
        lik = np.exp(ll)
        total = np.zeros(n, dtype)
        for k in range(M):
            total = total + rw[k].astype(dtype) * lik[:, k]
        ok = total > 0
        gam = np.zeros((n, M), dtype)
        gam[ok] = dtype(1.0) * rw[None, :].astype(dtype) * lik[ok] / total[ok, None]
    with np.errstate(divide="ignore"):
        sl = np.where(total < SAFE_FLOOR, np.log(dtype(SAFE_FLOOR)), np.log(np.where(total > 0, total, dtype(1.0))))
    return gam, ok, sl, total


def _in_order(terms, chunk=256):
    """sum over axis 0 in index order: np.cumsum adds one element after the other (np.sum is pairwise)"""
    acc = np.zeros(terms.shape[1:], terms.dtype)
    for b in range(0, len(terms), chunk):
        acc = np.cumsum(np.concatenate([acc[None], terms[b:b + chunk]]), axis=0)[-1]
    return acc


def restate(model, mix_w, x, pdf, frame_ll_init=0.0, extended=False):
    """The statistics of the frames x [F x D] with pdfs pdf[] (< 0: skipped) in double, the frames of a pdf summed in
    frame order; per pool Gaussian the records that share it added in record order.  extended=True: the same posteriors
    (double), every sum taken in np.longdouble by np.sum -- a reference that shares no summation order with the kernel.
    Returns the dictionary of capi.Stats.fetch plus frame_ll [F] and total [F] (nan on skipped frames)."""
    mean, var, off, idx, _ = model
    G, D, S, K = len(mean), mean.shape[1], len(off) - 1, len(idx)
    rmean, rprec, rcst, rw = records(model, mix_w)
    acc = np.longdouble if extended else np.float64
    racc_g, racc_a = np.zeros(K, acc), np.zeros(K, acc)
    racc_x, racc_xx = np.zeros((K, D), acc), np.zeros((K, D), acc)
    count, mll = np.zeros(S, np.int64), np.zeros(S, acc)
    frame_ll = np.full(len(pdf), frame_ll_init, np.float64)
    totals = np.full(len(pdf), np.nan)
    add = (lambda t: t.astype(acc).sum(axis=0)) if extended else _in_order
    for s in range(S):
        rows = np.nonzero(pdf == s)[0]          # ascending: frame order
        if len(rows) == 0:
            continue
        r = slice(off[s], off[s + 1])
        xs = x[rows]
        gam, ok, sl, total = posteriors(xs, rmean[r], rprec[r], rcst[r], rw[r])
        frame_ll[rows], totals[rows] = sl, total
        count[s] += int(ok.sum())
        mll[s] += add(1.0 * sl[:, None])[0]
        g, xo = gam[ok], xs[ok]
        racc_g[r] += add(g)
        racc_a[r] += add(np.abs(g))
        for k in range(off[s + 1] - off[s]):    # per component: [frames x D] terms
            gx = g[:, k, None] * xo
            racc_x[off[s] + k] += add(gx)
            racc_xx[off[s] + k] += add(gx * xo)
    out = dict(feacount=np.zeros(G, np.int64), gamma=np.zeros(G, acc), aux_gamma=np.zeros(G, acc),
               sum_x=np.zeros((G, D), acc), sum_xx=np.zeros((G, D), acc))
    rec_pdf = np.repeat(np.arange(S), np.diff(off))
    for k in range(K):                          # record order
        gi = idx[k]
        out["feacount"][gi] += count[rec_pdf[k]]
        out["gamma"][gi] += racc_g[k]
        out["aux_gamma"][gi] += racc_a[k]
        out["sum_x"][gi] += racc_x[k]
        out["sum_xx"][gi] += racc_xx[k]
    out.update(count=count, mixture_ll=mll, mix_gamma=racc_g, frame_ll=frame_ll, total=totals)
    return out


def compare(got, want, tol=TOL, worst=None, skip_pdfs=(), model=None):
    """[failure text] of a fetch dictionary (+ frame_ll) against a restatement; worst: {quantity: largest error in units of
    its tolerance}, updated.  skip_pdfs: pdfs whose values are not compared (counts still are) -- with `model`, the
    Gaussians and records of those pdfs are left out as well."""
    fails = []
    keep_g = keep_k = keep_s = keep_f = None
    if len(skip_pdfs) and model is not None:
        _, _, off, idx, _ = model
        rec_pdf = np.repeat(np.arange(len(off) - 1), np.diff(off))
        keep_k = ~np.isin(rec_pdf, skip_pdfs)
        keep_g = ~np.isin(np.arange(len(got["gamma"])), idx[~keep_k])
        keep_s = ~np.isin(np.arange(len(off) - 1), skip_pdfs)
        keep_f = ~np.isin(got["pdf"], skip_pdfs) if "pdf" in got else None
    sel = {"gamma": keep_g, "aux_gamma": keep_g, "sum_x": keep_g, "sum_xx": keep_g, "mix_gamma": keep_k,
           "mixture_ll": keep_s, "frame_ll": keep_f}
    for q in EXACT:
        if not np.array_equal(got[q], want[q]):
            fails.append("%s differs at %s" % (q, np.nonzero(np.asarray(got[q]) != np.asarray(want[q]))[0][:5]))
    for q, (rtol, atol) in tol.items():
        if q not in got:
            continue
        g, w = np.asarray(got[q], np.float64), np.asarray(want[q]).astype(np.float64)
        if sel[q] is not None:
            g, w = g[sel[q]], w[sel[q]]
        if g.shape != w.shape or not np.isfinite(g).all():
            fails.append("%s: shape %s against %s or a non-finite value" % (q, g.shape, w.shape))
            continue
        if g.size == 0:
            continue
        diff, lim = np.abs(g - w), atol + rtol * np.abs(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(diff == 0, 0.0, diff / lim)       # (an exact 0 against 0 passes a relative bound)
        if worst is not None:
            worst[q] = max(worst.get(q, 0.0), float(ratio.max()))
        if ratio.max() > 1.0:
            at = np.unravel_index(ratio.argmax(), ratio.shape)
            fails.append("%s at %s: %.17g against %.17g (%.3g of the tolerance)" % (q, at, g[at], w[at], ratio.max()))
    return fails


def run_handle(capi, gmm, topo, K, x, pdf, cuts=None, frame_ll_init=0.0):
    """the frames through a fresh handle in the calls cuts[i]:cuts[i+1] -> (fetch dictionary + frame_ll, launch shapes)"""
    import torch
    st = capi.Stats(gmm, topo, K)
    d_x = torch.tensor(x, device="cuda")
    d_ll = torch.full((max(1, len(pdf)),), frame_ll_init, dtype=torch.float64, device="cuda")
    cuts = [0, len(pdf)] if cuts is None else cuts
    shapes = []
    for b, e in zip(cuts[:-1], cuts[1:]):
        st.accumulate_dev(d_x[b:e], pdf[b:e], d_ll[b:e])
        if (pdf[b:e] >= 0).any():
            shapes.append(st.launch_shape())
    out = st.fetch()
    out["frame_ll"] = d_ll.cpu().numpy()[:len(pdf)]
    out["pdf"] = pdf
    st.close()
    return out, shapes


def draw(rng):
    """one random case, as shapes only: (D, mixture sizes, frames per pdf, skipped frames, zero weights, call cuts)"""
    D = int(rng.choice([int(rng.integers(1, MAX_DIM + 1)), int(rng.choice([8, 16, 24, 32, 39, 40, 48, 64, 96, 128, 192]))]))
    S = int(rng.integers(2, 9))
    top = int(rng.choice([int(rng.integers(0, MAX_COMPS + 1)), int(rng.choice([21, 22, 27, 28, 30, 31, 37, 38, 46, 47, 54, 55, 118]))]))
    sizes = rng.integers(0, top + 1, S)
    sizes[int(rng.integers(0, S))] = top
    big = int(rng.choice([3, 70, 300, 1100, 2600]))
    counts = np.where(rng.random(S) < 0.2, 0, rng.integers(0, big + 1, S))
    skipped = int(rng.integers(0, 20)) if rng.random() < 0.5 else 0
    zero_w = int(rng.integers(0, 3)) if (sizes >= 2).any() else 0
    F = int(counts.sum()) + skipped
    n_cuts = int(rng.integers(0, 4))
    cuts = [0] + sorted(int(c) for c in rng.integers(0, F + 1, n_cuts)) + [F]
    return D, sizes, counts, skipped, zero_w, cuts


def shapes_of(seed, N):
    """the launch shapes (dimp, block, lds_recs) that run(seed, N) draws, from the shapes of its models alone (no GPU)"""
    rng = np.random.default_rng(seed)
    out = set()
    for _ in range(N):
        D, sizes, counts, skipped, zero_w, cuts = draw(rng)
        rng.integers(0, 2 ** 31)   # the seed of the case's own stream, as run() draws it
        if counts.sum() > 0:
            out.add((dimp_for(D),) + launch_shape(D, int(sizes.max())))
    return out


def run(seed=1, N=20, verbose=False):
    import tempfile
    from aaltoasr_amd import capi
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(seed)
    worst, fails = {"shapes": set()}, []
    with tempfile.TemporaryDirectory() as d:
        write_ph(os.path.join(d, "t.ph"))
        topo = capi.Topology(os.path.join(d, "t.ph"))
        for it in range(N):
            D, sizes, counts, skipped, zero_w, cuts = draw(rng)
            sub = np.random.default_rng(int(rng.integers(0, 2 ** 31)))
            model = make_model(sub, D, sizes, zero_weights=zero_w)
            x, pdf = make_frames(sub, model, counts, skipped)
            ctx = "seed %d it %d D %d sizes %s frames %s skipped %d cuts %s" % (seed, it, D, list(sizes), list(counts),
                                                                                skipped, cuts)
            mix_w = O.DiagModel(*model).mix_w
            want = restate(model, mix_w, x, pdf, frame_ll_init=7.25)
            gmm = capi.Gmm.from_arrays(*model)
            got, shapes = run_handle(capi, gmm, topo, len(model[3]), x, pdf, cuts, frame_ll_init=7.25)
            gmm.close()
            expect = (dimp_for(D),) + launch_shape(D, int(sizes.max()))
            for sh in shapes:
                seen = (sh["dimp"], sh["block"], sh["lds_recs"])
                worst["shapes"].add(seen)
                if seen != expect or sh["max_comps"] != int(sizes.max()):
                    fails.append("%s: launch shape %s, expected %s" % (ctx, sh, expect))
            bad = compare(got, want, worst=worst)
            fails += ["%s: %s" % (ctx, b) for b in bad]
            if verbose:
                print("%s %s" % ("FAIL" if bad else "ok  ", ctx))
    return worst, fails


if __name__ == "__main__":
    worst, fails = run(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20, verbose=True)
    for k in sorted(worst):
        print("%-12s %s" % (k, worst[k] if k == "shapes" else "%.3g of its tolerance" % worst[k]))
    print("failures: %d" % len(fails))
    for f in fails[:20]:
        print(f)
    sys.exit(1 if fails else 0)

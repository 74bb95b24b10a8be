"""Outlier routing with the merge fused into the scoring kernel (k_gmm_diag_score_pl<..., HYB>, gmm_score_pl.h): which
kernel ran, its table and frame edges, and its arithmetic against the merge pass.

The models production loads have a few Gaussians far over the matrix layouts' conditioning limits (variance-floored
ones); find_outliers takes them out of the matrix rows, the centred kernel sums them per state, and on the grouped layout
at the default precision, without clustering, the scoring kernel adds those sums in its close logic instead of a merge
pass (score_outliers / k_outlier_merge).  Nothing in a score says which of the two ran, so every
case here asserts

1. the path: the handle's own layout has routing on with the expected counts, and the call's counters
   (aasr_debug_outlier_path) say the fused instance was launched and no merge pass ran -- or the reverse for the cases
   built to fall back;
2. parity: conftest.assert_ll against the oracle in double, on frames that make the outliers matter -- frames drawn on
   every outlier at its own sigma (the state IS the outlier there: a wrong record, frame or table entry moves it by tens of
   nats), frames on the state's ordinary components (the outlier's share at the floor) and frames placed where the two
   shares meet; that the visible values hold all three kinds is asserted from the oracle's per-Gaussian values;
3. fused against the merge pass: the same handle with the fused merge switched off returns the same bits (the kernel's
   comment promises k_outlier_merge's arithmetic, "the same bits").
"""
import ctypes as C

import numpy as np
import pytest

from conftest import LL_FLUSH, assert_ll

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu

WIDE_FROM = 8192   # launch_split (gmm_score_pl.h): the 8-wave form from this many frames on, the 4-wave form below


# ---- inputs ------------------------------------------------------------------------------------------------------

def _comp_ll(model, s, x):
    """log(w_k N_k(x)) of state s's components in double: [frames x components], and their pool indices (the reference's
    Gaussian, as the oracle's: exp(-0.5 sum p (x - mu)^2) / sqrt(prod var), no power of 2 pi)."""
    mean, var, off, idx, w = model
    ks = np.arange(off[s], off[s + 1])
    gs = idx[ks]
    x = np.asarray(x, np.float64)
    d = x[:, None, :] - mean[gs][None, :, :]
    ll = -0.5 * ((d * d) / var[gs][None]).sum(2) - 0.5 * np.log(var[gs]).sum(1)[None]
    with np.errstate(divide="ignore"):
        return ll + np.log(w[ks] / w[ks].sum())[None], gs


def _lse(a):
    m = a.max(1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(a - m).sum(1, keepdims=True)))[:, 0]


def _log_share(model, s, gs_out, x):
    """log of the outliers' share of state s's likelihood, and the state's log-likelihood (no floor), per frame."""
    ll, gs = _comp_ll(model, s, x)
    tot = _lse(ll)
    sel = np.isin(gs, gs_out)
    with np.errstate(invalid="ignore"):
        return _lse(ll[:, sel]) - tot, tot


def _between(model, s, gs_out, at, lo=0.0, hi=60.0, target=np.log(1e-3)):
    """t such that the outliers' share of state s at the float32 frame at(t) is ~1e-3 (it falls monotonically along a ray
    from an outlier's mean); None where the ray never gets there (a state made of outliers only)."""
    f = lambda t: _log_share(model, s, gs_out, at(t).astype(np.float32)[None])[0][0]
    if not (f(lo) > target > f(hi)):
        return None
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > target else (lo, mid)
    return 0.5 * (lo + hi)


def outlier_frames(model, outl, F, seed, xf=None):
    """F frames [F x D] float32: for every outlier state one frame ON its first outlier (0.5 sigma of its own), one where
    the outliers' share is ~1e-3, one on an ordinary component of the state; six more on the outlier at random places; the
    rest N(0, 1).  The special frames are
    dealt to both ends of the range (frame 0, frame F - 1, frame 1, ...), so that the last real frame of a launch is one
    of them.  xf = (a, b): the model sees a * frame + b (a diagonal transform) and the frames are placed for that."""
    mean, var, off, idx, w = model
    D = mean.shape[1]
    rng = np.random.default_rng(seed)
    special = []
    for s, gs in outl.items():
        g = gs[0]
        sig = np.sqrt(var[g])
        special.append(mean[g] + 0.5 * sig * rng.standard_normal(D))
        u = rng.standard_normal(D)
        t = _between(model, s, gs, lambda t: mean[g] + t * sig * u)
        if t is not None:
            special.append(mean[g] + t * sig * u)
        rest = [int(q) for q in idx[off[s]:off[s + 1]] if int(q) not in gs]
        if rest:
            special.append(mean[rest[0]] + 0.3 * np.sqrt(var[rest[0]]) * rng.standard_normal(D))
    x = rng.standard_normal((F, D))
    if F >= 64:   # more frames on the outliers, anywhere in the range
        for s, gs in outl.items():
            for f in rng.choice(F, 6, replace=False):
                x[f] = mean[gs[0]] + np.sqrt(var[gs[0]]) * rng.uniform(0.3, 1.0) * rng.standard_normal(D)
    for i, fr in enumerate(special[:F]):
        x[i // 2 if i % 2 == 0 else F - 1 - i // 2] = fr
    if xf is not None:
        x = (x - xf[1][None]) / xf[0][None]
    return x.astype(np.float32)


def sharp_model(S, picks, D=39, comps=8, seed=700, tie=None, weightless=(), **kw):
    """make_model + sharpen_outliers; tie = (states): the first component of each is ONE pool Gaussian (a tied pool);
    weightless: states whose first component gets weight 1e-20."""
    mean, var, off, idx, w = synth.make_model(D=D, G=S * comps, S=S, comps=comps, seed=seed, **kw)
    idx, w = idx.copy(), w.copy()
    if tie:
        for s in tie[1:]:
            idx[off[s]] = idx[off[tie[0]]]
    for s in weightless:
        w[off[s] + 1] += w[off[s]] - 1e-20
        w[off[s]] = 1e-20
    return synth.sharpen_outliers((mean, var, off, idx, w), picks)


def trio_model(S=64, D=39, comps=8, seed=710, a=5, b=38, c=None):
    """Three outlier states such that ONE frame holds all three kinds of value: it lies on state a's outlier, state c's
    outlier is placed next to it where c's two shares meet (~1e-3), state b's is elsewhere.  Returns model, outl and that
    frame."""
    c = S - 2 if c is None else c
    (mean, var, off, idx, w), outl = sharp_model(S, [(a, 1), (b, 1), (c, 1)], D=D, comps=comps, seed=seed)
    rng = np.random.default_rng(seed + 1)
    ga, gc = outl[a][0], outl[c][0]
    x0 = (mean[ga] + 0.5 * np.sqrt(var[ga]) * rng.standard_normal(D)).astype(np.float32)
    u = rng.standard_normal(D)

    def moved(t):
        m2 = mean.copy()
        m2[gc] = x0 + t * np.sqrt(var[gc]) * u
        return m2, var, off, idx, w
    lo, hi, target = 0.0, 60.0, np.log(1e-3)
    f = lambda t: _log_share(moved(t), c, outl[c], x0[None])[0][0]
    assert f(lo) > target > f(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > target else (lo, mid)
    return moved(0.5 * (lo + hi)), outl, x0


def trio_frames(model, outl, x0, F, seed):
    fr = outlier_frames(model, outl, F, seed)
    fr[0] = x0
    fr[F - 1] = x0      # the last real frame of the launch
    return fr


def coverage(model, outl, frames, xf=None, bias=0.0):
    """How many visible (frame, outlier state) values have the outliers' share > 0.9, in between, < 1e-6."""
    x = frames.astype(np.float64)
    if xf is not None:
        x = x * xf[0][None] + xf[1][None]
    n = [0, 0, 0]
    for s, gs in outl.items():
        ls, tot = _log_share(model, s, gs, x)
        vis = tot + bias > LL_FLUSH
        n[0] += int((vis & (ls > np.log(0.9))).sum())
        n[1] += int((vis & (ls < np.log(0.9)) & (ls > np.log(1e-6))).sum())
        n[2] += int((vis & (ls < np.log(1e-6))).sum())
    return n


# ---- the three assertions ------------------------------------------------------------------------------------------

def expected_counts(model, outl):
    mean, var, off, idx, w = model
    bad = {g for gs in outl.values() for g in gs}
    return int(np.isin(idx, list(bad)).sum()), len(outl)


def assert_path(g, model, outl):
    lay = g.own_layout()
    rows, states = expected_counts(model, outl)
    assert lay["routing"] and not lay["all_centred"], lay
    assert (lay["outlier_comps"], lay["outlier_states"]) == (rows, states), (lay, rows, states)


def scored(g, call, fused):
    """Runs call() and asserts from the handle's counters which of the two merges it used (fused = None: not the fused
    one -- a clustered model with engine parts scores through the parts' own handles, whose passes this one does not
    count)."""
    a = g.outlier_path()
    out = call()
    b = g.outlier_path()
    d = (b[0] - a[0], b[1] - a[1])
    if fused is None:
        assert d[0] == 0, "expected no fused launch, got (fused launches, merge passes) = %s" % (d,)
    elif fused:
        assert d[0] >= 1 and d[1] == 0, "expected the fused instance, got (fused launches, merge passes) = %s" % (d,)
    else:
        assert d[0] == 0 and d[1] >= 1, "expected the merge pass, got (fused launches, merge passes) = %s" % (d,)
    return out


def check(g, model, outl, frames, ref, what, fused=True, need=(1, 1, 1), xf=None, bias=0.0):
    """Assertions 2 and 3 (and the counters of 1) for one scoring call on handle g; returns the scores."""
    cov = coverage(model, outl, frames, xf, bias)
    assert all(c >= n for c, n in zip(cov, need)), "%s: visible values by outlier share (> 0.9, between, < 1e-6) = %s" % (what, cov)
    got = scored(g, lambda: g.score(frames), fused)
    g.set_outlier_fuse(False)
    try:
        merged = scored(g, lambda: g.score(frames), False)
    finally:
        g.set_outlier_fuse(True)
    differ = got.view(np.uint32) != merged.view(np.uint32)
    vis = ref > LL_FLUSH
    print("OUTLIER_CASE %s: worst visible |dll| %.3g (merge pass %.3g), coverage %s, differing values %d (max |d| %.3g)" % (
        what, np.abs(got - ref)[vis].max(), np.abs(merged - ref)[vis].max(), cov, int(differ.sum()),
        float(np.abs(got.astype(np.float64) - merged).max())))
    assert_ll(got, ref, what)
    assert_ll(merged, ref, what + ", merge pass")
    assert not differ.any(), "%s: %d values differ between the fused merge and the merge pass, first at %s" % (
        what, int(differ.sum()), np.argwhere(differ)[0])
    return got


def run_case(capi, oracle, model, outl, frames, what, fused=True, need=(1, 1, 1)):
    ref = oracle.DiagModel(*model).score(frames.astype(np.float64))
    g = capi.Gmm.from_arrays(*model)
    try:
        assert_path(g, model, outl)
        assert g.effective_precision() == 4
        return check(g, model, outl, frames, ref, what, fused, need)
    finally:
        g.close()


# ---- cases ---------------------------------------------------------------------------------------------------------

TABLE_EDGES = {
    "state 0": (64, [(0, 1)]),
    "last state, S even": (64, [(63, 1)]),
    "last state, S odd": (65, [(64, 2)]),
    "s, s+2": (64, [(20, 1), (22, 1)]),
    "s, s+2, s+4, s+6": (64, [(21, 1), (23, 2), (25, 1), (27, 1)]),
    "s, s+1 (even first)": (64, [(20, 1), (21, 1)]),
    "s, s+1 (odd first)": (64, [(21, 1), (22, 1)]),
    "15, 16, 17": (64, [(15, 1), (16, 1), (17, 1)]),
    "31, 32, 33": (64, [(31, 1), (32, 1), (33, 1)]),
    "14 and 15 of a group, first and last state": (65, [(0, 1), (14, 1), (15, 1), (64, 1)]),
}


@pytest.mark.parametrize("name", list(TABLE_EDGES))
def test_table_edges(capi, oracle, name):
    """hyb_tab says per track parity which state comes next and where its sums are: first and last states, states that
    follow each other on one track (the request behind the barrier has not come when the next one closes) and on both,
    states on both sides of the 16- and 32-column output groups."""
    S, picks = TABLE_EDGES[name]
    model, outl = sharp_model(S, picks, seed=720 + len(name))
    run_case(capi, oracle, model, outl, outlier_frames(model, outl, 300, 721), name)


def test_a_state_of_outliers_only_and_an_outlier_without_weight(capi, oracle):
    """Matrix share at the floor (every component of state 10 is an outlier: null rows only), and an outlier share that
    is nothing whatever the frame (weight 1e-20 in state 30)."""
    model, outl = sharp_model(64, [(10, 8), (30, 1), (41, 1)], seed=730, weightless=(30,))
    got = run_case(capi, oracle, model, outl, outlier_frames(model, outl, 300, 731), "outliers only / weightless")
    assert (got[:, 10] > LL_FLUSH).any()


def test_tied_pool(capi, oracle):
    """One outlier Gaussian in three states: three records, three table entries, one set of parameters."""
    model, outl = sharp_model(64, [(20, 1), (23, 1), (50, 1)], seed=740, tie=(20, 23, 50))
    assert outl[20] == outl[23] == outl[50]
    run_case(capi, oracle, model, outl, outlier_frames(model, outl, 300, 741), "tied pool")


def test_frame_counts(capi, oracle):
    """The partial sums' pitch is the frame count rounded up to 64 and a lane reads frames n and 32 + n: counts that put
    the last real frame in either half, a single frame, both sides of the 4- / 8-wave threshold.  The last frame lies ON an
    outlier."""
    model, outl, x0 = trio_model()
    om = oracle.DiagModel(*model)
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    for F in (1, 31, 32, 33, 63, 64, 65, WIDE_FROM - 1, WIDE_FROM, WIDE_FROM + 1):
        fr = trio_frames(model, outl, x0, F, 750 + F)
        check(g, model, outl, fr, om.score(fr.astype(np.float64)), "F = %d" % F)
    g.close()


@pytest.mark.parametrize("D,comps", [(13, 8), (24, 8), (39, 8), (47, 8), (39, 1), (39, 4), (39, 16)])
def test_dimensions_and_components(capi, oracle, D, comps):
    """One NK16 instance of the kernel per dimension.  One component per state: every outlier state is outliers only --
    and the model is not on the grouped layout at all (a pair of states fills a quarter of its eight rows:
    build_track_layout refuses the padding), so it takes the independent tracks and the merge pass, asserted as such; from
    four components on the grouped layout and the fused merge."""
    F = 333
    if comps > 1:
        model, outl, x0 = trio_model(D=D, comps=comps, seed=760 + D + comps)
        fr = trio_frames(model, outl, x0, F, 762)
    else:
        model, outl = sharp_model(96, [(3, 1), (40, 1), (94, 1)], D=D, comps=1, seed=761)
        fr = outlier_frames(model, outl, F, 762)
    # (one component per state: the outliers' share of a state is all or nothing)
    run_case(capi, oracle, model, outl, fr, "D = %d, %d components" % (D, comps), fused=comps > 1,
             need=(1, 1, 1) if comps > 1 else (1, 0, 0))


def test_pitched_output(capi, oracle):
    """aasr_gmm_score_dev_pitched on the fused path: the dense bits, the padding untouched."""
    import torch
    S = 100
    model, outl = sharp_model(S, [(7, 1), (8, 1), (40, 2), (99, 1)], comps=16, seed=770)
    fr = outlier_frames(model, outl, 9000, 771)
    dense = run_case(capi, oracle, model, outl, fr, "dense, before the pitched calls")
    g = capi.Gmm.from_arrays(*model)
    assert g.score_pitch_ok()
    d_fr = torch.from_numpy(fr).cuda()
    for pitch in (128, 103):
        padded = torch.full((len(fr), pitch), -7.0, dtype=torch.float32, device="cuda")

        def call():
            g.score_dev_pitched(d_fr, padded, pitch)
            torch.cuda.synchronize()
        scored(g, call, True)
        out = padded.cpu().numpy()
        assert np.array_equal(out[:, :S].view(np.uint32), dense.view(np.uint32)) and np.all(out[:, S:] == -7.0), pitch
    g.close()


def _diag_transform(D, logdet, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.2, 0.2, D)
    c += (logdet - c.sum()) / D
    W = np.zeros((1, D, D + 1))
    W[0][:, 1:] = np.diag(np.exp(c))
    W[0][:, 0] = 0.2 * rng.standard_normal(D)
    return W, (np.exp(c), W[0][:, 0].copy())


@pytest.mark.parametrize("logdet", [6.0, -6.0])
def test_global_transform_in_place(capi, oracle, logdet):
    """log|det| of an in-place transform enters the matrix rows at the kernel's output and the outliers' sums where they
    are merged (hyb_bias); taken off again, the untransformed bits return."""
    D = 39
    model, outl = sharp_model(64, [(9, 1), (36, 2), (62, 1)], seed=780)
    W, xf = _diag_transform(D, logdet, 781)
    fr = outlier_frames(model, outl, 400, 782, xf=xf)
    g2t = np.zeros(model[0].shape[0], np.int32)
    om = oracle.DiagModel(*model)
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    plain = scored(g, lambda: g.score(fr), True)
    g.set_cmllr(g2t, W)
    assert_path(g, model, outl)
    ref = oracle.score_adapted(om, fr.astype(np.float64), g2t, W)
    check(g, model, outl, fr, ref, "log|det| = %+g" % logdet, xf=xf, bias=logdet)
    g.set_cmllr()
    again = scored(g, lambda: g.score(fr), True)
    assert np.array_equal(plain.view(np.uint32), again.view(np.uint32))
    assert_ll(again, om.score(fr.astype(np.float64)), "transform taken off")
    g.close()


@pytest.mark.parametrize("S,picks", [(1, [(0, 1)]), (2, [(1, 1)]), (3, [(0, 1), (2, 1)]), (16, [(2, 1), (9, 1), (15, 1)]),
                                     (64, [(k, 1) for k in range(3, 64, 7)])])
def test_dense_outlier_states(capi, oracle, S, picks):
    """8 * states > S.  The density rule belongs to the PLANNER (find_outliers / engine_parts_public price such a model's
    merge as a pass of its own when they choose between its own layout and the engine parts); hyb_fuse_begin has no such
    rule, so a model that stays on its own grouped layout is merged in the close logic however dense its outlier states
    are -- measured, and asserted as what it is.  One, two and three states: a row cut whose track has no state at all."""
    assert 8 * len(picks) > S
    model, outl = sharp_model(S, picks, seed=790 + S)
    run_case(capi, oracle, model, outl, outlier_frames(model, outl, 300, 791), "S = %d, %d outlier states" % (S, len(picks)))


def test_other_arithmetics_layouts_and_budgets_take_the_merge_pass(capi, oracle):
    """A model the fused path admits, under the settings it does not: three bf16 terms, f32, independent tracks, a
    partial-sum budget smaller than the call's sums.  Each runs the merge pass and matches the oracle; back on the
    defaults the fused bits return."""
    model, outl, x0 = trio_model(seed=800)
    fr = trio_frames(model, outl, x0, 500, 801)
    ref = oracle.DiagModel(*model).score(fr.astype(np.float64))
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    first = check(g, model, outl, fr, ref, "defaults")
    for prec in (3, 0):
        g.set_precision(prec)
        assert_ll(scored(g, lambda: g.score(fr), False), ref, "precision %d" % prec)
    g.set_precision(4)
    g.set_layouts(2)
    assert g.active_layout() == 2
    assert_ll(scored(g, lambda: g.score(fr), False), ref, "independent tracks")
    g.set_layouts(7)
    L = capi.lib()
    L.aasr_debug_set_pass_bytes.argtypes = [C.c_double]
    L.aasr_debug_set_pass_bytes.restype = None
    try:
        L.aasr_debug_set_pass_bytes(float(512 * len(outl) * 4 - 1))   # (the call's sums: 512 frames x 3 states x 4 bytes)
        assert_ll(scored(g, lambda: g.score(fr), False), ref, "partial sums over the budget")
    finally:
        L.aasr_debug_set_pass_bytes(0.0)
    again = scored(g, lambda: g.score(fr), True)
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    g.close()


def test_clustering_leaves_the_fused_path(capi, oracle):
    """Gaussian clustering: the masked passes merge the outliers' exact parts themselves, the HYB instance is not
    launched; scores and exact-evaluation counts as the oracle's cluster branch, on frames that lie on the outliers."""
    model, outl, x0 = trio_model(S=128, comps=16, seed=810)
    fr = trio_frames(model, outl, x0, 500, 811)
    g2c = synth.make_clustering(model[0], 64)
    pairs = [(int(a), int(c)) for a, c in enumerate(g2c)]
    om = oracle.DiagModel(*model)
    om.set_clustering(64, pairs, 0.0, 0.25)
    want, want_n = om.score_clustered(fr.astype(np.float64), want_counts=True)
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    scored(g, lambda: g.score(fr), True)
    g.set_clustering(64, pairs)
    g.set_clustering_min_evals(0.0, 0.25)
    got = scored(g, lambda: g.score(fr), None)
    assert np.array_equal(g.cluster_exact_counts(len(fr)), want_n)
    assert_ll(got, want, "clustered")
    g.close()


@pytest.mark.parametrize("S,fused", [(65534, True), (65535, False)])
def test_the_16_bit_table_limit(capi, oracle, S, fused):
    """State and record share a 32-bit table entry, 0xffff means none: 65 534 states are the most the fused path takes.
    Four components per state (the fewest the grouped layout takes), 13 dimensions; the oracle scores a sample of the
    states."""
    D, comps = 13, 4
    picks = [(0, 1), (4097, 1), (32768, 1), (S - 1, 1)]
    model, outl = sharp_model(S, picks, D=D, comps=comps, seed=820, var_lo=0.5, var_hi=2.0)
    fr = outlier_frames(model, outl, 64, 821)
    rng = np.random.default_rng(822)
    sample = np.unique(np.concatenate([sorted(outl), [1, 2, 4096, 4098, S - 3, S - 2, S - 1], rng.choice(S, 2000, replace=False)]))
    mean, var, off, idx, w = model
    ks = (off[sample][:, None] + np.arange(comps)[None]).ravel()      # (a disjoint pool: the sample's Gaussians, in order)
    sub = oracle.DiagModel(mean[idx[ks]], var[idx[ks]], np.arange(0, len(ks) + 1, comps, dtype=np.int32),
                           np.arange(len(ks), dtype=np.int32), w[ks])
    ref = sub.score(fr.astype(np.float64))
    assert max(outl) == S - 1 and all(c >= 1 for c in coverage(model, outl, fr))
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    got = scored(g, lambda: g.score(fr), fused)
    assert_ll(got[:, sample], ref, "S = %d" % S)
    g.set_outlier_fuse(False)
    merged = scored(g, lambda: g.score(fr), False)
    assert np.array_equal(got.view(np.uint32), merged.view(np.uint32))
    g.close()


def test_repeat_and_growth(capi, oracle):
    """The partial sums' buffer grows with the frame count (hyb_fuse_begin): 64 frames, 8193, 64 again on one handle; the
    third result is the first, bit for bit."""
    model, outl, x0 = trio_model(seed=830)
    om = oracle.DiagModel(*model)
    g = capi.Gmm.from_arrays(*model)
    assert_path(g, model, outl)
    small, big = trio_frames(model, outl, x0, 64, 831), trio_frames(model, outl, x0, WIDE_FROM + 1, 832)
    first = check(g, model, outl, small, om.score(small.astype(np.float64)), "64 frames, fresh handle")
    check(g, model, outl, big, om.score(big.astype(np.float64)), "8193 frames, grown buffer")
    third = scored(g, lambda: g.score(small), True)
    assert np.array_equal(first.view(np.uint32), third.view(np.uint32))
    g.close()

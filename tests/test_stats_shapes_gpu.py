"""The statistics handle (csrc/stats.cc, stats_accum.hip) over every launch shape of its accumulation kernel.

The host picks k_stats_items' shape from the model: the dimension instance (ten of them, 8 ... 192) from the feature
dimension, the sub-block (256 / 192 / 128 / 64 frames) from the largest mixture, and whether the mixture's records are
staged in LDS from both.  tests/test_stats_gpu.py runs <40> / <24> / <8> at block 256 with staged records only.  Every
case here states the shape it expects as a literal, asserts it from the handle (capi.Stats.launch_shape), and checks the
handle against tools/fuzz_stats.py's restate() -- Mixture::accumulate / DiagonalStatisticsAccumulator::accumulate in
double, operation by operation as stats_accum.hip's header states, the frames of a pdf summed in frame order, weights
normalised by oracle.DiagModel -- and against the same posteriors summed in np.longdouble by np.sum, which shares no
summation order with the kernel.  The last test asserts that the shapes seen are the full set.

Tolerances: those of tests/test_stats_gpu.py (fuzz_stats.TOL) against the in-order restatement.  The kernel is compiled
with -ffp-contract=off and performs the restatement's operations one for one, so only the device's exp / log (one ulp)
and the grouping of a pdf's sums into items differ, at every dimension; measured on the CPU, the in-order restatement
against the extended-precision sums of the widest case here (D = 192, 118 components): gamma 1.2e-15 relative, sum_x
7e-15 absolute (at D = 39 with a pdf of 3 600 frames: 4e-15 and 2e-12), i.e. 1/800 of the tolerance and less -- no wider
value is needed for 192 dimensions.  Against the
extended-precision reference the bound is twice the tolerance: the restatement is asserted (on the host) to be within
one tolerance of it, the handle within one tolerance of the restatement.

CPU-side mutation check (a Python emulation of the kernel's LDS / slab structure in place of the handle, the same
checks): lg indexed by max_comps where M is meant, the slab carry dropped, a record read at stride rec - 2,
total < 1e-50 treated as "no accumulation" and pdf = -1 frames counted each fail cases of this module (see the
pull request text for the failing test of each)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FS = _load("fuzz_stats")
TOL2 = {q: (2 * r, 2 * a) for q, (r, a) in FS.TOL.items()}   # against the extended-precision sums (module docstring)
SEEN = set()          # (dimp, block, lds_recs) of every launch of this module
LL_INIT = 7.25        # what the caller leaves in frame_ll: skipped frames keep it

# largest mixture -> (block, records staged) at 39 dimensions (dimp 40, 82 doubles a record)
GRID39 = {4: (256, 1), 22: (256, 0), 25: (192, 1), 30: (192, 0), 34: (128, 1), 42: (128, 0), 50: (64, 1), 118: (64, 0)}
# dimension -> its instance: each at its exact width and one past the previous
DIMS = {1: 8, 8: 8, 9: 16, 16: 16, 17: 24, 31: 32, 33: 40, 47: 48, 48: 48, 49: 64, 64: 64, 65: 96, 96: 96, 97: 128,
        128: 128, 129: 192, 192: 192}
ALL_SHAPES = {(40,) + v for v in GRID39.values()} | {(n, 256, 1) for n in set(DIMS.values())} | \
             {(n, 64, 0) for n in set(DIMS.values())}


@pytest.fixture(scope="module")
def topo(capi, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("shapes") / "t.ph")
    FS.write_ph(path)
    return capi.Topology(path)


def n_items(counts):
    """work items of one call: a pdf of c frames is cut into ceil(c / 1024) pieces of equal size (stats.h)"""
    total, sizes = 0, set()
    for c in counts:
        if c == 0:
            continue
        pieces = -(-c // 1024)
        per = -(-c // pieces)
        for b in range(0, c, per):
            sizes.add(min(per, c - b))
            total += 1
    return total, sizes


def check(capi, oracle, topo, model, x, pdf, shape, cuts_list, skip_pdfs=()):
    """the frames through a fresh handle per entry of cuts_list, each against both references; -> the fetches"""
    mix_w = oracle.DiagModel(*model).mix_w
    want = FS.restate(model, mix_w, x, pdf, frame_ll_init=LL_INIT)
    ext = FS.restate(model, mix_w, x, pdf, frame_ll_init=LL_INIT, extended=True)
    assert not FS.compare(want, ext, model=model, skip_pdfs=skip_pdfs)   # the two references, on the host
    gmm = capi.Gmm.from_arrays(*model)
    outs = []
    for cuts in cuts_list:
        got, shapes = FS.run_handle(capi, gmm, topo, len(model[3]), x, pdf, cuts, frame_ll_init=LL_INIT)
        assert shapes, "no launch"
        for sh in shapes:
            SEEN.add((sh["dimp"], sh["block"], sh["lds_recs"]))
            assert (sh["dimp"], sh["block"], sh["lds_recs"], sh["max_comps"]) == shape, (sh, shape)
        if cuts is None:
            counts = np.bincount(pdf[pdf >= 0], minlength=len(model[2]) - 1)
            assert shapes[0]["items"] == n_items(counts)[0]
        worst = {}
        fails = FS.compare(got, want, worst=worst, model=model, skip_pdfs=skip_pdfs)
        print("cuts %s worst (in units of the tolerance) %s" % (cuts, {k: "%.3g" % v for k, v in worst.items()}))
        assert not fails, "\n".join(fails)
        fails = FS.compare(got, ext, tol=TOL2, model=model, skip_pdfs=skip_pdfs)
        assert not fails, "extended-precision reference:\n" + "\n".join(fails)
        outs.append(got)
    gmm.close()
    return outs, want


def ragged_sizes(M):
    """most mixtures smaller than the largest, one of a single component, one of none"""
    return [M, 1, 0, max(1, M // 2), max(1, M - 1), min(M, 3), M]


@pytest.mark.parametrize("M", sorted(GRID39))
def test_mixture_grid_at_39_dimensions(capi, oracle, topo, M):
    """every (block, staged) shape at D = 39, on a ragged tied model; items of 1, block - 1, block, block + 1 and 1 024
    frames (16 sub-blocks at block 64: the slab carry), a pdf of 3 600 frames cut into four items; once in one call,
    once over six calls with uneven cuts"""
    block, staged = GRID39[M]
    rng = np.random.default_rng(1000 + M)
    sizes = ragged_sizes(M)
    model = FS.make_model(rng, 39, sizes, zero_weights=1)
    counts = [block + 1, 1, 5, block - 1, 1024, block, 3600]
    assert {1, block - 1, block, block + 1, 1024, 900} <= n_items(counts)[1]
    x, pdf = FS.make_frames(rng, model, counts)
    F = len(pdf)
    cuts = [0, 1, 300, 301 + block, F // 2 + 7, F - 1, F]
    outs, want = check(capi, oracle, topo, model, x, pdf, (40, block, staged, M), [None, cuts])
    assert (want["count"] == np.where(np.array(sizes) > 0, counts, 0)).all()
    assert want["feacount"][-3:].sum() == 0 and outs[0]["feacount"][-3:].sum() == 0   # Gaussians of no mixture


@pytest.mark.parametrize("D", sorted(DIMS))
@pytest.mark.parametrize("M", [3, 118])
def test_dimension_grid(capi, oracle, topo, D, M):
    """every dimension instance, with a small mixture (block 256, records staged) and the largest one allowed (block 64,
    records read from global memory: 118 records fit no LDS next to the posteriors at any dimension)"""
    block, staged = (256, 1) if M == 3 else (64, 0)
    rng = np.random.default_rng(2000 + 7 * D + M)
    model = FS.make_model(rng, D, ragged_sizes(M), zero_weights=1)
    counts = [block + 1, 1, 5, block - 1, 330, block, 2 * block + 3]
    x, pdf = FS.make_frames(rng, model, counts, skipped=9)
    F = len(pdf)
    check(capi, oracle, topo, model, x, pdf, (DIMS[D], block, staged, M), [None, [0, 2, F // 3, F]])


def test_too_wide_model_is_refused(capi, topo):
    rng = np.random.default_rng(5)
    model = FS.make_model(rng, 193, [2, 1])
    gmm = capi.Gmm.from_arrays(*model)
    with pytest.raises(capi.AasrError) as ei:
        capi.Stats(gmm, topo, 3)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "193" in ei.value.msg
    gmm.close()


def test_too_large_mixture_is_refused_at_create(capi, oracle, topo):
    """119 components at D = 39: 64 frames of posteriors no longer fit 60 KB.  Refused where the model is known, at
    aasr_stats_create (no handle, nothing launched); the model stays usable and a handle of another model that was
    accumulating meanwhile is unchanged and goes on."""
    rng = np.random.default_rng(6)
    ok_model = FS.make_model(rng, 39, [118, 2, 0])
    x, pdf = FS.make_frames(rng, ok_model, [70, 3, 2])
    g_ok = capi.Gmm.from_arrays(*ok_model)
    import torch
    d_x = torch.tensor(x, device="cuda")
    st = capi.Stats(g_ok, topo, len(ok_model[3]))
    st.accumulate_dev(d_x[:40], pdf[:40])
    big = FS.make_model(rng, 39, [119, 2])
    g_big = capi.Gmm.from_arrays(*big)
    with pytest.raises(capi.AasrError) as ei:
        capi.Stats(g_big, topo, len(big[3]))
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "119" in ei.value.msg
    assert np.isfinite(g_big.score_f64(x[:4])).all()           # the model itself is fine
    st.accumulate_dev(d_x[40:], pdf[40:])
    got = st.fetch()
    want = FS.restate(ok_model, oracle.DiagModel(*ok_model).mix_w, x, pdf)
    assert not FS.compare(got, want)
    st.close()
    g_ok.close()
    g_big.close()


def edge_model(rng, D=39):
    """pdf 0: three components, one of weight 0 on a Gaussian of its own; pdf 1: every total in (1e-300, 1e-50); pdf 2:
    subnormal likelihoods; pdf 3: Gaussians with a zero and a negative variance; pdf 4: no components; pdf 5: ordinary"""
    sizes = [3, 2, 2, 2, 0, 4]
    G = 13 + 2
    mean = rng.standard_normal((G, D)) * (2.0 / np.sqrt(D))
    var = rng.uniform(1.0, 3.0, (G, D))
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    idx = np.arange(13, dtype=np.int32)
    w = rng.uniform(0.2, 1.0, 13)
    w[1] = 0.0
    mean[3:7], var[3:7] = 0.0, 1.0          # pdfs 1 and 2: unit Gaussians at the origin, frames placed at a distance
    var[7, 5] = 0.0
    var[8, 11] = -1.0
    return mean, var, off, idx, w


def edge_frames(rng, model, n=150, skipped=40):
    D = model[0].shape[1]
    counts = [n, n, n, n, 7, n]
    x, pdf = FS.make_frames(rng, model, counts, skipped=skipped)
    # |x|^2 = 800: ll = -400, total 1e-174; |x|^2 = 1428: ll = -714, likelihood 8e-311 (subnormal below 2.2e-308)
    for s, r2, noise in ((1, 800.0, 0.3), (2, 1428.0, 0.005)):
        rows = pdf == s
        x[rows] = np.sqrt(r2 / D) + noise * rng.standard_normal((int(rows.sum()), D))
    return x, pdf, counts


def test_arithmetic_edges(capi, oracle, topo):
    rng = np.random.default_rng(77)
    model = edge_model(rng)
    x, pdf, counts = edge_frames(rng, model)
    assert (np.diff(np.nonzero(pdf == -1)[0]) > 1).any()           # the skipped frames are interleaved
    # pdf 2 is not compared by value: one ulp of exp is a large relative error on a subnormal
    (got, cut), want = check(capi, oracle, topo, model, x, pdf, (40, 256, 1, 4), [None, [0, 11, 400, len(pdf)]], skip_pdfs=(2,))
    off = model[2]
    t1, t2 = want["total"][pdf == 1], want["total"][pdf == 2]
    assert ((t1 > 1e-300) & (t1 < 1e-50)).all() and ((t2 > 0) & (t2 < 2.2250738585072014e-308)).all()
    for g in (got, cut):
        # totals in (1e-300, 1e-50): the frames count and their posteriors accumulate; log(1e-50) per frame
        assert g["count"][1] == counts[1] and g["mix_gamma"][off[1]:off[2]].sum() == pytest.approx(counts[1], rel=1e-12)
        np.testing.assert_allclose(g["frame_ll"][pdf == 1], np.log(1e-50), rtol=1e-13)
        assert g["mixture_ll"][1] == pytest.approx(counts[1] * np.log(1e-50), rel=1e-12)
        assert (g["feacount"][3:5] == counts[1]).all() and (g["sum_xx"][3:5] > 0).all()
        # subnormal likelihoods: invariants only
        assert g["count"][2] == counts[2] == int((t2 > 0).sum()) and (g["feacount"][5:7] == counts[2]).all()
        assert abs(g["mix_gamma"][off[2]:off[3]].sum() - counts[2]) <= 1e-9
        assert all(np.isfinite(g[q]).all() for q in ("gamma", "aux_gamma", "sum_x", "sum_xx", "mix_gamma", "mixture_ll"))
        np.testing.assert_allclose(g["frame_ll"][pdf == 2], np.log(1e-50), rtol=1e-13)
        # the component of weight 0: gamma 0 on every frame, its Gaussian's feacount advances
        assert g["mix_gamma"][1] == 0.0 and g["gamma"][1] == 0.0 and (g["sum_x"][1] == 0.0).all()
        assert g["feacount"][1] == counts[0] > 0
        # a mixture without components: safe_log(0) per frame, nothing else
        assert g["count"][4] == 0 and g["mixture_ll"][4] == pytest.approx(counts[4] * np.log(1e-50), rel=1e-12)
        # skipped frames keep the caller's value and count nowhere
        assert (g["frame_ll"][pdf == -1] == LL_INIT).all() and (g["frame_ll"][pdf >= 0] != LL_INIT).all()
        assert g["count"].sum() == sum(counts) - counts[4]
    # non-positive variances: precision 0 in that dimension, constant 0 (gmm_build_f64's rule), restated
    _, rprec, rcst, _ = FS.records(model, oracle.DiagModel(*model).mix_w)
    assert rprec[7, 5] == 0.0 and rprec[8, 11] == 0.0 and rcst[7] == 0.0 and rcst[8] == 0.0 and (rcst[9:] < 0).all()
    assert got["count"][3] == counts[3] and (got["gamma"][7:9] > 0).all()


def test_skipped_frames_do_not_change_the_others(capi, oracle, topo):
    """the same frames with and without pdf = -1 frames between them: the same bytes"""
    rng = np.random.default_rng(78)
    model = FS.make_model(rng, 39, ragged_sizes(25))
    x, pdf = FS.make_frames(rng, model, [400, 1, 5, 191, 193, 30, 1500], skipped=300)
    gmm = capi.Gmm.from_arrays(*model)
    K = len(model[3])
    a, _ = FS.run_handle(capi, gmm, topo, K, x, pdf)
    keep = pdf >= 0
    b, _ = FS.run_handle(capi, gmm, topo, K, np.ascontiguousarray(x[keep]), np.ascontiguousarray(pdf[keep]))
    gmm.close()
    for q in ("feacount", "count", "gamma", "aux_gamma", "sum_x", "sum_xx", "mix_gamma", "mixture_ll"):
        assert a[q].tobytes() == b[q].tobytes(), q
    assert a["frame_ll"][keep].tobytes() == b["frame_ll"].tobytes()
    assert a["count"].sum() == int(keep.sum()) - 5


def test_out_of_range_pdf_is_refused_and_accumulates_nothing(capi, oracle, topo):
    import torch
    rng = np.random.default_rng(79)
    model = FS.make_model(rng, 24, [4, 2, 3])
    x, pdf = FS.make_frames(rng, model, [50, 20, 30])
    gmm = capi.Gmm.from_arrays(*model)
    st = capi.Stats(gmm, topo, len(model[3]))
    d_x = torch.tensor(x, device="cuda")
    st.accumulate_dev(d_x[:60], pdf[:60])
    bad = pdf[60:].copy()
    bad[-1] = 3                                  # S = 3
    d_ll = torch.full((len(bad),), LL_INIT, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.AasrError) as ei:
        st.accumulate_dev(d_x[60:], bad, d_ll)
    assert ei.value.code == capi.AASR_ERR_INVALID and "out of range" in ei.value.msg
    assert (d_ll.cpu().numpy() == LL_INIT).all()
    got = st.fetch()
    want = FS.restate(model, oracle.DiagModel(*model).mix_w, x[:60], pdf[:60])
    assert not FS.compare(got, want)
    st.accumulate_dev(d_x[60:], pdf[60:])        # the handle goes on
    assert not FS.compare(st.fetch(), FS.restate(model, oracle.DiagModel(*model).mix_w, x, pdf))
    st.close()
    gmm.close()


@pytest.mark.parametrize("M", [4, 25, 34, 118])
def test_two_handles_return_the_same_bytes(capi, topo, M):
    """no atomics, fixed order: one case per block size, two fresh handles, identical bytes"""
    rng = np.random.default_rng(3000 + M)
    model = FS.make_model(rng, 39, ragged_sizes(M), zero_weights=1)
    x, pdf = FS.make_frames(rng, model, [700, 1, 5, 63, 1024, 257, 2100], skipped=11)
    gmm = capi.Gmm.from_arrays(*model)
    a, sa = FS.run_handle(capi, gmm, topo, len(model[3]), x, pdf)
    b, sb = FS.run_handle(capi, gmm, topo, len(model[3]), x, pdf)
    gmm.close()
    assert sa == sb and sa[0]["block"] == GRID39[M][0]
    for q in ("feacount", "count", "gamma", "aux_gamma", "sum_x", "sum_xx", "mix_gamma", "mixture_ll", "frame_ll"):
        assert a[q].tobytes() == b[q].tobytes(), q


def test_zz_every_launch_shape_ran():
    """last in the module: all ten dimension instances, all four blocks with both staging values at dimp 40, and both
    staging values of every dimension instance were launched (and asserted, case by case, above)"""
    assert SEEN == ALL_SHAPES, (sorted(ALL_SHAPES - SEEN), sorted(SEEN - ALL_SHAPES))
    assert {s[0] for s in SEEN} == {8, 16, 24, 32, 40, 48, 64, 96, 128, 192}
    assert {(s[1], s[2]) for s in SEEN if s[0] == 40} == {(b, l) for b in (256, 192, 128, 64) for l in (0, 1)}

"""The log-likelihood-only handle (csrc/seg_loglik.cc, seg_loglik.hip): per frame safe_log(likelihood) of the one pdf its
segmentation gives it.

* Where capi.Stats accepts the model, the yardstick is the existing accumulation kernel: SegLL's values are the BYTES of
  the frame_ll that Stats.accumulate_dev writes for the same frames (both kernels perform the same operations in the
  same order under -ffp-contract=off; the padded dimensions of k_stats_items add +0).
* Beyond k_stats_items' limits (more than 118 components, more than 192 dimensions) the references are
  tools/fuzz_stats.py's posteriors() in double, with fuzz_stats.TOL["frame_ll"], and in np.longdouble with twice that:
  the project's own tolerances for this quantity (tests/test_stats_shapes_gpu.py's docstring derives them: the
  restatement's operations one for one, the device's exp / log within an ulp; against extended precision one tolerance
  for the restatement and one for the handle).
* Edges, against the restatement: zero weights, non-positive variances, totals between 1e-300 and 1e-50, subnormal
  likelihoods, a NaN and an Inf in a frame.
* The same input gives the same bytes, whatever the calls are cut into; the LDS of a workgroup stays within 64 KB.
* Full-covariance and subspace pools and model-side transforms are refused at create."""
import importlib.util
import os

import numpy as np
import pytest

from aaltoasr_amd import synth

pytestmark = pytest.mark.gpu
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FS = _load("fuzz_stats")
LL_INIT = 7.25        # what the caller leaves in frame_ll: skipped frames keep it
SIZES = [0, 1, 2, 16, 55, 118]
COUNTS = [0, 1, 255, 256, 257, 1025]


@pytest.fixture(scope="module")
def topo(capi, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("segll") / "t.ph")
    FS.write_ph(path)
    return capi.Topology(path)


def segll(capi, gmm, x, pdf, cuts=None, handle=None):
    """the frames through SegLL in the calls cuts[i]:cuts[i+1] -> (frame_ll, launch shape of the last call)"""
    import torch
    h = handle or capi.SegLL(gmm)
    d_x = torch.tensor(np.ascontiguousarray(x), device="cuda")
    d_ll = torch.full((max(1, len(pdf)),), LL_INIT, dtype=torch.float64, device="cuda")
    cuts = [0, len(pdf)] if cuts is None else cuts
    for b, e in zip(cuts[:-1], cuts[1:]):
        h.score_dev(d_x[b:e], pdf[b:e], d_ll[b:e])
    torch.cuda.synchronize()
    shape = h.launch_shape()
    if handle is None:
        h.close()
    return d_ll.cpu().numpy()[:len(pdf)], shape


def stats_ll(capi, gmm, topo, K, x, pdf):
    got, _ = FS.run_handle(capi, gmm, topo, K, x, pdf, None, frame_ll_init=LL_INIT)
    return got["frame_ll"]


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("turn,D", list(enumerate([1, 8, 39, 40, 64, 127])))
def test_bytes_of_the_accumulation_kernels_frame_ll(capi, topo, turn, D):
    """mixtures of 0 ... 118 components (Gaussians shared between them, a zero weight), pdfs owning 0, 1, 255, 256, 257
    and 1 025 rows -- turned against the mixtures with the dimension, so that every mixture size meets several row
    counts -- skipped rows, rows shuffled"""
    rng = np.random.default_rng(100 + D)
    model = FS.make_model(rng, D, SIZES, zero_weights=1)
    counts = COUNTS[turn:] + COUNTS[:turn]
    x, pdf = FS.make_frames(rng, model, counts, skipped=37)
    gmm = capi.Gmm.from_arrays(*model)
    want = stats_ll(capi, gmm, topo, len(model[3]), x, pdf)
    got, shape = segll(capi, gmm, x, pdf)
    items = sum(-(-c // 256) for c in counts)
    assert shape["items"] == items and shape["item_rows"] == 256 and shape["lds_bytes"] <= 64 * 1024, shape
    assert shape["stride"] % 2 == 1 and shape["stride"] >= D and shape["sub"] * shape["stride"] * 8 == shape["lds_bytes"]
    assert (got[pdf < 0] == LL_INIT).all() and (want[pdf < 0] == LL_INIT).all()
    diff = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]
    print("D %d: %d frames, %d differ" % (D, len(pdf), len(diff)))
    assert len(diff) == 0, (diff[:5], got[diff[:5]], want[diff[:5]], pdf[diff[:5]])
    assert len(set(got[pdf == SIZES.index(0)])) <= 1 and (got[pdf == 0] == np.log(1e-50)).all()   # the empty mixture
    gmm.close()


def test_out_of_range_pdfs_are_refused_as_by_the_accumulation(capi, topo):
    """a pdf >= the number of states: AASR_ERR_INVALID from both handles, naming the frame, and nothing is written"""
    import torch
    rng = np.random.default_rng(7)
    model = FS.make_model(rng, 8, [2, 3])
    x, pdf = FS.make_frames(rng, model, [5, 6], skipped=2)
    pdf = pdf.copy()
    pdf[4] = 2
    gmm = capi.Gmm.from_arrays(*model)
    d_x = torch.tensor(x, device="cuda")
    for make, call in ((lambda: capi.Stats(gmm, topo, 5), "accumulate_dev"), (lambda: capi.SegLL(gmm), "score_dev")):
        h = make()
        d_ll = torch.full((len(pdf),), LL_INIT, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.AasrError) as ei:
            getattr(h, call)(d_x, pdf, d_ll)
        assert ei.value.code == capi.AASR_ERR_INVALID and "pdf 2 of frame 4 out of range" in ei.value.msg, ei.value.msg
        torch.cuda.synchronize()
        assert (d_ll.cpu().numpy() == LL_INIT).all()
        h.close()
    gmm.close()


def restated(oracle, model, x, pdf, dtype=np.float64):
    mix_w = oracle.DiagModel(*model).mix_w
    rmean, rprec, rcst, rw = FS.records(model, mix_w)
    off = model[2]
    out = np.full(len(pdf), LL_INIT)
    for s in range(len(off) - 1):
        rows = np.nonzero(pdf == s)[0]
        if len(rows):
            r = slice(off[s], off[s + 1])
            out[rows] = FS.posteriors(x[rows], rmean[r], rprec[r], rcst[r], rw[r], dtype=dtype)[2].astype(np.float64)
    return out


def within(got, want, tol, scale=1.0):
    rtol, atol = tol
    lim = scale * (atol + rtol * np.abs(want))
    err = np.abs(got - want)
    print("worst error %.3g of the tolerance" % float((err / lim).max()))
    return (err <= lim).all()


@pytest.mark.parametrize("D,sizes", [(39, [119, 300, 2]), (193, [119, 3, 0]), (256, [300, 5, 1])])
def test_beyond_the_accumulation_kernels_limits(capi, oracle, topo, D, sizes):
    """more than 118 components and more than 192 dimensions: one kernel, its loops over D and M from memory; the rows of
    a 257-row pdf cross an item, and at these dimensions an item takes several LDS sub-blocks"""
    rng = np.random.default_rng(300 + D)
    model = FS.make_model(rng, D, sizes, zero_weights=1)
    x, pdf = FS.make_frames(rng, model, [257, 70, 33], skipped=5)
    gmm = capi.Gmm.from_arrays(*model)
    got, shape = segll(capi, gmm, x, pdf)
    assert shape["lds_bytes"] <= 64 * 1024 and shape["sub"] >= 1, shape
    if D >= 193:
        assert shape["sub"] < 64, shape     # several sub-blocks per item
    assert np.isfinite(got).all() and (got[pdf < 0] == LL_INIT).all()
    assert within(got, restated(oracle, model, x, pdf), FS.TOL["frame_ll"])
    assert within(got, restated(oracle, model, x, pdf, np.longdouble), FS.TOL["frame_ll"], 2.0)
    gmm.close()


def test_edges_against_the_restatement(capi, oracle, topo):
    """zero weights, non-positive variances (precision 0, an "invalid" Gaussian's constant), frames so far out that the
    total falls between 1e-300 and 1e-50 (log(1e-50) exactly), is subnormal or 0, a NaN and an Inf"""
    rng = np.random.default_rng(11)
    D = 6
    model = FS.make_model(rng, D, [3, 2, 4, 1])
    mean, var, off, idx, w = model
    idx[off[3]] = len(mean) - 1             # a Gaussian of its own for pdf 3 (one of the pool's spares)
    w[off[0] + 1] = 0.0
    w[off[1]] = 0.0
    var[idx[off[2]], 2] = 0.0               # non-positive variances
    var[idx[off[2] + 1], 4] = -1.5
    assert len(mean) - 1 not in idx[:off[3]]
    x, pdf = FS.make_frames(rng, model, [40, 10, 40, 60])
    s3 = np.nonzero(pdf == 3)[0]
    g = idx[off[3]]
    sd = np.sqrt(var[g])
    # distance r in every dimension: log lik = const - 0.5 D r^2; r = 7.2 -> about e^-158 (below 1e-50, above 1e-300),
    # r = 15.4 -> about e^-714 (subnormal), r = 16.5 -> 0
    for k, r in enumerate([7.2, 8.5, 15.4, 15.6, 16.5]):
        x[s3[k]] = mean[g] + r * sd
    x[s3[10], 1] = np.nan
    x[s3[11], 3] = np.inf
    gmm = capi.Gmm.from_arrays(*model)
    got, _ = segll(capi, gmm, x, pdf)
    mix_w = oracle.DiagModel(*model).mix_w
    rmean, rprec, rcst, rw = FS.records(model, mix_w)
    total = FS.posteriors(x[s3], rmean[off[3]:off[4]], rprec[off[3]:off[4]], rcst[off[3]:off[4]], rw[off[3]:off[4]])[3]
    assert 1e-300 < total[0] < 1e-50 and 1e-300 < total[1] < 1e-50, total[:2]
    assert 0 < total[2] < 2.3e-308 and 0 < total[3] < 2.3e-308 and total[4] == 0, total[2:5]
    floor = np.log(1e-50)
    assert (got[s3[:5]] == floor).all(), got[s3[:5]]
    with np.errstate(all="ignore"):
        want = restated(oracle, model, x, pdf)
    # a NaN total is not below 1e-50: log(NaN), as in k_stats_items (the restatement's np.where has no such branch);
    # the Inf gives inf * inf * precision, exp(-inf) = 0 -> the floor
    assert np.isnan(got[s3[10]])
    assert got[s3[11]] == floor and want[s3[11]] == floor
    keep = np.ones(len(pdf), bool)
    keep[s3[10]] = False
    assert np.isfinite(got[keep]).all()
    assert within(got[keep], want[keep], FS.TOL["frame_ll"])
    # and the accumulation kernel's bytes on the same frames
    acc = stats_ll(capi, gmm, topo, len(idx), x, pdf)
    assert same_bytes(got[keep], acc[keep]) and np.isnan(acc[s3[10]])
    gmm.close()


def test_same_bytes_from_two_runs_and_from_uneven_calls(capi, topo):
    rng = np.random.default_rng(21)
    model = FS.make_model(rng, 39, [16, 3, 55])
    x, pdf = FS.make_frames(rng, model, [600, 257, 300], skipped=11)
    gmm = capi.Gmm.from_arrays(*model)
    F = len(pdf)
    a, _ = segll(capi, gmm, x, pdf)
    b, _ = segll(capi, gmm, x, pdf)
    h = capi.SegLL(gmm)
    assert h.launch_shape() == {"items": 0, "sub": 0, "lds_bytes": 0, "stride": 0, "item_rows": 0}
    c, _ = segll(capi, gmm, x, pdf, cuts=[0, 1, F // 3 + 5, F], handle=h)
    h.close()
    assert same_bytes(a, b) and same_bytes(a, c)
    gmm.close()


def test_lds_stays_within_64_kb_at_256_dimensions(capi, topo):
    rng = np.random.default_rng(31)
    model = FS.make_model(rng, 256, [2])
    x, pdf = FS.make_frames(rng, model, [256])
    gmm = capi.Gmm.from_arrays(*model)
    _, shape = segll(capi, gmm, x, pdf)
    assert shape == {"items": 1, "sub": 31, "lds_bytes": 31 * 257 * 8, "stride": 257, "item_rows": 256}, shape
    assert shape["lds_bytes"] <= 64 * 1024
    gmm.close()


def test_models_the_accumulation_refuses_are_refused_at_create(capi, oracle, tmp_path):
    """full-covariance Gaussians, subspace Gaussians, model-side transforms: AASR_ERR_UNSUPPORTED, no handle"""
    rng = np.random.default_rng(41)
    D = 5
    mean, var, off, idx, w = synth.make_model(D=D, G=6, S=2, comps=3, seed=3)
    cov = np.array([np.diag(v) for v in var])
    full = capi.Gmm.from_full(mean, cov, off, idx, w)
    with pytest.raises(capi.AasrError) as ei:
        capi.SegLL(full)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "full-covariance" in ei.value.msg
    full.close()
    # a precision-subspace pool (a pcgmm Gaussian beside diagonal ones)
    a = rng.standard_normal((D, D))
    basis = np.array([a @ a.T / D + np.eye(D)])
    entries = [("precision_subspace", 7, basis)]
    entries += [("pcgmm", 7, rng.standard_normal(D), np.array([1.0]))] + \
               [("diag", rng.standard_normal(D), np.ones(D)) for _ in range(5)]
    base = str(tmp_path / "sub")
    oracle.write_gk_subspace(base + ".gk", D, entries)
    oracle.write_mc(base + ".mc", off, idx, w)
    oracle.write_ph(base + ".ph", 2)
    sub = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
    with pytest.raises(capi.AasrError) as ei:
        capi.SegLL(sub)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "subspace" in ei.value.msg
    sub.close()
    # a model-side transform, set and removed again
    diag = capi.Gmm.from_arrays(mean, var, off, idx, w)
    W = np.zeros((1, D, D + 1))
    W[0, :, 1:] = np.eye(D) * 1.1
    diag.set_cmllr(np.zeros(len(mean), np.int32), W)
    with pytest.raises(capi.AasrError) as ei:
        capi.SegLL(diag)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "transforms" in ei.value.msg
    diag.set_cmllr()
    capi.SegLL(diag).close()
    diag.close()

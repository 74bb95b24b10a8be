"""The weighted pass 1 of the CMLLR statistics handle (csrc/mllr_entries.hip, aasr_mllr_accumulate_weighted_dev): frames
with lists of (pdf, weight) entries uploaded from NumPy.

Yardstick: tools/mllr_bw_restate.py.  collect() is MllrTrainer::collect_data once per (pdf, probability) of a frame, in
double in the reference's order; collect(extended=True) forms the same sums in np.longdouble in another order.  The rule
is check() of tests/test_mllr_gpu.py: every case's restatement meets that file's TOL against the extended sums on the
host, and the handle is within 4 x the case's own restatement-to-extended distance (never below 4 x 4 roundings of a
double) of the restatement, within twice that of the extended sums.

With one entry of weight 1.0 per frame the call must leave the bytes of aasr_mllr_accumulate_dev: 1.0 * x is x, the
frames are cut into the same launches and chunks, and passes 2 and 3 are the same kernels."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"G": 4 * 2.9e-14, "k": 4 * 5.0e-14, "beta": 4 * 9.7e-15}     # tests/test_mllr_gpu.py
CHUNK = 1024
EPS = 2.0 ** -52


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MB = _load("mllr_bw_restate")
MR = MB.MR


def upload(lists):
    import torch
    off, pdf, weight = MB.flatten(lists)
    return torch.tensor(off, device="cuda"), torch.tensor(pdf, device="cuda"), torch.tensor(weight, device="cuda")


def run_weighted(capi, gmm, x, lists, cuts=None, h=None, fetch=True):
    import torch
    own = h is None
    h = h or capi.Mllr(gmm)
    d_x = torch.tensor(x, device="cuda")
    d_off, d_pdf, d_w = upload(lists)
    cuts = cuts or [0, len(lists)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            h.accumulate_weighted_dev(d_x[a:b], d_off[a:b + 1], d_pdf, d_w)      # the offsets stay absolute
    out = h.fetch() if fetch else None
    if own:
        h.close()
    return out


def run_plain(capi, gmm, x, pdf, cuts=None):
    import torch
    h = capi.Mllr(gmm)
    d_x = torch.tensor(x, device="cuda")
    cuts = cuts or [0, len(pdf)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            h.accumulate_dev(d_x[a:b], pdf[a:b])
    out = h.fetch()
    h.close()
    return out


def errs(got, want):
    return {"G": MR.rel_err(got[0], want[0]), "k": MR.rel_err(got[1], want[1]),
            "beta": abs(float(got[2]) - float(want[2])) / max(float(want[2]), 1e-300)}


def check_rule(got, want, ext, what=""):
    e = errs(want, ext)
    print("%s restatement against extended sums %s" % (what, {q: "%.3g" % v for q, v in e.items()}))
    assert all(e[q] <= TOL[q] for q in TOL), e                       # the two references, on the host
    tol = {q: 4 * max(e[q], 4 * EPS) for q in TOL}
    e1, e2 = errs(got, want), errs(got, ext)
    print("%s handle against restatement %s, against extended %s" %
          (what, {q: "%.3g" % v for q, v in e1.items()}, {q: "%.3g" % v for q, v in e2.items()}))
    assert all(e1[q] <= tol[q] for q in TOL), ("restatement", e1, tol)
    assert all(e2[q] <= 2 * tol[q] for q in TOL), ("extended", e2, tol)
    assert (got[0] == got[0].transpose(0, 2, 1)).all()


def random_lists(rng, n, S, most=6, long_at=None, long_len=40):
    lists = []
    for f in range(n):
        m = long_len if f == long_at else int(rng.integers(0, most + 1))
        w = rng.uniform(0.05, 1.0, m)
        w = w / w.sum() if m else w
        lists.append([(int(rng.integers(0, S)), float(w[j])) for j in range(m)])
    return lists


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 3 * CHUNK + 77])
def test_one_entry_of_weight_one_is_the_plain_call_byte_for_byte(capi, n):
    rng = np.random.default_rng(700 + n)
    skipped = min(n // 8, 60)
    rest = n - skipped
    counts = [rest - 3 * (rest // 4), rest // 4, rest // 4, rest // 4]
    model, x, pdf = MR.make_case(rng, 39, [16, 8, 16, 1], counts, skipped=skipped)
    assert len(pdf) == n and (pdf == -1).sum() == skipped
    lists = [[(int(p), 1.0)] if p >= 0 else [] for p in pdf]        # a skipped frame is a frame without entries
    gmm = capi.Gmm.from_arrays(*model)
    cuts_list = [None]
    if n > 4:
        cuts_list.append(sorted(set([0, 1, 3, n // 3, min(n, CHUNK + 3), n - 1, n])))
    for cuts in cuts_list:
        a = run_plain(capi, gmm, x, pdf, cuts)
        b = run_weighted(capi, gmm, x, lists, cuts)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], cuts
        assert a[2] > 0
    gmm.close()


@pytest.mark.parametrize("D,n,sizes", [(1, 300, [3, 1, 2]), (15, 300, [3, 1, 2]), (16, 300, [3, 1, 2]), (63, 300, [3, 1, 2]),
                                       (39, 2310, [4, 2, 3, 1])])
def test_random_entries_against_the_restatement(capi, D, n, sizes):
    """0 to 6 entries a frame, one frame with 40 (more rounds than any other frame of its workgroup), several chunks at
    39 dimensions; as one call and cut unevenly"""
    rng = np.random.default_rng(800 + D)
    S = len(sizes)
    model, x, _ = MR.make_case(rng, D, sizes, [n // S + (1 if s < n % S else 0) for s in range(S)])
    assert len(x) == n
    lists = random_lists(rng, n, S, long_at=n // 2 + 7)
    assert max(len(l) for l in lists) == 40 and min(len(l) for l in lists) == 0
    want, ext = MB.collect(model, x, lists), MB.collect(model, x, lists, extended=True)
    gmm = capi.Gmm.from_arrays(*model)
    for cuts in (None, [0, 2, n // 3, n // 2 + 8, n]):
        check_rule(run_weighted(capi, gmm, x, lists, cuts), want, ext, "D %d cuts %s:" % (D, cuts))
    gmm.close()


def test_edges(capi):
    """a weight of 1e-300; frames far from every mean under two pdfs (both sums 0: nothing added, beta unchanged); frames
    where one of the two pdfs underflows and the other does not; pdf indices -1 and n_states (skipped, never
    dereferenced); a zero and a negative variance (precision 0 in the likelihood, no weight in that dimension's sums)"""
    rng = np.random.default_rng(91)
    D = 39
    mean, var, off, idx, w = MR.FS.make_model(rng, D, [3, 2, 4, 2])
    S, G0 = len(off) - 1, len(mean)
    mean, var, idx = np.vstack([mean, mean[:2] + 60.0]), np.vstack([var, var[:2]]), idx.copy()
    idx[off[3]:off[4]] = [G0, G0 + 1]                                # pdf 3 has Gaussians of its own, far from every frame
    model = (mean, var, off, idx, w)
    var[idx[off[1]], 5] = 0.0
    var[idx[off[1] + 1], 11] = -1.0
    x, pdf = MR.FS.make_frames(rng, model, [90, 80, 70, 0])
    n = len(x)
    lists = [[(int(p), 0.6), (int((p + 1) % 3), 0.4)] for p in pdf]
    far = np.arange(0, 20)
    x[far] += 200.0                                                  # far from pdf 3's means too
    for f in far:
        lists[f] = [(0, 0.5), (2, 0.5)]
    half = np.arange(20, 40)                                         # pdf 3 underflows here, the frame's own pdf does not
    for f in half:
        lists[f] = [(3, 0.5), (int(pdf[f]), 0.5)]
    lists[40] = [(int(pdf[40]), 1e-300), (int(pdf[40]), 1.0 - 1e-300)]
    lists[41] = [(-1, 0.3), (int(pdf[41]), 0.4), (S, 0.3)]
    lists[42] = [(S, 1.0)]
    post = MB.posteriors(model, x, lists)
    assert all(g.sum() == 0 for f in far for _, g in post[f])
    assert all(post[f][0][1].sum() == 0 and post[f][1][1].sum() > 0.49 for f in half)
    assert post[41][0] is None and post[41][2] is None and post[42][0] is None
    assert 0 < post[40][0][1].sum() < 1e-299
    want, ext = MB.collect(model, x, lists), MB.collect(model, x, lists, extended=True)
    gmm = capi.Gmm.from_arrays(*model)
    got = run_weighted(capi, gmm, x, lists)
    check_rule(got, want, ext, "edges:")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the far frames alone, the skipped entries alone: nothing at all
    G, k, beta = run_weighted(capi, gmm, np.ascontiguousarray(x[far]), [lists[f] for f in far])
    assert beta == 0.0 and not G.any() and not k.any()
    G, k, beta = run_weighted(capi, gmm, np.ascontiguousarray(x[42:43]), [lists[42]])
    assert beta == 0.0 and not G.any() and not k.any()
    # ... and with them left out the sums keep their bytes when the chunk's other frames are the same
    quiet = [([] if f in set(far.tolist()) or f == 42 else lists[f]) for f in range(n)]
    again = run_weighted(capi, gmm, x, quiet)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2]
    gmm.close()


def test_two_runs_give_equal_bytes_and_reset(capi):
    rng = np.random.default_rng(92)
    model, x, _ = MR.make_case(rng, 39, [5, 3, 2], [900, 700, 500])
    lists = random_lists(rng, len(x), 3, long_at=1100)
    gmm = capi.Gmm.from_arrays(*model)
    a = run_weighted(capi, gmm, x, lists)
    b = run_weighted(capi, gmm, x, lists)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]   # no atomics, fixed order
    h = capi.Mllr(gmm)
    run_weighted(capi, gmm, x[:700], lists[:700], h=h)
    h.reset()
    c = run_weighted(capi, gmm, x, lists, h=h)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[2] == a[2]
    h.close()
    gmm.close()


def test_plain_and_weighted_calls_mix_on_one_handle(capi):
    import torch
    rng = np.random.default_rng(93)
    model, x, pdf = MR.make_case(rng, 39, [4, 2, 3], [500, 400, 300], skipped=15)
    x2, _ = MR.FS.make_frames(rng, model, [300, 300, 200])
    lists = random_lists(rng, len(x2), 3)
    want = MB.add(MR.collect(model, x, pdf), MB.collect(model, x2, lists))
    ext = MB.add(MR.collect(model, x, pdf, extended=True), MB.collect(model, x2, lists, extended=True))
    gmm = capi.Gmm.from_arrays(*model)
    for order in ("plain first", "weighted first"):
        h = capi.Mllr(gmm)
        if order == "plain first":
            h.accumulate_dev(torch.tensor(x, device="cuda"), pdf)
        run_weighted(capi, gmm, x2, lists, h=h, fetch=False)
        if order != "plain first":
            h.accumulate_dev(torch.tensor(x, device="cuda"), pdf)
        check_rule(h.fetch(), want, ext, order + ":")
        h.close()
    gmm.close()


def test_bad_arguments(capi):
    import torch
    rng = np.random.default_rng(94)
    model, x, _ = MR.make_case(rng, 5, [2, 1], [10, 10])
    gmm = capi.Gmm.from_arrays(*model)
    h = capi.Mllr(gmm)
    L = capi.lib()
    d_x = torch.tensor(x, device="cuda")
    d_off = torch.zeros(len(x) + 1, dtype=torch.int64, device="cuda")
    assert L.aasr_mllr_accumulate_weighted_dev(h._h, d_x.data_ptr(), len(x), None, None, None, 0, None) == capi.AASR_ERR_INVALID
    assert L.aasr_mllr_accumulate_weighted_dev(h._h, d_x.data_ptr(), len(x), d_off.data_ptr(), None, None, 3, None) == capi.AASR_ERR_INVALID
    # frames without a single entry: a valid call that adds nothing
    h.accumulate_weighted_dev(d_x, d_off, torch.zeros(0, dtype=torch.int32, device="cuda"),
                              torch.zeros(0, dtype=torch.float64, device="cuda"))
    G, k, beta = h.fetch()
    assert beta == 0.0 and not G.any() and not k.any()
    h.close()
    gmm.close()

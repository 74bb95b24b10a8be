"""The weighted accumulation (aasr_stats_accumulate_weighted_dev, csrc/stats_weighted.hip).

1. Weight one is the plain path, byte for byte: the row list in rows_by_pdf order with every weight 1.0 against
   aasr_stats_accumulate_dev on the same frames and model -- the fetched Gaussian and mixture sums and the written .gks
   / .mcs are identical bytes; plain then weighted on one handle equals two plain calls.
2. Weights uniform in (0, 1], one of 1e-300, a row listed under three pdfs and a frame so far from its mixture that its
   total is 0 (no count; mixture_ll gets w * log 1e-50), against tools/stats_bw_restate.py's accumulate(): counts exact,
   the rest under tools/fuzz_stats.py's TOL -- the bounds of tests/test_stats_gpu.py that the plain path is held to
   against its own restatement (gamma, aux gamma, mixture_ll 1e-12 relative; component gammas 1e-11; sum x, sum x^2
   1e-10 relative + 1e-9): the weighted sums have the same length and the same order.  Two runs give identical bytes.
3. <192> once at D = 150 with 40 entries; a full handle refuses the call (AASR_ERR_UNSUPPORTED) and keeps its sums.
4. Entries whose row is outside the frame buffer (a caller's mistake) read no frame and add nothing.

Shapes: D = 3 (instance 8) and D = 39 (instance 40), mixtures of 0 ... 4 components; a pdf with 1 100 entries (two
items), one with 300 (two sub-blocks of 256), one with 1, one with none, one without components."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stats_bw_restate as BW  # noqa: E402

FS = BW.FS
pytestmark = pytest.mark.gpu
SIZES = [4, 3, 1, 0, 2, 4]
COUNTS = [1100, 300, 1, 7, 0, 40]


@pytest.fixture(scope="module")
def topo(capi, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("weighted") / "t.ph")
    FS.write_ph(path)
    return capi.Topology(path)


@pytest.fixture(scope="module", params=[3, 39])
def case(request, capi, oracle):
    D = request.param
    rng = np.random.default_rng(700 + D)
    model = FS.make_model(rng, D, SIZES)
    x, pdf = FS.make_frames(rng, model, COUNTS, skipped=5)
    return dict(D=D, model=model, x=x, pdf=pdf, mix_w=oracle.DiagModel(*model).mix_w, K=len(model[3]))


def row_list(pdf, S):
    """rows_by_pdf: the frames with a pdf grouped by pdf, frame order within a pdf"""
    rows = np.concatenate([np.nonzero(pdf == s)[0] for s in range(S)]).astype(np.int32)
    cnt = np.concatenate([[0], np.cumsum(np.bincount(pdf[pdf >= 0], minlength=S))]).astype(np.int64)
    return cnt, rows


def fetch_bytes(out):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def dump_bytes(st, base):
    st.write(base)
    return [open(base + ext, "rb").read() for ext in (".gks", ".mcs")]


def test_weight_one_is_the_plain_path_byte_for_byte(capi, topo, case, tmp_path):
    import torch
    model, x, pdf = case["model"], case["x"], case["pdf"]
    S = len(SIZES)
    gmm = capi.Gmm.from_arrays(*model)
    d_x = torch.tensor(x, device="cuda")
    cnt, rows = row_list(pdf, S)
    assert np.diff(cnt).tolist() == COUNTS
    d_rows = torch.tensor(rows, device="cuda")
    d_w = torch.ones(len(rows), dtype=torch.float64, device="cuda")
    plain = capi.Stats(gmm, topo, case["K"])
    plain.accumulate_dev(d_x, pdf)
    shape_plain = plain.launch_shape()
    a = plain.fetch()
    weighted = capi.Stats(gmm, topo, case["K"])
    weighted.accumulate_weighted_dev(d_x, cnt, d_rows, d_w)
    shape_w = weighted.launch_shape()
    b = weighted.fetch()
    assert shape_w == shape_plain and shape_w["dimp"] == (8 if case["D"] == 3 else 40) and shape_w["items"] == 6
    assert fetch_bytes(a) == fetch_bytes(b)
    assert a["count"].tolist() == [1100, 300, 1, 0, 0, 40]
    assert dump_bytes(plain, str(tmp_path / "p")) == dump_bytes(weighted, str(tmp_path / "w"))
    # mixed on one handle: plain then weighted equals two plain calls
    two = capi.Stats(gmm, topo, case["K"])
    two.accumulate_dev(d_x, pdf)
    two.accumulate_dev(d_x, pdf)
    mixed = capi.Stats(gmm, topo, case["K"])
    mixed.accumulate_dev(d_x, pdf)
    mixed.accumulate_weighted_dev(d_x, cnt, d_rows, d_w)
    assert fetch_bytes(two.fetch()) == fetch_bytes(mixed.fetch())
    for h in (plain, weighted, two, mixed):
        h.close()
    gmm.close()


def weighted_entries(case):
    """per pdf its rows ascending, one row under three pdfs, weights in (0, 1] with one of 1e-300, and a far frame"""
    rng = np.random.default_rng(31 + case["D"])
    x, pdf = case["x"].copy(), case["pdf"]
    S = len(SIZES)
    shared = int(np.nonzero(pdf == 0)[0][3])
    far = int(np.nonzero(pdf == 5)[0][7])
    x[far] = 1e3                                   # every Gaussian of pdf 5 underflows: total 0
    per = []
    for s in range(S):
        r = np.nonzero(pdf == s)[0]
        if s in (1, 5):
            r = np.union1d(r, [shared])
        per.append(r.astype(np.int32))
    cnt = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    rows = np.concatenate(per)
    weights = 1.0 - rng.uniform(0.0, 1.0, len(rows))   # (0, 1]
    weights[cnt[0] + 17] = 1e-300
    assert (rows == shared).sum() == 3
    return x, cnt, rows, weights, far


def test_weighted_against_the_restatement(capi, topo, case):
    import torch
    model = case["model"]
    x, cnt, rows, weights, far = weighted_entries(case)
    want = BW.accumulate(model, case["mix_w"], x, cnt, rows, weights)
    e_far = int(cnt[5] + np.nonzero(rows[cnt[5]:cnt[6]] == far)[0][0])
    assert want["count"].tolist() == [1100, 301, 1, 0, 0, 40]          # 41 entries of pdf 5, the far one not counted
    gmm = capi.Gmm.from_arrays(*model)
    d_x = torch.tensor(x, device="cuda")
    d_rows, d_w = torch.tensor(rows, device="cuda"), torch.tensor(weights, device="cuda")
    outs = []
    for _ in range(2):
        st = capi.Stats(gmm, topo, case["K"])
        st.accumulate_weighted_dev(d_x, cnt, d_rows, d_w)
        outs.append(st.fetch())
        st.close()
    got = outs[0]
    worst = {}
    fails = FS.compare(got, want, worst=worst)
    print("D = %d: worst difference in units of the tolerance %s" % (case["D"], {k: "%.3g" % v for k, v in worst.items()}))
    assert not fails, "\n".join(fails)
    # the far frame alone: without it mixture_ll of pdf 5 is short of exactly w * log 1e-50
    keep = np.ones(len(rows), bool)
    keep[e_far] = False
    cnt2 = cnt.copy()
    cnt2[6:] -= 1
    less = BW.accumulate(model, case["mix_w"], x, cnt2, rows[keep], weights[keep])
    assert less["count"].tolist() == want["count"].tolist()
    assert abs((want["mixture_ll"][5] - less["mixture_ll"][5]) - weights[e_far] * np.log(1e-50)) <= 1e-9
    assert abs(got["mixture_ll"][5] - want["mixture_ll"][5]) <= 1e-12 * abs(want["mixture_ll"][5])
    assert fetch_bytes(outs[0]) == fetch_bytes(outs[1])                # two runs, identical bytes
    gmm.close()


def test_the_widest_instance_and_the_refusal_on_a_full_handle(capi, oracle, topo):
    import torch
    rng = np.random.default_rng(9)
    model = FS.make_model(rng, 150, [2, 3])
    x, pdf = FS.make_frames(rng, model, [25, 15])
    cnt, rows = row_list(pdf, 2)
    weights = 1.0 - rng.uniform(0.0, 1.0, len(rows))
    gmm = capi.Gmm.from_arrays(*model)
    d_x = torch.tensor(x, device="cuda")
    d_rows, d_w = torch.tensor(rows, device="cuda"), torch.tensor(weights, device="cuda")
    st = capi.Stats(gmm, topo, 5)
    st.accumulate_weighted_dev(d_x, cnt, d_rows, d_w)
    sh = st.launch_shape()
    assert (sh["dimp"], sh["items"], sh["max_comps"]) == (192, 2, 3), sh
    fails = FS.compare(st.fetch(), BW.accumulate(model, oracle.DiagModel(*model).mix_w, x, cnt, rows, weights))
    assert not fails, "\n".join(fails)
    st.close()
    gmm.close()
    # a handle with full second moments refuses, before anything is queued: its sums stay what they were
    small = FS.make_model(rng, 5, [2, 1])
    xs, ps = FS.make_frames(rng, small, [9, 4])
    g2 = capi.Gmm.from_arrays(*small)
    full = capi.Stats(g2, topo, 3, full=True)
    d_xs = torch.tensor(xs, device="cuda")
    full.accumulate_dev(d_xs, ps)
    before = fetch_bytes(full.fetch())
    c2, r2 = row_list(ps, 2)
    with pytest.raises(capi.AasrError) as ei:
        full.accumulate_weighted_dev(d_xs, c2, torch.tensor(r2, device="cuda"),
                                     torch.ones(len(r2), dtype=torch.float64, device="cuda"))
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "full" in ei.value.msg
    assert fetch_bytes(full.fetch()) == before
    full.close()
    g2.close()


def test_rows_outside_the_frames_add_nothing(capi, topo, case):
    import torch
    model, x, pdf = case["model"], case["x"], case["pdf"]
    S = len(SIZES)
    gmm = capi.Gmm.from_arrays(*model)
    d_x = torch.tensor(x, device="cuda")
    cnt, rows = row_list(pdf, S)
    weights = np.full(len(rows), 0.5)
    good = capi.Stats(gmm, topo, case["K"])
    good.accumulate_weighted_dev(d_x, cnt, torch.tensor(rows, device="cuda"), torch.tensor(weights, device="cuda"))
    a = good.fetch()
    # two more entries under pdf 5, one row below 0 and one past the last frame
    rows2 = np.concatenate([rows[:cnt[6]], np.array([-1, len(x)], np.int32), rows[cnt[6]:]])
    w2 = np.concatenate([weights[:cnt[6]], [0.5, 0.5], weights[cnt[6]:]])
    cnt2 = cnt.copy()
    cnt2[6:] += 2
    bad = capi.Stats(gmm, topo, case["K"])
    bad.accumulate_weighted_dev(d_x, cnt2, torch.tensor(rows2, device="cuda"), torch.tensor(w2, device="cuda"))
    assert fetch_bytes(bad.fetch()) == fetch_bytes(a)
    good.close()
    bad.close()
    gmm.close()

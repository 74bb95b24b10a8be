"""The class-scatter accumulator fed with weighted entries (csrc/scatter_entries.hip,
aasr_scatter_accumulate_weighted_dev): a pdf-major entry list in which a frame may stand under several classes, as a
Baum-Welch segmentation gives it.

Yardsticks: the handle's own row-list call for bytes (one entry per frame in that call's order must give that call's
bytes), and tools/lda_networks_restate.py's entry-by-entry sums in double and in np.longdouble.  Tolerance: the rule of
tests/test_scatter_gpu.py -- per quantity max(4 x the double restatement's own distance from the extended sums, four
roundings of a double), relative to the largest entry, printed before it is asserted."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ITEM = 256                    # entries per work item (SCATTER_ITEM)
SIZES = [0, 1, 31, 32, 33, 256, 257, 600]
EPS4 = 4 * 2.0 ** -53


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LN = _load("lda_networks_restate")
LR = LN.LR


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def features(rng, n, d):
    return rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, d) + rng.uniform(-2, 2, d)


def hard_rows(seed, d, sizes, skipped=60):
    """rows of len(sizes) classes in random order with class -1 rows in between, and per-row weights with zeros and ones"""
    rng = np.random.default_rng(seed)
    cls = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(sizes)] + [np.full(skipped, -1, np.int32)])
    cls = cls[rng.permutation(len(cls))]
    w = rng.uniform(0.0, 1.5, len(cls))
    w[rng.random(len(cls)) < 0.1] = 0.0
    w[rng.random(len(cls)) < 0.1] = 1.0
    return features(rng, len(cls), d), cls, w


def soft_entries(seed, n, n_classes, empty, dyadic=False):
    """every frame under 1 ... 4 of the classes (never `empty`) with positive weights summing to 1; dyadic: under three
    with 1/2, 1/4, 1/4 -> cnt, rows, weights in pdf-major order, frames ascending within a class"""
    rng = np.random.default_rng(seed)
    usable = [c for c in range(n_classes) if c != empty]
    per = [[] for _ in range(n_classes)]
    for t in range(n):
        k = 3 if dyadic else int(rng.integers(1, 5))
        members = rng.choice(usable, size=k, replace=False)
        if dyadic:
            w = np.array([0.5, 0.25, 0.25])
        else:
            w = rng.uniform(0.05, 1.0, k)
            w = w / w.sum()
        for c, wc in zip(members, w):
            per[int(c)].append((t, float(wc)))
    cnt = np.zeros(n_classes + 1, np.int64)
    cnt[1:] = np.cumsum([len(p) for p in per])
    rows = np.array([t for p in per for t, _ in p], np.int32)
    weights = np.array([w for p in per for _, w in p], np.float64)
    return cnt, rows, weights


def run_weighted(capi, x, C, cnt, rows, weights, slab_bytes=None, before=None):
    """-> (gamma, sum_x, packed sum_xx), the weighted call's launch shape; before: (cls, w) of a row-list call first"""
    h = capi.Scatter(C, x.shape[1])
    if slab_bytes:
        h.set_slab_bytes(slab_bytes)
    dx = dev(x)
    if before is not None:
        h.accumulate_dev(dx, before[0], dev(before[1]) if before[1] is not None else None)
    h.accumulate_weighted_dev(dx, cnt, dev(rows), dev(weights))
    shape = h.launch_shape()
    out = h.fetch()
    h.close()
    return out, shape


def run_rows(capi, x, C, cls, w):
    h = capi.Scatter(C, x.shape[1])
    h.accumulate_dev(dev(x), cls, dev(w) if w is not None else None)
    out = h.fetch()
    h.close()
    return out


def same_bytes(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def check(tag, got, dbl, ext):
    """got: (gamma, sum_x, packed sum_xx) of the handle; dbl / ext: (gamma, sum_x, full sum_xx) in double / extended"""
    for name, have, a, b in (("gamma", got[0], dbl[0], ext[0]), ("sum_x", got[1], dbl[1], ext[1]),
                             ("sum_xx", got[2], LR.pack(dbl[2]), LR.pack(ext[2]))):
        big = float(np.abs(b).max()) or 1.0
        own = float(np.abs(a.astype(np.longdouble) - b).max()) / big
        err = float(np.abs(have.astype(np.longdouble) - b).max()) / big
        tol = max(4 * own, EPS4)
        print("%s %s: restatement %.3g, handle %.3g from the extended sums (tolerance %.3g)" % (tag, name, own, err, tol))
        assert err <= tol, (tag, name, err, tol)


@pytest.mark.parametrize("d", [15, 16, 39, 127])
def test_one_entry_per_frame_gives_the_row_list_calls_bytes(capi, d):
    x, cls, w = hard_rows(300 + d, d, SIZES)
    C = len(SIZES)
    for tag, weight in (("ones", None), ("row weights", w)):
        cnt, rows, ew = LN.entries_of_classes(cls, C, weight)
        assert cnt[-1] == sum(SIZES) and (np.diff(cnt) == SIZES).all()
        got, shape = run_weighted(capi, x, C, cnt, rows, ew)
        assert shape == {"pb": (d + 1 + 15) // 16, "items": sum((n + ITEM - 1) // ITEM for n in SIZES), "launches": 1}
        assert same_bytes(got, run_rows(capi, x, C, cls, weight)), (d, tag)
        again, _ = run_weighted(capi, x, C, cnt, rows, ew)
        assert same_bytes(got, again), (d, tag)
        if weight is None:
            assert got[0].tolist() == [float(n) for n in SIZES]


_soft = {}


def soft_case(d):
    """frames, entries and the two restatements of the multi-membership case, once per dimension"""
    if d not in _soft:
        n, C, empty = 700, 9, 4
        x = features(np.random.default_rng(500 + d), n, d)
        cnt, rows, weights = soft_entries(600 + d, n, C, empty)
        _soft[d] = (x, C, empty, cnt, rows, weights,
                    LN.scatter_entries_in_order(x, cnt, rows, weights, C),
                    LN.scatter_entries_in_order(x, cnt, rows, weights, C, dtype=np.longdouble))
    return _soft[d]


@pytest.mark.parametrize("d", [1, 39, 64])
def test_frames_under_several_classes(capi, d):
    x, C, empty, cnt, rows, weights, dbl, ext = soft_case(d)
    per_frame = np.bincount(rows, minlength=len(x))
    assert per_frame.min() >= 1 and per_frame.max() == 4 and cnt[empty] == cnt[empty + 1]
    assert np.allclose(np.bincount(rows, weights=weights, minlength=len(x)), 1.0, rtol=0, atol=1e-15)
    got, shape = run_weighted(capi, x, C, cnt, rows, weights)
    assert shape["pb"] == (d + 1 + 15) // 16
    assert shape["items"] == int(sum((n + ITEM - 1) // ITEM for n in np.diff(cnt)))
    check("d %d" % d, got, dbl, ext)
    assert got[0][empty] == 0 and not got[1][empty].any() and not got[2][empty].any()
    assert abs(got[0].sum() - len(x)) <= 1e-9 * len(x)
    # dyadic weights: every partial sum of gamma is a multiple of 1/4 far below 2^53, so gamma is exact
    cnt2, rows2, w2 = soft_entries(700 + d, len(x), C, empty, dyadic=True)
    got2, _ = run_weighted(capi, x, C, cnt2, rows2, w2)
    exact = np.array([w2[cnt2[c]:cnt2[c + 1]].sum() for c in range(C)])
    assert got2[0].tolist() == exact.tolist() and got2[0].sum() == len(x)


def test_launch_cuts_keep_the_bytes(capi):
    d, C = 39, 3
    rng = np.random.default_rng(41)
    n = 1200
    x = features(rng, n, d)
    sizes = [3000, 0, 300]
    cnt = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = rng.integers(0, n, cnt[-1]).astype(np.int32)         # a frame several times in a class: nothing forbids it
    weights = rng.uniform(0.0, 1.0, cnt[-1])
    one, shape = run_weighted(capi, x, C, cnt, rows, weights)
    items = sum((s + ITEM - 1) // ITEM for s in sizes)
    assert shape == {"pb": 3, "items": items, "launches": 1}
    item_bytes = 6 * 256 * 8
    for per_launch in (5, 4, 1):
        cut, shape = run_weighted(capi, x, C, cnt, rows, weights, slab_bytes=per_launch * item_bytes)
        assert shape == {"pb": 3, "items": items, "launches": (items + per_launch - 1) // per_launch}
        assert shape["launches"] >= 3
        assert same_bytes(one, cut), per_launch
    check("cuts", one, LN.scatter_entries_in_order(x, cnt, rows, weights, C),
          LN.scatter_entries_in_order(x, cnt, rows, weights, C, dtype=np.longdouble))


def test_weight_zero_does_not_read_its_row(capi):
    d, C = 39, 6
    rng = np.random.default_rng(43)
    n = 400
    x = features(rng, n, d)
    cnt, rows, weights = soft_entries(44, n, C, empty=2)
    bad = [7, 300, n - 1]                                       # frame rows of NaN, of Inf
    keep = ~np.isin(rows, bad)
    x_bad = x.copy()
    x_bad[bad[0]] = np.nan
    x_bad[bad[1]] = np.inf
    x_bad[bad[2], 3] = np.nan
    assert (~keep).sum() >= 3
    w0 = np.where(keep, weights, 0.0)
    # where they fall in their classes' runs: finite, and the sums of the other entries (the restatement skips an entry
    # of weight 0).  An entry of weight 0 takes a place in its item, so the rows that share a matrix instruction are
    # not those of a list without it: the tolerance rule, not bytes
    got, _ = run_weighted(capi, x_bad, C, cnt, rows, w0)
    assert all(np.isfinite(a).all() for a in got)
    check("zero weights", got, LN.scatter_entries_in_order(x_bad, cnt, rows, w0, C),
          LN.scatter_entries_in_order(x_bad, cnt, rows, w0, C, dtype=np.longdouble))
    # at the end of their classes' runs they move no other entry: the bytes of the run without them.  Every class gets
    # enough of them to open an item of nothing else
    cls_of = np.repeat(np.arange(C), np.diff(cnt))
    sizes_k = np.bincount(cls_of[keep], minlength=C)
    cnt_k = np.concatenate([[0], np.cumsum(sizes_k)]).astype(np.int64)
    rows_k, weights_k = rows[keep], weights[keep]
    without, _ = run_weighted(capi, x_bad, C, cnt_k, rows_k, weights_k)
    extra = np.resize(np.array(bad, np.int32), ITEM + 5)
    rows_t = np.concatenate([np.concatenate([rows_k[cnt_k[c]:cnt_k[c + 1]], extra]) for c in range(C)]).astype(np.int32)
    weights_t = np.concatenate([np.concatenate([weights_k[cnt_k[c]:cnt_k[c + 1]], np.zeros(len(extra))]) for c in range(C)])
    cnt_t = np.concatenate([[0], np.cumsum(sizes_k + len(extra))]).astype(np.int64)
    tail, shape = run_weighted(capi, x_bad, C, cnt_t, rows_t, weights_t)
    assert shape["items"] > int(sum((s + ITEM - 1) // ITEM for s in sizes_k))
    assert all(np.isfinite(a).all() for a in tail)
    assert same_bytes(tail, without)


def test_refusals_add_nothing(capi):
    d, C = 5, 6
    x = features(np.random.default_rng(45), 40, d)
    cnt, rows, weights = soft_entries(46, 40, C, empty=1)
    h = capi.Scatter(C, d)
    dx, dr, dw = dev(x), dev(rows), dev(weights)
    h.accumulate_weighted_dev(dx, cnt, dr, dw)
    before = h.fetch()
    shifted = cnt.copy()
    shifted[0] = 1
    falling = cnt.copy()
    falling[1] = cnt[2] + 1
    assert falling[2] < falling[1]
    for name, args in (("cnt[0]", (dx, shifted, dr, dw)), ("decreasing", (dx, falling, dr, dw)),
                       ("no rows", (dx, cnt, None, dw)), ("no weights", (dx, cnt, dr, None))):
        with pytest.raises(capi.AasrError) as ei:
            h.accumulate_weighted_dev(*args)
        assert ei.value.code == capi.AASR_ERR_INVALID, name
        assert same_bytes(before, h.fetch()), name
    h.accumulate_weighted_dev(dx, np.zeros(C + 1, np.int64), None, None)        # no entries: nothing to refuse
    assert same_bytes(before, h.fetch())
    h.close()


def test_mixed_with_the_row_list_call(capi):
    d = 39
    x, C, empty, cnt, rows, weights, dbl, ext = soft_case(d)
    rng = np.random.default_rng(47)
    cls = rng.integers(-1, C, len(x)).astype(np.int32)
    w = rng.uniform(0.1, 1.5, len(x))
    got, _ = run_weighted(capi, x, C, cnt, rows, weights, before=(cls, w))
    hard_d = LR.scatter_in_order(x, cls, C, w)
    hard_e = LR.scatter_in_order(x, cls, C, w, dtype=np.longdouble)
    check("mixed", got, tuple(a + b for a, b in zip(hard_d, dbl)), tuple(a + b for a, b in zip(hard_e, ext)))

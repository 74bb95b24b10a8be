"""The class-scatter accumulator on the device (csrc/scatter_accum.hip) against two NumPy computations of the same sums
(tools/lda_restate.py): the in-order restatement in double -- frame by frame, (gamma x_j) x_i as dsyr forms it -- and the
same sums in np.longdouble.

Tolerance (DESIGN 4.9's rule): per case and per quantity the restatement's own distance from the extended sums, relative
to the largest entry, is measured; the handle is held to 4 x that distance from the extended sums, never tighter than
four roundings of a double.  No figure is picked beforehand; every case prints what it measured.

Cases: every dimension on both sides of an instance edge (d + 1 against multiples of 16; the instance is asserted from
the handle's launch shape), 128 refused; classes of 1, 3, 4, 5 rows, of one below, at and one above a work item
(256 rows, scatter.h), of several items, of none; class -1 rows in between; one class holding most rows; NULL weights
against ones (bytes), zero and fractional weights; three uneven calls against one; two runs (bytes); a slab bound
that cuts a call into many launches (bytes again: the slab pass adds a class's items in item order whatever the cut);
the diagonal statistics' sums at 39 dimensions."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ITEM = 256                    # rows per work item (SCATTER_ITEM)
SIZES = [1, 3, 4, 5, ITEM - 1, ITEM, ITEM + 1, 2 * ITEM + 77, 0]
EPS4 = 4 * 2.0 ** -53


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LR = _load("lda_restate")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_rows(seed, d, sizes, skipped=60, weights=True):
    """rows of len(sizes) classes in random order with class -1 rows in between; features with an offset, as real ones"""
    rng = np.random.default_rng(seed)
    cls = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(sizes)] + [np.full(skipped, -1, np.int32)])
    cls = cls[rng.permutation(len(cls))]
    x = rng.standard_normal((len(cls), d)) * rng.uniform(0.2, 3.0, d) + rng.uniform(-2, 2, d)
    w = None
    if weights:
        w = rng.uniform(0.0, 1.5, len(cls))
        w[rng.random(len(cls)) < 0.1] = 0.0
        w[rng.random(len(cls)) < 0.1] = 1.0
    return x, cls, w


_refs = {}


def reference(key, x, cls, C, w):
    """the two NumPy computations of a case, once"""
    if key not in _refs:
        _refs[key] = (LR.scatter_in_order(x, cls, C, w), LR.scatter_in_order(x, cls, C, w, dtype=np.longdouble))
    return _refs[key]


def check(tag, got, ref, d):
    """got: (gamma, sum_x, packed sum_xx) of the handle; ref: (restatement, extended)"""
    (g, sx, sxx), (eg, esx, esxx) = ref
    worst = 0.0
    for name, have, dbl, ext in (("gamma", got[0], g, eg), ("sum_x", got[1], sx, esx),
                                 ("sum_xx", got[2], LR.pack(sxx), LR.pack(esxx))):
        big = float(np.abs(ext).max()) or 1.0
        own = float(np.abs(dbl.astype(np.longdouble) - ext).max()) / big
        err = float(np.abs(have.astype(np.longdouble) - ext).max()) / big
        tol = max(4 * own, EPS4)
        print("%s %s: restatement %.3g, handle %.3g from the extended sums (tolerance %.3g)" % (tag, name, own, err, tol))
        assert err <= tol, (tag, name, err, tol)
        worst = max(worst, err)
    return worst


def run_handle(capi, x, cls, C, w=None, calls=None, slab_bytes=None):
    d = x.shape[1]
    h = capi.Scatter(C, d)
    if slab_bytes:
        h.set_slab_bytes(slab_bytes)
    dx, dw = dev(x), (dev(w) if w is not None else None)
    shapes = []
    for a, b in (calls or [(0, len(cls))]):
        h.accumulate_dev(dx[a:b], cls[a:b], dw[a:b] if dw is not None else None)
        shapes.append(h.launch_shape())
    out = h.fetch()
    h.close()
    return out, shapes


@pytest.mark.parametrize("d", [1, 15, 16, 39, 47, 48, 63, 64, 127])
def test_every_instance_against_the_two_restatements(capi, d):
    x, cls, w = make_rows(100 + d, d, SIZES)
    C = len(SIZES)
    got, shapes = run_handle(capi, x, cls, C, w)
    assert shapes[0]["pb"] == (d + 1 + 15) // 16
    assert shapes[0]["items"] == sum((n + ITEM - 1) // ITEM for n in SIZES) and shapes[0]["launches"] == 1
    check("d %d" % d, got, reference(("w", d), x, cls, C, w), d)
    assert got[0][-1] == 0 and not got[1][-1].any() and not got[2][-1].any()      # the class without rows
    # two runs: the same bytes
    again, _ = run_handle(capi, x, cls, C, w)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_dimension_128_and_bad_classes_are_refused(capi):
    with pytest.raises(capi.AasrError) as ei:
        capi.Scatter(3, 128)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED
    h = capi.Scatter(3, 4)
    x = dev(np.ones((5, 4)))
    for bad in (3, -2):
        with pytest.raises(capi.AasrError) as ei:
            h.accumulate_dev(x, np.array([0, 1, bad, 2, 0], np.int32))
        assert ei.value.code == capi.AASR_ERR_INVALID
    g, sx, sxx = h.fetch()
    assert not g.any() and not sx.any() and not sxx.any()                          # a refused call adds nothing


@pytest.mark.parametrize("d", [16, 39])
def test_null_weights_are_ones_and_unit_counts_are_exact(capi, d):
    x, cls, _ = make_rows(7 + d, d, SIZES, weights=False)
    C = len(SIZES)
    none, _ = run_handle(capi, x, cls, C, None)
    ones, _ = run_handle(capi, x, cls, C, np.ones(len(cls)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(none, ones))
    assert none[0].tolist() == [float(n) for n in SIZES]
    check("d %d, no weights" % d, none, reference(("1", d), x, cls, C, None), d)


def test_one_heavy_class_call_cuts_and_launch_cuts(capi):
    d = 39
    sizes = [3000, 5, ITEM + 1, 0, 40]
    x, cls, w = make_rows(55, d, sizes, skipped=200)
    C, n = len(sizes), len(cls)
    ref = reference(("heavy", d), x, cls, C, w)
    one, shapes = run_handle(capi, x, cls, C, w)
    assert shapes[0]["launches"] == 1
    check("heavy class", one, ref, d)
    # the same rows in three uneven calls: other item boundaries, the same tolerance
    cut, _ = run_handle(capi, x, cls, C, w, calls=[(0, 17), (17, n - 900), (n - 900, n)])
    check("three calls", cut, ref, d)
    # a slab bound of three items: many launches, and the same bytes as the single launch
    item_bytes = 6 * 256 * 8
    small, shapes = run_handle(capi, x, cls, C, w, slab_bytes=3 * item_bytes)
    assert shapes[0]["launches"] == (shapes[0]["items"] + 2) // 3 and shapes[0]["launches"] > 4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, small))
    again, _ = run_handle(capi, x, cls, C, w, slab_bytes=3 * item_bytes)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(small, again))
    tiny, shapes = run_handle(capi, x, cls, C, w, slab_bytes=1)                   # one item a launch at the least
    assert shapes[0]["launches"] == shapes[0]["items"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, tiny))


def test_consistent_with_the_diagonal_statistics(capi):
    """gamma, sum gamma x and the diagonal of sum gamma x x^T against the sums as the diagonal accumulator forms them
    (gamma x, then (gamma x) x, Distributions.cc:249-260) over the same rows, in double and extended"""
    d = 39
    x, cls, w = make_rows(91, d, [ITEM + 3, 700, 2], skipped=30)
    C = 3
    got, _ = run_handle(capi, x, cls, C, w)

    def diag_sums(dtype):
        g, sx, sxx = np.zeros(C, dtype), np.zeros((C, d), dtype), np.zeros((C, d), dtype)
        xx, ww = x.astype(dtype), w.astype(dtype)
        for t in range(len(cls)):
            if cls[t] >= 0:
                gx = ww[t] * xx[t]
                g[cls[t]] += ww[t]
                sx[cls[t]] += gx
                sxx[cls[t]] += gx * xx[t]
        return g, sx, sxx

    dbl, ext = diag_sums(np.float64), diag_sums(np.longdouble)
    i = np.arange(d)
    diag = got[2][:, i * (i + 1) // 2 + i]
    for name, have, a, b in (("gamma", got[0], dbl[0], ext[0]), ("sum_x", got[1], dbl[1], ext[1]),
                             ("diag sum_xx", diag, dbl[2], ext[2])):
        big = float(np.abs(b).max())
        own = float(np.abs(a.astype(np.longdouble) - b).max()) / big
        err = float(np.abs(have.astype(np.longdouble) - b).max()) / big
        print("diagonal %s: restatement %.3g, handle %.3g" % (name, own, err))
        assert err <= max(4 * own, EPS4)

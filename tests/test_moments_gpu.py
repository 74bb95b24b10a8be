"""The blocked-moments handle on the device (csrc/moments_accum.hip) against two NumPy computations of the same sums
(tools/feanorm_restate.py): the in-order restatement in double -- frame by frame, as feanorm's loop adds -- and the same
sums in np.longdouble.

Tolerance: per case and per quantity the restatement's own distance from the extended sums, relative to the largest
entry, is measured; the handle may be at most 4 x that far from the extended sums (the tiled order is another, equally
valid summation).  The count must be exact.  No figure is picked beforehand; every case prints what it measured.

Cases: block sizes 1, 7, 64 and 1000; utterances of 1, block - 1, block and 2 block + 3 rows, so that there are
segments of 1, block - 1 and block rows, and at block size 1000 segments of four workgroup passes (256 rows a pass,
moments.h); dimensions 1, 13, 15 (d + 1 = 16: one tile block exactly), 16 (two), 39 and 127, 128 refused in full mode
and taken in diagonal mode; both modes; one call against three uneven calls (bytes); launch bounds of one and of three
segments (bytes: a segment's sums do not depend on the launches around it); two runs (bytes); the full mode's diagonal
against the diagonal mode's sum x^2."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

RUN = 256                     # rows per work item (MOMENTS_RUN)
DIMS = [1, 13, 15, 16, 39, 127]
BLOCKS = [1, 7, 64, 1000]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FR = _load("feanorm_restate")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def utterance_rows(bs):
    return [n for n in (bs, bs - 1, 1, 2 * bs + 3, 1, bs) if n > 0]


def make_case(d, bs):
    """features with an offset and uneven spreads, as real ones; -> x, rows per utterance, segments"""
    rng = np.random.default_rng(1000 * d + bs)
    rows = utterance_rows(bs)
    x = rng.standard_normal((sum(rows), d)) * rng.uniform(0.2, 3.0, d) + rng.uniform(-2, 2, d)
    return x, rows, FR.cut(rows, bs)


_refs = {}


def reference(d, bs, full):
    """the two NumPy computations of a case, once"""
    key = (d, bs, full)
    if key not in _refs:
        x, _, segs = make_case(d, bs)
        _refs[key] = (FR.segment_sums(x, segs, full), FR.segment_sums(x, segs, full, dtype=np.longdouble))
    return _refs[key]


def check(tag, got, ref, full):
    """got: (count, utterance, sum_x, sum_xx) of the handle; ref: (restatement, extended)"""
    (c, sx, sxx), (ec, esx, esxx) = ref
    assert got[0].tolist() == c.tolist(), tag                                   # the count: exact
    worst = {}
    for name, have, dbl, ext in (("sum_x", got[2], sx, esx),
                                 ("sum_xx", got[3], FR.pack(sxx) if full else sxx, FR.pack(esxx) if full else esxx)):
        big = float(np.abs(ext).max()) or 1.0
        own = float(np.abs(dbl.astype(np.longdouble) - ext).max()) / big
        err = float(np.abs(have.astype(np.longdouble) - ext).max()) / big
        print("%s %s: restatement %.3g, handle %.3g from the extended sums (tolerance %.3g)" % (tag, name, own, err, 4 * own))
        assert err <= 4 * own, (tag, name, err, own)
        worst[name] = err
    return worst


def run_handle(capi, x, segs, full, calls=None, launch_segments=None):
    """calls: [(first segment, end segment)]: each call gets its segments' rows alone, the segments rebased"""
    h = capi.Moments(x.shape[1], capi.MOMENTS_FULL if full else capi.MOMENTS_DIAG)
    if launch_segments:
        h.set_launch_segments(launch_segments)
    dx = dev(x)
    shapes = []
    for a, b in (calls or [(0, len(segs))]):
        part = segs[a:b].copy()
        r0, r1 = int(part[0, 0]), int(part[-1, 0] + part[-1, 1])
        part[:, 0] -= r0
        h.accumulate_dev(dx[r0:r1], part)
        shapes.append(h.launch_shape())
    out = h.fetch()
    h.close()
    return out, shapes


@pytest.mark.parametrize("bs", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
def test_both_modes_against_the_two_restatements(capi, d, bs):
    x, rows, segs = make_case(d, bs)
    items = int(sum((n + RUN - 1) // RUN for n in segs[:, 1]))
    lens = sorted(set(segs[:, 1].tolist()))
    assert 1 in lens and bs in lens and (bs - 1 in lens or bs == 1)
    results = {}
    for full in (False, True):
        got, shapes = run_handle(capi, x, segs, full)
        assert shapes[0] == {"pb": (d + 1 + 15) // 16 if full else 0, "items": items, "launches": 1}
        assert got[1].tolist() == segs[:, 2].tolist()
        check("d %d, block %d, %s" % (d, bs, "full" if full else "diagonal"), got, reference(d, bs, full), full)
        again, _ = run_handle(capi, x, segs, full)                                # two runs: the same bytes
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
        results[full] = got
    # the full mode's diagonal is the diagonal mode's sum x^2, to the same bound
    i = np.arange(d)
    diag = results[True][3][:, i * (i + 1) // 2 + i]
    (_, _, sxx), (_, _, esxx) = reference(d, bs, False)
    big = float(np.abs(esxx).max())
    own = float(np.abs(sxx.astype(np.longdouble) - esxx).max()) / big
    err = float(np.abs(diag.astype(np.longdouble) - esxx).max()) / big
    print("d %d, block %d, full diagonal: restatement %.3g, handle %.3g" % (d, bs, own, err))
    assert err <= 4 * own
    # ... and sum x is the same quantity in both modes
    (_, sx, _), (_, esx, _) = reference(d, bs, False)
    big = float(np.abs(esx).max())
    assert float(np.abs(results[True][2].astype(np.longdouble) - esx).max()) / big <= \
        4 * float(np.abs(sx.astype(np.longdouble) - esx).max()) / big


def test_dimension_128_and_bad_segments(capi):
    with pytest.raises(capi.AasrError) as ei:
        capi.Moments(128, capi.MOMENTS_FULL)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED
    h = capi.Moments(4, capi.MOMENTS_DIAG)
    x = dev(np.ones((5, 4)))
    for bad in ([[0, 6, 0]], [[4, 2, 0]], [[-1, 2, 0]], [[0, 2, 0], [2, 0, 0]]):
        with pytest.raises(capi.AasrError) as ei:
            h.accumulate_dev(x, np.array(bad, np.int32))
        assert ei.value.code == capi.AASR_ERR_INVALID
    assert len(h.fetch()[0]) == 0                                                 # a refused call adds nothing
    h.close()


@pytest.mark.parametrize("d", [128, 300])
def test_the_diagonal_mode_has_no_dimension_bound(capi, d):
    """past 256 dimensions a second block column of the kernel takes over"""
    rng = np.random.default_rng(d)
    rows = [300, 5]
    x = rng.standard_normal((sum(rows), d)) + 1.0
    segs = FR.cut(rows, 1000)
    got, _ = run_handle(capi, x, segs, False)
    ref = (FR.segment_sums(x, segs), FR.segment_sums(x, segs, dtype=np.longdouble))
    check("d %d, diagonal" % d, got, ref, False)


@pytest.mark.parametrize("full", [False, True])
def test_call_cuts_and_launch_cuts_give_the_same_bytes(capi, full):
    d, bs = 39, 64
    x, rows, segs = make_case(d, bs)
    n = len(segs)
    one, shapes = run_handle(capi, x, segs, full)
    assert shapes[0]["launches"] == 1 and n >= 7
    # the same segments in three uneven calls, each with its own slice of the rows
    cut, _ = run_handle(capi, x, segs, full, calls=[(0, 1), (1, n - 2), (n - 2, n)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, cut))
    for bound in (1, 3):
        small, shapes = run_handle(capi, x, segs, full, launch_segments=bound)
        assert shapes[0]["launches"] == (n + bound - 1) // bound
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, small))
    # a segment of several workgroup passes under the bounds as well
    x, rows, segs = make_case(d, 1000)
    one, shapes = run_handle(capi, x, segs, full)
    assert shapes[0]["items"] > len(segs)
    small, shapes = run_handle(capi, x, segs, full, launch_segments=1)
    assert shapes[0]["launches"] == len(segs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, small))
    check("launch bound 1", small, reference(d, 1000, full), full)


@pytest.mark.parametrize("full", [False, True])
def test_blocked_sums_are_the_restated_blocked_sums(capi, full):
    """the host reduction: global += segment / block size in order, a dropped segment left out"""
    d, bs = 13, 7
    x, rows, segs = make_case(d, bs)
    keep = np.ones(len(segs), np.int32)
    keep[[1, len(segs) - 1]] = 0
    h = capi.Moments(d, capi.MOMENTS_FULL if full else capi.MOMENTS_DIAG)
    h.accumulate_dev(dev(x), segs)
    c, _, sx, sxx = h.fetch()
    for k in (None, keep):
        g, gx, gxx = h.blocked(bs, k)
        wg, wx, wxx = FR.blocked(c, sx, sxx, bs, k)                                # the handle's own segment sums, restated
        assert g == wg and gx.tobytes() == wx.tobytes() and gxx.tobytes() == wxx.tobytes()
    kept = segs[keep == 1]
    assert h.blocked(bs, keep)[0] == sum(n / bs for n in kept[:, 1].tolist())
    h.close()

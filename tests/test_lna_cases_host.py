"""The rows of tools/lna_cases.py against the oracle alone (no device): what tests/test_lna_paths_gpu.py asserts of the
LNA kernel's fast path without a tolerance is true of the reference, and every row kind is what its label says.

The claim the fast path rests on: on a row whose best state is >= -51, a state below ln 2^-126 (the reference stores its
linear likelihood as a float denormal, or as zero) leaves as FF FF whichever way it is quantised: lp <= -87.33 - logZ <=
-87.33 + 51 < -36.008 (logZ >= the row's maximum), and unnormalised lp = ll < -87.33 itself."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lna_cases as LC  # noqa: E402

SIZES = [3, 130, 255, 1000, 1024, 1025, 2048, 2049, 2560, 2561, 3125, 3328, 3329, 4096, 4097, 5000]
SEED = 11


def _ref(oracle, ll, normalize):
    return oracle.lna_encode(np.maximum(np.exp(ll.astype(np.float64)), 1e-50), normalize, 2)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("S", SIZES)
def test_states_below_the_float_normal_range_of_a_fast_row_encode_as_ffff(oracle, S, normalize):
    ll, labels = LC.rows(S, SEED)
    _, by = _ref(oracle, ll, normalize)
    code = LC.codes(by, S)
    n_fast = n_low = 0
    for r, row in enumerate(ll):
        if LC.fast(row):
            low = row < LC.LN_FLT_MIN
            n_fast += 1
            n_low += int(low.sum())
            assert (code[r][low] == 0xFFFF).all(), (labels[r], r)
    assert n_fast >= 16 and n_low >= 16
    for kind in ("all_floor", "all_ninf"):
        for r in np.flatnonzero(np.array(labels) == kind):
            assert (code[r] == 0xFFFF).all(), kind


@pytest.mark.parametrize("S", SIZES)
def test_every_row_kind_is_what_its_label_says(S):
    ll, labels = LC.rows(S, SEED)
    assert ll.dtype == np.float32 and ll.shape == (44, S) and len(labels) == 44
    assert set(labels) == set(LC.KINDS) and len(LC.KINDS) == 11
    assert all(labels.count(kind) == 4 for kind in LC.KINDS)
    assert not np.isnan(ll).any() and not np.isposinf(ll).any()
    lab = np.array(labels)
    floor = np.float32(np.log(1e-50))
    below = np.nextafter(np.float32(-51.0), np.float32(-np.inf))

    def flushed(row):
        return row < np.float32(-104.0)

    for r in np.flatnonzero(lab == "plain"):
        assert ll[r].min() >= -80.0 and ll[r].max() <= -5.0
    for r in np.flatnonzero(lab == "gt1"):
        assert ll[r].min() >= -10.0 and ll[r].max() <= 5.0 and LC.fast(ll[r])
        assert S < 100 or ll[r].max() > 0.0
    seen = set()
    for r in np.flatnonzero(lab == "band_fast"):
        row = ll[r]
        assert LC.fast(row)
        assert LC.in_band(row).any() and flushed(row).any()
        assert ((row >= LC.LN_FLT_MIN) | LC.in_band(row) | flushed(row)).all()      # nothing on an edge of the band
        if S >= 100:
            assert 0.25 <= LC.in_band(row).mean() <= 0.35 and 0.07 <= flushed(row).mean() <= 0.13
        fl = row[flushed(row)]
        seen |= {"floor"} if (fl == floor).any() else set()
        seen |= {"-200"} if (fl == np.float32(-200.0)).any() else set()
        seen |= {"-inf"} if np.isneginf(fl).any() else set()
        seen |= {"below"} if ((fl >= np.float32(-114.0)) & (fl <= np.float32(-104.1))).any() else set()
    assert seen == {"floor", "-200", "-inf", "below"}, seen
    hi, lo = np.flatnonzero(lab == "edge_hi"), np.flatnonzero(lab == "edge_lo")
    assert len(hi) == len(lo) == 4
    for a, b in zip(hi, lo):
        assert ll[a].max() == np.float32(-51.0) and LC.fast(ll[a])
        assert ll[b].max() == below and not LC.fast(ll[b])
        at = ll[a] == np.float32(-51.0)
        assert at.sum() == 1 and np.array_equal(ll[a][~at], ll[b][~at]) and ll[b][at][0] == below
        rest = ll[a][~at]
        assert LC.in_band(rest).any()
        assert (LC.in_band(rest) | ((rest >= -86.0) & (rest <= -52.0))).all()
    for r in np.flatnonzero(lab == "band_max"):
        assert ll[r].min() >= -100.0 and ll[r].max() <= -88.0 and not LC.fast(ll[r])
    for r in np.flatnonzero(lab == "all_floor"):
        assert (ll[r] == floor).all() and not LC.fast(ll[r])
    for r in np.flatnonzero(lab == "all_ninf"):
        assert np.isneginf(ll[r]).all() and not LC.fast(ll[r])
    for r in np.flatnonzero(lab == "one_hot"):
        hot = ll[r] == np.float32(-3.0)
        assert hot.sum() == 1 and flushed(ll[r][~hot]).all() and LC.fast(ll[r])
    for r in np.flatnonzero(lab == "flat"):
        assert (ll[r] == np.float32(-30.0)).all() and LC.fast(ll[r])
    # neighbouring rows differ in kind, and rows(S, seed) is a function of its arguments
    for r in np.flatnonzero(lab == "band_mid"):
        row = ll[r]
        rest = row[~LC.in_band(row) & ~flushed(row)]
        assert not LC.fast(row) and LC.in_band(row).any()
        assert rest.size and rest.min() >= -86.0 and rest.max() <= -75.0 and row.max() == rest.max()
    assert all(labels[r] != labels[r + 1] for r in range(43))
    again, _ = LC.rows(S, SEED)
    assert np.array_equal(again.view(np.uint32), ll.view(np.uint32))
    more, more_labels = LC.rows(S, SEED, frames=57)
    assert more.shape == (57, S) and more_labels[:44] == labels


@pytest.mark.parametrize("S", SIZES)
def test_band_mid_rows_show_the_denormal_quantisation(oracle, S):
    """The other side of the claim: on a row whose best state is well below -51 the band states are visible, and the
    raw value gives another code than the reference's denormal float -- so a fast path taken on such a row (a switch
    moved from -51 towards ln 2^-126) changes bytes that the exact comparisons of the GPU tests hold."""
    ll, labels = LC.rows(S, SEED)
    lp, by = _ref(oracle, ll, True)
    code = LC.codes(by, S)
    n_band = n_shown = 0
    for r in np.flatnonzero(np.array(labels) == "band_mid"):
        row = ll[r]
        band = LC.in_band(row)
        assert (code[r][band] != 0xFFFF).any()
        top = int(row.argmax())
        logz = float(row[top]) - float(lp[r, top])
        raw = (row[band].astype(np.float64) - logz).astype(np.float32).astype(np.float64)
        raw_code = np.where(raw < -36.008, 0xFFFF, np.trunc(-1820.0 * raw + .5).astype(np.int64))
        n_band += int(band.sum())
        n_shown += int((raw_code != code[r][band]).sum())
    assert n_band >= 4
    assert S < 100 or n_shown >= 0.2 * n_band, (n_shown, n_band)


def test_fast_restates_the_kernels_comparison():
    assert LC.fast(np.array([-51.0, -90.0], np.float32))
    assert not LC.fast(np.array([np.nextafter(np.float32(-51.0), np.float32(-np.inf)), -90.0], np.float32))
    assert not LC.fast(np.full(4, -np.inf, np.float32))
    assert LC.fast(np.array([-np.inf, 3.0], np.float32))
    with pytest.raises(AssertionError):
        LC.fast(np.array([-51.0]))                  # the test is the float32 one

"""The LNA pass (csrc/lna_encode.hip, csrc/lna_device.h) as production calls it -- 2-byte codes, no float output, which
takes the fast path of lna_row_from_registers -- and its column map, row pitch and grid, each on its own.

Inputs are the rows of tools/lna_cases.py (tests/test_lna_cases_host.py proves with the oracle alone what is asserted
of them here without a tolerance).  Comparisons of two routes through the same arithmetic (mapped against dense, padded
against dense, one grid against another, a row among others against the row alone, the bytes-only call against the call
with a float output on rows that take the exact path either way) are byte for byte.  Comparisons with the oracle carry
the bounds of tests/test_lna_gpu.py.

Every device buffer a call is given lies between 64 bytes of 0xA5 on either side; every call checks them afterwards,
and that its inputs still hold what was uploaded."""
import os
import sys

import numpy as np
import pytest

from conftest import CODES_EQUAL_MIN, assert_lp_denormal_band, observed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lna_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SEED = 11
REG_SIZES = [3, 255, 1024, 1025, 2048, 2049, 2560, 2561, 3328, 3329, 4096]     # both ends of every register instance
GENERIC_SIZES = [4097, 5000]
MAP_SIZES = [1000, 1025, 2049, 2561, 3329, 4096]                               # <4>, <8>, <10>, <13>, <16>, <16> full
LOG_TINY = np.log(1e-50)


class _Buf:
    """A device region of `nbytes` with GUARD bytes of 0xA5 before and after it (the region itself starts as 0xA5 too)."""

    def __init__(self, host=None, nbytes=None):
        import torch
        self.host = None if host is None else np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()
        self.nbytes = nbytes if host is None else self.host.size
        self.raw = torch.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.body = self.raw[GUARD:GUARD + self.nbytes]
        if host is not None:
            self.body.copy_(torch.from_numpy(self.host))

    def fetch(self, what) -> np.ndarray:
        """the region's bytes, after the sentinels (and an input's content) have been found untouched"""
        got = self.raw.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all(), "%s: bytes in front of the buffer were written" % what
        assert (got[GUARD + self.nbytes:] == 0xA5).all(), "%s: bytes behind the buffer were written" % what
        body = got[GUARD:GUARD + self.nbytes]
        if self.host is not None:
            assert np.array_equal(body, self.host), "%s: an input buffer was written" % what
        return body.copy()


def _encode(capi, ll, normalize, nbytes, want_lp, S=None, colmap=None, wgs=None):
    """One call of lna_encode_dev on guarded buffers: ll [F x P] float32 (P = S unless S is given), colmap int32 [S].
    -> (lp [F x S] float32 or None, bytes [F x S * nbytes])."""
    import torch
    assert ll.dtype == np.float32 and ll.ndim == 2
    F, P = ll.shape
    S = P if S is None else S
    what = "F=%d S=%d P=%d normalize=%d nbytes=%d lp=%d map=%d wgs=%s" % (
        F, S, P, normalize, nbytes, want_lp, colmap is not None, wgs)
    d_in = _Buf(host=ll)
    d_map = None if colmap is None else _Buf(host=np.asarray(colmap, np.int32))
    d_by = _Buf(nbytes=F * S * nbytes)
    d_lp = _Buf(nbytes=F * S * 4) if want_lp else None
    capi.lna_encode_dev(d_in.body.view(torch.float32).view(F, P), bool(normalize), nbytes,
                        None if d_lp is None else d_lp.body, d_by.body, num_states=S,
                        colmap=None if d_map is None else d_map.body, wgs_per_cu=wgs)
    torch.cuda.synchronize()
    by = d_by.fetch(what + " (bytes)").reshape(F, S * nbytes)
    lp = None if d_lp is None else d_lp.fetch(what + " (lp)").view(np.float32).reshape(F, S)
    d_in.fetch(what + " (input)")
    if d_map is not None:
        d_map.fetch(what + " (column map)")
    return lp, by


_ROWS, _REFS = {}, {}


def _rows(S):
    if S not in _ROWS:
        ll, labels = LC.rows(S, SEED)
        ll.setflags(write=False)
        _ROWS[S] = (ll, np.array(labels), np.array([LC.fast(r) for r in ll]))
    return _ROWS[S]


def _ref(oracle, S, normalize, nbytes):
    """the oracle's (lp, bytes, linear likelihoods) of _rows(S), computed once"""
    key = (S, bool(normalize), nbytes)
    if key not in _REFS:
        lik = np.maximum(np.exp(_rows(S)[0].astype(np.float64)), 1e-50)
        lp, by = oracle.lna_encode(lik, bool(normalize), nbytes)
        for a in (lp, by, lik):
            a.setflags(write=False)
        _REFS[key] = (lp, by, lik)
    return _REFS[key]


def _distance(a, b):
    """Steps between two 2-byte codes.  The code is the low 16 bits of (int)(-1820 lp + .5), which is negative for
    lp > 0 (unnormalised likelihoods above 1: the `gt1` rows), so neighbours can sit on either side of the wrap."""
    d = np.abs(a - b)
    return np.minimum(d, 65536 - d)


def _assert_lp(lp, ll, lp_ref, lik, normalize, what):
    """The bounds of test_lna_gpu.test_lna_matches_oracle on the float output: 1e-5 outside the float-denormal band of
    the reference's likelihood storage, one quantum inside it (conftest.assert_lp_denormal_band)."""
    ok = (ll > -87.0) | (ll < -104.5)
    assert np.isfinite(lp).all(), what
    assert np.abs(lp.astype(np.float64) - lp_ref)[ok].max() <= 1e-5, what
    # the helper divides by the oracle's Z; the unnormalised output has Z = 1, so it is handed lp - log Z
    shift = 0.0
    if not normalize:
        z = lik.astype(np.float32).astype(np.float64).sum(axis=1, keepdims=True)
        z[z == 0] = 1.0
        shift = np.log(z)
    n_band = assert_lp_denormal_band(lp.astype(np.float64) - shift, lik, what)
    assert n_band >= int(LC.in_band(ll).sum()) > 0, what


# ---------------------------------------------------------------------------------------------------------------------
# a. the fast path against the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("S", REG_SIZES)
def test_fast_path_against_the_oracle(capi, oracle, S, normalize):
    ll, labels, isfast = _rows(S)
    lp_ref, by_ref, lik = _ref(oracle, S, normalize, 2)
    _, by = _encode(capi, ll, normalize, 2, False)             # as production calls it: the fast path where a row allows
    lp_x, by_x = _encode(capi, ll, normalize, 2, True)         # a float output wanted: the exact path on every row
    code, cref = LC.codes(by, S), LC.codes(by_ref, S)
    low = ll < LC.LN_FLT_MIN
    onfast = np.broadcast_to(isfast[:, None], ll.shape)
    assert isfast.sum() >= 20 and (onfast & low).sum() >= 16
    assert (code[onfast & low] == 0xFFFF).all()
    d = _distance(code, cref)[onfast & ~low]
    assert d.max() <= 1
    # observed 0.999787 (S=255) - 1.0 normalised; unnormalised 1.0 but for S=3329 (0.999984: the reference's float
    # storage of the likelihood moves lp by up to 6e-8 relative, the fast path keeps the input float)
    observed("lna fast path codes equal S=%d norm=%d" % (S, normalize), float((d == 0).mean()), CODES_EQUAL_MIN)
    for kind in ("all_floor", "all_ninf"):
        assert (labels == kind).sum() == 4 and (code[labels == kind] == 0xFFFF).all(), kind
    # rows that fail the fast path's test run the same code with and without a float output.  Normalised, the band
    # states of the `band_mid` rows are visible codes (test_lna_cases_host), so a switch moved below -51 changes bytes
    # here; no other row kind shows it (edge_lo: log Z ~ -51, its band states are FF FF on either path)
    assert (~isfast).sum() >= 20
    assert np.array_equal(by[~isfast], by_x[~isfast])
    # ... and that code is held to the oracle through its float output, on every row
    _assert_lp(lp_x, ll, lp_ref, lik, normalize, "S=%d normalize=%d" % (S, normalize))
    assert np.allclose(lp_x[labels == "all_floor"], LOG_TINY, atol=1e-5)
    assert np.allclose(lp_x[labels == "all_ninf"], LOG_TINY, atol=1e-5)
    want = np.where(lp_x.astype(np.float64) < -36.008, 0xFFFF,
                    np.trunc(-1820.0 * lp_x.astype(np.float64) + .5).astype(np.int64) & 0xFFFF)
    assert np.array_equal(LC.codes(by_x, S), want)             # the exact path's codes follow its own float output


# ---------------------------------------------------------------------------------------------------------------------
# b. the fast path against the exact path
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("S", REG_SIZES)
def test_fast_path_against_the_exact_path(capi, S, normalize):
    ll, labels, isfast = _rows(S)
    _, by = _encode(capi, ll, normalize, 2, False)
    _, by_x = _encode(capi, ll, normalize, 2, True)
    code, cx = LC.codes(by, S), LC.codes(by_x, S)
    low = ll < LC.LN_FLT_MIN
    # no state below the float normal range: the same maximum, the same v_exp_f32 arguments, the same tree, the same
    # subtraction on both paths
    clean = isfast & ~low.any(axis=1)
    assert clean.sum() >= 8
    assert np.array_equal(by[clean], by_x[clean])
    # band or flushed states: FF FF both ways; they move Z by at most S * 2^-52 relative, log Z by < 1e-12 against a
    # float ulp of 4e-6 at |lp| ~ 36, so fewer than one other code in a million may differ, by one step
    mixed = isfast & low.any(axis=1)
    assert mixed.sum() >= 12
    m = mixed[:, None] & low
    assert (code[m] == 0xFFFF).all() and (cx[m] == 0xFFFF).all()
    d = _distance(code, cx)[mixed[:, None] & ~low]
    assert d.size and d.max() <= 1
    observed("lna fast path codes equal the exact path's S=%d norm=%d" % (S, normalize), float((d == 0).mean()),
             0.9999)    # observed 1.0 for every S, normalised and not


# ---------------------------------------------------------------------------------------------------------------------
# c. packing, no tolerance
# ---------------------------------------------------------------------------------------------------------------------

def _packing_values():
    rng = np.random.default_rng(5)
    edge = np.float32(-36.008)
    vals = [edge, np.float32(0.0), np.float32(-0.0)]
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        v = edge
        for _ in range(8):
            v = np.nextafter(v, toward)
            vals.append(v)
    vals += list(rng.uniform(-36.1, 0.0, 2000).astype(np.float32))
    # the rounding ties of the code: -(k + 1/2) / 1820, the nearest float and its two neighbours
    tie = (-(rng.choice(65535, 200, replace=False) + 0.5) / 1820.0).astype(np.float32)
    vals += list(tie) + list(np.nextafter(tie, np.float32(np.inf))) + list(np.nextafter(tie, np.float32(-np.inf)))
    v = np.array(vals, np.float32)
    v64 = v.astype(np.float64)
    want = np.where(v64 < -36.008, 0xFFFF, np.trunc(-1820.0 * v64 + .5).astype(np.int64))
    assert (want == 0xFFFF).sum() >= 8 and ((want >= 0) & (want <= 0xFFFF)).all()
    return v, want


@pytest.mark.parametrize("shape", [(3, 875), (1, 4097)])     # a register instance with odd rows; the generic kernel
def test_packing_of_the_unnormalised_fast_path_is_exact(capi, shape):
    """Unnormalised and on the fast path (or through the generic kernel) lp is the input float itself, so the code is
    a function of the input: FF FF below -36.008, else (int)(-1820 lp + .5), big-endian."""
    v, want = _packing_values()
    F, S = shape
    assert v.size <= F * S
    ll = np.full(F * S, -1.0, np.float32)
    ll[:v.size] = v
    ll = ll.reshape(F, S)
    assert all(LC.fast(r) for r in ll)
    _, by = _encode(capi, ll, False, 2, False)
    code = LC.codes(by, S).reshape(-1)
    assert np.array_equal(code[:v.size], want)
    assert (code[v.size:] == 1820).all()


# ---------------------------------------------------------------------------------------------------------------------
# d. the column map, every instance
# ---------------------------------------------------------------------------------------------------------------------

_COMBOS = [(nbytes, normalize, want_lp) for nbytes in (2, 4) for normalize in (True, False) for want_lp in (True, False)]


def _same(a, b):
    (lp_a, by_a), (lp_b, by_b) = a, b
    if (lp_a is None) != (lp_b is None) or not np.array_equal(by_a, by_b):
        return False
    return lp_a is None or np.array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32))


@pytest.mark.parametrize("S", MAP_SIZES)
def test_column_map_gives_the_bytes_of_the_dense_rows(capi, S):
    ll, _, _ = _rows(S)
    F, P = ll.shape[0], S + 91
    colmap = np.random.default_rng(S).permutation(P)[:S].astype(np.int32)
    scattered = np.full((F, P), 50.0, np.float32)        # one read of an unmapped column wrecks Z
    scattered[:, colmap] = ll
    assert np.array_equal(scattered[:, colmap].view(np.uint32), ll.view(np.uint32))
    assert (colmap != np.arange(S)).mean() > 0.9
    identity = np.arange(S, dtype=np.int32)
    for nbytes, normalize, want_lp in _COMBOS:
        dense = _encode(capi, ll, normalize, nbytes, want_lp)
        mapped = _encode(capi, scattered, normalize, nbytes, want_lp, S=S, colmap=colmap)
        assert _same(mapped, dense), (nbytes, normalize, want_lp)
        ident = _encode(capi, ll, normalize, nbytes, want_lp, colmap=identity)
        assert _same(ident, dense), (nbytes, normalize, want_lp)


def test_column_map_needs_a_register_instance(capi):
    S = 4097
    ll = np.full((2, S), -20.0, np.float32)
    with pytest.raises(capi.AasrError) as ei:
        _encode(capi, ll, True, 2, False, colmap=np.arange(S, dtype=np.int32))
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# e. row pitch
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", MAP_SIZES + GENERIC_SIZES)
def test_row_pitch_gives_the_bytes_of_the_dense_rows(capi, S):
    ll, _, _ = _rows(S)
    F, P = ll.shape[0], S + 37
    padded = np.full((F, P), 50.0, np.float32)
    padded[:, :S] = ll
    for nbytes, normalize, want_lp in _COMBOS:
        dense = _encode(capi, ll, normalize, nbytes, want_lp)
        assert _same(_encode(capi, padded, normalize, nbytes, want_lp, S=S), dense), (nbytes, normalize, want_lp)


# ---------------------------------------------------------------------------------------------------------------------
# f. grid and prefetch
# ---------------------------------------------------------------------------------------------------------------------

def _path(row):
    return "ninf" if np.isneginf(row).all() else "fast" if LC.fast(row) else "exact"


@pytest.mark.parametrize("S", [130, 3125])
def test_which_workgroup_encodes_a_row_changes_no_byte(capi, oracle, S):
    """2 cus + 5 rows: at one workgroup per CU every workgroup walks two or three rows, each loaded while the one
    before it is encoded (vn[] -> v[]).  The rows of one workgroup, and neighbouring rows, take different paths --
    fast, exact, all -inf -- so the number of barriers a workgroup passes changes from frame to frame."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= 8
    F = 2 * cus + 5
    pool, _ = LC.rows(S, SEED + 1, frames=200)
    by_path = {"fast": [], "exact": [], "ninf": []}
    for row in pool:
        by_path[_path(row)].append(row)
    order = ("fast", "exact", "ninf")
    bump = 1 if (cus + 1) % 3 else 2             # rows b, b + cus, b + 2 cus of workgroup b: three different paths
    ll = np.empty((F, S), np.float32)
    used = dict.fromkeys(order, 0)
    for r in range(F):
        p = order[(r + bump * (r // cus)) % 3]
        ll[r] = by_path[p][used[p] % len(by_path[p])]
        used[p] += 1
    for b in range(5):
        assert len({_path(ll[b]), _path(ll[b + cus]), _path(ll[b + 2 * cus])}) == 3
    for b in range(5, cus):
        assert _path(ll[b]) != _path(ll[b + cus])
    picks = sorted({0, 1, cus - 1, cus, cus + 1, cus + 4, cus + 5, 2 * cus - 1, 2 * cus, 2 * cus + 1, 2 * cus + 3, F - 1})
    assert len(picks) == 12
    for nbytes, want_lp in ((2, False), (4, True)):            # production's call; the exact path with both outputs
        one = _encode(capi, ll, True, nbytes, want_lp, wgs=1)
        for wgs in (2, 32):
            assert _same(_encode(capi, ll, True, nbytes, want_lp, wgs=wgs), one), (nbytes, wgs)
        assert _same(_encode(capi, ll, True, nbytes, want_lp), one), nbytes       # the entry point without a grid
        for r in picks:
            lp1, by1 = _encode(capi, ll[r:r + 1], True, nbytes, want_lp, wgs=1)
            assert np.array_equal(by1[0], one[1][r]), (nbytes, r, _path(ll[r]))
            if want_lp:
                assert np.array_equal(lp1[0].view(np.uint32), one[0][r].view(np.uint32)), (nbytes, r)
        if nbytes == 2:
            # ... and the rows are their own: the second and third row of a workgroup against the oracle
            _, by_ref = oracle.lna_encode(np.maximum(np.exp(ll[picks].astype(np.float64)), 1e-50), True, 2)
            ok = (ll[picks] > -87.0) | (ll[picks] < -104.5)
            assert _distance(LC.codes(one[1][picks], S), LC.codes(by_ref, S))[ok].max() <= 1


@pytest.mark.parametrize("wgs", [0, 1025])
def test_grid_outside_its_range_is_refused(capi, wgs):
    ll = np.full((2, 130), -20.0, np.float32)
    with pytest.raises(capi.AasrError) as ei:
        _encode(capi, ll, True, 2, False, wgs=wgs)
    assert ei.value.code == capi.AASR_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# g. the generic kernel against the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("nbytes", [2, 4])
@pytest.mark.parametrize("S", GENERIC_SIZES)
def test_generic_kernel_against_the_oracle(capi, oracle, S, nbytes, normalize):
    ll, labels, _ = _rows(S)
    lp_ref, by_ref, lik = _ref(oracle, S, normalize, nbytes)
    lp, by = _encode(capi, ll, normalize, nbytes, True)
    ok = (ll > -87.0) | (ll < -104.5)
    _assert_lp(lp, ll, lp_ref, lik, normalize, "S=%d nbytes=%d normalize=%d" % (S, nbytes, normalize))
    # inside the band the quantum index may differ by one step at a rounding tie
    q = np.abs(lp - lp_ref)[~ok]
    observed("lna generic denormal band within 1e-5 S=%d" % S, float((q <= 1e-5).mean()), 0.99)    # observed 0.99947 - 0.99962
    if nbytes == 4:
        assert np.array_equal(by.view(np.float32), lp)
    else:
        d = _distance(LC.codes(by, S), LC.codes(by_ref, S))[ok]
        assert d.max() <= 1                      # |dlp| 1e-5 * 1820 << 1 code
        observed("lna generic codes equal S=%d norm=%d" % (S, normalize), float((d == 0).mean()), 0.995)
        # observed 0.99997 normalised, 1.0 unnormalised
    assert np.allclose(lp[labels == "all_floor"], LOG_TINY, atol=1e-5)
    assert np.allclose(lp[labels == "all_ninf"], LOG_TINY, atol=1e-5)
    # the generic kernel has one path: the call without a float output gives the same bytes
    assert np.array_equal(_encode(capi, ll, normalize, nbytes, False)[1], by)

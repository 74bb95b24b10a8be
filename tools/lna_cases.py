"""lna_cases.py -- rows of state log-likelihoods for the tests of the LNA pass (csrc/lna_device.h, csrc/lna_encode.hip),
shared by tests/test_lna_cases_host.py (the oracle alone, no device) and tests/test_lna_paths_gpu.py.  NumPy only.

The register-resident kernels encode a row on one of two paths (lna_row_from_registers): with 2-byte codes and no float
output wanted, a row whose best state is >= -51 uses the raw values (`fast`); every other row, and every call with 4-byte
output or a float output, goes through the emulation of the reference's float storage of the linear likelihood (the
float-denormal band ln 2^-150 <= ll < ln 2^-126 quantised, below it flushed to the floor).  The rows below put values on
both sides of each of those switches.
"""
from __future__ import annotations

import numpy as np

LOG_TINY = np.float32(np.log(1e-50))          # the floor of safe_log as the float a score buffer holds
LN_FLT_MIN = np.float32(-87.33654475)         # ln 2^-126: below it (float) exp(ll) is a denormal or zero
FAST_MIN = np.float32(-51.0)                  # the kernel's `mr >= -51.0f`
BAND = (-103.9, -87.4)                        # inside the denormal band, clear of both of its edges
FLUSH = (-114.0, -104.1)                      # (float) exp(ll) == 0

# the order keeps rows that take different paths next to one another: F(ast), N(ot fast)
KINDS = ("plain",      # F (unless every state of a very short row falls below -51)
         "edge_lo",    # N
         "band_fast",  # F
         "all_ninf",   # N
         "gt1",        # F
         "band_max",   # N
         "edge_hi",    # F
         "all_floor",  # N
         "one_hot",    # F
         "flat",       # F
         "band_mid")   # N: the row that needs the exact path -- its band states leave as codes other than FF FF


def fast(row) -> bool:
    """The kernel's test for its fast path, on the float32 row: max >= -51."""
    row = np.asarray(row)
    assert row.dtype == np.float32
    return bool(row.max() >= FAST_MIN)


def _flushed(rng, n: int, turn: int) -> np.ndarray:
    """n values whose float likelihood is zero: below the band, the floor itself, far below it, -inf (a row with one
    such value takes them in turn)"""
    out = rng.uniform(FLUSH[0], FLUSH[1], n).astype(np.float32)
    flavour = (np.arange(n) + turn) % 4
    out[flavour == 1] = LOG_TINY
    out[flavour == 2] = np.float32(-200.0)
    out[flavour == 3] = -np.inf
    return out[rng.permutation(n)]


def _edge(rng, S: int) -> np.ndarray:
    """max exactly -51 at a random place, the rest in [-86, -52], a few band entries"""
    row = rng.uniform(-86.0, -52.0, S).astype(np.float32)
    where = rng.permutation(S)
    n_band = min(3, max(1, (S - 1) // 2))
    row[where[1:1 + n_band]] = rng.uniform(BAND[0], BAND[1], n_band).astype(np.float32)
    row[where[0]] = FAST_MIN
    return row


def _row(kind: str, rng, S: int, turn: int) -> np.ndarray:
    if kind == "plain":
        return rng.uniform(-80.0, -5.0, S).astype(np.float32)
    if kind == "gt1":
        return rng.uniform(-10.0, 5.0, S).astype(np.float32)
    if kind == "band_fast":
        row = rng.uniform(-80.0, -5.0, S).astype(np.float32)
        where = rng.permutation(S)
        row[where[0]] = np.float32(rng.uniform(-51.0, -5.0))      # max >= -51 whatever the rest drew
        n_band = max(1, int(round(0.3 * S)))
        n_flush = max(1, int(round(0.1 * S)))
        row[where[1:1 + n_band]] = rng.uniform(BAND[0], BAND[1], n_band).astype(np.float32)
        row[where[1 + n_band:1 + n_band + n_flush]] = _flushed(rng, n_flush, turn)
        return row
    if kind == "edge_hi":
        return _edge(rng, S)
    if kind == "edge_lo":
        row = _edge(rng, S)
        row[row == FAST_MIN] = np.nextafter(FAST_MIN, np.float32(-np.inf))
        return row
    if kind == "band_max":
        return rng.uniform(-100.0, -88.0, S).astype(np.float32)
    if kind == "all_floor":
        return np.full(S, LOG_TINY, np.float32)
    if kind == "all_ninf":
        return np.full(S, -np.inf, np.float32)
    if kind == "one_hot":
        row = _flushed(rng, S, turn)
        row[int(rng.integers(0, S))] = np.float32(-3.0)
        return row
    if kind == "flat":
        return np.full(S, -30.0, np.float32)
    if kind == "band_mid":
        # every normal state in [-86, -75]: log Z stays below -68 for 5000 states, so normalised every band state
        # has lp > -36.008 and its denormal quantum (a handful of quanta near the band's lower end: up to 0.4 nats)
        # shows in the code
        row = rng.uniform(-86.0, -75.0, S).astype(np.float32)
        where = rng.permutation(S)
        n_band = max(1, int(round(0.3 * S)))
        n_flush = int(round(0.05 * S))
        row[where[1:1 + n_band]] = rng.uniform(BAND[0], BAND[1], n_band).astype(np.float32)
        row[where[1 + n_band:1 + n_band + n_flush]] = _flushed(rng, n_flush, turn)
        return row
    raise ValueError(kind)


def rows(S: int, seed: int, frames: int = 4 * len(KINDS)):
    """([frames x S] float32, [frames] labels): row r is of kind KINDS[r % len(KINDS)].  edge_hi and edge_lo of one
    pass over KINDS are the same row but for the maximum."""
    if S < 3:
        raise ValueError("the band_fast and edge rows need three states")
    rng = np.random.default_rng([seed, S])
    ll = np.empty((frames, S), np.float32)
    labels = []
    edge_seed = 0
    for r in range(frames):
        kind = KINDS[r % len(KINDS)]
        if r % len(KINDS) == 0:
            edge_seed = int(rng.integers(0, 2 ** 31))
        # both edge rows of a pass draw from the same stream
        ll[r] = _row(kind, np.random.default_rng(edge_seed) if kind in ("edge_hi", "edge_lo") else rng, S,
                     r // len(KINDS))
        labels.append(kind)
    return ll, labels


def in_band(ll) -> np.ndarray:
    ll = np.asarray(ll)
    return (ll >= np.float32(BAND[0])) & (ll <= np.float32(BAND[1]))


def codes(by, S: int) -> np.ndarray:
    """[F x 2 S] bytes of 2-byte LNA rows -> [F x S] codes (big-endian on disk)"""
    b = np.asarray(by, np.uint8).reshape(-1, S, 2).astype(np.int32)
    return b[..., 0] * 256 + b[..., 1]

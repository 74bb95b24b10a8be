"""Full statistics (stats --full-stats, mode-3 dumps) on the host, no GPU: the mode-3 .gks writer
(FullStatisticsAccumulator::dump_statistics, aku/Distributions.cc:42-60) against hand-built bytes, against the
restatement's writer and through the estimate reader; the new symbols of aasr.h; the options; and what the stats tool
and aasr_stats_create_full decide before a device is opened."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from aaltoasr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stats_full_restate as SR  # noqa: E402

NEW_SYMBOLS = ["aasr_stats_create_full", "aasr_stats_mode", "aasr_stats_full_moments", "aasr_stats_write_gks_full",
               "aasr_debug_stats_full_shape", "aasr_debug_stats_set_slab_bytes"]

# the toy model of tests/test_stats_host.py: three HMMs over six states, two Gaussians of two dimensions
PH = """PHONE
3
1 5 a
-1 -2 0 1 2
0 1 2 1.0
1 0
2 3 2 0.6 3 0.3 4 0.1
3 2 3 0.7 4 0.3
4 2 4 0.8 1 0.2
2 3 b
-1 -2 3
0 1 2 1.0
1 0
2 2 2 0.5 1 0.5
3 4 c
-1 -2 4 5
0 1 2 1.0
1 0
2 3 2 0.5 3 0.25 1 0.25
3 2 3 0.9 1 0.1
"""


@pytest.fixture(scope="module")
def lib():
    from aaltoasr_amd import build
    build.build()
    return A.lib()


def _model(tmp_path, dim=2):
    base = str(tmp_path / "m")
    open(base + ".ph", "w").write(PH)
    with open(base + ".gk", "w") as f:
        f.write("2 %d variable\n" % dim)
        for g in range(2):
            f.write("diag " + " ".join([str(g)] * dim + ["1"] * dim) + "\n")
    with open(base + ".mc", "w") as f:
        f.write("6\n" + "1 0 1.0\n" * 6)
    open(str(tmp_path / "f.cfg"), "w").write("module\n{\n name fft\n type fft\n}\n")
    open(str(tmp_path / "r.rcp"), "w").write("audio=x.wav transcript=x.phn\n")
    return base


def _run(args):
    r = subprocess.run([os.path.join(BIN, "stats")] + args, capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


def test_write_gks_full_bytes(lib, tmp_path):
    """2 Gaussians of 3 dimensions, the second not accumulated"""
    p = str(tmp_path / "x.gks")
    fc, g, a = np.array([4, 0]), np.array([3.5, 0.0]), np.array([3.75, 0.0])
    sx = np.array([[1.0, -2.0, 0.1], [9, 9, 9]])
    sxx = np.array([[11.0, 21.0, 22.0, 31.0, 1e10, 33.3], [9] * 6])      # (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    A.stats_write_gks_full(p, fc, g, a, sx, sxx)
    want = struct.pack("<3i", 2, 3, 3)
    want += struct.pack("<i", 0) + struct.pack("<iidd", 0, 4, 3.5, 3.75) + np.asarray(sx[0], "<f4").tobytes() + \
        np.asarray(sxx[0], "<f4").tobytes() + struct.pack("<i", -1)
    want += struct.pack("<i", 1) + struct.pack("<i", -1)
    assert open(p, "rb").read() == want
    with pytest.raises(ValueError):
        A.stats_write_gks_full(p, fc, g, a, sx, sxx[:, :3])


def test_write_gks_full_equals_the_restatements_writer(lib, tmp_path):
    rng = np.random.default_rng(4)
    G, D = 9, 7
    fc = rng.integers(0, 3, G) * rng.integers(1, 1000, G)
    assert (fc == 0).any() and (fc > 0).any()
    g, sx, sxx = rng.uniform(1, 50, G), rng.normal(size=(G, D)) * 100, rng.normal(size=(G, SR.tri(D))) * 1e4
    A.stats_write_gks_full(str(tmp_path / "a.gks"), fc, g, np.zeros(G), sx, sxx)
    SR.write_gks_full(str(tmp_path / "b.gks"), fc, g, sx, sxx)
    assert open(tmp_path / "a.gks", "rb").read() == open(tmp_path / "b.gks", "rb").read()


def test_estimate_reads_the_file_back_as_mode_3(lib, tmp_path):
    base = _model(tmp_path, dim=3)
    rng = np.random.default_rng(5)
    fc, g = np.array([12, 0]), np.array([10.5, 0.0])
    sx, sxx = rng.normal(size=(2, 3)) * 10, rng.normal(size=(2, 6)) * 100
    out = str(tmp_path / "d")
    A.stats_write_gks_full(out + ".gks", fc, g, g.copy(), sx, sxx)
    A.stats_write_mcs(out + ".mcs", np.arange(7), np.zeros(6, np.int32), np.zeros(6, np.int64), np.zeros(6), np.zeros(6),
                      np.zeros(6), mode=3)
    A.stats_write_lls(out + ".lls", -1.0, 12)
    e = A.Estimate.from_base(base)
    e.add_dump(out)
    assert e.sizes()["mode"] == 3
    st = e.statistics()
    assert st["accumulated"].tolist() == [1, 0] and st["feacount"].tolist() == [12, 0] and st["gamma"][0] == 10.5
    assert (st["sum_x"][0] == sx[0].astype(np.float32)).all() and (st["sum_xx"][0] == sxx[0].astype(np.float32)).all()
    assert st["sum_xx"].shape == (2, 6) and (st["sum_xx"][1] == 0).all()
    e.close()


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_declared(lib, name):
    assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    header = open(os.path.join(ROOT, "include", "aasr.h")).read()
    assert re.search(r"\b%s\(" % name, header), name


def test_options_default_to_plain_statistics(lib):
    o = A.StatsOptions.defaults()
    assert o.full_stats == 0
    assert A.StatsOptions.defaults(full_stats=1).full_stats == 1
    assert A.StatsOptions._fields_[-1][0] == "full_stats"


def test_tool_accepts_full_stats(lib, tmp_path):
    """past option checking: it fails on the device or on its input, not as an unsupported option"""
    base = _model(tmp_path)
    rc, err = _run(["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o", str(tmp_path / "o"),
                    "--ml", "--full-stats"])
    assert rc != 0 and "not supported" not in err and "full-stats" not in err, err
    assert not os.path.exists(str(tmp_path / "o.gks"))
    # and --mllt stays refused as before
    rc, err = _run(["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o", str(tmp_path / "o"),
                    "--ml", "--mllt"])
    assert rc != 0 and "stats: --mllt is not supported; only --ml over .phn files is" in err, err
    r = subprocess.run([os.path.join(BIN, "stats"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--full-stats" in r.stdout + r.stderr


def test_tool_refuses_128_dimensions_before_the_device(lib, tmp_path):
    base = _model(tmp_path, dim=128)
    common = ["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o", str(tmp_path / "o"), "--ml"]
    rc, err = _run(common + ["--full-stats", "--device", "7"])      # (an ordinal that would be refused when opened)
    assert rc != 0 and "at most 127 dimensions" in err and "--full-stats" in err and "has 128" in err, err
    rc, err = _run(common + ["--device", "7"])                      # without the option the same pool gets further
    assert rc != 0 and "at most 127 dimensions" not in err, err


def test_create_full_without_a_device(lib):
    """A full handle is made from a model handle, and without a device there is none: the model's creation is
    AASR_ERR_NO_DEVICE (no fallback), and aasr_stats_create_full without a model is refused as a bad argument, leaving
    no handle.  (With a device, tests/test_stats_full_gpu.py creates the handle.)"""
    h = ctypes.c_void_p()
    assert lib.aasr_stats_create_full(None, None, ctypes.byref(h)) == A.AASR_ERR_INVALID and not h.value
    assert b"aasr_stats_create_full" in lib.aasr_last_error()
    assert lib.aasr_stats_mode(None) == -1
    if lib.aasr_device_count() > 0:
        return
    rng = np.random.default_rng(1)
    with pytest.raises(A.AasrError) as ei:
        A.Gmm.from_arrays(rng.normal(size=(2, 3)), np.ones((2, 3)), np.arange(7, dtype=np.int32), np.zeros(6, np.int32),
                          np.ones(6))
    assert ei.value.code == A.AASR_ERR_NO_DEVICE

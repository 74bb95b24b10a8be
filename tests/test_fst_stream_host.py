"""Streaming sessions of the FST decoder on the host: the C ABI's symbols and argument checks (aasr_fst_stream_*), the
module's lna_open_fd, and the fst_stream tool's refusals, all before a device is asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

SYMBOLS = ["aasr_fst_stream_create", "aasr_fst_stream_destroy", "aasr_fst_stream_device_bytes", "aasr_fst_stream_options",
           "aasr_fst_stream_reset", "aasr_fst_stream_feed_dev", "aasr_fst_stream_sync", "aasr_fst_stream_result",
           "aasr_fst_stream_tokens", "aasr_fst_live_default_options", "aasr_run_fst_live"]


def test_symbols_are_declared_and_resolve(capi):
    declared = capi.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert getattr(capi.lib(), name) is not None, name
    assert callable(capi.FstStream) and all(callable(getattr(capi.FstStream, m)) for m in ("feed_dev", "sync", "reset", "result", "tokens"))


def refused(capi, status, name):
    assert status == capi.AASR_ERR_INVALID, status
    assert name.encode() in capi.lib().aasr_last_error(), capi.lib().aasr_last_error()


def test_null_and_range_arguments_are_invalid(capi):
    L = capi.lib()
    net = capi.FstNet(os.path.join(GOLDEN, "toy.fst"))
    opts = capi.FstOptions.defaults()
    out = C.c_void_p()
    for args in ((None, None, C.byref(opts), 1, 10, C.byref(out)),
                 (net.handle, None, None, 1, 10, C.byref(out)),
                 (net.handle, None, C.byref(opts), 1, 10, None),
                 (net.handle, None, C.byref(opts), 0, 10, C.byref(out)),
                 (net.handle, None, C.byref(opts), -3, 10, C.byref(out)),
                 (net.handle, None, C.byref(opts), 1, 0, C.byref(out))):
        refused(capi, L.aasr_fst_stream_create(*args), "aasr_fst_stream_create")
        assert not out.value
    row0, n_new = np.zeros(1, np.int64), np.ones(1, np.int32)
    refused(capi, L.aasr_fst_stream_feed_dev(None, None, 2, 9, 0, row0.ctypes.data, n_new.ctypes.data, None), "aasr_fst_stream_feed_dev")
    refused(capi, L.aasr_fst_stream_reset(None, 0), "aasr_fst_stream_reset")
    refused(capi, L.aasr_fst_stream_reset(None, -1), "aasr_fst_stream_reset")
    refused(capi, L.aasr_fst_stream_sync(None, None), "aasr_fst_stream_sync")
    refused(capi, L.aasr_fst_stream_result(None, 0, None, None, None, None, None, None, None, 0, None, None, 0, None), "aasr_fst_stream_result")
    refused(capi, L.aasr_fst_stream_tokens(None, 0, 0, None, None, None, None, 0, None), "aasr_fst_stream_tokens")
    refused(capi, L.aasr_run_fst_live(None, None, net.handle, None, None, None), "aasr_run_fst_live")
    assert L.aasr_fst_stream_device_bytes(None) == -1
    L.aasr_fst_stream_destroy(None)
    live = (C.c_int32 * 14)()
    L.aasr_fst_live_default_options(live)
    assert list(live)[8:14] == [2, 16, 7500, 0, 0, 0]      # behind the eight words of aasr_fst_options


def test_module_has_lna_open_fd(capi, tmp_path):
    from aaltoasr_amd import FstDecoder
    s = FstDecoder.FstSearch(os.path.join(GOLDEN, "toy.fst"), None, None)
    assert callable(s.lna_open_fd)
    assert FstDecoder.STREAM_MAX_FRAMES >= 1 and "STREAM_MAX_FRAMES" in FstDecoder.__doc__
    for image, message in ((b"\0\0\0\3\7", "invalid LNA byte number 7"), (b"\0\0\0\0\2", "invalid number of states 0"),
                           (b"\0\0\0", "End of file reached")):
        rd, wr = os.pipe()
        os.write(wr, image)
        os.close(wr)
        try:
            with pytest.raises(RuntimeError, match=message):
                s.lna_open_fd(rd, 1024)
        finally:
            os.close(rd)
    with pytest.raises(RuntimeError, match="invalid LNA byte number"):      # as the file path does
        open(str(tmp_path / "bad.lna"), "wb").write(b"\0\0\0\3\7")
        s.lna_open(str(tmp_path / "bad.lna"), 1024)


ALL = ["--fst", os.path.join(GOLDEN, "toy.fst"), "-c", "x.cfg", "-b", "nowhere/model"]
REFUSALS = [(ALL[2:], "--fst is missing"),
            (ALL[:2] + ALL[4:], "--config is missing"),
            (ALL[:4], "Must give either --base or all --gk, --mc and --ph"),
            (ALL[:4] + ["-g", "a.gk", "-m", "a.mc"], "Must give either --base or all --gk, --mc and --ph"),
            (ALL + ["--beam", "-3"], "the beam must not be negative"),
            (ALL + ["--token-limit", "-1"], "the token limit must not be negative"),
            (ALL + ["--cap-candidates", "-1"], "a capacity must not be negative"),
            (ALL + ["--cap-history", "-4"], "a capacity must not be negative"),
            (ALL + ["--chunk-frames", "0"], "--chunk-frames must be at least 1"),
            (ALL + ["--max-frames", "0"], "--max-frames must be at least 1"),
            (ALL + ["--dur-by-state"], "--dur-by-state without --dur"),
            (ALL + ["--lnabytes", "1"], "--lnabytes is 2 or 4"),
            (ALL + ["--lnabytes", "3"], "--lnabytes is 2 or 4")]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[m for _, m in REFUSALS[:3]] + ["three of -g -m -p"] + [" ".join(f[6:]) for f, _ in REFUSALS[4:]])
def test_tool_refuses_before_the_device_is_opened(flags, message):
    r = subprocess.run([os.path.join(BIN, "fst_stream")] + flags, input=b"", capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stderr.startswith(b"exception: fst_stream: ") and message.encode() in r.stderr, r.stderr
    assert r.stdout == b""

"""Confidence on streaming sessions, on the host: the C ABI's symbols and argument checks (aasr_fst_conf_stream_*,
aasr_run_fst_live_confidence), the option structs, the confidence classes' lna_open_fd, and the fst_stream tool's refusals
of its --confidence options, all before a device is asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
CONF = os.path.join(ROOT, "tests", "golden", "fst_conf")
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

SYMBOLS = ["aasr_fst_conf_stream_create", "aasr_fst_conf_stream_destroy", "aasr_fst_conf_stream_device_bytes",
           "aasr_fst_conf_stream_options", "aasr_fst_conf_stream_reset", "aasr_fst_conf_stream_feed_dev", "aasr_fst_conf_stream_sync",
           "aasr_fst_conf_stream_result", "aasr_fst_conf_stream_search_result", "aasr_fst_conf_stream_tokens",
           "aasr_fst_conf_stream_record", "aasr_fst_conf_stream_best_acu", "aasr_fst_live_confidence_default_options",
           "aasr_run_fst_live_confidence"]


def test_symbols_are_declared_and_resolve(capi):
    declared = capi.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert getattr(capi.lib(), name) is not None, name
    assert callable(capi.FstConfStream)
    assert all(callable(getattr(capi.FstConfStream, m)) for m in ("feed_dev", "sync", "reset", "result", "search_result", "tokens", "close"))


def refused(capi, status, name):
    assert status == capi.AASR_ERR_INVALID, status
    assert name.encode() in capi.lib().aasr_last_error(), capi.lib().aasr_last_error()


def test_null_and_range_arguments_are_invalid(capi):
    L = capi.lib()
    net = capi.FstNet(os.path.join(GOLDEN, "toy.fst"))
    opts = capi.FstConfOptions.defaults()
    loop = capi.FstConfOptions.defaults(phone_loop=1)
    bad = capi.FstConfOptions.defaults()
    bad.phone.token_limit = -1
    out = C.c_void_p()
    for args in ((None, None, None, C.byref(opts), 1, 10, C.byref(out)),           # no grammar network
                 (net.handle, None, None, None, 1, 10, C.byref(out)),
                 (net.handle, None, None, C.byref(opts), 1, 10, None),
                 (net.handle, None, None, C.byref(opts), 0, 10, C.byref(out)),
                 (net.handle, None, None, C.byref(opts), -3, 10, C.byref(out)),
                 (net.handle, None, None, C.byref(opts), 1, 0, C.byref(out)),
                 (net.handle, None, None, C.byref(loop), 1, 10, C.byref(out)),     # phone_loop without a network
                 (net.handle, None, None, C.byref(bad), 1, 10, C.byref(out))):     # bad options of the phone search
        refused(capi, L.aasr_fst_conf_stream_create(*args), "aasr_fst_conf_stream_create")
        assert not out.value
    row0, n_new = np.zeros(1, np.int64), np.ones(1, np.int32)
    refused(capi, L.aasr_fst_conf_stream_feed_dev(None, None, 2, 9, 0, row0.ctypes.data, n_new.ctypes.data, None), "aasr_fst_conf_stream_feed_dev")
    refused(capi, L.aasr_fst_conf_stream_reset(None, 0), "aasr_fst_conf_stream_reset")
    refused(capi, L.aasr_fst_conf_stream_reset(None, -1), "aasr_fst_conf_stream_reset")
    refused(capi, L.aasr_fst_conf_stream_sync(None, None), "aasr_fst_conf_stream_sync")
    refused(capi, L.aasr_fst_conf_stream_result(None, 0, None), "aasr_fst_conf_stream_result")
    refused(capi, L.aasr_fst_conf_stream_search_result(None, 0, 0, None, None, None, None, None, None, None, 0, None, None, 0, None),
            "aasr_fst_conf_stream_search_result")
    refused(capi, L.aasr_fst_conf_stream_tokens(None, 0, 0, 0, None, None, None, None, 0, None), "aasr_fst_conf_stream_tokens")
    refused(capi, L.aasr_fst_conf_stream_record(None, 0, 0, None, None, None, None, None), "aasr_fst_conf_stream_record")
    refused(capi, L.aasr_fst_conf_stream_best_acu(None, 0, None, None), "aasr_fst_conf_stream_best_acu")
    refused(capi, L.aasr_run_fst_live_confidence(None, None, net.handle, None, None, None, None), "aasr_run_fst_live_confidence")
    live = (C.c_int32 * 23)()
    L.aasr_fst_live_confidence_default_options(live)
    refused(capi, L.aasr_run_fst_live_confidence(None, None, net.handle, None, None, live, None), "aasr_run_fst_live_confidence")
    assert L.aasr_fst_conf_stream_device_bytes(None) == -1
    L.aasr_fst_conf_stream_destroy(None)
    L.aasr_fst_conf_stream_options(None, None)


def test_option_structs_and_their_defaults(capi):
    L = capi.lib()
    live = (C.c_int32 * 15)()
    live[14] = 77
    L.aasr_fst_live_default_options(live)
    assert list(live)[8:14] == [2, 16, 7500, 0, 0, 0] and live[14] == 77      # aasr_fst_live_options is still 14 words
    fst = (C.c_int32 * 8)()
    L.aasr_fst_default_options(fst)
    conf = (C.c_int32 * 24)()
    conf[23] = 77
    L.aasr_fst_live_confidence_default_options(conf)
    # an aasr_fst_live_options, the phone search's aasr_fst_options, phone_loop: 14 + 8 + 1 words
    assert list(conf)[:14] == list(live)[:14] and list(conf)[14:22] == list(fst) and conf[22] == 0 and conf[23] == 77
    L.aasr_fst_live_confidence_default_options(None)


@pytest.mark.parametrize("which", ["FstConfidence", "FstConfidenceWithPhoneLoop"])
def test_confidence_classes_have_lna_open_fd(capi, which):
    from aaltoasr_amd import FstDecoder
    fst = os.path.join(GOLDEN, "toy.fst")
    s = FstDecoder.FstConfidence(fst, None, None) if which == "FstConfidence" else \
        FstDecoder.FstConfidenceWithPhoneLoop(fst, os.path.join(CONF, "toy.ploop.fst"), None, None)
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
    with pytest.raises(RuntimeError, match="file not opened yet"):      # nothing was opened: run() still says so
        s.run()
    assert "FstConfStream" in FstDecoder.__doc__


ALL = ["--fst", os.path.join(GOLDEN, "toy.fst"), "-c", "x.cfg", "-b", "nowhere/model"]
PLOOP = ["--phone-loop", os.path.join(CONF, "toy.ploop.fst")]
REFUSALS = [(ALL + PLOOP, "--phone-loop without --confidence"),
            (ALL + ["--phone-beam", "10"], "--phone-beam without --confidence"),
            (ALL + ["--phone-token-limit", "10"], "--phone-token-limit without --confidence"),
            (ALL + ["--phone-duration-scale", "2"], "--phone-duration-scale without --confidence"),
            (ALL + ["--confidence", "--phone-beam", "10"], "--phone-beam without --phone-loop"),
            (ALL + ["--confidence", "--phone-token-limit", "10"], "--phone-token-limit without --phone-loop"),
            (ALL + ["--confidence"] + PLOOP + ["--phone-beam", "-1"], "the phone beam must not be negative"),
            (ALL + ["--confidence"] + PLOOP + ["--phone-token-limit", "-2"], "the phone token limit must not be negative"),
            (ALL + ["--confidence", "--beam", "-3"], "the beam must not be negative")]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_tool_refuses_before_the_device_is_opened(flags, message):
    r = subprocess.run([os.path.join(BIN, "fst_stream")] + flags, input=b"", capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stderr.startswith(b"exception: fst_stream: ") and message.encode() in r.stderr, r.stderr
    assert r.stdout == b""

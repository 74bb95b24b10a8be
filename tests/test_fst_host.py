"""FST decoder, host side (no GPU): the network reader and the duration tables of csrc/fst_net.cc against the
restatement tools/fst_restate.py, the restatement against the reference decoder's recorded answers
(tests/golden/fst/expected_*.txt, written by tools/make_fst_golden.py), its tie report, the ABI and the kernel's notes."""
import ctypes as C
import glob
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst")
CASES = sorted(os.path.basename(p)[9:-4] for p in glob.glob(os.path.join(GOLDEN, "expected_*.txt")))
HEAD = b"#FSTBasic MaxPlus\n"


def g9(x) -> str:
    return "%.9g" % float(x)


def expected(case):
    rows = []
    for line in open(os.path.join(GOLDEN, "expected_%s.txt" % case), "rb").read().split(b"\n"):
        if line:
            f = line.split(b"\t")
            rows.append((float(f[0]), int(f[1]), float(f[2]), float(f[3]), f[4].decode(), f[5].decode(), f[6].decode(), f[7]))
    return rows


def load_case(case):
    net = R.read_fst(open(os.path.join(GOLDEN, case + ".fst"), "rb").read())
    ac, lnabytes = R.read_lna(os.path.join(GOLDEN, case + ".lna"))
    dur = open(os.path.join(GOLDEN, case + ".dur")).read()
    return net, ac, lnabytes, dur


def test_the_golden_cases_are_there():
    assert CASES == ["durhi", "rand1", "rand2", "rand4", "toy", "wide"]
    assert {load_case(c)[2] for c in CASES} == {1, 2, 4}


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    """result strings equal, log-probabilities bit-equal (%.9g identifies a float), and no tie reported"""
    net, ac, _, dur = load_case(case)
    for beam, limit, ds, ts, lp, best, best_final, text in expected(case):
        r = R.search(net, ac, beam, limit, ds, ts, R.read_durations(dur))
        assert r.ties == [] and r.status == R.OK
        assert (r.text(net.symbols), g9(r.logprob), g9(r.best_logprob), g9(r.best_final_logprob)) == (text, lp, best, best_final), \
            (case, beam, limit)


def test_the_duration_term_of_durhi_is_not_zero():
    """the case whose pdfs lie in [n, 2n): with the reference's tables its answer depends on the duration scale"""
    net, ac, _, dur = load_case("durhi")
    with_dur = R.search(net, ac, durations=R.read_durations(dur))
    assert with_dur.logprob != R.search(net, ac, durations=None).logprob
    assert with_dur.logprob != R.search(net, ac, durations=R.read_durations(dur, by_state=True)).logprob
    assert g9(with_dur.logprob) == expected("durhi")[0][4]


# ---- the reader ---------------------------------------------------------------------------------------------------

def write(tmp_path, data: bytes, name="n.fst") -> str:
    p = os.path.join(str(tmp_path), name)
    open(p, "wb").write(data)
    return p


ACCEPTED = HEAD + (b"I 2\nT 2 0\nT 2 1\nT 1 1 3 ,\nT 1 4 0 sana\nT 4 4 0 , -1.5e-1\nT 4  6 -1 \xe4\xe4ni -2\n"
                   b"T 6 2 -1 sana 0.25\nT 0 0 -1 , -3\nF 6\nF 4\n")


def test_reader_accepts_every_form(capi, tmp_path):
    """3 ... 6 fields, `,`, bytes that are no UTF-8, runs of spaces, a first mention of -1 overridden later, file order"""
    want = R.read_fst(ACCEPTED)
    net = capi.FstNet(write(tmp_path, ACCEPTED))
    got = net.arrays()
    assert (net.num_nodes, net.num_arcs, net.initial, net.max_pdf) == (7, 8, 2, 3)
    assert net.symbols == want.symbols == [b"sana", b"\xe4\xe4ni"]
    for k in ("arc_begin", "arc_tgt", "arc_word", "node_pdf", "node_end"):
        assert np.array_equal(got[k], getattr(want, k)), k
    assert got["arc_lp"].tobytes() == want.arc_lp.tobytes()
    assert list(got["node_pdf"]) == [-1, 3, -1, -1, 0, -1, -1] and list(got["node_end"]) == [0, 0, 0, 0, 1, 0, 1]
    assert list(got["arc_lp"][[5, 6]]) == [np.float32(-0.15), np.float32(-2)]
    net.close()


REFUSED = [(b"#FSTBasic\nI 0\n", "Unknown header '#FSTBasic'."),
           (HEAD + b"I\n", "Too few fields 'I'."),
           (HEAD + b"I 0\n\nF 0\n", "Too few fields ''."),
           (HEAD + b"I 0 1\n", "Too many fields for I: 'I 0 1'."),
           (HEAD + b"I 0\nF 0 \n", "Too many fields for F: 'F 0 '."),
           (HEAD + b"I 0\nT 0\n", "Weird number of fields for T: 'T 0'."),
           (HEAD + b"I 0\nT 0 1 2 a -1 7\n", "Weird number of fields for T: 'T 0 1 2 a -1 7'."),
           (HEAD + b"I 0\nX 0 1\n", "Weird type indicator: 'X'."),
           (HEAD + b"I 0\nT 0 1 2\nT 1 1 3\n", "Conflicting emission_pdf_indices for node 1: 2 != 3."),
           (HEAD + b"T 0 1 2\n", "No initial node."),
           (HEAD + b"I 0\nT 0 -1 2\n", "Negative node index 'T 0 -1 2'.")]


@pytest.mark.parametrize("data,message", REFUSED)
def test_reader_refuses_with_the_reference_message(capi, tmp_path, data, message):
    with pytest.raises(R.FstReadError) as ei:
        R.read_fst(data)
    assert str(ei.value) == message
    h = C.c_void_p()
    assert capi.lib().aasr_fstnet_create_from_file(write(tmp_path, data).encode(), C.byref(h)) == capi.AASR_ERR_INVALID
    assert capi.lib().aasr_last_error().decode() == message and not h.value


def test_reader_keeps_pdf_indices_below_minus_one_as_written(capi, tmp_path):
    """atoi's value stays on the node; the search tests >= 0, so such a node does not emit -- in both readers"""
    data = HEAD + b"I 0\nT 0 1 -2\nT 1 1 -2\nF 1\n"
    want = R.read_fst(data)
    got = capi.FstNet(write(tmp_path, data)).arrays()
    assert list(got["node_pdf"]) == list(want.node_pdf) == [-1, -2]
    assert R.search(want, np.zeros((2, 1), np.float32)).logprob == 0


def test_reader_missing_file_is_an_io_status(capi, tmp_path):
    h = C.c_void_p()
    assert capi.lib().aasr_fstnet_create_from_file(os.path.join(str(tmp_path), "none.fst").encode(), C.byref(h)) == capi.AASR_ERR_IO


@pytest.mark.parametrize("case", CASES)
def test_reader_on_the_golden_networks(capi, case):
    want = load_case(case)[0]
    net = capi.FstNet(os.path.join(GOLDEN, case + ".fst"))
    got = net.arrays()
    assert net.symbols == want.symbols and net.initial == want.initial
    for k in ("arc_begin", "arc_tgt", "arc_word", "node_pdf", "node_end"):
        assert np.array_equal(got[k], getattr(want, k)), k
    assert got["arc_lp"].tobytes() == want.arc_lp.tobytes()


# ---- duration tables ----------------------------------------------------------------------------------------------

def test_duration_tables_in_both_indexings(capi, tmp_path):
    text = "4\n3\n0 2.5000 1.2500\n1 0.0000 0.0000\n2 7.1250 0.6250\n"
    d = capi.FstDurations(write(tmp_path, text.encode(), "m.dur"))
    assert d.num_states == 3
    ref_a, ref_b = R.read_durations(text)
    st_a, st_b = R.read_durations(text, by_state=True)
    assert list(ref_a) == [0, 0, 0, 2.5, 0, 7.125] and list(st_a) == [2.5, 0, 7.125]
    nonzero = 0
    for pdf in range(8):
        for dd in (0, 1, 2, 3, 17, 500):
            a = R.duration_logprob(ref_a, ref_b, pdf, dd)
            b = R.duration_logprob(st_a, st_b, pdf, dd)
            assert d.logprob(pdf, dd).tobytes() == a.tobytes(), (pdf, dd)
            assert d.logprob(pdf, dd, by_state=True).tobytes() == b.tobytes(), (pdf, dd)
            assert (a == 0) == (pdf not in (3, 5)) and (b == 0) == (pdf not in (0, 2))
            nonzero += (a != 0) + (b != 0)
    assert nonzero == 24
    # the reference's float expression, spelled out once by hand: a = 2.5, b = 1.25, d = 3
    f = np.float32
    logf, lgammaf = (lambda x: f(R._libm.logf(float(x)))), (lambda x: f(R._libm.lgammaf(float(x))))
    want = f(f(f(f(1.5) * logf(3)) - f(f(3) / f(1.25))) + f(f(f(-2.5) * logf(1.25)) - lgammaf(2.5)))
    assert d.logprob(0, 3, by_state=True) == want


@pytest.mark.parametrize("text", ["3\n1\n0 1 1\n", "4\n2\n0 1 1\n2 1 1\n", "4\n2\n0 1 1\n"])
def test_duration_file_refused(capi, tmp_path, text):
    h = C.c_void_p()
    assert capi.lib().aasr_fst_durations_read(write(tmp_path, text.encode(), "bad.dur").encode(), C.byref(h)) == capi.AASR_ERR_INVALID
    assert b"invalid format" in capi.lib().aasr_last_error()


# ---- the tie report -----------------------------------------------------------------------------------------------

def flat(frames, models=1):
    return np.zeros((frames, models), np.float32)


def test_tie_report_limit_boundary():
    net = R.read_fst(HEAD + b"I 0\nT 0 1 -1 a -1\nT 0 2 -1 b -1\nT 0 3 -1 c -2\nF 1\n")
    assert R.search(net, flat(1), token_limit=0).ties == [("limit", 0)]
    assert R.search(net, flat(1), token_limit=1).ties == []        # a and b stay, c is behind both
    assert R.search(net, flat(1), token_limit=0, beam=0.5).ties == [("limit", 0)]
    r = R.search(net, flat(1), token_limit=0)
    assert [t[0] for t in r.tokens] == [1]                          # the earlier candidate wins


def test_tie_report_duplicates_that_differ_in_dur():
    # frame 2 reaches node 1 by its self-loop (dur 2) and from node 2 (dur 1) with the same words and the same score
    net = R.read_fst(HEAD + b"I 0\nT 0 1 0 , -1\nT 0 2 0 , -1\nT 1 1 0 , -1\nT 2 2 0 , -1\nT 2 1 0 , -1\nF 1\n")
    r = R.search(net, flat(3))
    assert r.ties == [("dur", 2)] and [(t[0], t[2]) for t in r.tokens] == [(1, 2), (2, 2)]
    net = R.read_fst(HEAD + b"I 0\nT 0 1 0 , -1\nT 0 2 0 , -1\nT 1 1 0 , -1\nT 2 2 0 , -1\nT 2 1 0 , -1.5\nF 1\n")
    assert R.search(net, flat(3)).ties == []


def test_tie_report_final_tokens_that_differ_in_words():
    net = R.read_fst(HEAD + b"I 0\nT 0 1 -1 a -1\nT 0 2 -1 b -1\nF 1\nF 2\n")
    assert R.search(net, flat(1)).ties == [("final",)]
    net = R.read_fst(HEAD + b"I 0\nT 0 1 -1 a -1\nT 0 2 -1 b -1\nF 1\n")
    assert R.search(net, flat(1)).ties == []


def test_restatement_results_without_tokens_or_end_nodes():
    dead = R.search(R.read_fst(HEAD + b"I 0\nT 0 1 0\nF 1\n"), flat(3))
    assert dead.status == R.NO_TOKENS and dead.tokens == [] and dead.frames_done == 1
    assert (g9(dead.logprob), g9(dead.best_logprob), g9(dead.best_final_logprob)) == ("-1", "-9999999", "-10000000")
    none = R.search(R.read_fst(HEAD + b"I 0\nT 0 0 0 w\n"), flat(2))
    assert none.status == R.OK and none.words == () and g9(none.logprob) == "-1" and g9(none.best_logprob) == "0"
    start = R.search(R.read_fst(HEAD + b"I 0\nT 0 0 0 w\nF 0\n"), flat(0))
    assert start.tokens == [(0, np.float32(0), 0, ())] and g9(start.logprob) == "0"


# ---- ABI, options, kernel notes ------------------------------------------------------------------------------------

def test_abi_symbols_and_defaults(capi):
    names = set(capi.declared_symbols())
    need = {"aasr_fstnet_create_from_file", "aasr_fstnet_destroy", "aasr_fstnet_symbol", "aasr_fstnet_arrays",
            "aasr_fst_default_options", "aasr_fst_durations_read", "aasr_fst_durations_destroy", "aasr_fst_batch_create",
            "aasr_fst_batch_destroy", "aasr_fst_batch_device_bytes", "aasr_fst_batch_dev", "aasr_fst_batch_sync",
            "aasr_fst_batch_result", "aasr_fst_batch_tokens", "aasr_fst_batch_options"}
    assert need <= names and all(hasattr(capi.lib(), n) for n in need)
    o = capi.FstOptions.defaults()
    assert (o.beam, o.token_limit, o.duration_scale, o.transition_scale) == (2600.0, 5000, 3.0, 1.0)
    assert (o.dur_by_state, o.cap_candidates, o.cap_recomb, o.cap_history) == (0, 0, 0, 0)
    assert C.sizeof(o) == 32


def test_batch_create_refuses_bad_options_before_the_device(capi):
    net = capi.FstNet(os.path.join(GOLDEN, "toy.fst"))
    T = np.array([3], np.int32)
    for kw, word in (({"beam": -1.0}, "beam"), ({"beam": float("nan")}, "beam"), ({"token_limit": -1}, "token limit"),
                     ({"duration_scale": float("inf")}, "scales"), ({"cap_history": -2}, "capacity")):
        b = C.c_void_p()
        o = capi.FstOptions.defaults(**kw)
        assert capi.lib().aasr_fst_batch_create(net.handle, None, C.byref(o), 1, T.ctypes.data, C.byref(b)) == capi.AASR_ERR_INVALID
        assert word in capi.lib().aasr_last_error().decode()


FST_THREADS, FST_LDS_BYTES = 256, 1280


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "fst_search.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_kernel_notes(notes):
    assert sorted(k.split("::")[-1] for k in notes) == ["k_fst_search"], sorted(notes)
    text = open(os.path.join(ROOT, "aaltoasr_amd", "csrc", "fst_search.h")).read()
    assert "FST_THREADS = %d" % FST_THREADS in text and "FST_LDS_BYTES = %d" % FST_LDS_BYTES in text
    k = list(notes.values())[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0, k
    assert 0 < k["lds"] <= FST_LDS_BYTES, k

"""The forced aligner's host side, no GPU: the topology handle read from .ph files (transitions
included), its refusal of back-pointer offsets the search cannot encode, transcripts in both line
forms of aku/PhnReader.cc, the .phn line format of aku/align.cc:print_line and the align tool's
option table (aku/align.cc:180-198)."""
import ctypes as C
import os
import subprocess

import pytest

from aaltoasr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

# three HMMs: a (3 states, a skip 0 -> 2, unequal probabilities), b (1 state), c (2 states, a skip from
# its first state over the second straight into the next HMM)
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

EXPECTED_STATES = {"a": [0, 1, 2], "b": [3], "c": [4, 5]}
# per state: (target offset, probability) in file order; the dummy final state is +1 past the HMM's last state
EXPECTED_TRANSITIONS = {
    0: [(0, 0.6), (1, 0.3), (2, 0.1)],
    1: [(0, 0.7), (1, 0.3)],
    2: [(0, 0.8), (1, 0.2)],
    3: [(0, 0.5), (1, 0.5)],
    4: [(0, 0.5), (1, 0.25), (2, 0.25)],
    5: [(0, 0.9), (1, 0.1)],
}


@pytest.fixture(scope="module")
def lib():
    from aaltoasr_amd import build
    build.build()
    return A.lib()


@pytest.fixture
def topo(lib, tmp_path):
    p = tmp_path / "t.ph"
    p.write_text(PH)
    t = A.Topology(str(p))
    yield t
    t.close()


def test_topology_table(topo):
    assert topo.num_hmms() == 3
    assert topo.num_states() == 6
    for h, label in enumerate("abc"):
        assert topo.hmm_index(label) == h
        assert topo.hmm_label(h) == label
        assert topo.hmm_states(h) == EXPECTED_STATES[label]
    assert topo.hmm_index("zz") == -1
    for s, want in EXPECTED_TRANSITIONS.items():
        assert topo.transitions(s) == pytest.approx(want), s
    assert topo.max_offset() == 2


def test_topology_tied_state_keeps_first_transitions(lib, tmp_path):
    """A pdf mentioned by a second phone keeps the transitions of the first (HmmSet.cc:208-329)."""
    ph = PH.replace("3\n1 5 a", "4\n1 5 a") + "4 3 d\n-1 -2 3\n0 1 2 1.0\n1 0\n2 2 2 0.9 1 0.1\n"
    p = tmp_path / "tied.ph"
    p.write_text(ph)
    t = A.Topology(str(p))
    assert t.hmm_states(t.hmm_index("d")) == [3]
    assert t.transitions(3) == pytest.approx([(0, 0.5), (1, 0.5)])


def test_topology_read_errors(lib, tmp_path):
    p = tmp_path / "bad.ph"
    p.write_text("NOTPHONE\n1\n")
    with pytest.raises(A.AasrError):
        A.Topology(str(p))
    with pytest.raises(A.AasrError):
        A.Topology(str(tmp_path / "missing.ph"))


def test_offset_over_255_is_refused(lib, tmp_path):
    """A 300-state HMM whose first state skips to the final state: offset 300, which the search's
    uint8 back-pointers cannot hold."""
    n = 300
    lines = ["PHONE", "1", "1 %d long" % (n + 2), " ".join(["-1", "-2"] + [str(i) for i in range(n)]), "0 1 2 1.0", "1 0"]
    lines.append("2 2 2 0.5 1 0.5")
    for j in range(1, n):
        lines.append("%d 2 %d 0.5 %d 0.5" % (2 + j, 2 + j, 3 + j if j + 1 < n else 1))
    p = tmp_path / "long.ph"
    p.write_text("\n".join(lines) + "\n")
    t = A.Topology(str(p))
    assert t.max_offset() == n
    opts = A.AlignOptions.defaults()
    one = (C.c_int32 * 2)(0, 1)
    zero = (C.c_int32 * 1)(0)
    b = C.c_void_p()
    st = A.lib().aasr_align_batch_create(t.handle, C.byref(opts), 1, one, zero, zero, zero, one, C.byref(b))
    assert st == A.AASR_ERR_INVALID
    assert "255" in A.lib().aasr_last_error().decode()


def test_state_index_beyond_the_model_is_refused(topo):
    """aasr_topo_validate's check against the model's state count (aasr_gmm_num_states), host only"""
    topo.check_states(6)
    with pytest.raises(A.AasrError) as e:
        topo.check_states(5)
    assert "HMM c" in str(e.value) and "state 5" in str(e.value)
    with pytest.raises(A.AasrError) as e:
        topo.check_states(3)
    assert "HMM b" in str(e.value)


def test_transcript_both_line_forms(topo, tmp_path):
    p = tmp_path / "t.phn"
    p.write_text("a first comment\n\nb\n\nc,x with two words\n")
    assert topo.read_transcript(str(p)) == [0, 1, 2]
    # timed lines: sample numbers, label[.state], comment; a state field > 0 adds no HMM
    q = tmp_path / "s.phn"
    q.write_text("0 128 a.0 c0\n128 256 a.1\n256 512 a.2\n\n512 1024 c hello there\n1024 2048 b.0\n2048 4096 b.1\n")
    assert topo.read_transcript(str(q)) == [0, -1, -1, 2, 1, -1]


def test_transcript_frame_limits(topo, tmp_path):
    """PhnReader::set_frame_limits: timed lines ending at or before the first frame are skipped, lines
    starting at or after the last frame end the transcript (125 frames/s: 128 samples a frame)."""
    q = tmp_path / "s.phn"
    q.write_text("0 1280 a\n1280 2560 b\n2560 3840 c\n3840 5120 a\n")
    assert topo.read_transcript(str(q), 125.0, 10, 30) == [1, 2]
    assert topo.read_transcript(str(q), 125.0, 0, 0) == [0, 1, 2, 0]


def test_transcript_unknown_label_is_named(topo, tmp_path):
    p = tmp_path / "u.phn"
    p.write_text("a\nqq\n")
    with pytest.raises(A.AasrError) as e:
        topo.read_transcript(str(p))
    assert "qq" in str(e.value) and "u.phn" in str(e.value)


def test_phn_line_format(lib):
    # m = (int)(16000 / frame_rate): 128 at 125 frames/s, 160 at 100
    assert A.align_format_line(125.0, 3, 7, "a.0", "hello") == "384 896 a.0 hello\n"
    assert A.align_format_line(100.0, 0, 12, "b", "") == "0 1920 b \n"
    assert A.align_format_line(125.0, -1, 7, "a", "x") == ""
    # the last line of a file ends at window_start + 1
    assert A.align_format_line(125.0, 40, 50 + 1, "c.1", "") == "5120 6528 c.1 \n"


def test_align_help_lists_every_option(lib):
    exe = os.path.join(BIN, "align")
    assert os.access(exe, os.X_OK), exe
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for opt in ("--help", "--base", "--gk", "--mc", "--ph", "--config", "--recipe", "--swins", "--beam", "--sbeam",
                "--maxbeam", "--overlap", "--no-force-end", "--phoseg", "--speakers", "--batch", "--bindex", "--info"):
        assert opt in text, opt
    for short in ("-b", "-g", "-m", "-p", "-c", "-r", "-S", "-B", "-I", "-i"):
        assert short in text, short
    for default in ("1000", "100.0", "1600.0", "0.4"):
        assert default in text, default


@pytest.mark.parametrize("kw", [dict(beam=0.0), dict(beam=-5.0), dict(sbeam=-1), dict(maxbeam=float("inf"))])
def test_beams_that_would_retry_without_end_are_refused(topo, kw):
    """doubling a beam <= 0 never passes maxbeam: the search would restart forever"""
    opts = A.AlignOptions.defaults(**kw)
    one = (C.c_int32 * 2)(0, 1)
    zero = (C.c_int32 * 1)(0)
    b = C.c_void_p()
    st = A.lib().aasr_align_batch_create(topo.handle, C.byref(opts), 1, one, zero, zero, zero, one, C.byref(b))
    assert st == A.AASR_ERR_INVALID
    assert "beam" in A.lib().aasr_last_error().decode()


@pytest.mark.parametrize("overlap", [0.0, -0.5, float("nan"), 1.0, float("inf"), -1e30])
def test_overlaps_that_commit_a_whole_window_or_nothing_are_refused(topo, overlap):
    """overlap <= 0 commits all swins frames of a window and then moves to path[swins], one past the path;
    overlap >= 1 commits none.  Both are refused before any device is asked for."""
    opts = A.AlignOptions.defaults(overlap=overlap)
    one = (C.c_int32 * 2)(0, 1)
    zero = (C.c_int32 * 1)(0)
    b = C.c_void_p()
    st = A.lib().aasr_align_batch_create(topo.handle, C.byref(opts), 1, one, zero, zero, zero, one, C.byref(b))
    assert st == A.AASR_ERR_INVALID
    assert "overlap" in A.lib().aasr_last_error().decode()


def test_smallest_and_largest_overlap_pass_the_option_checks(topo):
    """swins 10: overlap 0.1 commits 9 frames, 0.9 commits 1 (the float product rounds up to 1.0)-- neither is
    refused for its overlap (what comes next needs a device, or succeeds on one)"""
    for overlap in (0.1, 0.9, 0.4):
        opts = A.AlignOptions.defaults(overlap=overlap, swins=10)
        one = (C.c_int32 * 2)(0, 1)
        zero = (C.c_int32 * 1)(0)
        b = C.c_void_p()
        st = A.lib().aasr_align_batch_create(topo.handle, C.byref(opts), 1, one, zero, zero, zero, one, C.byref(b))
        if st == A.AASR_OK:
            A.lib().aasr_align_batch_destroy(b)
        else:
            assert "overlap" not in A.lib().aasr_last_error().decode()


def test_align_tool_refuses_overlap_zero(lib, tmp_path):
    """the tool checks its options before it loads a model or asks for a device"""
    ph = tmp_path / "m.ph"
    ph.write_text(PH)
    exe = os.path.join(BIN, "align")
    r = subprocess.run([exe, "-g", str(tmp_path / "m.gk"), "-m", str(tmp_path / "m.mc"), "-p", str(ph),
                        "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.recipe"), "--overlap", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "overlap" in r.stderr and "must be positive" in r.stderr

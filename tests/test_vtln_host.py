"""VTLN estimation, the host side (no GPU): the tool's messages before a device is opened, the grid arithmetic, the
summary text, and the .phn reader's two modes (state-number labels, relative sample numbers) against a short
restatement of aku/PhnReader.cc's rules."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")


# ---- the tool's messages: before the device is opened (this runs without one) -----------------------------------------

@pytest.fixture(scope="module")
def files(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("vtln_host")
    open(str(d / "m.gk"), "w").write("1 2 diagonal_cov\n0 0 1 1\n")
    open(str(d / "m.mc"), "w").write("1\n1 0 1.0\n")
    open(str(d / "m.ph"), "w").write("PHONE\n1\n1 3 a\n-1 -2 0\n0 1 2 1.0\n1 0\n2 2 2 0.5 1 0.5\n")
    open(str(d / "full.gk"), "w").write("1 2 full_cov\n0 0 1 0 0 1\n")
    for e in ("mc", "ph"):
        open(str(d / ("full." + e)), "w").write(open(str(d / ("m." + e))).read())
    open(str(d / "f.cfg"), "w").write("module\n{\n  name a\n  type audiofile\n}\nmodule\n{\n  name fft\n  type fft\n  sources a\n}\n"
                                      "module\n{\n  name warp\n  type vtln\n  sources fft\n}\n")
    open(str(d / "r.rcp"), "w").write("audio=a.wav transcript=a.phn speaker=s1\n")
    open(str(d / "nospk.rcp"), "w").write("audio=b.wav transcript=b.phn\naudio=a.wav transcript=a.phn speaker=s1\n")
    open(str(d / "lines.rcp"), "w").write("audio=a.wav transcript=a.phn speaker=s1 start-line=3 end-line=5\n")
    open(str(d / "s.spkc"), "w").write("speaker default\n{\n}\n")
    return d


def run_tool(files, *extra, model=("-b", "m"), recipe="r.rcp", module="warp"):
    cmd = [os.path.join(BIN, "vtln")]
    if model:
        cmd += [model[0], str(files / model[1])]
    cmd += ["-c", str(files / "f.cfg"), "-r", str(files / recipe), "-S", str(files / "s.spkc"), "-v", module] + list(extra)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("kw,extra,message", [
    ({}, ["-B", "2"], "exception: Must give both --batch and --bindex"),
    ({}, ["-I", "1"], "exception: Must give both --batch and --bindex"),
    ({"module": "fft"}, [], "exception: Module fft is not a VTLN module"),
    ({"module": "nowhere"}, [], "exception: unknown module requested: nowhere"),
    ({"recipe": "nospk.rcp"}, [], "exception: Speaker ID is missing"),
    ({"model": None}, [], "exception: Must give either --base or all --gk, --mc and --ph"),
    ({"model": ("-g", "m.gk")}, [], "exception: Must give either --base or all --gk, --mc and --ph"),
    ({"recipe": "lines.rcp"}, [], "start-line / end-line"),
    ({"model": ("-b", "full")}, [], "only diagonal Gaussians are supported"),
])
def test_messages_before_the_device_is_opened(files, kw, extra, message):
    r = run_tool(files, *extra, **kw)
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert "hip" not in r.stderr.lower()


def test_an_accepted_command_line_reaches_the_device_and_fails_there(files):
    """the counterpart: what is not refused goes on to open the device, and says so when there is none"""
    r = run_tool(files, "--snl", "--rsamp", "--relative", "-B", "2", "-I", "1")
    assert r.returncode == 1 and "exception: " in r.stderr
    for m in ("Must give", "VTLN module", "Speaker ID", "not supported"):
        assert m not in r.stderr, r.stderr


# ---- grid arithmetic (aku/vtln.cc:214-225, 72-73), all in float ---------------------------------------------------------

def grid_restated(size, rad, relative, size_given, rad_given):
    f = np.float32
    start = f(rad)
    n = max(int(size), 1)
    step = f(f(2) * start) / f(max(n - 1, 1))
    if relative:
        if not rad_given:
            start = f(0.03)
        if not size_given:
            n = 5
        step = f(f(2) * start) / f(max(n - 1, 1))
    return f(-start), f(step), n


@pytest.mark.parametrize("kw", [
    {},                                                                         # the default grid: 21 points, 0.1
    {"relative": 1},                                                            # 5 points, 0.03
    {"relative": 1, "grid_size": 9, "grid_size_given": 1},
    {"relative": 1, "grid_rad": 0.05, "grid_rad_given": 1},
    {"grid_size": 1, "grid_size_given": 1},                                     # one point: the step divides by 1
    {"grid_size": 0, "grid_size_given": 1},
    {"grid_size": 5, "grid_size_given": 1, "grid_rad": 0.04, "grid_rad_given": 1},
])
def test_grid_arithmetic_in_float(capi, kw):
    kw = {k: (np.float32(v) if k == "grid_rad" else v) for k, v in kw.items()}
    o = capi.VtlnOptions.defaults(**kw)
    assert o.grid_size == kw.get("grid_size", 21) and np.float32(o.grid_rad) == np.float32(kw.get("grid_rad", 0.1))
    start, step, n = capi.vtln_grid(o)
    want = grid_restated(o.grid_size, o.grid_rad, o.relative, o.grid_size_given, o.grid_rad_given)
    assert (start.tobytes(), step.tobytes(), n) == (want[0].tobytes(), want[1].tobytes(), want[2]), (start, step, n, want)
    # the warp factors around a centre of 1: symmetric to float rounding, the first at 1 - radius
    warps = [np.float32(np.float32(1) + start + np.float32(i) * step) for i in range(n)]
    assert warps[0] == np.float32(np.float32(1) + start)
    if n > 1:
        assert abs(float(warps[-1]) - (1 - float(start))) < 1e-6 and all(b > a for a, b in zip(warps, warps[1:]))


# ---- the summary file (aku/vtln.cc:118-129) ---------------------------------------------------------------------------

def test_summary_text_for_two_speakers_given_out_of_order(capi):
    text = capi.vtln_summary_text(["spkB", "spkA"], [[np.float32(0.96), np.float32(1.0)], [np.float32(1.04)]],
                                  [[-1234.5678, -1200.0004], [-99.9996]])
    assert text == "[spkA]\n1.040: -100.000\n\n[spkB]\n0.960: -1234.568\n1.000: -1200.000\n\n"
    assert capi.vtln_summary_text([], [], []) == ""
    assert capi.vtln_summary_text(["x"], [[]], [[]]) == "[x]\n\n"


# ---- the reader's modes (aku/PhnReader.cc:96-124, 164-167, 360-386) ---------------------------------------------------

PH = """PHONE
3
1 5 a
-1 -2 0 1 2
0 1 2 1.0
1 0
2 2 2 0.5 3 0.5
3 2 3 0.5 4 0.5
4 2 4 0.5 1 0.5
2 5 b
-1 -2 3 4 5
0 1 2 1.0
1 0
2 2 2 0.5 3 0.5
3 2 3 0.5 4 0.5
4 2 4 0.5 1 0.5
3 4 c
-1 -2 6 7
0 1 2 1.0
1 0
2 2 2 0.5 3 0.5
3 2 3 0.5 1 0.5
"""
HMM_STATES = {"a": [0, 1, 2], "b": [3, 4, 5], "c": [6, 7]}
SPF = 128.0      # samples per frame at 125 frames a second


def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


class Restated:
    """PhnReader over a file's text: next_phn_line (:294-399), set_frame_limits (:102-124), and next_frame (:138-221)
    driven until the reader's end or the generator's end of file"""

    def __init__(self, text, first, last, snl, rsamp):
        self.lines, self.pos = text.split("\n"), 0
        self.first, self.last, self.snl, self.rsamp = first, last, snl, rsamp

    def next_line(self):
        while True:
            if self.pos >= len(self.lines):
                return None
            line = self.lines[self.pos]
            self.pos += 1
            if line:
                break
        state, start, end = -1, -1, -1
        if line[0].isdigit():
            f = re.split(r"[ \t]+", line, maxsplit=3)
            start, end = int(int(f[0]) / SPF), int(int(f[1]) / SPF)
            head = f[2]
            if "." in head:
                i = head.index(".")
                state = atoi(head[i + 1:])
                head = head[:i] + head[i + 2:]
        else:
            head = re.split(r"[ \t]+", line, maxsplit=1)[0]
        if self.rsamp and start >= 0:
            start, end = start + self.first, end + self.first
        if self.last > 0:
            if start >= self.last:
                return None
            if end >= self.last:
                end = self.last
        if self.first > 0 and 0 <= start < self.first:
            start = self.first
        if self.snl:
            return start, end, atoi(head), None
        return start, end, state, head.split(",")[0]

    def set_frame_limits(self):
        if self.rsamp:
            return
        while True:
            old = self.pos
            line = self.next_line()
            if line is None:
                return
            if line[1] < 0 or line[1] > self.first:
                self.pos = old
                return

    def frames(self, eof_frame=-1):
        if self.first > 0 or self.last > 0:
            self.set_frame_limits()
        cur = self.next_line()
        if cur is None:
            return None
        frame, out, start_frame, eof = -1, [], 0, False
        while not eof:
            frame = cur[0] if frame == -1 else frame + 1
            state = cur[2] if self.snl else HMM_STATES[cur[3]][cur[2]]
            while frame + 1 >= cur[1]:
                cur = self.next_line()
                if cur is None:
                    eof = True
                    break
            if eof_frame >= 0 and frame >= eof_frame:
                break
            if not out:
                start_frame = frame
            out.append(state)
        return start_frame, out


@pytest.fixture(scope="module")
def topo(capi, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vtln_phn") / "t.ph")
    open(path, "w").write(PH)
    t = capi.Topology(path)
    assert t.num_states() == 8
    return t


SNL_FILE = "0 1280 3\n1280 1408 7 a comment\n\n1408 2560 abc\n2560 3840 2x\n3840 5120 5.1\n"
LABEL_FILE = "0 1280 a.0\n1280 2560 a.1\n2560 3840 b.2,x\n3840 5120 c.0\n5120 6400 c.1\n"


@pytest.mark.parametrize("text,snl,rsamp,first,last,eof", [
    (SNL_FILE, True, False, 0, 0, -1),
    (SNL_FILE, True, False, 0, 0, 25),            # the generator's end of file inside a line
    (SNL_FILE, True, False, 12, 33, -1),          # a start-time / end-time window: lines skipped, times clipped
    (SNL_FILE, True, True, 12, 33, -1),           # the same window over relative sample numbers: shifted, nothing skipped
    (SNL_FILE, True, True, 100, 0, -1),
    (LABEL_FILE, False, False, 0, 0, -1),         # the modes off: aasr_stats_read_segmentation's behaviour
    (LABEL_FILE, False, False, 15, 42, -1),
    (LABEL_FILE, False, True, 15, 42, -1),
    (LABEL_FILE, False, True, 15, 0, 40),
])
def test_reader_modes_against_the_restatement(capi, topo, tmp_path, text, snl, rsamp, first, last, eof):
    path = str(tmp_path / "u.phn")
    open(path, "w").write(text)
    want = Restated(text, first, last, snl, rsamp).frames(eof)
    got = capi.phn_read_segmentation(topo, path, 125.0, first, last, eof, snl=snl, rsamp=rsamp)
    assert want is not None and got is not None
    assert got[0] == want[0] and got[1].tolist() == want[1], (got, want)
    assert len(want[1]) > 0 and (got[2] == -1).all()
    if not snl and not rsamp:      # the flags' defaults change nothing for the present callers
        old = capi.stats_read_segmentation(topo, path, 125.0, first, last, eof, transitions=False)
        assert old[0] == got[0] and old[1].tolist() == got[1].tolist()


def test_a_label_that_is_no_number_counts_as_state_0(capi, topo, tmp_path):
    path = str(tmp_path / "u.phn")
    open(path, "w").write("0 256 abc\n256 512 2x\n512 768 c.1\n")
    start, pdf, _ = capi.phn_read_segmentation(topo, path, 125.0, snl=True)
    assert start == 0 and pdf.tolist() == [0, 0, 2, 2, 0, 0]       # atoi("abc") = 0, atoi("2x") = 2, atoi("c") = 0


def test_relative_sample_numbers_shift_by_the_first_frame(capi, topo, tmp_path):
    path = str(tmp_path / "u.phn")
    open(path, "w").write("0 640 4\n640 1280 6\n")
    start, pdf, _ = capi.phn_read_segmentation(topo, path, 125.0, 50, 58, snl=True, rsamp=True)
    assert start == 50 and pdf.tolist() == [4] * 5 + [6] * 3
    # without --rsamp the same window lies past the file's lines
    assert capi.phn_read_segmentation(topo, path, 125.0, 50, 58, snl=True) is None


def test_refusals_of_the_reader(capi, topo, tmp_path):
    path = str(tmp_path / "u.phn")
    open(path, "w").write("0 256 1\n256 512 8\n")
    with pytest.raises(capi.AasrError) as ei:      # no transitions from state-number labels
        capi.phn_read_segmentation(topo, path, 125.0, snl=True, transitions=True)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "state number labels" in ei.value.msg
    with pytest.raises(capi.AasrError) as ei:      # a state the model does not have
        capi.phn_read_segmentation(topo, path, 125.0, snl=True)
    assert ei.value.code == capi.AASR_ERR_INVALID and "state 8" in ei.value.msg
    open(path, "w").write("0 256 a.0\n256 512 a.1\n")
    start, pdf, tr = capi.phn_read_segmentation(topo, path, 125.0, rsamp=True, transitions=True)    # rsamp alone: allowed
    assert pdf.tolist() == [0, 0, 1, 1] and tr[-1] == -1 and (tr[:-1] >= 0).all()

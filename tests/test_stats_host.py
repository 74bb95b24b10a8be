"""ML statistics on the host, no GPU: the segmentation reader (aku/PhnReader.cc:138-292 as stats
configures it) against a Python restatement over crafted .phn files, the dump writers of
HmmSet::dump_statistics against hand-built bytes and text, and the stats tool's refusals, which all
happen before a device is opened."""
import os
import struct
import subprocess

import numpy as np
import pytest

from aaltoasr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

# a: 3 states with a skip 0 -> 2; b: 1 state; c: 2 states whose first state can skip straight out
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
HMMS = {"a": [0, 1, 2], "b": [3], "c": [4, 5]}
OFFSETS = {0: [0, 1, 2], 1: [0, 1], 2: [0, 1], 3: [0, 1], 4: [0, 1, 2], 5: [0, 1]}
SPF = 128  # samples per frame at 125 frames/s


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


def tr_base():
    base, n = {}, 0
    for s in sorted(OFFSETS):
        base[s] = n
        n += len(OFFSETS[s])
    return base


def restate(lines, first=0, last=0, eof=-1, transitions=True):
    """PhnReader::next_frame with state_num_labels = false, driven as stats.cc:simple_train drives it.
    lines: (start frame, end frame, label, state) as the file holds them."""
    # next_phn_line's frame limits and set_frame_limits' skip of the lines that end before the first frame
    clipped = []
    for s, e, lab, k in lines:
        if last > 0 and s >= last:
            break
        if last > 0 and e >= last:
            e = last
        if first > 0 and 0 <= s < first:
            s = first
        clipped.append((s, e, lab, k))
    if first > 0 or last > 0:
        while clipped and not (clipped[0][1] < 0 or clipped[0][1] > first):
            clipped.pop(0)
    if not clipped:
        return None
    base = tr_base()
    it = iter(clipped)
    cur = next(it)
    frame, eof_flag, start = -1, False, None
    pdf, trs = [], []
    while not eof_flag:
        frame = cur[0] if frame == -1 else frame + 1
        if cur[3] < 0:
            raise ValueError("A state segmented phn file is required")
        if cur[2] not in HMMS:
            raise ValueError("Unknown HMM")
        state = HMMS[cur[2]][cur[3]]
        prev, loaded = cur, False
        while frame + 1 >= cur[1]:
            nxt = next(it, None)
            if nxt is None:
                eof_flag = True
                break
            cur, loaded = nxt, True
        t = -1
        if transitions and not eof_flag:
            offs = OFFSETS[state]
            if loaded:
                n_states = len(HMMS[prev[2]])
                for i, o in enumerate(offs):
                    nx = o + prev[3]
                    if (nx >= n_states and cur[3] == 0) or (o != 0 and nx == cur[3]):
                        t = base[state] + i
                        break
            else:
                t = base[state] + offs.index(0) if 0 in offs else -1
            if t < 0:
                raise ValueError("Correct transition was not found")
        if eof >= 0 and frame >= eof:
            break
        if start is None:
            start = frame
        pdf.append(state)
        trs.append(t)
    return (start if start is not None else 0), pdf, trs


def write_phn(path, lines):
    with open(path, "w") as f:
        for s, e, lab, k in lines:
            f.write("%d %d %s%s comment\n" % (s * SPF, e * SPF, lab, "" if k < 0 else ".%d" % k))


CASES = {
    "contiguous": [(0, 3, "a", 0), (3, 5, "a", 1), (5, 9, "a", 2), (9, 12, "b", 0), (12, 14, "c", 0), (14, 20, "c", 1)],
    "gaps_overlaps_zero_length": [(2, 4, "a", 0), (6, 9, "a", 1), (7, 7, "a", 2), (9, 10, "a", 2), (5, 11, "b", 0),
                                  (11, 11, "c", 0), (12, 16, "c", 0)],
    "skips_and_leaving": [(0, 2, "a", 0), (2, 5, "a", 2), (5, 8, "c", 0), (8, 10, "b", 0), (10, 13, "c", 1)],
    "c_skips_out": [(0, 4, "c", 0), (4, 6, "a", 0), (6, 9, "a", 1), (9, 12, "a", 2)],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("limits", [(0, 0, -1), (4, 0, -1), (0, 10, -1), (3, 11, -1), (0, 0, 7), (2, 0, 12)])
def test_segmentation_matches_restatement(topo, tmp_path, name, limits):
    first, last, eof = limits
    p = str(tmp_path / "s.phn")
    write_phn(p, CASES[name])
    want = restate(CASES[name], first, last, eof)
    got = A.stats_read_segmentation(topo, p, 125.0, first, last, eof)
    assert (got is None) == (want is None)
    if want is None:
        return
    assert got[0] == want[0]
    assert got[1].tolist() == want[1]
    assert got[2].tolist() == want[2]


def test_segmentation_by_hand(topo, tmp_path):
    p = str(tmp_path / "s.phn")
    write_phn(p, [(1, 3, "a", 0), (3, 4, "a", 2), (4, 6, "b", 0)])
    start, pdf, tr = A.stats_read_segmentation(topo, p)
    base = tr_base()
    assert start == 1
    assert pdf.tolist() == [0, 0, 2, 3, 3]
    # self, skip 0 -> 2 (offset 2), out of a (offset 1 leaves the HMM into b.0), self, none on the last frame
    assert tr.tolist() == [base[0], base[0] + 2, base[2] + 1, base[3], -1]
    # without -t no transitions
    assert A.stats_read_segmentation(topo, p, transitions=False)[2].tolist() == [-1] * 5


def test_segmentation_errors(topo, tmp_path):
    p = str(tmp_path / "s.phn")
    write_phn(p, [(0, 3, "a", -1)])
    with pytest.raises(A.AasrError, match="A state segmented phn file is required"):
        A.stats_read_segmentation(topo, p)
    write_phn(p, [(0, 3, "a", 0), (3, 5, "zz", 0)])
    with pytest.raises(A.AasrError, match="Unknown HMM in transcription"):
        A.stats_read_segmentation(topo, p, transitions=False)
    write_phn(p, [(0, 3, "a", 2), (3, 5, "a", 1)])
    with pytest.raises(A.AasrError, match="Correct transition was not found"):
        A.stats_read_segmentation(topo, p)
    assert A.stats_read_segmentation(topo, p, transitions=False)[1].tolist() == [2, 2, 2, 1, 1]
    # the EOF cut ends the frames before a bad line is reached
    write_phn(p, [(0, 3, "a", 0), (3, 5, "a", -1)])
    assert A.stats_read_segmentation(topo, p, eof_frame=2, transitions=False)[1].tolist() == [0, 0]
    open(p, "w").close()
    assert A.stats_read_segmentation(topo, p) is None


def test_write_gks_bytes(lib, tmp_path):
    p = str(tmp_path / "x.gks")
    fc = np.array([3, 0, 1_000_001])
    g = np.array([2.5, 0.0, 7.25])
    a = np.array([2.5, 0.0, 7.5])
    sx = np.array([[1.0, 2.0], [0, 0], [0.1, -3.0]])
    sxx = np.array([[4.0, 5.0], [0, 0], [1e10, 3.0]])
    A.stats_write_gks(p, fc, g, a, sx, sxx)
    want = struct.pack("<3i", 3, 2, 1)
    for i in range(3):
        want += struct.pack("<i", i)
        if fc[i] > 0:
            want += struct.pack("<iidd", 0, int(fc[i]), g[i], a[i]) + np.asarray(sx[i], "<f4").tobytes() + \
                np.asarray(sxx[i], "<f4").tobytes()
        want += struct.pack("<i", -1)
    assert open(p, "rb").read() == want


def test_write_mcs_text(lib, tmp_path):
    p = str(tmp_path / "x.mcs")
    A.stats_write_mcs(p, [0, 2, 3, 5], [4, 1, 0, 2, 3], [10, 0, 2_000_000],
                      [1.0 / 3, 2.0 / 3, 5.0, 1234567.891234, 1e-20], [0, 0, 0], [-12.345678901234, 0.0, -1.5e7])
    assert open(p).read() == (
        "3\n1\n"
        "0\n0 2 4 0.3333333333 1 0.6666666667 0 -12.3456789\n-1\n"
        "1\n-1\n"
        "2\n0 2 2 1234567.891 3 1e-20 0 -15000000\n-1\n")


def test_write_phs_text(lib, tmp_path):
    p = str(tmp_path / "x.phs")
    A.stats_write_phs(p, [0, 0, 1, 2], [0, 1, 0, 2], [999999.0, 0.0, 1e6, 1234567.0])
    assert open(p).read() == "4\n0 0 999999\n1 0 1e+06\n2 2 1.23457e+06\n"


def test_write_lls_text(lib, tmp_path):
    p = str(tmp_path / "x.lls")
    A.stats_write_lls(p, -1234567.123456789, 2345678)
    assert open(p).read() == "Numerator loglikelihood: -1234567.12346\nNumber of frames: 2345678\n"


def _model(tmp_path):
    base = str(tmp_path / "m")
    open(base + ".ph", "w").write(PH)
    with open(base + ".gk", "w") as f:
        f.write("2 2 variable\ndiag 0 0 1 1\ndiag 1 1 1 1\n")
    with open(base + ".mc", "w") as f:
        f.write("6\n" + "1 0 1.0\n" * 6)
    open(str(tmp_path / "f.cfg"), "w").write("module\n{\n name fft\n type fft\n}\n")
    open(str(tmp_path / "r.rcp"), "w").write("audio=x.wav transcript=x.phn\n")
    return base


def _run(args):
    r = subprocess.run([os.path.join(BIN, "stats")] + args, capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("opt,msg", [
    (["-H"], "-H"), (["--mmi"], "--mmi"), (["--mpe"], "--mpe"), (["--grad"], "--grad"), (["--mllt"], "--mllt"),
    (["-P"], "-P"), (["--savelat"], "--savelat"), (["-a"], "-a"), (["--nseggk", "x.gk"], "--nseggk"),
    (["--nsegmc", "x.mc"], "--nsegmc"),
])
def test_tool_refuses_other_modes(lib, tmp_path, opt, msg):
    base = _model(tmp_path)
    rc, err = _run(["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o",
                    str(tmp_path / "o"), "--ml"] + opt)
    assert rc != 0 and msg in err and "not supported" in err, err


def test_tool_needs_a_mode(lib, tmp_path):
    base = _model(tmp_path)
    rc, err = _run(["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o", str(tmp_path / "o")])
    assert rc != 0 and "At least one mode (--ml, --mmi, --mpe) must be given!" in err


def test_tool_refuses_full_and_subspace_pools(lib, tmp_path):
    base = _model(tmp_path)
    common = ["-b", base, "-c", str(tmp_path / "f.cfg"), "-r", str(tmp_path / "r.rcp"), "-o", str(tmp_path / "o"),
              "--ml", "-t", "-F", "0", "-W", "0", "-A", "1"]
    with open(base + ".gk", "w") as f:
        f.write("2 2 variable\ndiag 0 0 1 1\nfull 1 1 1 0 0 1\n")
    rc, err = _run(common)
    assert rc != 0 and "only diagonal Gaussians" in err and "'full'" in err, err
    with open(base + ".gk", "w") as f:
        f.write("1 2 full_cov\n0 0 1 0 0 1\n")
    rc, err = _run(common)
    assert rc != 0 and "only diagonal Gaussians" in err, err
    with open(base + ".gk", "w") as f:
        f.write("2 2 variable\ndiag 0 0 1 1\npcgmm 1 1 0.5 0.5\n")
    rc, err = _run(common)
    assert rc != 0 and "'pcgmm'" in err, err


def test_tool_refuses_model_transforms_and_line_limits(lib, tmp_path):
    base = _model(tmp_path)
    spk = str(tmp_path / "s.spkc")
    open(spk, "w").write("speaker default\n{\nmodel cmllr\n{\nunit no\n}\n}\n")
    common = ["-b", base, "-c", str(tmp_path / "f.cfg"), "-o", str(tmp_path / "o"), "--ml"]
    rc, err = _run(common + ["-r", str(tmp_path / "r.rcp"), "-S", spk])
    assert rc != 0 and "model transforms" in err, err
    rcp = str(tmp_path / "l.rcp")
    open(rcp, "w").write("audio=x.wav transcript=x.phn start-line=2 end-line=5\n")
    rc, err = _run(common + ["-r", rcp])
    assert rc != 0 and "line limits" in err, err
    rc, err = _run(common + ["-r", str(tmp_path / "r.rcp"), "-B", "2"])
    assert rc != 0 and "Must give both --batch and --bindex" in err, err
